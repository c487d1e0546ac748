// inflate_core.h — one RFC 1951 (raw DEFLATE) decoder for the host and the device (DESIGN.md §2 "BGZF inflate").  No dependencies.
//
// ccsx_infl_stream<L>() decodes exactly ONE stream of in_len bytes into exactly out_len bytes and returns an enum ccsx_inflate_status.  The code is written for a
// group of L::nlanes() lanes that run it in lock step: the symbol loop is uniform (every lane holds the same bit buffer and decodes the same symbol), the decode
// tables are built by all lanes, and match / stored copies are spread over the lanes.  On the host the group is one lane (ccsx_infl_serial); k_inflate
// (ccsx_inflate.hip) runs it as one wave64 with the tables and the output window in LDS.
//
// Robust by construction — it eats file bytes:
//   - every loop is bounded by the input bits that remain, the output bytes that remain, or a constant;
//   - every table index is masked to the primary table or range-checked against the table's capacity;
//   - every read is inside in[0, in_len), every write inside win[0, out_len);
//   - a corrupt stream ends in a status, never in an access out of range or a loop without end.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define CCSX_INFL_HD __host__ __device__
#else
#define CCSX_INFL_HD
#endif

#ifndef CCSX_INFLATE_STATUS_DEFINED
#define CCSX_INFLATE_STATUS_DEFINED
enum ccsx_inflate_status {
    CCSX_INFLATE_OK                = 0,
    CCSX_INFLATE_TRUNCATED_INPUT   = 1,  /* the stream needs bits beyond in_len                                              */
    CCSX_INFLATE_BAD_BLOCK_TYPE    = 2,  /* BTYPE 3                                                                          */
    CCSX_INFLATE_BAD_STORED_LENGTH = 3,  /* LEN != ~NLEN                                                                     */
    CCSX_INFLATE_BAD_CODE_LENGTHS  = 4,  /* over- or under-subscribed code (except zlib's `max == 1` rule: a literal / length or a distance
                                            code of exactly one 1-bit codeword passes, its unused codeword reads as BAD_SYMBOL; the
                                            code-length code is strict), a repeat without a previous length or past the end, more than
                                            286 / 30 codes, no end-of-block code                                               */
    CCSX_INFLATE_BAD_SYMBOL        = 5,  /* a code that stands for no symbol (litlen 286/287, distance 30/31, unassigned)     */
    CCSX_INFLATE_BAD_DISTANCE      = 6,  /* a match reaches before the start of this stream's output                         */
    CCSX_INFLATE_OUTPUT_OVERRUN    = 7,  /* the stream holds more than out_len bytes                                          */
    CCSX_INFLATE_OUTPUT_SHORT      = 8   /* the final block ended before out_len bytes                                        */
};
#endif

#define CCSX_INFL_LIT_BITS  10     /* primary table bits, literal / length code */
#define CCSX_INFL_DIST_BITS 8      /* primary table bits, distance code          */
#define CCSX_INFL_LIT_CAP   2048   /* >= 1334: the most a complete 288-symbol code of <= 15 bits needs with a 10-bit primary table (zlib's `enough 288 10 15`) */
#define CCSX_INFL_DIST_CAP  512    /* >= 402:  `enough 32 8 15`                                                                                                  */
#define CCSX_INFL_MAX_SYMS  320    /* 288 + 32 code lengths of a dynamic block                                                                                   */

// a table entry: bits 0..3 bits to consume (a sub-table pointer: the sub-table's index bits), bits 4..6 kind, bits 8..11 extra bits,
// bits 16..31 literal byte / base length / base distance / first entry of the sub-table
enum { CCSX_INFL_K_INVALID = 0, CCSX_INFL_K_LIT = 1, CCSX_INFL_K_BASE = 2, CCSX_INFL_K_EOB = 3, CCSX_INFL_K_SUB = 4, CCSX_INFL_K_BADSYM = 5 };
enum { CCSX_INFL_LITLEN = 0, CCSX_INFL_DIST = 1, CCSX_INFL_PRECODE = 2 };

struct ccsx_infl_tables {
    uint32_t lit[CCSX_INFL_LIT_CAP];
    uint32_t dist[CCSX_INFL_DIST_CAP];
    uint16_t sorted[CCSX_INFL_MAX_SYMS];   // symbols in canonical order (by length, then by value)
    uint8_t  lens[CCSX_INFL_MAX_SYMS];
};

// the one-lane group of the host
struct ccsx_infl_serial {
    static CCSX_INFL_HD int lane() { return 0; }
    static CCSX_INFL_HD int nlanes() { return 1; }
    static CCSX_INFL_HD void sync() {}
    static CCSX_INFL_HD uint64_t ballot(bool p) { return p ? 1u : 0u; }
    static CCSX_INFL_HD uint64_t lanes_below() { return 0; }
    static CCSX_INFL_HD uint32_t uniform(uint32_t v) { return v; }
};

static inline CCSX_INFL_HD uint32_t ccsx_infl_rev(uint32_t v, int n)   // the low n <= 16 bits of v, reversed
{
    v = ((v & 0x5555u) << 1) | ((v >> 1) & 0x5555u);
    v = ((v & 0x3333u) << 2) | ((v >> 2) & 0x3333u);
    v = ((v & 0x0f0fu) << 4) | ((v >> 4) & 0x0f0fu);
    v = ((v & 0x00ffu) << 8) | ((v >> 8) & 0x00ffu);
    return v >> (16 - n);
}

static inline CCSX_INFL_HD uint32_t ccsx_infl_entry(int kind, int sym, int nbits)
{
    uint32_t k = CCSX_INFL_K_LIT, val = (uint32_t)sym, extra = 0;
    if (kind == CCSX_INFL_LITLEN && sym >= 256) {
        if (sym == 256) { k = CCSX_INFL_K_EOB; val = 0; }
        else if (sym < 265) { k = CCSX_INFL_K_BASE; val = (uint32_t)(sym - 254); }
        else if (sym < 285) { k = CCSX_INFL_K_BASE; extra = (uint32_t)(sym - 261) >> 2; val = 3u + ((4u + ((uint32_t)(sym - 261) & 3u)) << extra); }
        else if (sym == 285) { k = CCSX_INFL_K_BASE; val = 258; }
        else { k = CCSX_INFL_K_BADSYM; val = 0; }
    } else if (kind == CCSX_INFL_DIST) {
        if (sym < 4) { k = CCSX_INFL_K_BASE; val = (uint32_t)sym + 1u; }
        else if (sym < 30) { k = CCSX_INFL_K_BASE; extra = ((uint32_t)sym >> 1) - 1u; val = 1u + ((2u + ((uint32_t)sym & 1u)) << extra); }
        else { k = CCSX_INFL_K_BADSYM; val = 0; }
    }
    return (uint32_t)nbits | (k << 4) | (extra << 8) | (val << 16);
}

// Build the decode table of a canonical code from lens[0, n) (n <= 288): a primary table of 2^P entries and, for codes longer than P bits, sub-tables behind it
// (the layout of libdeflate / zlib).  All lanes call it together.  cap = entries the table holds.
template <class L>
static inline CCSX_INFL_HD int ccsx_infl_build(const uint8_t *lens, int n, uint32_t *table, int P, int cap, int kind, uint16_t *sorted)
{
    const int lane = L::lane(), nl = L::nlanes();
    const uint64_t below = L::lanes_below();
    uint32_t cnt[16];
#pragma unroll
    for (int l = 0; l < 16; ++l) cnt[l] = 0;
    for (int base = 0; base < n; base += nl) {
        const int i = base + lane;
        const int mylen = i < n ? (lens[i] & 15) : 0;
#pragma unroll
        for (int l = 1; l < 16; ++l) cnt[l] += (uint32_t)__builtin_popcountll(L::ballot(mylen == l));
    }
    // Kraft sum in units of 2^-15
    uint32_t used = 0, total = 0;
#pragma unroll
    for (int l = 1; l < 16; ++l) { used += cnt[l] << (15 - l); total += cnt[l]; }
    for (int i = lane; i < (1 << P); i += nl) table[i] = 0;            // CCSX_INFL_K_INVALID: a code nothing was assigned to
    if (total == 0) { L::sync(); return kind == CCSX_INFL_DIST ? CCSX_INFLATE_OK : CCSX_INFLATE_BAD_CODE_LENGTHS; }   // a block of literals only may carry no distance code
    if (used > 32768u) { L::sync(); return CCSX_INFLATE_BAD_CODE_LENGTHS; }
    // zlib's `max == 1` rule: a literal / length or distance code of exactly one 1-bit codeword is the one incomplete code that passes (its other codeword stays
    // CCSX_INFL_K_INVALID); the code-length code is strict
    if (used < 32768u && !(kind != CCSX_INFL_PRECODE && total == 1 && cnt[1] == 1)) { L::sync(); return CCSX_INFLATE_BAD_CODE_LENGTHS; }
    uint32_t offs[16], first[16];
    {
        uint32_t o = 0, c = 0;
#pragma unroll
        for (int l = 1; l < 16; ++l) { c <<= 1; offs[l] = o; first[l] = c; o += cnt[l]; c += cnt[l]; }
    }
    // canonical order: sorted[offs[len] + rank among the symbols of that length]
    {
        uint32_t next[16];
#pragma unroll
        for (int l = 1; l < 16; ++l) next[l] = offs[l];
        for (int base = 0; base < n; base += nl) {
            const int i = base + lane;
            const int mylen = i < n ? (lens[i] & 15) : 0;
#pragma unroll
            for (int l = 1; l < 16; ++l) {
                const uint64_t m = L::ballot(mylen == l);
                if (mylen == l) {
                    const uint32_t at = next[l] + (uint32_t)__builtin_popcountll(m & below);
                    if (at < CCSX_INFL_MAX_SYMS) sorted[at] = (uint16_t)i;
                }
                next[l] += (uint32_t)__builtin_popcountll(m);
            }
        }
    }
    L::sync();
    uint32_t nshort = 0;
#pragma unroll
    for (int l = 1; l < 16; ++l) if (l <= P) nshort += cnt[l];
    // codes of up to P bits: every lane fills the entries of its symbols
    for (uint32_t idx = (uint32_t)lane; idx < nshort; idx += (uint32_t)nl) {
        const int sym = sorted[idx];
        const int len = sym < n ? (lens[sym] & 15) : 0;
        uint32_t f = 0, o = 0;
#pragma unroll
        for (int l = 1; l < 16; ++l) if (len == l) { f = first[l]; o = offs[l]; }
        if (len < 1 || len > P) continue;
        const uint32_t e = ccsx_infl_entry(kind, sym, len);
        for (uint32_t k = ccsx_infl_rev(f + (idx - o), len); k < (1u << P); k += 1u << len) table[k] = e;
    }
    // longer codes, one after the other (they are the rare symbols): a sub-table per P-bit prefix, sized by the longest code behind that prefix
    if (nshort < total) {
        uint32_t code = 0;
#pragma unroll
        for (int l = 1; l < 16; ++l) if (l == P) code = first[l] + cnt[l];   // the first code after the short ones, at P bits
        int curlen = P;
        uint32_t next_free = 1u << P, cur_prefix = 0xffffffffu, sub_start = 0;
        int sub_bits = 0;
        for (uint32_t idx = nshort; idx < total && idx < CCSX_INFL_MAX_SYMS; ++idx) {
            const int sym = (int)L::uniform(sorted[idx]);
            const int len = sym < n ? (int)L::uniform(lens[sym] & 15) : 0;
            if (len <= P || len < curlen) { L::sync(); return CCSX_INFLATE_BAD_CODE_LENGTHS; }   // (cannot happen: sorted is in canonical order)
            code <<= (len - curlen); curlen = len;
            const uint32_t prefix = code >> (len - P);
            if (prefix != cur_prefix) {
                if (prefix >= (1u << P)) { L::sync(); return CCSX_INFLATE_BAD_CODE_LENGTHS; }
                uint32_t acc = 0; int maxl = len;
                for (uint32_t j = idx; j < total && j < CCSX_INFL_MAX_SYMS && acc < (1u << (15 - P)); ++j) {
                    const int sj = (int)L::uniform(sorted[j]);
                    const int lj = sj < n ? (int)L::uniform(lens[sj] & 15) : 15;
                    if (lj < 1) break;
                    acc += 1u << (15 - lj); maxl = lj;
                }
                sub_bits = maxl - P;
                if (sub_bits < 1 || sub_bits > 15 - P || next_free + (1u << sub_bits) > (uint32_t)cap) { L::sync(); return CCSX_INFLATE_BAD_CODE_LENGTHS; }
                sub_start = next_free; next_free += 1u << sub_bits; cur_prefix = prefix;
                for (uint32_t k = (uint32_t)lane; k < (1u << sub_bits); k += (uint32_t)nl) table[sub_start + k] = 0;
                if (lane == 0) table[ccsx_infl_rev(prefix, P)] = (uint32_t)sub_bits | ((uint32_t)CCSX_INFL_K_SUB << 4) | (sub_start << 16);
                L::sync();
            }
            const int rest = len - P;
            if (rest > sub_bits) { L::sync(); return CCSX_INFLATE_BAD_CODE_LENGTHS; }
            const uint32_t e = ccsx_infl_entry(kind, sym, rest);
            for (uint32_t k = ccsx_infl_rev(code & ((1u << rest) - 1u), rest) + ((uint32_t)lane << rest); k < (1u << sub_bits); k += (uint32_t)nl << rest)
                table[sub_start + k] = e;
            ++code;
        }
    }
    L::sync();
    return CCSX_INFLATE_OK;
}

// the bit reader: `cnt` valid bits in `buf`, `pos` = input bytes loaded so far.  Uniform over the lanes.
struct ccsx_infl_bits {
    uint64_t buf;
    int cnt;
    int64_t pos;
};

template <class L>
static inline CCSX_INFL_HD void ccsx_infl_refill(ccsx_infl_bits &b, const uint8_t *in, int64_t in_len)
{
    if (b.cnt <= 32 && b.pos + 4 <= in_len) {
        uint32_t w;
        memcpy(&w, in + b.pos, 4);                     // (little-endian hosts and the device)
        b.buf |= (uint64_t)L::uniform(w) << b.cnt;
        b.cnt += 32; b.pos += 4;
    }
    while (b.cnt <= 56 && b.pos < in_len) {
        b.buf |= (uint64_t)L::uniform(in[b.pos]) << b.cnt;
        b.cnt += 8; ++b.pos;
    }
}

// one symbol of a code: the entry that decodes it, its bits consumed.  kind INVALID with cnt untouched = not enough input
template <class L>
static inline CCSX_INFL_HD int ccsx_infl_symbol(ccsx_infl_bits &b, const uint32_t *table, int P, int cap, uint32_t *entry)
{
    uint32_t e = L::uniform(table[(uint32_t)b.buf & ((1u << P) - 1u)]);
    if (((e >> 4) & 7u) == CCSX_INFL_K_SUB) {
        if (b.cnt < P) return CCSX_INFLATE_TRUNCATED_INPUT;
        const uint32_t sub_bits = e & 15u, start = e >> 16;
        const uint32_t at = start + ((uint32_t)(b.buf >> P) & ((1u << sub_bits) - 1u));
        if (at >= (uint32_t)cap) return CCSX_INFLATE_BAD_SYMBOL;
        b.buf >>= P; b.cnt -= P;
        e = L::uniform(table[at]);
        if (((e >> 4) & 7u) == CCSX_INFL_K_SUB) return CCSX_INFLATE_BAD_SYMBOL;
    }
    const uint32_t k = (e >> 4) & 7u;
    const int nb = (int)(e & 15u);
    if (k == CCSX_INFL_K_INVALID) return b.cnt < 15 ? CCSX_INFLATE_TRUNCATED_INPUT : CCSX_INFLATE_BAD_SYMBOL;   // (short input reads as zero bits: blame the input first)
    if (nb > b.cnt) return CCSX_INFLATE_TRUNCATED_INPUT;
    b.buf >>= nb; b.cnt -= nb;
    if (k == CCSX_INFL_K_BADSYM) return CCSX_INFLATE_BAD_SYMBOL;
    *entry = e;
    return CCSX_INFLATE_OK;
}

#define CCSX_INFL_TAKE(var, nbits)                                                                  \
    do {                                                                                            \
        if ((nbits) > b.cnt) return CCSX_INFLATE_TRUNCATED_INPUT;                                   \
        (var) = (uint32_t)(b.buf & ((1ull << (nbits)) - 1ull)); b.buf >>= (nbits); b.cnt -= (nbits); \
    } while (0)

// Decode one raw DEFLATE stream in[0, in_len) into win[0, out_len).  All lanes of the group call it with the same arguments; the status is the same on every lane.
// After the call a lane sees the other lanes' bytes only behind an L::sync().
template <class L>
static inline CCSX_INFL_HD int ccsx_infl_stream(const uint8_t *in, int64_t in_len, uint8_t *win, int64_t out_len, ccsx_infl_tables *T)
{
    const int lane = L::lane(), nl = L::nlanes();
    ccsx_infl_bits b;
    b.buf = 0; b.cnt = 0; b.pos = 0;
    int64_t op = 0;
    if (in_len < 0 || out_len < 0) return CCSX_INFLATE_TRUNCATED_INPUT;
    for (;;) {                                                   // every block consumes at least 3 bits of input
        ccsx_infl_refill<L>(b, in, in_len);
        uint32_t bfinal, btype;
        CCSX_INFL_TAKE(bfinal, 1);
        CCSX_INFL_TAKE(btype, 2);
        if (btype == 3) return CCSX_INFLATE_BAD_BLOCK_TYPE;
        if (btype == 0) {
            uint32_t drop, len, nlen;
            CCSX_INFL_TAKE(drop, b.cnt & 7);                     // to the byte boundary
            (void)drop;
            ccsx_infl_refill<L>(b, in, in_len);
            CCSX_INFL_TAKE(len, 16);
            CCSX_INFL_TAKE(nlen, 16);
            if ((len ^ nlen) != 0xffffu) return CCSX_INFLATE_BAD_STORED_LENGTH;
            b.pos -= b.cnt >> 3; b.buf = 0; b.cnt = 0;           // hand the whole bytes in the bit buffer back
            if (b.pos < 0 || (int64_t)len > in_len - b.pos) return CCSX_INFLATE_TRUNCATED_INPUT;
            if ((int64_t)len > out_len - op) return CCSX_INFLATE_OUTPUT_OVERRUN;
            for (uint32_t i = (uint32_t)lane; i < len; i += (uint32_t)nl) win[op + i] = in[b.pos + i];
            b.pos += len; op += len;
        } else {
            if (btype == 1) {
                for (int i = lane; i < 288; i += nl) T->lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
                for (int i = lane; i < 32; i += nl) T->lens[288 + i] = 5;
                L::sync();
                int rc = ccsx_infl_build<L>(T->lens, 288, T->lit, CCSX_INFL_LIT_BITS, CCSX_INFL_LIT_CAP, CCSX_INFL_LITLEN, T->sorted);
                if (rc) return rc;
                rc = ccsx_infl_build<L>(T->lens + 288, 32, T->dist, CCSX_INFL_DIST_BITS, CCSX_INFL_DIST_CAP, CCSX_INFL_DIST, T->sorted);
                if (rc) return rc;
            } else {
                uint32_t hlit, hdist, hclen;
                CCSX_INFL_TAKE(hlit, 5);
                CCSX_INFL_TAKE(hdist, 5);
                CCSX_INFL_TAKE(hclen, 4);
                hlit += 257; hdist += 1; hclen += 4;
                if (hlit > 286 || hdist > 30) return CCSX_INFLATE_BAD_CODE_LENGTHS;
                for (int i = lane; i < 19; i += nl) T->lens[i] = 0;
                L::sync();
                for (uint32_t i = 0; i < hclen; ++i) {
                    ccsx_infl_refill<L>(b, in, in_len);
                    uint32_t v;
                    CCSX_INFL_TAKE(v, 3);
                    // the order of RFC 1951 §3.2.7: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, five bits each in two words
                    const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
                    const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
                    const uint32_t at = (uint32_t)((i < 12 ? lo >> (5 * i) : hi >> (5 * (i - 12))) & 31u);
                    if (lane == 0 && at < 19) T->lens[at] = (uint8_t)v;
                }
                L::sync();
                // the code-length code borrows the literal table, which is rebuilt below
                int rc = ccsx_infl_build<L>(T->lens, 19, T->lit, 7, CCSX_INFL_LIT_CAP, CCSX_INFL_PRECODE, T->sorted);
                if (rc) return rc;
                const uint32_t nsym = hlit + hdist;              // <= 316
                uint32_t i = 0, prev = 0;
                while (i < nsym) {                               // every round consumes at least one bit and writes at least one length
                    ccsx_infl_refill<L>(b, in, in_len);
                    uint32_t e;
                    rc = ccsx_infl_symbol<L>(b, T->lit, 7, CCSX_INFL_LIT_CAP, &e);
                    if (rc) return rc == CCSX_INFLATE_BAD_SYMBOL ? CCSX_INFLATE_BAD_CODE_LENGTHS : rc;
                    const uint32_t s = e >> 16;
                    uint32_t rep = 1, val = s;
                    if (s == 16) { if (i == 0) return CCSX_INFLATE_BAD_CODE_LENGTHS; CCSX_INFL_TAKE(rep, 2); rep += 3; val = prev; }
                    else if (s == 17) { CCSX_INFL_TAKE(rep, 3); rep += 3; val = 0; }
                    else if (s == 18) { CCSX_INFL_TAKE(rep, 7); rep += 11; val = 0; }
                    else if (s > 15) return CCSX_INFLATE_BAD_CODE_LENGTHS;
                    if (rep > nsym - i) return CCSX_INFLATE_BAD_CODE_LENGTHS;
                    // (the lengths collect in sorted[], free until the next build: lens[0, 19) still holds the code-length code's own lengths)
                    for (uint32_t k = (uint32_t)lane; k < rep; k += (uint32_t)nl) T->sorted[i + k] = (uint16_t)val;
                    i += rep; prev = val;
                }
                L::sync();
                for (uint32_t k = (uint32_t)lane; k < nsym; k += (uint32_t)nl) T->lens[k] = (uint8_t)T->sorted[k];
                L::sync();
                if (T->lens[256] == 0) return CCSX_INFLATE_BAD_CODE_LENGTHS;   // no end-of-block code
                L::sync();
                rc = ccsx_infl_build<L>(T->lens, (int)hlit, T->lit, CCSX_INFL_LIT_BITS, CCSX_INFL_LIT_CAP, CCSX_INFL_LITLEN, T->sorted);
                if (rc) return rc;
                rc = ccsx_infl_build<L>(T->lens + hlit, (int)hdist, T->dist, CCSX_INFL_DIST_BITS, CCSX_INFL_DIST_CAP, CCSX_INFL_DIST, T->sorted);
                if (rc) return rc;
            }
            // the symbol loop: uniform.  Every round consumes at least one bit or returns
            for (;;) {
                ccsx_infl_refill<L>(b, in, in_len);
                uint32_t e;
                int rc = ccsx_infl_symbol<L>(b, T->lit, CCSX_INFL_LIT_BITS, CCSX_INFL_LIT_CAP, &e);
                if (rc) return rc;
                const uint32_t k = (e >> 4) & 7u;
                if (k == CCSX_INFL_K_LIT) {
                    if (op >= out_len) return CCSX_INFLATE_OUTPUT_OVERRUN;
                    if (lane == 0) win[op] = (uint8_t)(e >> 16);
                    ++op;
                    continue;
                }
                    if (k == CCSX_INFL_K_EOB) break;
                uint32_t x, len = e >> 16, dist;
                CCSX_INFL_TAKE(x, (int)((e >> 8) & 15u));
                len += x;
                rc = ccsx_infl_symbol<L>(b, T->dist, CCSX_INFL_DIST_BITS, CCSX_INFL_DIST_CAP, &e);
                if (rc) return rc;
                dist = e >> 16;
                CCSX_INFL_TAKE(x, (int)((e >> 8) & 15u));
                dist += x;
                if ((int64_t)dist > op || dist == 0) return CCSX_INFLATE_BAD_DISTANCE;
                if ((int64_t)len > out_len - op) return CCSX_INFLATE_OUTPUT_OVERRUN;
                L::sync();                                       // the bytes behind op, written by any lane, are visible to every lane
                const uint8_t *from = win + (op - dist);
                uint8_t *to = win + op;
                if (dist >= len) { for (uint32_t i = (uint32_t)lane; i < len; i += (uint32_t)nl) to[i] = from[i]; }
                else if (dist == 1) { const uint8_t v = from[0]; for (uint32_t i = (uint32_t)lane; i < len; i += (uint32_t)nl) to[i] = v; }
                else { for (uint32_t i = (uint32_t)lane; i < len; i += (uint32_t)nl) to[i] = from[i % dist]; }   // an overlapping copy reads only bytes behind op
                op += len;
                }
        }
        if (bfinal) break;
    }
    L::sync();
    return op == out_len ? CCSX_INFLATE_OK : CCSX_INFLATE_OUTPUT_SHORT;
}

// the host's form: one lane, the output written in place
static inline int ccsx_infl_stream_host(const uint8_t *in, int64_t in_len, uint8_t *out, int64_t out_len, ccsx_infl_tables *T)
{
    return ccsx_infl_stream<ccsx_infl_serial>(in, in_len, out, out_len, T);
}

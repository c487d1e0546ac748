// deflate_core.h — one RFC 1951 (raw DEFLATE) encoder and its CRC32 for the host and the device (DESIGN.md §2 "BGZF deflate").  No dependencies.
//
// ccsx_defl_span<L>() encodes ONE span of 0 .. CCSX_DEFL_MAX_IN bytes into one raw DEFLATE stream and computes the span's CRC32 (zlib polynomial).  The code is
// written for a group of L::nlanes() lanes that run it in lock step: every branch around an L::sync() is uniform, the shared state lives in a ccsx_defl_work, and
// the only operations whose order differs between groups are integer atomics (add, or, xor, max), whose results do not depend on order.  The stream and the CRC are
// therefore a pure function of the input bytes and the rule version, whatever the lane count.  On the host the group is one lane (ccsx_defl_serial); k_deflate
// (ccsx_deflate.hip) runs it as one workgroup with the input and the work area in LDS.
//
// The rule (version 1):
//   - the span is coded as sub-blocks of CCSX_DEFL_SUB positions, one dynamic-Huffman block (BTYPE 2) per sub-block, the last with BFINAL; a token belongs to the
//     sub-block its first byte lies in (a match may run over the boundary, never past the span's end);
//   - match finder: positions are hashed (4 bytes, CCSX_DEFL_HASH_BITS bits) chunk by chunk of CCSX_DEFL_CHUNK positions.  The hash candidate of position p is the
//     largest q < p with the same hash that lies in an EARLIER chunk (atomic max of q + 1 per bucket, taken after the chunk's look-ups); the second candidate is
//     p - 1 (runs).  A candidate counts with distance <= 32768 and length >= 4 (minimum match 4), lengths are cut at 258 and at the span's end, the longer one wins,
//     the tie goes to p - 1;
//   - greedy parse: next = p + max(1, len(p)) from position 0;
//   - Huffman: lengths of the minimum-redundancy code of the block's own counts (ties by symbol value), limited to 15 bits (7 for the code-length code) by folding
//     the longer codes to the limit and repairing the Kraft sum (one code of the limit removed, the deepest shorter code split, until the sum is exactly 1); an
//     alphabet with fewer than two used symbols gets symbol 0 and / or 1 added with count 1, so no code ever has a single codeword; canonical codes;
//   - header: HLIT / HDIST / HCLEN trimmed, the two length lists run-length coded as one sequence with 16 / 17 / 18 (greedy: longest repeat first);
//   - if the coded stream is not smaller than the stored form (BTYPE 0 blocks of at most 65535 bytes), or a sub-block does not fit the staging area of
//     CCSX_DEFL_STAGE_BYTES, the stream is the stored form.  An empty span is one empty stored block;
//   - CRC32: slices of CCSX_DEFL_CRC_SLICE bytes, each shifted to its place by multiplication with x^(8 * bytes behind it) in GF(2)[x] / P and xor-ed together.
//
// Robust by construction: every loop is bounded by the bytes or bits that remain or by a constant, every table index is masked or checked, every read is inside
// in[0, n), every write inside out[0, out_cap); a span that does not fit is CCSX_DEFLATE_OUTPUT_FULL.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define CCSX_DEFL_HD __host__ __device__
#else
#define CCSX_DEFL_HD
#endif

#ifndef CCSX_DEFLATE_STATUS_DEFINED
#define CCSX_DEFLATE_STATUS_DEFINED
enum ccsx_deflate_status {
    CCSX_DEFLATE_OK          = 0,
    CCSX_DEFLATE_OUTPUT_FULL = 1   /* the stream (coded or stored, whichever the rule picks) is longer than out_cap */
};
#endif

#define CCSX_DEFL_RULE_VERSION 1
#define CCSX_DEFL_MAX_IN      65536
#define CCSX_DEFL_MIN_MATCH   4
#define CCSX_DEFL_MAX_MATCH   258
#define CCSX_DEFL_MAX_DIST    32768
#define CCSX_DEFL_CHUNK       256                        /* positions hashed together: a candidate lies in an earlier chunk                        */
#define CCSX_DEFL_HASH_BITS   13
#define CCSX_DEFL_HASH_SIZE   (1 << CCSX_DEFL_HASH_BITS)
#define CCSX_DEFL_SUB         8192                       /* positions per sub-block (a multiple of the chunk)                                      */
#define CCSX_DEFL_STAGE_BYTES 13312                      /* coded bytes of one sub-block that the staging area holds                                */
#define CCSX_DEFL_STAGE_WORDS (CCSX_DEFL_STAGE_BYTES / 4 + 4)
#define CCSX_DEFL_CRC_SLICE   256
#define CCSX_DEFL_MAX_LANES   256
#define CCSX_DEFL_NLIT        286
#define CCSX_DEFL_NDIST       30
#define CCSX_DEFL_NPRE        19
#define CCSX_DEFL_DIST0       CCSX_DEFL_NLIT                         /* the three alphabets share one index space */
#define CCSX_DEFL_PRE0        (CCSX_DEFL_NLIT + CCSX_DEFL_NDIST)
#define CCSX_DEFL_NSYM        (CCSX_DEFL_PRE0 + CCSX_DEFL_NPRE + 1)  /* 336 */

// match[]: bit 31 = a token starts here, bits 16..24 = match length (0: literal), bits 0..15 = distance - 1
#define CCSX_DEFL_TOKEN 0x80000000u

enum { CCSX_DEFL_S_CRC = 0, CCSX_DEFL_S_POS = 1, CCSX_DEFL_S_USED = 2, CCSX_DEFL_S_HDR = 3, CCSX_DEFL_S_HLIT = 4, CCSX_DEFL_S_HDIST = 5, CCSX_DEFL_S_HCLEN = 6,
       CCSX_DEFL_S_NOPS = 7, CCSX_DEFL_S_N = 8 };

struct ccsx_defl_work {
    uint32_t head[CCSX_DEFL_HASH_SIZE];        // bucket -> 1 + the largest position of an earlier chunk with that hash (0: none)
    uint32_t match[CCSX_DEFL_SUB];
    uint32_t stage[CCSX_DEFL_STAGE_WORDS];     // the sub-block's bits, zeroed, then or-ed in
    uint32_t freq[CCSX_DEFL_NSYM];
    uint32_t key[CCSX_DEFL_NLIT + 2];          // code construction: counts in ascending order, then tree depths
    uint32_t part[CCSX_DEFL_MAX_LANES];        // bits per lane slice
    uint32_t first[16];                        // first canonical code of a length
    uint32_t scal[CCSX_DEFL_S_N];              // values one lane hands to all
    uint16_t order[CCSX_DEFL_NLIT + 2];        // the used symbols in ascending order of (count, symbol)
    uint16_t code[CCSX_DEFL_NSYM];             // canonical codes, bit-reversed: ready to be or-ed in LSB first
    uint16_t ops[CCSX_DEFL_NLIT + CCSX_DEFL_NDIST + 4];   // the header's code-length sequence: symbol | extra << 8
    uint8_t  len[CCSX_DEFL_NSYM];
};

// the one-lane group of the host
struct ccsx_defl_serial {
    static CCSX_DEFL_HD int lane() { return 0; }
    static CCSX_DEFL_HD int nlanes() { return 1; }
    static CCSX_DEFL_HD void sync() {}
    static CCSX_DEFL_HD void atomic_add(uint32_t *p, uint32_t v) { *p += v; }
    static CCSX_DEFL_HD void atomic_or(uint32_t *p, uint32_t v) { *p |= v; }
    static CCSX_DEFL_HD void atomic_xor(uint32_t *p, uint32_t v) { *p ^= v; }
    static CCSX_DEFL_HD void atomic_max(uint32_t *p, uint32_t v) { if (v > *p) *p = v; }
};

// ---- CRC32 (zlib polynomial, reflected: x^0 is bit 31)
#define CCSX_DEFL_POLY 0xedb88320u

static inline CCSX_DEFL_HD uint32_t ccsx_defl_gf2_mul(uint32_t a, uint32_t b)     // a * b mod P
{
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b >> 1) ^ (CCSX_DEFL_POLY & (0u - (b & 1u)));
    }
    return p;
}

static inline CCSX_DEFL_HD uint32_t ccsx_defl_gf2_xpow_bytes(uint32_t nbytes)     // x^(8 * nbytes) mod P: the operator that shifts a CRC over nbytes bytes
{
    uint32_t r = 0x80000000u, sq = 0x00800000u;                                   // x^0, x^8
    for (int i = 0; i < 32 && nbytes; ++i, nbytes >>= 1) {
        if (nbytes & 1u) r = ccsx_defl_gf2_mul(r, sq);
        sq = ccsx_defl_gf2_mul(sq, sq);
    }
    return r;
}

static inline CCSX_DEFL_HD uint32_t ccsx_defl_crc_bytes(const uint8_t *p, uint32_t n)   // the CRC32 of p[0, n), byte by byte
{
    uint32_t c = 0xffffffffu;
    for (uint32_t i = 0; i < n; ++i) {
        c ^= p[i];
#pragma unroll
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (CCSX_DEFL_POLY & (0u - (c & 1u)));
    }
    return ~c;
}

// the part of the CRC32 of p[0, n) that slice s contributes: xor over all slices = the CRC
static inline CCSX_DEFL_HD uint32_t ccsx_defl_crc_slice(const uint8_t *p, uint32_t n, uint32_t s)
{
    const uint32_t at = s * CCSX_DEFL_CRC_SLICE;
    if (at >= n) return 0;
    const uint32_t m = n - at < CCSX_DEFL_CRC_SLICE ? n - at : CCSX_DEFL_CRC_SLICE;
    return ccsx_defl_gf2_mul(ccsx_defl_gf2_xpow_bytes(n - at - m), ccsx_defl_crc_bytes(p + at, m));
}

// the rule's CRC of p[0, n): every lane takes slices, acc (shared, set to 0 by this call) collects them.  Uniform result behind the last sync
template <class L>
static inline CCSX_DEFL_HD uint32_t ccsx_defl_crc(const uint8_t *p, uint32_t n, uint32_t *acc)
{
    if (L::lane() == 0) *acc = 0;
    L::sync();
    const uint32_t ns = (n + CCSX_DEFL_CRC_SLICE - 1) / CCSX_DEFL_CRC_SLICE;
    for (uint32_t s = (uint32_t)L::lane(); s < ns; s += (uint32_t)L::nlanes()) L::atomic_xor(acc, ccsx_defl_crc_slice(p, n, s));
    L::sync();
    return *acc;
}

// ---- symbols
static inline CCSX_DEFL_HD uint32_t ccsx_defl_rev(uint32_t v, int n)   // the low n (1 .. 16) bits of v, reversed
{
    v = ((v & 0x5555u) << 1) | ((v >> 1) & 0x5555u);
    v = ((v & 0x3333u) << 2) | ((v >> 2) & 0x3333u);
    v = ((v & 0x0f0fu) << 4) | ((v >> 4) & 0x0f0fu);
    v = ((v & 0x00ffu) << 8) | ((v >> 8) & 0x00ffu);
    return v >> (16 - n);
}

static inline CCSX_DEFL_HD int ccsx_defl_log2(uint32_t v) { return 31 - __builtin_clz(v | 1u); }

// length 3 .. 258 -> symbol 257 .. 285, extra bits and their value
static inline CCSX_DEFL_HD void ccsx_defl_len_sym(uint32_t len, uint32_t *sym, uint32_t *eb, uint32_t *ev)
{
    const uint32_t l = len - 3u;
    if (len >= 258u) { *sym = 285; *eb = 0; *ev = 0; return; }
    if (l < 4u) { *sym = 257u + l; *eb = 0; *ev = 0; return; }
    const uint32_t e = (uint32_t)ccsx_defl_log2(l) - 2u;
    *sym = 261u + 4u * e + ((l >> e) & 3u); *eb = e; *ev = l & ((1u << e) - 1u);
}

// distance - 1 (0 .. 32767) -> symbol 0 .. 29, extra bits and their value
static inline CCSX_DEFL_HD void ccsx_defl_dist_sym(uint32_t d, uint32_t *sym, uint32_t *eb, uint32_t *ev)
{
    d &= 32767u;
    if (d < 4u) { *sym = d; *eb = 0; *ev = 0; return; }
    const uint32_t lg = (uint32_t)ccsx_defl_log2(d), e = lg - 1u;
    *sym = 2u * lg + ((d >> e) & 1u); *eb = e; *ev = d & ((1u << e) - 1u);
}

static inline CCSX_DEFL_HD uint32_t ccsx_defl_hash(const uint8_t *p)
{
    uint32_t w;
    memcpy(&w, p, 4);
    return (w * 2654435761u) >> (32 - CCSX_DEFL_HASH_BITS);
}

static inline CCSX_DEFL_HD uint32_t ccsx_defl_match_len(const uint8_t *a, const uint8_t *b, uint32_t maxl)
{
    uint32_t l = 0;
    while (l < maxl && a[l] == b[l]) ++l;
    return l;
}

// or nbits (<= 48) of v into the zeroed staging words at bit `at`
template <class L>
static inline CCSX_DEFL_HD void ccsx_defl_put(uint32_t *stage, uint32_t at, uint64_t v, uint32_t nbits)
{
    const uint32_t w = at >> 5, sh = at & 31u;
    if (!nbits || w + 2u >= CCSX_DEFL_STAGE_WORDS) return;
    const uint64_t lo = (uint64_t)(uint32_t)v << sh, hi = (uint64_t)(uint32_t)(v >> 32) << sh;
    if ((uint32_t)lo) L::atomic_or(stage + w, (uint32_t)lo);
    const uint32_t mid = (uint32_t)(lo >> 32) | (uint32_t)hi;
    if (mid) L::atomic_or(stage + w + 1, mid);
    if ((uint32_t)(hi >> 32)) L::atomic_or(stage + w + 2, (uint32_t)(hi >> 32));
}

// the bits of the token that starts at position p: m = its match[] word, lit = in[p]
static inline CCSX_DEFL_HD uint32_t ccsx_defl_token(const ccsx_defl_work *W, uint32_t m, uint32_t lit, uint64_t *bits)
{
    const uint32_t mlen = (m >> 16) & 511u;
    if (!mlen) { *bits = W->code[lit & 255u]; return W->len[lit & 255u]; }
    uint32_t ls, le, lv, ds, de, dv;
    ccsx_defl_len_sym(mlen, &ls, &le, &lv);
    ccsx_defl_dist_sym(m & 0xffffu, &ds, &de, &dv);
    ds += CCSX_DEFL_DIST0;
    uint32_t n = W->len[ls];
    uint64_t b = W->code[ls];
    b |= (uint64_t)lv << n; n += le;
    b |= (uint64_t)W->code[ds] << n; n += W->len[ds];
    b |= (uint64_t)dv << n; n += de;
    *bits = b;
    return n;
}

// Code lengths (<= maxbits) and canonical codes of the alphabet freq[0, nsym) into len / code[0, nsym).  All lanes call it together.
template <class L>
static inline CCSX_DEFL_HD void ccsx_defl_build(ccsx_defl_work *W, int sym0, int nsym, int maxbits)
{
    const int lane = L::lane(), nl = L::nlanes();
    uint32_t *freq = W->freq + sym0;
    uint8_t *len = W->len + sym0;
    uint16_t *code = W->code + sym0;
    if (lane == 0) W->scal[CCSX_DEFL_S_USED] = 0;
    L::sync();
    for (int i = lane; i < nsym; i += nl) { len[i] = 0; if (freq[i]) L::atomic_add(&W->scal[CCSX_DEFL_S_USED], 1u); }
    L::sync();
    uint32_t nu = W->scal[CCSX_DEFL_S_USED];
    if (nu < 2u) {                                               // never a code of a single codeword
        L::sync();
        if (lane == 0) { if (nu == 0u) freq[0] = freq[1] = 1; else if (!freq[0]) freq[0] = 1; else freq[1] = 1; }   // (one used and it is symbol 0: symbol 1 is free)
        nu = 2;
        L::sync();
    }
    // ascending order of (count, symbol): the rank of a used symbol is the number of used symbols before it
    for (int i = lane; i < nsym; i += nl) {
        const uint32_t f = freq[i];
        if (!f) continue;
        uint32_t r = 0;
        for (int j = 0; j < nsym; ++j) { const uint32_t g = freq[j]; r += (g && (g < f || (g == f && j < i))) ? 1u : 0u; }
        if (r < (uint32_t)(CCSX_DEFL_NLIT + 2)) { W->order[r] = (uint16_t)i; W->key[r] = f; }
    }
    L::sync();
    if (lane == 0) {
        uint32_t *A = W->key;
        const int n = (int)(nu > (uint32_t)nsym ? (uint32_t)nsym : nu);
        // minimum-redundancy code lengths in place (Moffat & Katajainen 1995): A[] ascending counts -> A[] depths
        A[0] += A[1];
        int root = 0, leaf = 2;
        for (int next = 1; next < n - 1; ++next) {
            if (leaf >= n || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = (uint32_t)next; } else A[next] = A[leaf++];
            if (leaf >= n || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = (uint32_t)next; } else A[next] += A[leaf++];
        }
        A[n - 2] = 0;
        for (int next = n - 3; next >= 0; --next) A[next] = A[A[next] < (uint32_t)n ? A[next] : 0] + 1u;
        int avbl = 1, used = 0, dpth = 0, next = n - 1;
        root = n - 2;
        while (avbl > 0 && next >= 0) {
            while (root >= 0 && (int)A[root] == dpth) { ++used; --root; }
            while (avbl > used && next >= 0) { A[next--] = (uint32_t)dpth; --avbl; }
            avbl = 2 * used; ++dpth; used = 0;
        }
        // fold the codes longer than maxbits to maxbits, then repair the Kraft sum (in units of 2^-maxbits)
        uint32_t cnt[16];
        for (int l = 0; l < 16; ++l) cnt[l] = 0;
        for (int i = 0; i < n; ++i) { const uint32_t d = A[i]; ++cnt[d < 1u ? 1u : d > (uint32_t)maxbits ? (uint32_t)maxbits : d]; }
        uint32_t total = 0;
        for (int l = 1; l <= maxbits; ++l) total += cnt[l] << (maxbits - l);
        for (int guard = 0; total > (1u << maxbits) && guard < 65536; ++guard) {
            --cnt[maxbits];
            for (int l = maxbits - 1; l > 0; --l) if (cnt[l]) { --cnt[l]; cnt[l + 1] += 2; break; }
            --total;
        }
        // the most frequent symbols take the shortest codes
        int j = n;
        for (int l = 1; l <= maxbits; ++l) for (uint32_t k = cnt[l]; k > 0 && j > 0; --k) { const int s = W->order[--j]; if (s < nsym) len[s] = (uint8_t)l; }
        uint32_t c = 0;
        W->first[0] = 0;
        for (int l = 1; l < 16; ++l) { c = (c + (l - 1 <= maxbits && l > 1 ? cnt[l - 1] : 0u)) << 1; W->first[l] = c; }
    }
    L::sync();
    // canonical codes: first code of the length + the number of symbols of that length before this one
    for (int i = lane; i < nsym; i += nl) {
        const int l = len[i] & 15;
        uint32_t r = 0;
        if (l) for (int j = 0; j < i; ++j) r += (len[j] == l) ? 1u : 0u;
        code[i] = l ? (uint16_t)ccsx_defl_rev(W->first[l] + r, l) : (uint16_t)0;
    }
    L::sync();
}

static inline CCSX_DEFL_HD int32_t ccsx_defl_stored_len(int32_t n) { return n <= 0 ? 5 : n + 5 * ((n + 65534) / 65535); }

// The stored form of in[0, n) into out (out_cap >= ccsx_defl_stored_len(n): checked by the caller)
template <class L>
static inline CCSX_DEFL_HD void ccsx_defl_stored(const uint8_t *in, int32_t n, uint8_t *out)
{
    const int lane = L::lane(), nl = L::nlanes();
    const int32_t nb = n <= 0 ? 1 : (n + 65534) / 65535;
    for (int32_t b = 0; b < nb && b < 2; ++b) {
        const int32_t from = b * 65535, m = (n - from < 65535 ? n - from : 65535);
        uint8_t *o = out + (int64_t)b * 65540;
        if (lane == 0) {
            o[0] = (uint8_t)(b == nb - 1 ? 1 : 0);
            o[1] = (uint8_t)(m & 255); o[2] = (uint8_t)(m >> 8); o[3] = (uint8_t)(~m & 255); o[4] = (uint8_t)((~m >> 8) & 255);
        }
        for (int32_t i = lane; i < m; i += nl) o[5 + i] = in[from + i];
    }
}

// Encode in[0, n) into out[0, out_cap).  All lanes of the group call it with the same arguments; *out_len, *crc and the returned status are the same on every lane.
template <class L>
static inline CCSX_DEFL_HD int ccsx_defl_span(const uint8_t *in, int32_t n, uint8_t *out, int32_t out_cap, ccsx_defl_work *W, int32_t *out_len, uint32_t *crc)
{
    const int lane = L::lane(), nl = L::nlanes();
    *out_len = 0; *crc = 0;
    if (n < 0 || n > CCSX_DEFL_MAX_IN || out_cap < 0 || nl > CCSX_DEFL_MAX_LANES) return CCSX_DEFLATE_OUTPUT_FULL;
    *crc = ccsx_defl_crc<L>(in, (uint32_t)n, &W->scal[CCSX_DEFL_S_CRC]);
    const int32_t stored_len = ccsx_defl_stored_len(n);
    bool coded = n > 0, fits = true;
    int32_t out_pos = 0;                                         // whole coded bytes so far
    uint32_t carry = 0, carry_byte = 0;                          // the bits (< 8) of the coded stream's last, partial byte
    int32_t pos = 0;                                             // where the next token starts
    for (int i = lane; i < CCSX_DEFL_HASH_SIZE; i += nl) W->head[i] = 0;
    L::sync();
    for (int32_t base = 0; coded && base < n && pos < n; base += CCSX_DEFL_SUB) {   // (a match of the last block may cover what is left of the span)
        const int32_t end = base + CCSX_DEFL_SUB < n ? base + CCSX_DEFL_SUB : n;
        // the best match of every position, chunk by chunk
        for (int32_t c0 = base; c0 < end; c0 += CCSX_DEFL_CHUNK) {
            const int32_t cend = c0 + CCSX_DEFL_CHUNK < end ? c0 + CCSX_DEFL_CHUNK : end;
            for (int32_t p = c0 + lane; p < cend; p += nl) {
                const uint32_t maxl = (uint32_t)(n - p < CCSX_DEFL_MAX_MATCH ? n - p : CCSX_DEFL_MAX_MATCH);
                uint32_t blen = 0, bdist = 0;
                if (maxl >= CCSX_DEFL_MIN_MATCH) {
                    const uint32_t q1 = W->head[ccsx_defl_hash(in + p) & (CCSX_DEFL_HASH_SIZE - 1)];
                    if (q1 && q1 <= (uint32_t)p && (uint32_t)p - (q1 - 1u) <= CCSX_DEFL_MAX_DIST) {
                        const uint32_t l = ccsx_defl_match_len(in + (q1 - 1u), in + p, maxl);
                        if (l >= CCSX_DEFL_MIN_MATCH) { blen = l; bdist = (uint32_t)p - (q1 - 1u); }
                    }
                    if (p >= 1) {
                        const uint32_t l = ccsx_defl_match_len(in + p - 1, in + p, maxl);
                        if (l >= CCSX_DEFL_MIN_MATCH && l >= blen) { blen = l; bdist = 1; }
                    }
                }
                W->match[(p - base) & (CCSX_DEFL_SUB - 1)] = blen ? (blen << 16) | (bdist - 1u) : 0u;
            }
            L::sync();                                           // the chunk's look-ups saw earlier chunks only
            for (int32_t p = c0 + lane; p < cend; p += nl)
                if (n - p >= CCSX_DEFL_MIN_MATCH) L::atomic_max(&W->head[ccsx_defl_hash(in + p) & (CCSX_DEFL_HASH_SIZE - 1)], (uint32_t)p + 1u);
            L::sync();
        }
        // the greedy parse: the one sequential chain
        for (int i = lane; i < CCSX_DEFL_NSYM; i += nl) W->freq[i] = 0;
        if (lane == 0) {
            int32_t p = pos < base ? base : pos;
            while (p < end) {
                const uint32_t m = W->match[(p - base) & (CCSX_DEFL_SUB - 1)], l = (m >> 16) & 511u;
                W->match[(p - base) & (CCSX_DEFL_SUB - 1)] = m | CCSX_DEFL_TOKEN;
                p += l ? (int32_t)l : 1;
            }
            W->scal[CCSX_DEFL_S_POS] = (uint32_t)p;
        }
        L::sync();
        pos = (int32_t)W->scal[CCSX_DEFL_S_POS];
        const bool final_block = pos >= n;
        // counts
        for (int32_t p = base + lane; p < end; p += nl) {
            const uint32_t m = W->match[p - base];
            if (!(m & CCSX_DEFL_TOKEN)) continue;
            const uint32_t l = (m >> 16) & 511u;
            if (!l) { L::atomic_add(&W->freq[in[p]], 1u); continue; }
            uint32_t s, eb, ev;
            ccsx_defl_len_sym(l, &s, &eb, &ev);
            L::atomic_add(&W->freq[s < CCSX_DEFL_NLIT ? s : 285u], 1u);
            ccsx_defl_dist_sym(m & 0xffffu, &s, &eb, &ev);
            L::atomic_add(&W->freq[CCSX_DEFL_DIST0 + (s < CCSX_DEFL_NDIST ? s : 29u)], 1u);
        }
        if (lane == 0) W->freq[256] = 1;                         // (no other lane touches the end-of-block count)
        L::sync();
        ccsx_defl_build<L>(W, 0, CCSX_DEFL_NLIT, 15);
        ccsx_defl_build<L>(W, CCSX_DEFL_DIST0, CCSX_DEFL_NDIST, 15);
        // the header's code-length sequence
        if (lane == 0) {
            int hlit = CCSX_DEFL_NLIT, hdist = CCSX_DEFL_NDIST;
            while (hlit > 257 && !W->len[hlit - 1]) --hlit;
            while (hdist > 1 && !W->len[CCSX_DEFL_DIST0 + hdist - 1]) --hdist;
            const int T = hlit + hdist;
            int nops = 0, t = 0;
#define CCSX_DEFL_SEQ(k) (W->len[(k) < hlit ? (k) : CCSX_DEFL_DIST0 + (k) - hlit])
#define CCSX_DEFL_OP(s, x) do { if (nops < CCSX_DEFL_NLIT + CCSX_DEFL_NDIST + 4) W->ops[nops++] = (uint16_t)((s) | ((x) << 8)); ++W->freq[CCSX_DEFL_PRE0 + (s)]; } while (0)
            while (t < T) {
                const int v = CCSX_DEFL_SEQ(t) & 15;
                int run = 1;
                while (t + run < T && (CCSX_DEFL_SEQ(t + run) & 15) == v) ++run;
                t += run;
                if (v == 0) {
                    while (run >= 11) { const int k = run < 138 ? run : 138; CCSX_DEFL_OP(18, k - 11); run -= k; }
                    if (run >= 3) { CCSX_DEFL_OP(17, run - 3); run = 0; }
                    while (run > 0) { CCSX_DEFL_OP(0, 0); --run; }
                } else {
                    CCSX_DEFL_OP(v, 0); --run;
                    while (run >= 3) { const int k = run < 6 ? run : 6; CCSX_DEFL_OP(16, k - 3); run -= k; }
                    while (run > 0) { CCSX_DEFL_OP(v, 0); --run; }
                }
            }
#undef CCSX_DEFL_SEQ
#undef CCSX_DEFL_OP
            W->scal[CCSX_DEFL_S_HLIT] = (uint32_t)hlit; W->scal[CCSX_DEFL_S_HDIST] = (uint32_t)hdist; W->scal[CCSX_DEFL_S_NOPS] = (uint32_t)nops;
        }
        L::sync();
        ccsx_defl_build<L>(W, CCSX_DEFL_PRE0, CCSX_DEFL_NPRE, 7);
        // the order of RFC 1951 §3.2.7: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, five bits each in two words
        const uint64_t ord_lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
        const uint64_t ord_hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
        if (lane == 0) {
            int hclen = 19;
            while (hclen > 4) {
                const int k = hclen - 1;
                const uint32_t s = (uint32_t)((k < 12 ? ord_lo >> (5 * k) : ord_hi >> (5 * (k - 12))) & 31u);
                if (W->len[CCSX_DEFL_PRE0 + (s < 19u ? s : 0u)]) break;
                --hclen;
            }
            uint32_t hdr = 3 + 5 + 5 + 4 + 3 * (uint32_t)hclen;
            const uint32_t nops = W->scal[CCSX_DEFL_S_NOPS];
            for (uint32_t k = 0; k < nops && k < (uint32_t)(CCSX_DEFL_NLIT + CCSX_DEFL_NDIST + 4); ++k) {
                const uint32_t s = W->ops[k] & 31u;
                hdr += W->len[CCSX_DEFL_PRE0 + (s < 19u ? s : 0u)] + (s == 16u ? 2u : s == 17u ? 3u : s == 18u ? 7u : 0u);
            }
            W->scal[CCSX_DEFL_S_HCLEN] = (uint32_t)hclen; W->scal[CCSX_DEFL_S_HDR] = hdr;
        }
        // the bits of every lane's slice of positions
        const int32_t per = (end - base + nl - 1) / nl;
        const int32_t s0 = base + lane * per < end ? base + lane * per : end, s1 = s0 + per < end ? s0 + per : end;
        {
            uint32_t sum = 0;
            for (int32_t p = s0; p < s1; ++p) {
                const uint32_t m = W->match[p - base];
                uint64_t b;
                if (m & CCSX_DEFL_TOKEN) sum += ccsx_defl_token(W, m, in[p], &b);
            }
            W->part[lane] = sum;
        }
        L::sync();
        uint32_t before = 0, tokens = 0;
        for (int j = 0; j < nl; ++j) { const uint32_t v = W->part[j]; tokens += v; if (j < lane) before += v; }
        const uint32_t hdr = W->scal[CCSX_DEFL_S_HDR];
        const uint32_t block_bits = hdr + tokens + W->len[256];
        if (carry + block_bits > CCSX_DEFL_STAGE_BYTES * 8u - 64u) { coded = false; break; }
        const uint32_t all_bits = carry + block_bits, all_words = (all_bits + 31u) / 32u + 2u;
        L::sync();                                               // (every lane has read part[] and scal[] of this sub-block)
        for (uint32_t i = (uint32_t)lane; i < all_words && i < CCSX_DEFL_STAGE_WORDS; i += (uint32_t)nl) W->stage[i] = i ? 0u : carry_byte;
        L::sync();
        if (lane == 0) {                                         // the header
            uint32_t at = carry;
            const uint32_t hlit = W->scal[CCSX_DEFL_S_HLIT], hdist = W->scal[CCSX_DEFL_S_HDIST], hclen = W->scal[CCSX_DEFL_S_HCLEN], nops = W->scal[CCSX_DEFL_S_NOPS];
            ccsx_defl_put<L>(W->stage, at, (final_block ? 1u : 0u) | 2u << 1 | (hlit - 257u) << 3 | (hdist - 1u) << 8 | (hclen - 4u) << 13, 17); at += 17;
            for (uint32_t k = 0; k < hclen && k < 19u; ++k) {
                const uint32_t s = (uint32_t)((k < 12u ? ord_lo >> (5 * k) : ord_hi >> (5 * (k - 12u))) & 31u);
                ccsx_defl_put<L>(W->stage, at, W->len[CCSX_DEFL_PRE0 + (s < 19u ? s : 0u)], 3); at += 3;
            }
            for (uint32_t k = 0; k < nops && k < (uint32_t)(CCSX_DEFL_NLIT + CCSX_DEFL_NDIST + 4); ++k) {
                const uint32_t s = W->ops[k] & 31u, x = (uint32_t)W->ops[k] >> 8, sl = W->len[CCSX_DEFL_PRE0 + (s < 19u ? s : 0u)];
                const uint32_t xb = s == 16u ? 2u : s == 17u ? 3u : s == 18u ? 7u : 0u;
                ccsx_defl_put<L>(W->stage, at, (uint64_t)W->code[CCSX_DEFL_PRE0 + (s < 19u ? s : 0u)] | (uint64_t)x << sl, sl + xb); at += sl + xb;
            }
            ccsx_defl_put<L>(W->stage, carry + hdr + tokens, W->code[256], W->len[256]);   // end of block
        }
        {
            uint32_t at = carry + hdr + before;
            for (int32_t p = s0; p < s1; ++p) {
                const uint32_t m = W->match[p - base];
                if (!(m & CCSX_DEFL_TOKEN)) continue;
                uint64_t b;
                const uint32_t nb = ccsx_defl_token(W, m, in[p], &b);
                ccsx_defl_put<L>(W->stage, at, b, nb);
                at += nb;
            }
        }
        L::sync();
        // whole bytes go out; the last, partial byte is carried into the next sub-block
        const uint32_t whole = final_block ? (all_bits + 7u) >> 3 : all_bits >> 3;
        const uint8_t *sb = (const uint8_t *)W->stage;
        carry = final_block ? 0u : all_bits & 7u;
        carry_byte = (whole < CCSX_DEFL_STAGE_BYTES && carry) ? sb[whole] : 0u;
        if ((int64_t)out_pos + whole >= (int64_t)stored_len) { coded = false; break; }          // not smaller than the stored form
        if (fits && (int64_t)out_pos + whole <= (int64_t)out_cap) { for (uint32_t i = (uint32_t)lane; i < whole; i += (uint32_t)nl) out[out_pos + i] = sb[i]; }
        else fits = false;
        out_pos += (int32_t)whole;
        L::sync();                                               // (the staging area and match[] are free again)
    }
    L::sync();
    if (coded) {
        if (!fits) return CCSX_DEFLATE_OUTPUT_FULL;
        *out_len = out_pos;
        return CCSX_DEFLATE_OK;
    }
    if (stored_len > out_cap) return CCSX_DEFLATE_OUTPUT_FULL;
    ccsx_defl_stored<L>(in, n, out);
    *out_len = stored_len;
    return CCSX_DEFLATE_OK;
}

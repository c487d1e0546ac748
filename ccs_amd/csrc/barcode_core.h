// barcode_core.h — the barcode rule for the host and the device (DESIGN.md §2 "Barcode calls"): Myers' bit-vector column update (also k_adapter's), the match
// masks of a pattern, one walk over a window, and the call.  ccsx_barcode_reads_host (ccsx_barcode_api.cpp) and k_barcode (ccsx_barcode.hip) are built from
// these and from nothing else of the rule.  Integers only.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "ccsx.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CCSX_BC_HD __host__ __device__ __forceinline__
#else
#define CCSX_BC_HD inline
#endif

// One column of the edit-distance table of a pattern of m <= 64 symbols against a text, as vertical differences: bit i of Pv / Mv = row i + 1 is one more / one
// less than row i; score = the last row, with top = 1ull << (m - 1).  Start: {~0ull, 0ull, m}.  Bits above m - 1 never reach the bits below them (carries and
// shifts go upwards), so the words need no masking and m = 64 is not special.
struct MyersCol { unsigned long long Pv, Mv; int score; };

// the column after one more text symbol whose match mask is Eq.  anchored 0: row 0 is 0 everywhere, a match may start at any text position; 1: row 0 charges the
// start, its horizontal difference is +1
CCSX_BC_HD void myers_step(MyersCol &c, unsigned long long Eq, unsigned long long top, unsigned long long anchored)
{
    const unsigned long long Xv = Eq | c.Mv;
    const unsigned long long Xh = (((Eq & c.Pv) + c.Pv) ^ c.Pv) | Eq;
    unsigned long long Ph = c.Mv | ~(Xh | c.Pv);
    unsigned long long Mh = c.Pv & Xh;
    c.score += (Ph & top) ? 1 : 0;
    c.score -= (Mh & top) ? 1 : 0;
    Ph = (Ph << 1) | anchored;                                      // (anchored: row 0 of the table charges the start, its horizontal difference is +1)
    Mh <<= 1;
    c.Pv = Mh | ~(Xv | Ph);
    c.Mv = Ph & Xv;
}

// the four match masks of a barcode: bit i of eq[code] = (codes[i] == code)
struct BarcodeMasks { unsigned long long eq[4]; };
CCSX_BC_HD BarcodeMasks ccsx_bc_masks(const uint8_t *codes, int m)
{
    BarcodeMasks k{{0ull, 0ull, 0ull, 0ull}};
    for (int i = 0; i < m; ++i) k.eq[codes[i] & 3] |= 1ull << i;
    return k;
}

// dist = min over 0 <= j <= W of E[j], E[j] the smallest edit distance between the whole barcode and any s[i..j); clip = the smallest such j (E[0] = m).
// base(j) is s[j], a code 0 .. 3.  The masks are passed as four words so that they stay in registers on the device.
struct BarcodeHit { int dist, clip; };
template <typename F>
CCSX_BC_HD BarcodeHit ccsx_bc_walk(unsigned long long e0, unsigned long long e1, unsigned long long e2, unsigned long long e3, int m, int W, F base)
{
    const unsigned long long top = 1ull << (m - 1);
    MyersCol c{~0ull, 0ull, m};
    BarcodeHit h{m, 0};
    for (int j = 0; j < W; ++j) {
        const int b = base(j);
        myers_step(c, b == 0 ? e0 : b == 1 ? e1 : b == 2 ? e2 : e3, top, 0ull);
        if (c.score < h.dist) { h.dist = c.score; h.clip = j + 1; }
    }
    return h;
}

// the bases of the two ends of a read c[0, L): end 0 reads c forwards, end 1 its reverse complement
CCSX_BC_HD int ccsx_bc_base(const uint8_t *c, int L, int end, int j) { return end ? 3 - (c[L - 1 - j] & 3) : (c[j] & 3); }

// an end's order key: smallest distance first, then smallest barcode (dist <= 64, b < 384)
CCSX_BC_HD int ccsx_bc_key(int dist, int b) { return (dist << 16) | b; }

// the call of one end from its best barcode's distance and length and the runner-up's distance
CCSX_BC_HD int ccsx_bc_called(int dist, int second, int m, const ccsx_barcode_opts &o)
{
    return dist <= m * o.max_dist_pct / 100 && second - dist >= o.min_margin;
}

// call and bq of a read from its two ends (m[e]: the length of barcode idx[e])
CCSX_BC_HD void ccsx_bc_read_call(const int dist[2], const int second[2], const int m[2], const ccsx_barcode_opts &o, int *call, int *bq)
{
    int c = 0, q = -1;
    for (int e = 0; e < 2; ++e) {
        if (!ccsx_bc_called(dist[e], second[e], m[e], o)) continue;
        const int qe = 100 * (m[e] - dist[e]) / m[e];
        c |= 1 << e;
        q = q < 0 || qe < q ? qe : q;
    }
    *call = c; *bq = q;
}

// the report of n reads as [CCSX_BC_PLANES][n] int32 on the device: tested, call, bq, then idx, dist, second and clip as [n][2] each
#define CCSX_BC_PLANES 11
struct BarcodeOut { int32_t *tested, *call, *bq, *idx, *dist, *second, *clip; };
CCSX_BC_HD BarcodeOut ccsx_bc_out(int32_t *rep, size_t n)
{
    return {rep, rep + n, rep + 2 * n, rep + 3 * n, rep + 5 * n, rep + 7 * n, rep + 9 * n};
}
CCSX_BC_HD void ccsx_bc_put_untested(const BarcodeOut &r, int z)
{
    r.tested[z] = 0; r.call[z] = 0; r.bq[z] = -1;
    for (int e = 0; e < 2; ++e) { r.idx[2 * z + e] = -1; r.dist[2 * z + e] = 255; r.second[2 * z + e] = 255; r.clip[2 * z + e] = 0; }
}

// what k_barcode is given (ccsx_barcode.hip).  masks / len: built once per request by the host (ccsx_bc_masks), 12 KB + 384 bytes for a full set
struct BarcodeParams {
    int32_t n, n_barcodes;
    ccsx_barcode_opts opts;
    const uint8_t *seq;                  // read z: seq_len[z] codes at seq + seq_off[z]
    const int64_t *seq_off;
    const int32_t *seq_len;
    const unsigned long long *masks;     // [n_barcodes][4]
    const uint8_t *len;                  // [n_barcodes]
    int32_t *rep;                        // [CCSX_BC_PLANES][n]; NULL: no request
};
#define CCSX_BARCODE_THREADS 256

// ---- the set and the report in memory, for the host (the one definition: the library, the bench and the sanitize programs).  A packed set is the masks, then one
// length byte per barcode, in whole 64-bit words; in one buffer the report of the reads stands behind it.
CCSX_BC_HD size_t ccsx_bc_set_words(int nb) { return (size_t)nb * 4 + ((size_t)nb + 7) / 8; }
CCSX_BC_HD size_t ccsx_bc_rep_bytes(size_t n) { return n * CCSX_BC_PLANES * 4; }
// masks, len and rep of B for the packed set of B.n_barcodes at `base`, device or host memory (rep: where the report would follow)
CCSX_BC_HD void ccsx_bc_bind(BarcodeParams &B, const void *base)
{
    B.masks = (const unsigned long long *)base;
    B.len = (const uint8_t *)(B.masks + (size_t)B.n_barcodes * 4);
    B.rep = (int32_t *)(B.masks + ccsx_bc_set_words(B.n_barcodes));
}
// a checked set, packed into ccsx_bc_set_words(n_barcodes) zeroed words
inline void ccsx_bc_pack(const ccsx_barcode_set *set, unsigned long long *packed)
{
    BarcodeParams B{};
    B.n_barcodes = set->n_barcodes;
    ccsx_bc_bind(B, packed);
    uint8_t *len = const_cast<uint8_t *>(B.len);
    for (int b = 0; b < set->n_barcodes; ++b) {
        const BarcodeMasks k = ccsx_bc_masks(set->seq[b], set->len[b]);
        for (int c = 0; c < 4; ++c) packed[4 * b + c] = k.eq[c];
        len[b] = (uint8_t)set->len[b];
    }
}
// a caller's report as the rule writes it
inline BarcodeOut ccsx_bc_out(const ccsx_barcode_report &r) { return {r.tested, r.call, r.bq, r.idx, r.dist, r.second, r.clip}; }

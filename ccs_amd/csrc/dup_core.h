// dup_core.h — the duplicate rule for the host and the device (DESIGN.md §2 "Duplicate rule"): the hash, the minimizer, the signature, the distance D of two end
// windows, the pair predicate, the key, and the layouts.  ccsx_dup_sign_reads_host / ccsx_dup_cluster_host (ccsx_dup_api.cpp) and the k_dup_* kernels
// (ccsx_dup.hip) are built from these and from nothing else of the rule.  myers_step and ccsx_bc_base are barcode_core.h's.  Integers only.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "ccsx.h"
#include "barcode_core.h"

#define CCSX_DUP_HD CCSX_BC_HD

// ---- the hash: murmur3's 32-bit finaliser.  Every step (xor with a right shift, multiplication by an odd constant) is invertible, so h is a bijection of 32-bit
// words: equal minimizers are the same k-mer
#define CCSX_DUP_HASH_M1 0x85ebca6bu
#define CCSX_DUP_HASH_M2 0xc2b2ae35u
#define CCSX_DUP_HASH_S1 16
#define CCSX_DUP_HASH_S2 13
#define CCSX_DUP_HASH_S3 16
CCSX_DUP_HD uint32_t ccsx_dup_hash32(uint32_t x)
{
    x ^= x >> CCSX_DUP_HASH_S1; x *= CCSX_DUP_HASH_M1;
    x ^= x >> CCSX_DUP_HASH_S2; x *= CCSX_DUP_HASH_M2;
    x ^= x >> CCSX_DUP_HASH_S3;
    return x;
}

// ---- a window of W <= 64 bases at 2 bits a base in two words: base j = bits 2 (j % 32) of word j / 32
struct DupWin { unsigned long long w0, w1; };                  // (named words, as the masks below: no indexed member, so that they stay in registers on the device)
template <typename F> CCSX_DUP_HD DupWin ccsx_dup_pack(int W, F base)
{
    DupWin a{0ull, 0ull};
    for (int j = 0; j < W; ++j) (j < 32 ? a.w0 : a.w1) |= (unsigned long long)(base(j) & 3) << (2 * (j & 31));
    return a;
}
// the even bits of x, squeezed into the low 32 bits; and back: bit i of x to bit 2 i
CCSX_DUP_HD unsigned long long ccsx_dup_squeeze(unsigned long long x)
{
    x &= 0x5555555555555555ull;
    x = (x | (x >> 1)) & 0x3333333333333333ull;
    x = (x | (x >> 2)) & 0x0f0f0f0f0f0f0f0full;
    x = (x | (x >> 4)) & 0x00ff00ff00ff00ffull;
    x = (x | (x >> 8)) & 0x0000ffff0000ffffull;
    x = (x | (x >> 16)) & 0x00000000ffffffffull;
    return x;
}
CCSX_DUP_HD unsigned long long ccsx_dup_spread(unsigned long long x)
{
    x &= 0x00000000ffffffffull;
    x = (x | (x << 16)) & 0x0000ffff0000ffffull;
    x = (x | (x << 8)) & 0x00ff00ff00ff00ffull;
    x = (x | (x << 4)) & 0x0f0f0f0f0f0f0f0full;
    x = (x | (x << 2)) & 0x3333333333333333ull;
    x = (x | (x << 1)) & 0x5555555555555555ull;
    return x;
}
// the window from the low bits lo and the high bits hi of its bases (bit j: base j), the form a wave's ballots give
CCSX_DUP_HD DupWin ccsx_dup_win_of_bits(unsigned long long lo, unsigned long long hi)
{
    return {ccsx_dup_spread(lo) | (ccsx_dup_spread(hi) << 1), ccsx_dup_spread(lo >> 32) | (ccsx_dup_spread(hi >> 32) << 1)};
}
// a window as the pattern of a walk: the low and the high bits of its W bases (bit i: base i).  The match mask of a text base b is where both bits agree with
// b's, made by arithmetic: no table, no select, nothing for a compiler to spill
struct DupMasks { unsigned long long lo, hi; };
CCSX_DUP_HD DupMasks ccsx_dup_masks(const DupWin &a)
{
    return {ccsx_dup_squeeze(a.w0) | (ccsx_dup_squeeze(a.w1) << 32), ccsx_dup_squeeze(a.w0 >> 1) | (ccsx_dup_squeeze(a.w1 >> 1) << 32)};
}
CCSX_DUP_HD unsigned long long ccsx_dup_eq(const DupMasks &p, int b)   // (bits past the pattern's last are set or not: they never reach the bits below, barcode_core.h)
{
    return ~((p.lo ^ (0ull - (unsigned long long)(b & 1))) | (p.hi ^ (0ull - (unsigned long long)((b >> 1) & 1))));
}

// ---- the minimizer: the k-mer at j, its first base most significant; and the smallest hash over the W - k + 1 k-mers of a window
// (the 2 k bits at base j of the 128-bit window hold the k-mer with its first base least significant: the 2-bit groups of a word are reversed)
CCSX_DUP_HD uint32_t ccsx_dup_rev_bases(uint32_t x)
{
    x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
    x = ((x >> 4) & 0x0f0f0f0fu) | ((x & 0x0f0f0f0fu) << 4);
    return (x >> 24) | ((x >> 8) & 0x0000ff00u) | ((x << 8) & 0x00ff0000u) | (x << 24);
}
CCSX_DUP_HD uint32_t ccsx_dup_kmer(const DupWin &a, int j, int k)
{
    const int s = 2 * j;
    const unsigned long long v = s >= 64 ? a.w1 >> (s - 64) : s ? (a.w0 >> s) | (a.w1 << (64 - s)) : a.w0;
    return ccsx_dup_rev_bases((uint32_t)v) >> (32 - 2 * k);
}
CCSX_DUP_HD uint32_t ccsx_dup_minimizer(const DupWin &a, int W, int k)
{
    uint32_t m = 0xffffffffu;
    for (int j = 0; j + k <= W; ++j) { const uint32_t h = ccsx_dup_hash32(ccsx_dup_kmer(a, j, k)); m = h < m ? h : m; }
    return m;
}

// ---- the signature.  Untested: window 0 and everything else but len 0
CCSX_DUP_HD ccsx_dup_sig ccsx_dup_sig_untested(int L) { return {{{0ull, 0ull}, {0ull, 0ull}}, {0u, 0u}, L > 0 ? L : 0, 0}; }
CCSX_DUP_HD ccsx_dup_sig ccsx_dup_sig_of(const DupWin &e0, const DupWin &e1, uint32_t m0, uint32_t m1, int L, int W)
{
    return {{{e0.w0, e0.w1}, {e1.w0, e1.w1}}, {m0, m1}, L, W};
}
// of a read c[0, L) on one thread
CCSX_DUP_HD ccsx_dup_sig ccsx_dup_sign(const uint8_t *c, int L, const ccsx_dup_opts &o)
{
    const int W = o.window;
    if (L < W) return ccsx_dup_sig_untested(L);
    const DupWin e0 = ccsx_dup_pack(W, [&](int j) { return ccsx_bc_base(c, L, 0, j); }), e1 = ccsx_dup_pack(W, [&](int j) { return ccsx_bc_base(c, L, 1, j); });
    return ccsx_dup_sig_of(e0, e1, ccsx_dup_minimizer(e0, W, o.kmer), ccsx_dup_minimizer(e1, W, o.kmer), L, W);
}

// ---- the key of a signature.  A tested read: (min, max) of its two minimizers, min in the high word.  An untested read: a word no tested read has (its high
// half is above its low half), so that a sort by key never puts an untested read into a tested bucket
#define CCSX_DUP_KEY_UNTESTED 0xffffffff00000000ull
CCSX_DUP_HD unsigned long long ccsx_dup_key(const ccsx_dup_sig &s)
{
    if (!s.window) return CCSX_DUP_KEY_UNTESTED;
    const uint32_t lo = s.mini[0] < s.mini[1] ? s.mini[0] : s.mini[1], hi = s.mini[0] < s.mini[1] ? s.mini[1] : s.mini[0];
    return ((unsigned long long)lo << 32) | hi;
}

// ---- D(a, b) = min(min_q ed(a, b[0, q)), min_p ed(a[0, p), b)), 0 <= p, q <= W: the last row and the last column of the start-anchored table, two walks of
// W anchored steps.  The walk of pattern a along text b passes ed(a, b[0, q)) for q = 1 .. W; q = 0 is W
CCSX_DUP_HD void ccsx_dup_walk_word(const DupMasks &pat, unsigned long long text, int steps, unsigned long long top, MyersCol &c, int &best)
{
    for (int j = 0; j < steps; ++j, text >>= 2) {
        myers_step(c, ccsx_dup_eq(pat, (int)(text & 3)), top, 1ull);
        best = c.score < best ? c.score : best;
    }
}
CCSX_DUP_HD int ccsx_dup_walk(const DupMasks &pat, const DupWin &text, int W)
{
    const unsigned long long top = 1ull << (W - 1);
    MyersCol c{~0ull, 0ull, W};
    int best = W;
    ccsx_dup_walk_word(pat, text.w0, W < 32 ? W : 32, top, c, best);
    ccsx_dup_walk_word(pat, text.w1, W - 32, top, c, best);
    return best;
}
CCSX_DUP_HD int ccsx_dup_dist(const DupWin &a, const DupMasks &ma, const DupWin &b, const DupMasks &mb, int W)
{
    const int r = ccsx_dup_walk(ma, b, W), c = ccsx_dup_walk(mb, a, W);
    return r < c ? r : c;
}

// ---- the pair predicate, for two reads of one bucket.  A read as the predicate sees it: its two windows with their masks, its length and its group
struct DupEnds { DupWin e0, e1; DupMasks m0, m1; };
template <typename U> CCSX_DUP_HD DupEnds ccsx_dup_ends(const U *end /* [2][2] 64-bit words */)
{
    const DupWin e0{(unsigned long long)end[0], (unsigned long long)end[1]}, e1{(unsigned long long)end[2], (unsigned long long)end[3]};
    return {e0, e1, ccsx_dup_masks(e0), ccsx_dup_masks(e1)};
}
CCSX_DUP_HD int ccsx_dup_kmax(const ccsx_dup_opts &o) { return o.window * o.max_dist_pct / 100; }
// the group and the length clause: what is asked before any walk
CCSX_DUP_HD bool ccsx_dup_may_pair(int Li, int gi, int Lj, int gj, const ccsx_dup_opts &o)
{
    if (gi != gj) return false;
    const long long d = Li < Lj ? (long long)Lj - Li : (long long)Li - Lj, m = Li < Lj ? Li : Lj;
    return d * 100 <= (long long)o.max_len_diff_pct * m;
}
// the distance clause: same strand first; the opposite strands only when that fails (up to 8 walks)
CCSX_DUP_HD bool ccsx_dup_ends_agree(const DupEnds &a, const DupEnds &b, const ccsx_dup_opts &o)
{
    const int W = o.window, kmax = ccsx_dup_kmax(o);
    if (ccsx_dup_dist(a.e0, a.m0, b.e0, b.m0, W) <= kmax && ccsx_dup_dist(a.e1, a.m1, b.e1, b.m1, W) <= kmax) return true;
    return ccsx_dup_dist(a.e0, a.m0, b.e1, b.m1, W) <= kmax && ccsx_dup_dist(a.e1, a.m1, b.e0, b.m0, W) <= kmax;
}

// ---- the report of n reads as [CCSX_DUP_PLANES][n] int32 on the device: status, rep, set_size, dup
#define CCSX_DUP_PLANES 4
struct DupOut { int32_t *status, *rep, *set_size, *dup; };
CCSX_DUP_HD DupOut ccsx_dup_out(int32_t *rep, size_t n) { return {rep, rep + n, rep + 2 * n, rep + 3 * n}; }
inline DupOut ccsx_dup_out(const ccsx_dup_report &r) { return {r.status, r.rep, r.set_size, r.dup}; }
// a read that stands alone: untested, overflowed, or a tested singleton
CCSX_DUP_HD void ccsx_dup_put_alone(const DupOut &r, int z, int status) { r.status[z] = status; r.rep[z] = z; r.set_size[z] = 1; r.dup[z] = 0; }

// ---- what the kernels are given (ccsx_dup.hip)
struct DupSignParams {
    int32_t n;
    ccsx_dup_opts opts;
    const uint8_t *seq;                  // read z: seq_len[z] codes at seq + seq_off[z]
    const int64_t *seq_off;
    const int32_t *seq_len;
    ccsx_dup_sig *sig;                   // [n], 16-byte aligned
};
struct DupClusterParams {
    int32_t n;
    ccsx_dup_opts opts;
    const ccsx_dup_sig *sig;             // [n]
    const int32_t *group, *score;        // [n] each; NULL: all 0
    unsigned long long *key[2];          // [n] each: the keys in read order, and sorted
    uint32_t *idx[2];                    // [n] each: 0 .. n - 1, and the reads in key order (equal keys in index order)
    void *sort_tmp; size_t sort_tmp_bytes;   // the sort's scratch, ccsx_dup_sort_bytes(n)
    int32_t *list;                       // [1 + n / 2]: the count, then the first sorted position of every bucket of 2 or more
    int32_t *rep;                        // [CCSX_DUP_PLANES][n]
};
#define CCSX_DUP_SIGN_THREADS 256        // four reads a workgroup, one wave each
#define CCSX_DUP_VERIFY_THREADS 256

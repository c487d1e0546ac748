// segment_core.h — the segment rule for the host and the device (DESIGN.md §2 "Segment rule"): the match masks of a search, the hit walk over a chunk of a read,
// the anchored start walk, the order key, the overlap test, the selection, the classification of a piece, the summary and the report's layout.
// ccsx_segment_reads_host (ccsx_segment_api.cpp) and k_segment (ccsx_segment.hip) are built from these and from nothing else of the rule.  Integers only.
// (MyersCol / myers_step: barcode_core.h, shared with k_barcode and k_adapter)
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "ccsx.h"
#include "barcode_core.h"

#define CCSX_SG_HD CCSX_BC_HD
#define CCSX_SEGMENT_CHUNK   256          // read bases of one item of k_segment
#define CCSX_SEGMENT_THREADS 256
#define CCSX_SG_PLANES       8            // tested, overflow, n_hits, n_cuts, n_segments, complete, orient, leftover_bases
#define CCSX_SG_MASK_WORDS   8            // per search: eq[4] of the pattern, then eq[4] of the reversed pattern

// the masks of search s = 2a + rc of adapter a (codes[0, m)): rc 0 the adapter as given, 1 its reverse complement.  w[code]: bit i = (p[i] == code);
// w[4 + code]: the same of the pattern reversed, for the anchored start walk
CCSX_SG_HD void ccsx_sg_masks(const uint8_t *codes, int m, int rc, unsigned long long *w)
{
    for (int c = 0; c < CCSX_SG_MASK_WORDS; ++c) w[c] = 0ull;
    for (int i = 0; i < m; ++i) {
        const int b = rc ? 3 - (codes[m - 1 - i] & 3) : (codes[i] & 3);
        w[b] |= 1ull << i;
        w[4 + b] |= 1ull << (m - 1 - i);
    }
}

// the edits an adapter of m bases may have
CCSX_SG_HD int ccsx_sg_k(int m, int max_dist_pct) { return m * max_dist_pct / 100; }

// The hits of one search that a chunk (lo, hi] of a read c[0, L) owns: hit(end, dist) for every maximal run of ends j with E[j] <= k whose FIRST end lies in
// (lo, hi]; end is the first j of the run that attains the run's minimum dist.  The walk starts m + k bases before the chunk from the all-ones column: after that
// warm-up every value <= k is exact and so is the predicate E <= k (a fresh start can only over-estimate, and a match of distance <= k spans at most m + k bases:
// k_adapter's argument), and it follows an owned run past hi until the run closes, so every hit is found by exactly one chunk.  lo = 0, hi = L: the whole read
// from its first base, which is the definition.  base(j) is c[j], a code 0 .. 3.
template <typename F, typename G>
CCSX_SG_HD void ccsx_sg_walk(unsigned long long e0, unsigned long long e1, unsigned long long e2, unsigned long long e3, int m, int k, int L, int lo, int hi, F base, G hit)
{
    const unsigned long long top = 1ull << (m - 1);
    MyersCol col{~0ull, 0ull, m};
    bool prev = false, own = false;
    int best = 0, end = 0;
    for (int j = lo - (m + k) > 0 ? lo - (m + k) : 0; j < L; ++j) {
        const int b = base(j);
        myers_step(col, b == 0 ? e0 : b == 1 ? e1 : b == 2 ? e2 : e3, top, 0ull);
        const int jj = j + 1;                                       // E[jj] = col.score
        const bool ok = col.score <= k;
        if (jj > lo) {
            if (ok && !prev) { own = true; best = col.score; end = jj; }                  // (jj <= hi: the walk stops at hi outside an owned run)
            else if (ok && own && col.score < best) { best = col.score; end = jj; }
            else if (!ok && prev && own) { hit(end, best); own = false; }
            if (jj >= hi && !own) return;
        }
        prev = ok;
    }
    if (own) hit(end, best);                                        // (the run reaches the read's end)
}

// the start of the hit (end, dist): the reversed pattern against the read read backwards from end, anchored there; the shortest c[start, end) at distance dist.
// eqr(code): the reversed pattern's mask
template <typename F, typename M>
CCSX_SG_HD int ccsx_sg_start(M eqr, int m, int dist, int end, F base)
{
    const unsigned long long top = 1ull << (m - 1);
    MyersCol rc{~0ull, 0ull, m};
    const int xmax = end < m + dist ? end : m + dist;
    int x = 0;
    while (x < xmax) {
        const int b = base(end - 1 - x);
        ++x;
        myers_step(rc, eqr(b), top, 1ull);
        if (x >= m - dist && rc.score == dist) break;
    }
    return end - x;
}

// a hit's order key: (dist, start, search, end) ascending.  dist <= 19, start < 2^31, search < 66, end - start <= 83
CCSX_SG_HD unsigned long long ccsx_sg_key(int dist, int start, int search, int end)
{
    return ((unsigned long long)dist << 56) | ((unsigned long long)start << 24) | ((unsigned long long)search << 16) | (unsigned long long)(end - start);
}
struct SegmentHit { int start, end, search, dist; };
CCSX_SG_HD SegmentHit ccsx_sg_hit(unsigned long long key)
{
    SegmentHit h;
    h.dist = (int)(key >> 56); h.start = (int)((key >> 24) & 0xffffffffull); h.search = (int)((key >> 16) & 0xffull); h.end = h.start + (int)(key & 0xffffull);
    return h;
}

// [s0, e0) and [s1, e1) share a base
CCSX_SG_HD int ccsx_sg_overlap(int s0, int e0, int s1, int e1) { return s0 < e1 && s1 < e0; }

// The selection: keys in ascending order, n <= CCSX_SEGMENT_MAX_HITS of them; a hit is taken iff it intersects no hit taken before.  cuts: the taken hits by
// increasing start (they are disjoint, so a new hit can only touch its two neighbours there).  Returns n_cuts.
CCSX_SG_HD int ccsx_sg_select(const unsigned long long *sorted, int n, SegmentHit *cuts)
{
    int nc = 0;
    for (int r = 0; r < n; ++r) {
        const SegmentHit h = ccsx_sg_hit(sorted[r]);
        int p = 0;
        while (p < nc && cuts[p].start <= h.start) ++p;             // h goes before cuts[p]
        if (p > 0 && ccsx_sg_overlap(cuts[p - 1].start, cuts[p - 1].end, h.start, h.end)) continue;
        if (p < nc && ccsx_sg_overlap(cuts[p].start, cuts[p].end, h.start, h.end)) continue;
        for (int q = nc; q > p; --q) cuts[q] = cuts[q - 1];
        cuts[p] = h; ++nc;
    }
    return nc;
}

// the piece of `len` bases between a cut of search `left` and one of search `right`: 1 and its index and orientation when it is a segment
CCSX_SG_HD int ccsx_sg_classify(int left, int right, int len, int min_len, int *index, int *reverse)
{
    if (len < min_len) return 0;
    if (!(left & 1) && right == left + 2) { *index = left >> 1; *reverse = 0; return 1; }      // searches 2a, 2(a + 1)
    if ((left & 1) && right == left - 2) { *index = right >> 1; *reverse = 1; return 1; }      // searches 2(a + 1) + 1, 2a + 1
    return 0;
}

// pieces and summary of a read of L bases from its cuts, for a set of A adapters.  pieces: the first n_segments entries are written
struct SegmentSummary { int n_cuts, n_segments, complete, orient, leftover; };
CCSX_SG_HD SegmentSummary ccsx_sg_pieces(const SegmentHit *cuts, int nc, int L, int A, int min_len, ccsx_segment_piece *pieces)
{
    SegmentSummary s{nc, 0, 0, -1, 0};
    int fwd = 0, rev = 0, ordered = 1;
    for (int i = 0; i <= nc; ++i) {                                 // piece i lies before cut i; position 0 stands before the first cut, L after the last
        const int from = i ? cuts[i - 1].end : 0, to = i < nc ? cuts[i].start : L;
        int index = 0, reverse = 0;
        if (i > 0 && i < nc && ccsx_sg_classify(cuts[i - 1].search, cuts[i].search, to - from, min_len, &index, &reverse)) {
            ccsx_segment_piece &p = pieces[s.n_segments];
            p.start = from; p.end = to; p.index = (uint8_t)index; p.reverse = (uint8_t)reverse;
            p.dist_left = (uint8_t)cuts[i - 1].dist; p.dist_right = (uint8_t)cuts[i].dist;
            if (index != (reverse ? A - 2 - s.n_segments : s.n_segments)) ordered = 0;
            ++s.n_segments; fwd += !reverse; rev += reverse;
        } else if (to > from) s.leftover += to - from;
    }
    if (s.n_segments) s.orient = !rev ? 0 : !fwd ? 1 : 2;
    s.complete = s.orient >= 0 && s.orient <= 1 && s.n_segments == A - 1 && ordered;
    return s;
}

// the report of n reads on the device: [CCSX_SG_PLANES][n] int32, then the piece list [n][CCSX_SEGMENT_MAX_PIECES]
struct SegmentOut { int32_t *tested, *overflow, *n_hits, *n_cuts, *n_segments, *complete, *orient, *leftover; ccsx_segment_piece *pieces; };
CCSX_SG_HD SegmentOut ccsx_sg_out(int32_t *rep, size_t n)
{
    return {rep, rep + n, rep + 2 * n, rep + 3 * n, rep + 4 * n, rep + 5 * n, rep + 6 * n, rep + 7 * n, (ccsx_segment_piece *)(rep + CCSX_SG_PLANES * n)};
}
CCSX_SG_HD size_t ccsx_sg_rep_bytes(size_t n) { return n * (CCSX_SG_PLANES * 4 + CCSX_SEGMENT_MAX_PIECES * sizeof(ccsx_segment_piece)); }
// the planes of a read that is untested (tested 0, n_hits 0) or overflowed (tested 1, n_hits as counted, overflow 1); its list entries are zero
CCSX_SG_HD void ccsx_sg_put_empty(const SegmentOut &r, size_t z, int tested, int overflow, int n_hits)
{
    r.tested[z] = tested; r.overflow[z] = overflow; r.n_hits[z] = n_hits; r.n_cuts[z] = 0; r.n_segments[z] = 0; r.complete[z] = 0; r.orient[z] = -1; r.leftover[z] = 0;
}
CCSX_SG_HD void ccsx_sg_put(const SegmentOut &r, size_t z, int n_hits, const SegmentSummary &s)
{
    r.tested[z] = 1; r.overflow[z] = 0; r.n_hits[z] = n_hits; r.n_cuts[z] = s.n_cuts; r.n_segments[z] = s.n_segments; r.complete[z] = s.complete;
    r.orient[z] = s.orient; r.leftover[z] = s.leftover;
}
CCSX_SG_HD void ccsx_sg_zero_piece(ccsx_segment_piece &p) { p.start = 0; p.end = 0; p.index = 0; p.reverse = 0; p.dist_left = 0; p.dist_right = 0; }

// what k_segment is given (ccsx_segment.hip).  masks / len: built once per request by the host (ccsx_sg_pack), 66 x 64 + 66 bytes for a full set
struct SegmentParams {
    int32_t n, n_adapters;
    ccsx_segment_opts opts;
    const uint8_t *seq;                  // read z: seq_len[z] codes at seq + seq_off[z]
    const int64_t *seq_off;
    const int32_t *seq_len;
    const unsigned long long *masks;     // [2 * n_adapters][CCSX_SG_MASK_WORDS]
    const uint8_t *len;                  // [2 * n_adapters] the pattern length of every search
    int32_t *rep;                        // ccsx_sg_out; NULL: no request
};

// ---- the set and the report in memory, for the host, as barcode_core.h has them.  A packed set is the masks of the 2 * n_adapters searches, then one length
// byte per search, in whole 64-bit words; in one buffer the report of the reads (ccsx_sg_out, ccsx_sg_rep_bytes) stands behind it.
CCSX_SG_HD size_t ccsx_sg_set_words(int na) { return (size_t)na * 2 * CCSX_SG_MASK_WORDS + ((size_t)na * 2 + 7) / 8; }
// masks, len and rep of G for the packed set of G.n_adapters at `base`, device or host memory (rep: where the report would follow)
CCSX_SG_HD void ccsx_sg_bind(SegmentParams &G, const void *base)
{
    G.masks = (const unsigned long long *)base;
    G.len = (const uint8_t *)(G.masks + (size_t)G.n_adapters * 2 * CCSX_SG_MASK_WORDS);
    G.rep = (int32_t *)(G.masks + ccsx_sg_set_words(G.n_adapters));
}
// a checked set, packed into ccsx_sg_set_words(n_adapters) zeroed words
inline void ccsx_sg_pack(const ccsx_segment_set *set, unsigned long long *packed)
{
    SegmentParams G{};
    G.n_adapters = set->n_adapters;
    ccsx_sg_bind(G, packed);
    uint8_t *len = const_cast<uint8_t *>(G.len);
    for (int s = 0; s < 2 * set->n_adapters; ++s) {
        ccsx_sg_masks(set->seq[s >> 1], set->len[s >> 1], s & 1, packed + (size_t)s * CCSX_SG_MASK_WORDS);
        len[s] = (uint8_t)set->len[s >> 1];
    }
}
// a caller's report as the rule writes it
inline SegmentOut ccsx_sg_out(const ccsx_segment_report &r)
{
    return {r.tested, r.overflow, r.n_hits, r.n_cuts, r.n_segments, r.complete, r.orient, r.leftover_bases, r.pieces};
}

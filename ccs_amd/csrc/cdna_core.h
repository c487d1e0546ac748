// cdna_core.h — the cDNA rule for the host and the device (DESIGN.md §2 "cDNA rule"): the packed primer set, the strand and the class from the two ends' calls,
// the poly(A) scan, the internal-hit predicate, the final class and slice, and the report's layout.  The calls at the ends are the barcode rule's
// (barcode_core.h: ccsx_bc_walk, ccsx_bc_key, ccsx_bc_called), the hits inside the read the segment rule's (segment_core.h: ccsx_sg_masks, ccsx_sg_k,
// ccsx_sg_walk, ccsx_sg_start); nothing of either is stated again here.  ccsx_cdna_reads_host (ccsx_cdna_api.cpp) and k_cdna (ccsx_cdna.hip) are built from
// these three headers and from nothing else of the rule.  Integers only.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "ccsx.h"
#include "barcode_core.h"
#include "segment_core.h"

#define CCSX_CD_HD CCSX_BC_HD
#define CCSX_CDNA_THREADS 256
#define CCSX_CD_PLANES    16           // tested, cls, strand, start, end, polya_len, n_internal, first_internal, then idx, dist, second and clip as [n][2] each

// the options of the ends' calls as the barcode rule takes them
CCSX_CD_HD ccsx_barcode_opts ccsx_cd_end_opts(const ccsx_cdna_opts &o) { return {o.window, o.max_dist_pct, o.min_margin}; }

// what the walks leave per end (e 0: the head, 1: the tail, read on the reverse complement), and what the rule makes of a read
struct CdnaEnds { int idx[2], dist[2], second[2], clip[2]; };
struct CdnaRead { int cls, strand, start, end, polya_len, n_internal, first_internal; };

// Steps 2 and 3: strand, and the class of a read at which the rule ends.  1: the rule goes on with the insert [clip[0], L - clip[1]) of *ins_len >= 1 bases
// (r->cls is not yet set); 0: it ends here, r is complete.  len / role: of every primer of the set
CCSX_CD_HD int ccsx_cd_orient(const CdnaEnds &e, const uint8_t *len, const uint8_t *role, int L, const ccsx_cdna_opts &o, CdnaRead *r, int *ins_len)
{
    const ccsx_barcode_opts bo = ccsx_cd_end_opts(o);
    const int c0 = ccsx_bc_called(e.dist[0], e.second[0], (int)len[e.idx[0]], bo), c1 = ccsx_bc_called(e.dist[1], e.second[1], (int)len[e.idx[1]], bo);
    *r = CdnaRead{CCSX_CDNA_NO_PRIMER, -1, 0, 0, 0, 0, -1};
    *ins_len = 0;
    if (!c0 || !c1) { r->cls = c0 + c1 ? CCSX_CDNA_ONE_END : CCSX_CDNA_NO_PRIMER; return 0; }
    if (role[e.idx[0]] == role[e.idx[1]]) { r->cls = CCSX_CDNA_SAME_ROLE; return 0; }
    r->strand = (int)role[e.idx[0]];
    *ins_len = L - e.clip[0] - e.clip[1];
    if (*ins_len < 1) { r->cls = CCSX_CDNA_SHORT; return 0; }
    return 1;
}

// Step 4.  x_k: the k-th insert base counted from the 3' primer (k >= 1) is A on the transcript strand.  base(j) is c[j], a code 0 .. 3
template <typename F> CCSX_CD_HD int ccsx_cd_is_a(int strand, int L, int clip0, int clip1, int k, F base)
{
    return strand ? base(clip0 + k - 1) == 3 : base(L - clip1 - k) == 0;
}
CCSX_CD_HD int ccsx_cd_polya_k(int ins_len, const ccsx_cdna_opts &o) { return ins_len < o.polya_max ? ins_len : o.polya_max; }
CCSX_CD_HD int ccsx_cd_polya_score(int x, const ccsx_cdna_opts &o) { return x ? 1 : -o.polya_mismatch; }
// the scan stops at a base whose running score s lies more than polya_xdrop below the running maximum M (M includes s)
CCSX_CD_HD int ccsx_cd_polya_stop(int M, int s, const ccsx_cdna_opts &o) { return M - s > o.polya_xdrop; }
// polya_len over x(k), k = 1 .. K: the first position of the largest score before the stop.  (A stop position is never a new maximum, so the running arg-max at
// the stop is the answer; k_cdna does the same 64 positions at a time, with the sum and the maximum carried between blocks.)
template <typename X> CCSX_CD_HD int ccsx_cd_polya(int K, const ccsx_cdna_opts &o, X x)
{
    int s = 0, M = 0, arg = 0;
    for (int k = 1; k <= K; ++k) {
        s += ccsx_cd_polya_score(x(k), o);
        if (s > M) { M = s; arg = k; }
        else if (ccsx_cd_polya_stop(M, s, o)) break;
    }
    return arg;
}

// Step 5: a hit [start, end) of any search lies inside the insert (the poly(A) stretch is part of it)
CCSX_CD_HD int ccsx_cd_internal(int start, int end, int L, int clip0, int clip1) { return clip0 <= start && end <= L - clip1; }

// Step 6: class and slice of a read that reached step 4, from polya_len, n_internal and the insert
CCSX_CD_HD void ccsx_cd_finish(CdnaRead *r, const CdnaEnds &e, int L, int ins_len, const ccsx_cdna_opts &o)
{
    const int trimmed = ins_len - r->polya_len;
    r->cls = trimmed < o.min_len ? CCSX_CDNA_SHORT : r->n_internal > 0 ? CCSX_CDNA_CONCATEMER :
             o.min_polya > 0 && r->polya_len < o.min_polya ? CCSX_CDNA_NO_TAIL : CCSX_CDNA_FULL_LENGTH;
    r->start = 0; r->end = 0;
    if (r->cls >= CCSX_CDNA_CONCATEMER) {
        r->start = e.clip[0] + (r->strand ? r->polya_len : 0);
        r->end = L - e.clip[1] - (r->strand ? 0 : r->polya_len);
    }
}

// the report of n reads on the device: [CCSX_CD_PLANES][n] int32, the last four as [n][2]
struct CdnaOut { int32_t *tested, *cls, *strand, *start, *end, *polya_len, *n_internal, *first_internal, *idx, *dist, *second, *clip; };
CCSX_CD_HD CdnaOut ccsx_cd_out(int32_t *rep, size_t n)
{
    return {rep, rep + n, rep + 2 * n, rep + 3 * n, rep + 4 * n, rep + 5 * n, rep + 6 * n, rep + 7 * n, rep + 8 * n, rep + 10 * n, rep + 12 * n, rep + 14 * n};
}
CCSX_CD_HD size_t ccsx_cd_rep_bytes(size_t n) { return n * CCSX_CD_PLANES * 4; }
// the [n] planes of read z
CCSX_CD_HD void ccsx_cd_put_read(const CdnaOut &o, size_t z, int tested, const CdnaRead &r)
{
    o.tested[z] = tested; o.cls[z] = r.cls; o.strand[z] = r.strand; o.start[z] = r.start; o.end[z] = r.end; o.polya_len[z] = r.polya_len;
    o.n_internal[z] = r.n_internal; o.first_internal[z] = r.first_internal;
}
// the [n][2] planes of end e of read z
CCSX_CD_HD void ccsx_cd_put_end(const CdnaOut &o, size_t z, int e, int idx, int dist, int second, int clip)
{
    o.idx[2 * z + e] = idx; o.dist[2 * z + e] = dist; o.second[2 * z + e] = second; o.clip[2 * z + e] = clip;
}
CCSX_CD_HD void ccsx_cd_put_untested(const CdnaOut &o, size_t z)
{
    ccsx_cd_put_read(o, z, 0, CdnaRead{CCSX_CDNA_NO_PRIMER, -1, 0, 0, 0, 0, -1});
    for (int e = 0; e < 2; ++e) ccsx_cd_put_end(o, z, e, -1, 255, 255, 0);
}

// what k_cdna is given (ccsx_cdna.hip).  masks / len / role: built once per request by the host (ccsx_cd_pack), 64 x 128 + 128 bytes for a full set
struct CdnaParams {
    int32_t n, n_primers;
    ccsx_cdna_opts opts;
    const uint8_t *seq;                  // read z: seq_len[z] codes at seq + seq_off[z]
    const int64_t *seq_off;
    const int32_t *seq_len;
    const unsigned long long *masks;     // [2 * n_primers][CCSX_SG_MASK_WORDS]: ccsx_sg_masks of search 2b + rc; words 0 .. 3 of search 2b are primer b's ccsx_bc_masks
    const uint8_t *len;                  // [n_primers]
    const uint8_t *role;                 // [n_primers]
    int32_t *rep;                        // ccsx_cd_out; NULL: no request
};

// ---- the set and the report in memory, for the host, as barcode_core.h has them.  A packed set is the masks of the 2 * n_primers searches, then one length
// byte and then one role byte per primer, in whole 64-bit words; in one buffer the report of the reads (ccsx_cd_out, ccsx_cd_rep_bytes) stands behind it.
CCSX_CD_HD size_t ccsx_cd_set_words(int np) { return (size_t)np * 2 * CCSX_SG_MASK_WORDS + ((size_t)np * 2 + 7) / 8; }
// masks, len, role and rep of D for the packed set of D.n_primers at `base`, device or host memory (rep: where the report would follow)
CCSX_CD_HD void ccsx_cd_bind(CdnaParams &D, const void *base)
{
    D.masks = (const unsigned long long *)base;
    D.len = (const uint8_t *)(D.masks + (size_t)D.n_primers * 2 * CCSX_SG_MASK_WORDS);
    D.role = D.len + D.n_primers;
    D.rep = (int32_t *)(D.masks + ccsx_cd_set_words(D.n_primers));
}
// a checked set, packed into ccsx_cd_set_words(n_primers) zeroed words
inline void ccsx_cd_pack(const ccsx_cdna_set *set, unsigned long long *packed)
{
    CdnaParams D{};
    D.n_primers = set->n_primers;
    ccsx_cd_bind(D, packed);
    uint8_t *len = const_cast<uint8_t *>(D.len), *role = const_cast<uint8_t *>(D.role);
    for (int b = 0; b < set->n_primers; ++b) {
        for (int rc = 0; rc < 2; ++rc) ccsx_sg_masks(set->seq[b], set->len[b], rc, packed + (size_t)(2 * b + rc) * CCSX_SG_MASK_WORDS);
        len[b] = (uint8_t)set->len[b]; role[b] = set->role[b];
    }
}
// a caller's report as the rule writes it
inline CdnaOut ccsx_cd_out(const ccsx_cdna_report &r)
{
    return {r.tested, r.cls, r.strand, r.start, r.end, r.polya_len, r.n_internal, r.first_internal, r.idx, r.dist, r.second, r.clip};
}

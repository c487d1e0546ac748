// cell_core.h — the cell-tag rule for the host and the device (DESIGN.md §2 "Cell-tag rule"): the packed fields, the one enumeration of the correction's
// candidates, the whitelist's table and its probe, the decision over what the candidates reach, the widened clip, and the report's layout.  The ends, the strand,
// the poly(A) scan, the internal hits, the class and the slice are the cDNA rule's (cdna_core.h, over barcode_core.h and segment_core.h), the hash the duplicate
// rule's (dup_core.h); nothing of them is stated again here.  ccsx_cell_reads_host (ccsx_cell_api.cpp) and k_cell (ccsx_cell.hip) are built from these headers and
// from nothing else of the rule.  Integers only.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "ccsx.h"
#include "cdna_core.h"
#include "dup_core.h"

#define CCSX_CL_HD CCSX_BC_HD
#define CCSX_CELL_THREADS CCSX_CDNA_THREADS
#define CCSX_CL_PLANES 8                 // tag, bc_raw, bc, bc_hi, kind, shift, umi, tag_clip: [n] each, behind the CCSX_CD_PLANES of the cDNA report

// ---- fields.  A field of n <= 16 bases in a uint32, the first base most significant
template <typename F> CCSX_CL_HD uint32_t ccsx_cl_pack(int n, F base)
{
    uint32_t x = 0u;
    for (int j = 0; j < n; ++j) x = (x << 2) | (uint32_t)(base(j) & 3);
    return x;
}
// the same field from the low and the high bits of a run of bases (bit j: base j), the form a wave's ballots give: bases [o, o + n)
CCSX_CL_HD uint32_t ccsx_cl_field_of_bits(unsigned long long lo, unsigned long long hi, int o, int n)
{
    if (n <= 0) return 0u;
    const unsigned long long m = (1ull << n) - 1ull;
    const uint32_t v = (uint32_t)(ccsx_dup_spread((lo >> o) & m) | (ccsx_dup_spread((hi >> o) & m) << 1));   // base j at bits 2 j
    return ccsx_dup_rev_bases(v) >> (32 - 2 * n);
}

// ---- the candidates of a barcode field raw of b bases that is no member of the whitelist: 8 b of them, numbered 0 .. 8 b - 1 (at most 128).
//   [0, 3 b)      kind 1: base i / 3 replaced by the (i % 3 + 1)-th next code
//   [3 b, 7 b)    kind 2: the first b - 1 bases with code i % 4 inserted at place i / 4           (indels only)
//   [7 b, 8 b)    kind 3: base i deleted, `next` (the base behind the field) appended             (indels, and only where that base is inside the insert)
// *kind: 1 .. 3, or 0: candidate i is not tried under these conditions
CCSX_CL_HD int ccsx_cl_n_candidates(int b) { return 8 * b; }
CCSX_CL_HD uint32_t ccsx_cl_low(int bases) { return (uint32_t)((1ull << (2 * bases)) - 1ull); }   // the low `bases` bases of a field, 0 .. 16
CCSX_CL_HD uint32_t ccsx_cl_candidate(uint32_t raw, int b, int next, int indels, int has_next, int i, int *kind)
{
    if (i < 3 * b) {
        const int pos = i / 3, sh = 2 * (b - 1 - pos);
        *kind = 1;
        return raw ^ ((uint32_t)(i - 3 * pos + 1) << sh);            // (x ^ d, d = 1 .. 3: the three other codes)
    }
    if (i < 7 * b) {
        const int j = i - 3 * b, pos = j >> 2, tail = b - 1 - pos;  // `tail` bases follow the inserted one
        *kind = indels ? 2 : 0;
        return (raw & ~ccsx_cl_low(tail + 1)) | ((uint32_t)(j & 3) << (2 * tail)) | ((raw >> 2) & ccsx_cl_low(tail));
    }
    const int pos = i - 7 * b, tail = b - pos;                       // `tail` bases of raw . next follow the deleted one
    const unsigned long long ext = ((unsigned long long)raw << 2) | (unsigned long long)(next & 3);
    *kind = indels && has_next ? 3 : 0;
    return (raw & ~ccsx_cl_low(tail)) | ((uint32_t)ext & ccsx_cl_low(tail));
}
CCSX_CL_HD int ccsx_cl_shift(int kind) { return kind == 2 ? -1 : kind == 3 ? 1 : 0; }

// ---- the whitelist's table: slots (key << 32) | (index + 1), 0 empty; the probe returns the index of key x, or -1
CCSX_CL_HD uint32_t ccsx_cl_slot(uint32_t x, uint32_t slots) { return ccsx_dup_hash32(x) & (slots - 1u); }
CCSX_CL_HD uint32_t ccsx_cl_n_slots(int n) { uint32_t s = 64u; while (s < 2u * (uint32_t)n) s <<= 1; return s; }
CCSX_CL_HD int ccsx_cl_probe(const unsigned long long *table, uint32_t slots, uint32_t x)
{
    uint32_t s = ccsx_cl_slot(x, slots);
    for (uint32_t i = 0; i < slots; ++i, s = (s + 1u) & (slots - 1u)) {   // (at most half of the slots are taken: an empty one ends every probe; the bound is a guard)
        const unsigned long long v = table[s];                      // one 8-byte load per slot
        if (!v) return -1;
        if ((uint32_t)(v >> 32) == x) return (int)(uint32_t)v - 1;
    }
    return -1;
}

// ---- what the rule makes of a read's tag
struct CellTag { int tag; uint32_t bc_raw; int bc, bc_hi, kind, shift; uint32_t umi; int tag_clip; };
CCSX_CL_HD CellTag ccsx_cl_none() { return {CCSX_CELL_NONE, 0u, -1, -1, 0, 0, 0u, 0}; }
// step 2: the tag end, and where the fields begin on it
CCSX_CL_HD int ccsx_cl_tag_end(int strand, const ccsx_cell_design &d) { return strand == d.side ? 0 : 1; }
CCSX_CL_HD int ccsx_cl_bc_at(int p0, const ccsx_cell_design &d) { return p0 + (d.bc_first ? 0 : d.umi_len); }
CCSX_CL_HD int ccsx_cl_umi_at(int p0, int shift, const ccsx_cell_design &d) { return d.bc_first ? p0 + d.bc_len + shift : p0; }
// step 4's decision from the smallest and the largest index reached (lo > hi or lo < 0: none) and the smallest kind that reaches lo
CCSX_CL_HD void ccsx_cl_decide(CellTag *t, int lo, int hi, int kind)
{
    t->bc = -1; t->bc_hi = -1; t->kind = 0; t->shift = 0;
    if (lo < 0 || hi < lo) { t->tag = CCSX_CELL_ABSENT; return; }
    t->bc = lo; t->bc_hi = hi;
    if (lo != hi) { t->tag = CCSX_CELL_AMBIGUOUS; return; }
    t->tag = CCSX_CELL_CORRECTED; t->kind = kind; t->shift = ccsx_cl_shift(kind);
}
// step 6: the ends with the tag end's clip widened
CCSX_CL_HD CdnaEnds ccsx_cl_widen(const CdnaEnds &e, int e_t, int tag_clip) { CdnaEnds w = e; w.clip[e_t] += tag_clip; return w; }

// ---- the report of n reads on the device: the cDNA report's planes (ccsx_cd_out), then [CCSX_CL_PLANES][n] words
struct CellOut { CdnaOut cd; int32_t *tag; uint32_t *bc_raw; int32_t *bc, *bc_hi, *kind, *shift; uint32_t *umi; int32_t *tag_clip; };
CCSX_CL_HD CellOut ccsx_cl_out(int32_t *rep, size_t n)
{
    int32_t *c = rep + (size_t)CCSX_CD_PLANES * n;
    return {ccsx_cd_out(rep, n), c, (uint32_t *)(c + n), c + 2 * n, c + 3 * n, c + 4 * n, c + 5 * n, (uint32_t *)(c + 6 * n), c + 7 * n};
}
CCSX_CL_HD size_t ccsx_cl_rep_bytes(size_t n) { return n * (CCSX_CD_PLANES + CCSX_CL_PLANES) * 4; }
CCSX_CL_HD void ccsx_cl_put_tag(const CellOut &o, size_t z, const CellTag &t)
{
    o.tag[z] = t.tag; o.bc_raw[z] = t.bc_raw; o.bc[z] = t.bc; o.bc_hi[z] = t.bc_hi; o.kind[z] = t.kind; o.shift[z] = t.shift; o.umi[z] = t.umi;
    o.tag_clip[z] = t.tag_clip;
}

// what k_cell is given (ccsx_cell.hip): k_cdna's parameters (D.rep: ccsx_cl_out), the design, and the resident table (NULL: no whitelist)
struct CellParams {
    CdnaParams D;
    ccsx_cell_design design;
    const unsigned long long *table;
    uint32_t slots;
};

// ---- the host's whitelist (ccsx_cell_api.cpp builds it)
struct ccsx_cell_whitelist {
    int32_t n, bc_len;
    uint32_t slots;
    uint64_t serial;                     // of this object among all a process has made; never 0
    unsigned long long *table;
};

// a caller's report as the rule writes it
inline CellOut ccsx_cl_out(const ccsx_cell_report &r) { return {ccsx_cd_out(r.cdna), r.tag, r.bc_raw, r.bc, r.bc_hi, r.kind, r.shift, r.umi, r.tag_clip}; }

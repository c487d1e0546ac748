// ccsx_cell.hip — cell barcodes and UMIs on final reads (DESIGN.md §2 "Cell-tag rule", §4 "k_cell").  The rule itself is cell_core.h over cdna_core.h; this file
// is its layout on the device.  Integers only; no byte of the report depends on the launch geometry, on the order of the lanes or on scheduling: the atomics are
// LDS integer minima and one LDS integer add whose sum alone is used, and what the candidates reach is joined by wave minima and maxima.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ccsx.h"
#include "cell_core.h"
#include "wave_ops.h"

namespace {

constexpr int NT = CCSX_CELL_THREADS, CH = CCSX_SEGMENT_CHUNK;
constexpr int NONE = 0x7fffffff;
static_assert(2 * CCSX_CDNA_MAX_PRIMERS <= NT, "the (end, primer) items are one pass of the workgroup");
static_assert(8 * CCSX_CELL_MAX_FIELD <= 128 && 2 * CCSX_CELL_MAX_FIELD + 1 <= 64, "two candidates a lane; the fields and the base behind them are one wave's ballots");

__device__ __forceinline__ int wave_min_i32(int v) { return -wave_reduce_max_i32(-v); }   // (v > INT_MIN)

// ---- the poly(A) scan of one wave (all 64 lanes): ccsx_cd_polya, 64 positions a round, as k_cdna's (ccsx_cdna.hip: the carried sum and maximum, the stop as the
// first lane of a ballot, the smallest k of the largest score before it)
template <typename X> __device__ __forceinline__ int wave_polya(int K, const ccsx_cdna_opts &o, int lane, X x)
{
    int cs = 0, cM = 0, arg = 0;
    for (int k0 = 0; k0 < K; k0 += 64) {
        const int k = k0 + lane + 1;
        const bool valid = k <= K;
        const int s = cs + wave_scan_add_i32(valid ? ccsx_cd_polya_score(x(k), o) : 0);
        const int M = imax(cM, wave_scan_max_i32(s));
        const unsigned long long stop = __ballot(valid && ccsx_cd_polya_stop(M, s, o));
        const int f = stop ? __ffsll(stop) - 1 : min(64, K - k0);   // lanes [0, f) lie before the stop
        if (f > 0) {
            const int Mx = __shfl(M, f - 1);
            if (Mx > cM) { arg = k0 + __ffsll(__ballot(lane < f && s == Mx)); cM = Mx; }
        }
        if (stop) break;
        cs = __shfl(s, 63);
    }
    return arg;
}

// ---- the tag of one read, by one wave (all 64 lanes; every argument and the result are the same in every lane).  Lane j holds base j of the tag end behind the
// primer's clip p0: the T bases of the fields and, where the insert has it, the one behind them.  Two ballots give their low and high bits, from which every lane
// packs the fields (ccsx_cl_field_of_bits).  The exact probe is the same address in every lane.  The 8 bc_len candidates are dealt two to a lane, lane and
// lane + 64 of ccsx_cl_candidate's numbering; a lane probes its own, one 8-byte load per slot; the smallest and the largest index reached are a wave minimum and
// maximum, the smallest kind that reaches the smallest index a second minimum.
__device__ __forceinline__ CellTag wave_tag(const CellParams &C, const uint8_t *c, int L, int e_t, int p0, int ins_len, int lane)
{
    const ccsx_cell_design &d = C.design;
    const int b = d.bc_len, T = d.umi_len + b, has_next = ins_len >= T + 1, o_bc = ccsx_cl_bc_at(0, d);
    const int x = lane < T + has_next ? ccsx_bc_base(c, L, e_t, p0 + lane) : 0;   // (ins_len >= T + has_next: inside the insert)
    const unsigned long long lo = __ballot(x & 1), hi = __ballot(x & 2);
    CellTag t = ccsx_cl_none();
    t.tag = CCSX_CELL_RAW;
    t.bc_raw = ccsx_cl_field_of_bits(lo, hi, o_bc, b);
    if (b > 0 && C.table) {                                          // (wave-uniform, as the exact probe's result)
        const int exact = ccsx_cl_probe(C.table, C.slots, t.bc_raw);
        if (exact >= 0) { t.tag = CCSX_CELL_EXACT; t.bc = t.bc_hi = exact; }
        else {
            const int next = (int)((lo >> (o_bc + b)) & 1ull) | (int)(((hi >> (o_bc + b)) & 1ull) << 1), nc = ccsx_cl_n_candidates(b);
            int w0 = -1, w1 = -1, k0 = 0, k1 = 0;
            if (lane < nc) {
                const uint32_t q = ccsx_cl_candidate(t.bc_raw, b, next, d.indels, has_next, lane, &k0);
                if (k0) w0 = ccsx_cl_probe(C.table, C.slots, q);
            }
            if (lane + 64 < nc) {
                const uint32_t q = ccsx_cl_candidate(t.bc_raw, b, next, d.indels, has_next, lane + 64, &k1);
                if (k1) w1 = ccsx_cl_probe(C.table, C.slots, q);
            }
            const int wlo = wave_min_i32(min(w0 < 0 ? NONE : w0, w1 < 0 ? NONE : w1)), whi = wave_reduce_max_i32(max(w0, w1));
            const int kind = wave_min_i32(min(w0 == wlo ? k0 : 4, w1 == wlo ? k1 : 4));
            ccsx_cl_decide(&t, whi < 0 ? -1 : wlo, whi, kind);
        }
    }
    t.umi = ccsx_cl_field_of_bits(lo, hi, ccsx_cl_umi_at(0, t.shift, d), d.umi_len);
    t.tag_clip = T + t.shift;
    return t;
}

// ---- k_cell: one 256-thread workgroup per read, k_cdna's phases with the tag between the ends and the rest.
// Phase A, the ends: as k_cdna's (both windows in LDS, one 64-bit Myers word per (end, primer) item, LDS minima); every thread makes the same decision
// (ccsx_cd_orient).  A read at which the rule ends there, or whose insert is shorter than the fields, is written with tag NONE and left by the whole workgroup.
// Phase T, the tag: wave 0 alone (wave_tag); lane 0 writes the tag's planes and leaves tag_clip in LDS.  After the barrier every thread widens the tag end's clip.
// Phase B, the poly(A): wave 0 alone (wave_polya) while the other waves begin phase C.
// Phase C, the internal hits: as k_cdna's, against the widened insert.
// Reads: seq[seq_off[z] + (0 .. L - 1)], masks[0 .. 16 P), len / role[0 .. P), table[0 .. slots); writes: the read's own report words only, every one of them.
__global__ __launch_bounds__(NT) void k_cell(CellParams C)
{
    __shared__ uint8_t sWin[2][CCSX_BARCODE_MAX_WINDOW];
    __shared__ int sBest[2], sSecond[2], sClip[2], sPolya, sCount, sFirst, sTagClip;
    const CdnaParams &D = C.D;
    const int tid = threadIdx.x, z = blockIdx.x;
    if (z >= D.n) return;
    const CellOut out = ccsx_cl_out(D.rep, (size_t)D.n);
    const int L = D.seq_len[z];
    if (L <= 0) {                                                    // untested
        if (tid == 0) { ccsx_cd_put_untested(out.cd, (size_t)z); ccsx_cl_put_tag(out, (size_t)z, ccsx_cl_none()); }
        return;
    }
    const int W = min(L, min(D.opts.window, CCSX_BARCODE_MAX_WINDOW)), P = D.n_primers;
    const uint8_t *c = D.seq + D.seq_off[z];
    for (int j = tid; j < W; j += NT) { sWin[0][j] = (uint8_t)ccsx_bc_base(c, L, 0, j); sWin[1][j] = (uint8_t)ccsx_bc_base(c, L, 1, j); }
    if (tid < 2) { sBest[tid] = NONE; sSecond[tid] = 255; sClip[tid] = 0; }
    if (tid == 0) { sPolya = 0; sCount = 0; sFirst = NONE; sTagClip = 0; }
    __syncthreads();
    const bool have = tid < 2 * P;
    const int e = have && tid >= P ? 1 : 0, b = have ? tid - e * P : 0;
    BarcodeHit h{0, 0};
    if (have) {
        const unsigned long long *k = D.masks + (size_t)2 * b * CCSX_SG_MASK_WORDS;
        const uint8_t *w = sWin[e];
        h = ccsx_bc_walk(k[0], k[1], k[2], k[3], (int)D.len[b], W, [&](int j) { return (int)w[j]; });
        atomicMin(&sBest[e], ccsx_bc_key(h.dist, b));
    }
    __syncthreads();
    if (have) {
        if (b == (sBest[e] & 0xffff)) sClip[e] = h.clip;             // (one item per end)
        else atomicMin(&sSecond[e], h.dist);
    }
    __syncthreads();
    if (tid < 2) ccsx_cd_put_end(out.cd, (size_t)z, tid, sBest[tid] & 0xffff, sBest[tid] >> 16, sSecond[tid], sClip[tid]);
    const CdnaEnds ends{{sBest[0] & 0xffff, sBest[1] & 0xffff}, {sBest[0] >> 16, sBest[1] >> 16}, {sSecond[0], sSecond[1]}, {sClip[0], sClip[1]}};
    CdnaRead r;
    int ins_len;
    const int T = C.design.umi_len + C.design.bc_len;
    const bool on = ccsx_cd_orient(ends, D.len, D.role, L, D.opts, &r, &ins_len);   // (the same in every thread)
    if (!on || ins_len < T) {
        if (on) r.cls = CCSX_CDNA_SHORT;
        if (tid == 0) { ccsx_cd_put_read(out.cd, (size_t)z, 1, r); ccsx_cl_put_tag(out, (size_t)z, ccsx_cl_none()); }
        return;
    }
    const int e_t = ccsx_cl_tag_end(r.strand, C.design);
    if (tid < 64) {
        const CellTag t = wave_tag(C, c, L, e_t, e_t ? ends.clip[1] : ends.clip[0], ins_len, tid);
        if (tid == 0) { ccsx_cl_put_tag(out, (size_t)z, t); sTagClip = t.tag_clip; }
    }
    __syncthreads();
    const int tag_clip = sTagClip, ins2 = ins_len - tag_clip;
    const int clip0 = ends.clip[0] + (e_t ? 0 : tag_clip), clip1 = ends.clip[1] + (e_t ? tag_clip : 0);   // ccsx_cl_widen, in named registers
    if (ins2 < 1) {
        r.cls = CCSX_CDNA_SHORT;
        if (tid == 0) ccsx_cd_put_read(out.cd, (size_t)z, 1, r);
        return;
    }
    const auto base = [&](int j) { return (int)(c[j] & 3); };
    if (tid < 64) {
        const int len = wave_polya(ccsx_cd_polya_k(ins2, D.opts), D.opts, tid, [&](int k) { return ccsx_cd_is_a(r.strand, L, clip0, clip1, k, base); });
        if (tid == 0) sPolya = len;
    }
    const int S = 2 * P;
    const long long items = (long long)((L + CH - 1) / CH) * S;
    for (long long it = tid; it < items; it += NT) {
        const int chunk = (int)(it / S), s = (int)(it - (long long)chunk * S);
        const int lo = chunk * CH, hi = min(L, lo + CH), m = (int)D.len[s >> 1];
        const unsigned long long *w = D.masks + (size_t)s * CCSX_SG_MASK_WORDS;
        ccsx_sg_walk(w[0], w[1], w[2], w[3], m, ccsx_sg_k(m, D.opts.max_dist_pct), L, lo, hi, base, [&](int end, int dist) {
            const int start = ccsx_sg_start([&](int code) { return w[4 + code]; }, m, dist, end, base);
            if (!ccsx_cd_internal(start, end, L, clip0, clip1)) return;
            atomicAdd(&sCount, 1);
            atomicMin(&sFirst, start);
        });
    }
    __syncthreads();
    if (tid == 0) {
        r.polya_len = sPolya; r.n_internal = sCount; r.first_internal = sCount ? sFirst : -1;
        const CdnaEnds wide{{ends.idx[0], ends.idx[1]}, {ends.dist[0], ends.dist[1]}, {ends.second[0], ends.second[1]}, {clip0, clip1}};
        ccsx_cd_finish(&r, wide, L, ins2, D.opts);
        ccsx_cd_put_read(out.cd, (size_t)z, 1, r);
    }
}

}  // namespace

const char *ccsx_cell_launch(const CellParams &C, hipStream_t st)
{
    if (C.D.n <= 0) return nullptr;
    hipLaunchKernelGGL(k_cell, dim3((unsigned)C.D.n), dim3(NT), 0, st, C);
    return hipGetLastError() != hipSuccess ? "k_cell" : nullptr;
}

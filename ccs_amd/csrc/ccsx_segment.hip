// ccsx_segment.hip — segmentation of concatenated-array reads on final reads (DESIGN.md §2 "Segment rule", §4 "k_segment").  The rule itself is segment_core.h;
// this file is its layout on the device.  Integers only; no byte of the report depends on the launch geometry, on the order of the lanes or on scheduling: the
// only atomic is one LDS integer add (the hit count, which also hands out buffer places), and the hits are ranked by key before anything looks at their order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ccsx.h"
#include "segment_core.h"

namespace {

constexpr int NT = CCSX_SEGMENT_THREADS, CH = CCSX_SEGMENT_CHUNK, NH = CCSX_SEGMENT_MAX_HITS, NP = CCSX_SEGMENT_MAX_PIECES;
static_assert(NH <= 64 && NP <= 64 && NT >= 64, "the ranking and the list are one wave's work");

// ---- k_segment: one 256-thread workgroup per read.  An item is (chunk c of CH read bases, search s), numbered c * S + s, S = 2 * n_adapters searches: the lanes
// of a wave hold the searches of one chunk, or of neighbouring chunks, so the bases they read at a step are the same byte or a few bytes CH apart; lane tid takes
// the items tid, tid + 256, ...  An item is one 64-bit word walked serially over its chunk after a warm-up of m + k bases (ccsx_sg_walk); the four match masks and
// the column live in registers.  The lane that owns a run closes it, finds the hit's start by the reversed pattern, anchored (ccsx_sg_start), and puts the key
// into an LDS buffer of 64 at the place an atomicAdd hands out; the count is not capped, the buffer is.  More than 64 hits: overflow, the keys are not looked at.
// Otherwise wave 0 ranks the keys (they are distinct: a search has one hit per end), thread 0 makes the selection and the pieces from the sorted keys
// (ccsx_sg_select, ccsx_sg_pieces: at most 64 hits, each against its two neighbours) and writes the planes, and wave 0 writes all 64 list entries, zero beyond
// n_segments.  Reads: seq[seq_off[z] + (0 .. L - 1)], masks[0 .. 8 S), len[0 .. S); writes: the read's own report words and list entries only.
__global__ __launch_bounds__(NT) void k_segment(SegmentParams G)
{
    __shared__ unsigned long long sKey[NH], sSorted[NH];
    __shared__ SegmentHit sCut[NH];
    __shared__ ccsx_segment_piece sPiece[NP];
    __shared__ int sHits, sSegments;
    const int tid = threadIdx.x, z = blockIdx.x;
    if (z >= G.n) return;
    const SegmentOut out = ccsx_sg_out(G.rep, (size_t)G.n);
    ccsx_segment_piece *list = out.pieces + (size_t)z * NP;
    const int L = G.seq_len[z];
    if (L <= 0) {                                                    // untested
        if (tid == 0) ccsx_sg_put_empty(out, (size_t)z, 0, 0, 0);
        if (tid < NP) ccsx_sg_zero_piece(list[tid]);
        return;
    }
    if (tid == 0) sHits = 0;
    __syncthreads();
    const uint8_t *c = G.seq + G.seq_off[z];
    const auto base = [&](int j) { return (int)(c[j] & 3); };
    const int A = G.n_adapters, S = 2 * A;
    const long long items = (long long)((L + CH - 1) / CH) * S;
    for (long long it = tid; it < items; it += NT) {
        const int chunk = (int)(it / S), s = (int)(it - (long long)chunk * S);
        const int lo = chunk * CH, hi = min(L, lo + CH), m = (int)G.len[s];
        const unsigned long long *w = G.masks + (size_t)s * CCSX_SG_MASK_WORDS;
        ccsx_sg_walk(w[0], w[1], w[2], w[3], m, ccsx_sg_k(m, G.opts.max_dist_pct), L, lo, hi, base, [&](int end, int dist) {
            const int i = atomicAdd(&sHits, 1);
            if (i < NH) sKey[i] = ccsx_sg_key(dist, ccsx_sg_start([&](int b) { return w[4 + b]; }, m, dist, end, base), s, end);
        });
    }
    __syncthreads();
    const int n_hits = sHits;
    if (n_hits > NH) {                                               // overflow: adapter junk
        if (tid == 0) ccsx_sg_put_empty(out, (size_t)z, 1, 1, n_hits);
        if (tid < NP) ccsx_sg_zero_piece(list[tid]);
        return;
    }
    if (tid < n_hits) {
        const unsigned long long key = sKey[tid];
        int rank = 0;
        for (int q = 0; q < n_hits; ++q) rank += sKey[q] < key ? 1 : 0;
        sSorted[rank] = key;
    }
    __syncthreads();
    if (tid == 0) {
        const int nc = ccsx_sg_select(sSorted, n_hits, sCut);
        const SegmentSummary sum = ccsx_sg_pieces(sCut, nc, L, A, G.opts.min_len, sPiece);
        ccsx_sg_put(out, (size_t)z, n_hits, sum);
        sSegments = sum.n_segments;
    }
    __syncthreads();
    if (tid < NP) {
        if (tid < sSegments) list[tid] = sPiece[tid];
        else ccsx_sg_zero_piece(list[tid]);
    }
}

}  // namespace

const char *ccsx_segment_launch(const SegmentParams &G, hipStream_t st)
{
    if (G.n <= 0) return nullptr;
    hipLaunchKernelGGL(k_segment, dim3((unsigned)G.n), dim3(NT), 0, st, G);
    return hipGetLastError() != hipSuccess ? "k_segment" : nullptr;
}

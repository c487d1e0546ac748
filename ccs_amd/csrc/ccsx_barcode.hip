// ccsx_barcode.hip — barcode calls on final reads (DESIGN.md §2 "Barcode calls", §4 "k_barcode").  The rule itself is barcode_core.h; this file is its layout on
// the device.  Integers only; no result depends on the launch geometry, on the order of the lanes or on scheduling: the only atomics are LDS minima.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ccsx.h"
#include "barcode_core.h"
#include "wave_ops.h"

namespace {

constexpr int NT = CCSX_BARCODE_THREADS;
constexpr int PASSES = (2 * CCSX_BARCODE_MAX + NT - 1) / NT;   // items of a full set over the workgroup: 768 / 256 = 3
constexpr int NONE = 0x7fffffff;

// the minimum of v over the wave, in every lane (v >= 0 or NONE)
__device__ __forceinline__ int wave_min_i32(int v) { return -wave_reduce_max_i32(-v); }

// ---- k_barcode: one 256-thread workgroup per read.  Both windows sit in LDS as bytes, end 1 already reverse-complemented.  An item is (end e, barcode b),
// numbered e * n_barcodes + b; lane tid takes the items tid, tid + 256, tid + 512 (a full set of 384 barcodes is exactly three passes; up to 128 barcodes are one).
// An item is one 64-bit word walked serially over the W' columns of its window: the four match masks and the column live in registers, the base of a step is one
// LDS byte that every lane of the same end reads from the same address (a broadcast; a wave that holds the boundary between the ends reads two addresses).
// Per end, the best barcode is the minimum of dist << 16 | b: a wave reduction, then one LDS atomicMin per wave; after a barrier the runner-up is the minimum
// of dist over the items with b != idx, taken the same way, and the item with b == idx leaves its clip.  Thread 0 makes the call and writes the eleven words.
// Reads: seq[seq_off[z] + (0 .. L - 1)] only; writes: the read's own report words only.
__global__ __launch_bounds__(NT) void k_barcode(BarcodeParams B)
{
    __shared__ uint8_t sWin[2][CCSX_BARCODE_MAX_WINDOW];
    __shared__ int sBest[2], sSecond[2], sClip[2];
    const int tid = threadIdx.x, z = blockIdx.x;
    if (z >= B.n) return;
    const BarcodeOut out = ccsx_bc_out(B.rep, (size_t)B.n);
    const int L = B.seq_len[z];
    if (L <= 0) {                                                    // untested
        if (tid == 0) ccsx_bc_put_untested(out, z);
        return;
    }
    const int W = min(L, min(B.opts.window, CCSX_BARCODE_MAX_WINDOW)), nb = B.n_barcodes, items = 2 * nb;
    const uint8_t *c = B.seq + B.seq_off[z];
    for (int j = tid; j < W; j += NT) { sWin[0][j] = (uint8_t)ccsx_bc_base(c, L, 0, j); sWin[1][j] = (uint8_t)ccsx_bc_base(c, L, 1, j); }
    if (tid < 2) { sBest[tid] = NONE; sSecond[tid] = 255; sClip[tid] = 0; }
    __syncthreads();
    int dist[PASSES], clip[PASSES];
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
        const int it = tid + p * NT;
        dist[p] = NONE; clip[p] = 0;
        if ((it & ~63) >= items) continue;                           // (wave-uniform: no lane of this wave has an item in this pass)
        const bool have = it < items;
        const int e = have && it >= nb ? 1 : 0, b = have ? it - e * nb : 0;
        if (have) {
            const unsigned long long *k = B.masks + (size_t)b * 4;
            const uint8_t *w = sWin[e];
            const BarcodeHit h = ccsx_bc_walk(k[0], k[1], k[2], k[3], (int)B.len[b], W, [&](int j) { return (int)w[j]; });
            dist[p] = h.dist; clip[p] = h.clip;
        }
        for (int q = 0; q < 2; ++q) {
            const int best = wave_min_i32(have && e == q ? ccsx_bc_key(dist[p], b) : NONE);
            if ((tid & 63) == 0 && best != NONE) atomicMin(&sBest[q], best);
        }
    }
    __syncthreads();
    const int idx0 = sBest[0] & 0xffff, idx1 = sBest[1] & 0xffff;
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
        const int it = tid + p * NT;
        if ((it & ~63) >= items) continue;
        const bool have = it < items;
        const int e = have && it >= nb ? 1 : 0, b = have ? it - e * nb : 0;
        const bool winner = have && b == (e ? idx1 : idx0);
        if (winner) sClip[e] = clip[p];                              // (one item per end)
        for (int q = 0; q < 2; ++q) {
            const int second = wave_min_i32(have && !winner && e == q ? dist[p] : NONE);
            if ((tid & 63) == 0 && second != NONE) atomicMin(&sSecond[q], second);
        }
    }
    __syncthreads();
    if (tid == 0) {
        const int idx[2] = {idx0, idx1}, d[2] = {sBest[0] >> 16, sBest[1] >> 16}, s2[2] = {sSecond[0], sSecond[1]};
        const int m[2] = {(int)B.len[idx0], (int)B.len[idx1]};
        int call, bq;
        ccsx_bc_read_call(d, s2, m, B.opts, &call, &bq);
        out.tested[z] = 1; out.call[z] = call; out.bq[z] = bq;
        for (int e = 0; e < 2; ++e) { out.idx[2 * z + e] = idx[e]; out.dist[2 * z + e] = d[e]; out.second[2 * z + e] = s2[e]; out.clip[2 * z + e] = sClip[e]; }
    }
}

}  // namespace

const char *ccsx_barcode_launch(const BarcodeParams &B, hipStream_t st)
{
    if (B.n <= 0) return nullptr;
    hipLaunchKernelGGL(k_barcode, dim3((unsigned)B.n), dim3(NT), 0, st, B);
    return hipGetLastError() != hipSuccess ? "k_barcode" : nullptr;
}

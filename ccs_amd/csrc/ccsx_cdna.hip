// ccsx_cdna.hip — full-length cDNA reads on final reads (DESIGN.md §2 "cDNA rule", §4 "k_cdna").  The rule itself is cdna_core.h over barcode_core.h and
// segment_core.h; this file is its layout on the device.  Integers only; no byte of the report depends on the launch geometry, on the order of the lanes or on
// scheduling: the atomics are LDS integer minima and one LDS integer add whose sum alone is used.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ccsx.h"
#include "cdna_core.h"
#include "wave_ops.h"

namespace {

constexpr int NT = CCSX_CDNA_THREADS, CH = CCSX_SEGMENT_CHUNK;
constexpr int NONE = 0x7fffffff;
static_assert(2 * CCSX_CDNA_MAX_PRIMERS <= NT, "the (end, primer) items are one pass of the workgroup");

// ---- the poly(A) scan of one wave (all 64 lanes): ccsx_cd_polya, 64 positions a round.  Lane l of round k0 holds position k = k0 + l + 1; its running score is
// the carried sum plus a prefix sum, the running maximum the carried maximum joined with a prefix maximum of the scores.  The stop is the first lane of a 64-bit
// ballot; the lanes before it are the round's candidates: the maximum over them stands in the last one, and when it exceeds the carried maximum the first lane
// that holds it (a second ballot) is the new arg-max, else the earlier one stays: the smallest k wins a tie.  The wave leaves at the round that holds the stop.
// x(k): position k is A, asked for 1 <= k <= K only.
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

// ---- k_cdna: one 256-thread workgroup per read.
// Phase A, the ends (k_barcode's layout): both windows sit in LDS as bytes, end 1 already reverse-complemented.  An item is (end e, primer b), numbered
// e * P + b: at most 128, one pass.  An item is one 64-bit word walked serially over its window (ccsx_bc_walk), masks and column in registers.  Per end the best
// primer is the LDS minimum of ccsx_bc_key; after a barrier the winner leaves its clip and every other item joins the runner-up's minimum.  Every thread then
// makes the same decision from the LDS words (ccsx_cd_orient); a read at which the rule ends there is written and left by the whole workgroup.
// Phase B, the poly(A): wave 0 alone (wave_polya) while the other waves begin phase C, which does not need its result.
// Phase C, the internal hits (k_segment's layout): an item is (chunk of CH read bases, search s of 2 P), lane tid takes the items tid, tid + 256, ...; the lane
// that owns a run closes it, finds the start (ccsx_sg_start) and, if the hit lies inside the insert, adds one to the count and joins the minimum of the starts.
// Thread 0 makes the class and the slice and writes the [n] planes, threads 0 and 1 the [n][2] planes of their end.
// Reads: seq[seq_off[z] + (0 .. L - 1)], masks[0 .. 16 P), len / role[0 .. P); writes: the read's own report words only.
__global__ __launch_bounds__(NT) void k_cdna(CdnaParams D)
{
    __shared__ uint8_t sWin[2][CCSX_BARCODE_MAX_WINDOW];
    __shared__ int sBest[2], sSecond[2], sClip[2], sPolya, sCount, sFirst;
    const int tid = threadIdx.x, z = blockIdx.x;
    if (z >= D.n) return;
    const CdnaOut out = ccsx_cd_out(D.rep, (size_t)D.n);
    const int L = D.seq_len[z];
    if (L <= 0) {                                                    // untested
        if (tid == 0) ccsx_cd_put_untested(out, (size_t)z);
        return;
    }
    const int W = min(L, min(D.opts.window, CCSX_BARCODE_MAX_WINDOW)), P = D.n_primers;
    const uint8_t *c = D.seq + D.seq_off[z];
    for (int j = tid; j < W; j += NT) { sWin[0][j] = (uint8_t)ccsx_bc_base(c, L, 0, j); sWin[1][j] = (uint8_t)ccsx_bc_base(c, L, 1, j); }
    if (tid < 2) { sBest[tid] = NONE; sSecond[tid] = 255; sClip[tid] = 0; }
    if (tid == 0) { sPolya = 0; sCount = 0; sFirst = NONE; }
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
    if (tid < 2) ccsx_cd_put_end(out, (size_t)z, tid, sBest[tid] & 0xffff, sBest[tid] >> 16, sSecond[tid], sClip[tid]);
    const CdnaEnds ends{{sBest[0] & 0xffff, sBest[1] & 0xffff}, {sBest[0] >> 16, sBest[1] >> 16}, {sSecond[0], sSecond[1]}, {sClip[0], sClip[1]}};   // (never indexed by a lane: registers)
    CdnaRead r;
    int ins_len;
    if (!ccsx_cd_orient(ends, D.len, D.role, L, D.opts, &r, &ins_len)) {   // (the same in every thread)
        if (tid == 0) ccsx_cd_put_read(out, (size_t)z, 1, r);
        return;
    }
    const auto base = [&](int j) { return (int)(c[j] & 3); };
    if (tid < 64) {
        const int len = wave_polya(ccsx_cd_polya_k(ins_len, D.opts), D.opts, tid,
                                   [&](int k) { return ccsx_cd_is_a(r.strand, L, ends.clip[0], ends.clip[1], k, base); });
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
            if (!ccsx_cd_internal(start, end, L, ends.clip[0], ends.clip[1])) return;
            atomicAdd(&sCount, 1);
            atomicMin(&sFirst, start);
        });
    }
    __syncthreads();
    if (tid == 0) {
        r.polya_len = sPolya; r.n_internal = sCount; r.first_internal = sCount ? sFirst : -1;
        ccsx_cd_finish(&r, ends, L, ins_len, D.opts);
        ccsx_cd_put_read(out, (size_t)z, 1, r);
    }
}

}  // namespace

const char *ccsx_cdna_launch(const CdnaParams &D, hipStream_t st)
{
    if (D.n <= 0) return nullptr;
    hipLaunchKernelGGL(k_cdna, dim3((unsigned)D.n), dim3(NT), 0, st, D);
    return hipGetLastError() != hipSuccess ? "k_cdna" : nullptr;
}

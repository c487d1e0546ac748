// ccsx_train.hip — k_train: the E-step of the model training on the device (DESIGN.md §2 "Model training", §4).
//
// A pair is (window of a ZMW, pass); its rule is train_core.h, the code ccsx_train_pair_host runs cell by cell.  Here one wave64 fills a pair: lane = read
// row (n <= 63 makes rows 0 .. n one wave), an anti-diagonal sweep of n + J + 1 steps with lane i on column t - i.  alpha(i-1, .) comes from the lane below
// through one DPP wave shift, beta(i+1, .) from the lane above; both matrices go to LDS as [column][lane] (2 x 8 KB), so that after the gate — which needs
// alpha(n,J) AND beta(0,0), i.e. both sweeps finished — the three posteriors of every core cell are formed from LDS by the lane that owns the row.  The
// fixed-point values are added with 64-bit LDS integer atomics into the workgroup's [16][12] + [16][12] + [16] table; a one-wave workgroup walks TR_WG_WIN
// consecutive windows of the compact window order and flushes the table's non-zero entries with 64-bit global atomics when the ZMW changes and at its end.
// Integer sums only: the result does not depend on which workgroup or launch piece a pair ran in (float atomics would make it depend on arrival order).
// Flush traffic: <= 400 entries x 8 B per (workgroup, ZMW) — with 8 windows per workgroup an eighth of what a flush per window would send.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ccsx_kernels.h"
#include "train_core.h"
#include "wave_ops.h"

#define TR_WG_WIN 8                   // consecutive windows per workgroup

__device__ __forceinline__ int tr_obs_of(int base, int pw) { const int b = pw < 1 ? 1 : (pw > 3 ? 3 : pw); return (base & 3) * 3 + (b - 1); }

__global__ __launch_bounds__(64) void k_train(KParams P, long long group0)
{
    __shared__ float sA[32 * 64], sB[32 * 64];                // alpha / beta of the pair: [column][row]
    __shared__ unsigned long long sTab[CCSX_TR_NTAB + 1];     // match, stay, del of the current ZMW; [400] = loglik
    __shared__ int sCnt[4];                                   // n_pairs, n_gated, n_bases of the current ZMW
    __shared__ float sME[CCSX_NCTX * CCSX_NOBS], sINS[CCSX_NCTX * CCSX_NOBS], sDL[CCSX_NCTX], sZP[32];
    __shared__ int sK[2][32];                                 // [strand][column]: 12 x the column's context
    __shared__ float sDLc[2][32];                             // ... its deletion weight
    __shared__ float sZS[4];                                  // z-score sums of the window template: M fwd, V fwd, M rev, V rev
    const int lane = (int)threadIdx.x;
    const int nwin_all = P.wstart[P.n_zmw];
    const long long k0 = ((long long)blockIdx.x + group0) * TR_WG_WIN;
    if (k0 >= nwin_all) return;
    for (int q = lane; q <= CCSX_TR_NTAB; q += 64) sTab[q] = 0ull;
    if (lane < 4) sCnt[lane] = 0;
    const int maxins = P.opts.max_insertion_size == 0 ? 30 : P.opts.max_insertion_size;
    const float min_z = P.opts.min_zscore;
    int zcur = -1;

    // the table and the counters of ZMW z go out (non-zero entries only) and are cleared, each entry by the lane that read it
    auto flush = [&](int z) {
        unsigned long long *tab = (unsigned long long *)(P.train_tab + (size_t)z * CCSX_TR_NTAB);
        for (int q = lane; q < CCSX_TR_NTAB; q += 64) {
            const unsigned long long v = sTab[q];
            if (v) { atomicAdd(tab + q, v); sTab[q] = 0ull; }
        }
        if (lane == 0) {
            const unsigned long long ll = sTab[CCSX_TR_NTAB];
            if (ll) { atomicAdd((unsigned long long *)(P.train_ll + z), ll); sTab[CCSX_TR_NTAB] = 0ull; }
        }
        if (lane < 3) {
            const int c = sCnt[lane];
            if (c) { atomicAdd(P.train_zi + (size_t)lane * P.n_zmw + z, c); sCnt[lane] = 0; }
        }
    };

    for (int kk = 0; kk < TR_WG_WIN; ++kk) {
        const long long kl = k0 + kk;
        if (kl >= nwin_all) break;
        const int k = (int)kl;
        const int z = P.wslot_zmw[k];
        __syncthreads();                                      // the window before is done with the tables and the table
        if (z != zcur) {
            if (zcur >= 0) flush(zcur);
            zcur = z;
            for (int q = lane; q < CCSX_NCTX * CCSX_NOBS; q += 64) { sME[q] = P.tabME[(size_t)z * 192 + q]; sINS[q] = P.tabINS[(size_t)z * 192 + q]; }
            if (lane < CCSX_NCTX) sDL[lane] = P.tabDL[(size_t)z * 16 + lane];
            if (lane < 32) sZP[lane] = P.tabZ[(size_t)z * 32 + lane];
        }
        // ---- the window: k_polish's own (template draft[ws, we), flanks, core, the two entry rows)
        const int nw = P.nwin[z], Ld = P.draft_len[z], w = k - P.wstart[z];
        if (P.zstat[z] != CCSX_SUCCESS || w < 0 || w >= nw) continue;
        const int32_t *wb = P.wbounds + P.wb_off[z];
        const uint8_t *draft = P.draft + P.seq_off[z];
        const int wb0 = wb[w], wb1 = wb[w + 1];
        int ws = wb0 - CCSX_WIN_OVERHANG; if (ws < 0) ws = 0;
        int we = wb1 + CCSX_WIN_OVERHANG; if (we > Ld) we = Ld;
        const int J = we - ws;
        if (J < 1 || J > CCSX_JMAX) continue;                // (uniform: no window the polish can hold is left out)
        const int cs = wb0 - ws, ce = wb1 - ws;
        const int iws = (w == 0) ? 0 : 2 * w - 1, iwe = (w == nw - 1) ? 2 * nw - 1 : 2 * (w + 1);
        const int lf = ws > 0 ? (draft[ws - 1] & 3) : 4, rf = we < Ld ? (draft[we] & 3) : 4;
        const int r0 = P.read_off[z], nreads = P.nreads_used[z];
        const int fl0 = P.flags[r0 + (P.zref[z] & 255)] & 1;
        __syncthreads();                                      // (the ZMW's tables are in LDS)
        if (lane < J) {
            const int t = draft[ws + lane] & 3, tp = lane > 0 ? (draft[ws + lane - 1] & 3) : lf;
            const int kf = ccsx_tr_ctx(tp, t);
            sK[0][lane] = kf * CCSX_NOBS; sDLc[0][lane] = sDL[kf];
            // reverse strand: column j of the reverse complement = 3 - draft[we - 1 - j], its left flank the complement of the right one
            const int tr = 3 - (draft[we - 1 - lane] & 3), trp = lane > 0 ? 3 - (draft[we - lane] & 3) : (rf < 4 ? 3 - rf : 4);
            const int kr = ccsx_tr_ctx(trp, tr);
            sK[1][lane] = kr * CCSX_NOBS; sDLc[1][lane] = sDL[kr];
        }
        __syncthreads();
        if (min_z != 0.0f && lane < 2) {                      // the z-score sums of both strands, in column order
            float M = 0.0f, V = 0.0f;
            for (int j = 0; j < J; ++j) { const int kc = sK[lane][j] / CCSX_NOBS; M = M + sZP[kc]; V = V + sZP[16 + kc]; }
            sZS[2 * lane] = M; sZS[2 * lane + 1] = V;
        }
        __syncthreads();

        for (int p = 0; p < nreads; ++p) {
            const int r = r0 + p;
            if (!P.avalid[r]) continue;
            const int64_t eo = P.ent_off[r], bo = P.base_off[r];
            const int L = (int)(P.base_off[r + 1] - bo);
            const int a = P.ent[eo + iws], b = P.ent[eo + iwe], n = b - a;
            if (n < 0 || n > CCSX_IMAX || n > L) continue;
            if (maxins > 0 && n > J + maxins) continue;      // a segment the polish would trim is not a sample of the model
            const int st = ((P.flags[r] & 1) != fl0) ? 1 : 0;
            const int na = st ? L - b : a;
            if (na < 0 || na + n > L) continue;              // (entry rows are rows of this pass)
            int oi = 0;
            if (lane < n) oi = tr_obs_of(P.bases[bo + na + lane], P.pw[bo + na + lane]);
            const int om = wave_shr1_i32(oi, 0);              // o_{i-1}
            const int *Kc = sK[st];
            const float *DLc = sDLc[st];
            const bool row = lane <= n;
            // ---- alpha: step t, lane i on column t - i
            {
                float cur = 0.0f, diag = 0.0f;
                for (int t = 0; t <= n + J; ++t) {
                    const int j = t - lane;
                    const float up = wave_shr1_f32_z(cur);    // alpha(i-1, j): the lane below, one step ago
                    float v = 0.0f;
                    if (row && j >= 0 && j <= J) {
                        float g = (j == 0 && lane == 0) ? 1.0f : 0.0f;
                        if (j > 0) g = ccsx_tr_gamma(cur, DLc[j - 1], diag, sME[Kc[j - 1] + om]);
                        v = j < J ? ccsx_tr_alpha(up, sINS[Kc[j] + om], g) : g;
                        sA[j * 64 + lane] = v;
                    }
                    diag = up; cur = v;
                }
            }
            // ---- beta: the same sweep backwards
            {
                float cur = 0.0f, diag = 0.0f;
                for (int t = n + J; t >= 0; --t) {
                    const int j = t - lane;
                    const float dn = wave_shl1_f32_z(cur);    // beta(i+1, j): the lane above, one step ago
                    float v = 0.0f;
                    if (row && j >= 0 && j <= J) {
                        if (j == J) v = lane == n ? 1.0f : 0.0f;
                        else v = ccsx_tr_beta(DLc[j], cur, sINS[Kc[j] + oi], dn, sME[Kc[j] + oi], diag);
                        if (j < 32) sB[j * 64 + lane] = v;
                    }
                    diag = dn; cur = v;
                }
            }
            __syncthreads();
            const float aL = sA[J * 64 + n], b00 = sB[0];
            float la = 0.0f;
            const int ok = ccsx_tr_gate(aL, b00, n, min_z, sZS[2 * st], sZS[2 * st + 1], &la);
            if (ok) {
                const float inv = ccsx_tr_div(1.0f, aL);
                const int c0 = st ? J - ce : cs, c1 = st ? J - cs : ce;
                if (row) for (int j = c0; j < c1; ++j) {
                    const float al = sA[j * 64 + lane];
                    const int kc = Kc[j];
                    if (lane < n) {
                        const int e = kc + oi;
                        const int64_t m = ccsx_tr_fix(ccsx_tr_post(al, sME[e], sB[(j + 1) * 64 + lane + 1], inv));
                        const int64_t s = ccsx_tr_fix(ccsx_tr_post(al, sINS[e], sB[j * 64 + lane + 1], inv));
                        if (m) atomicAdd(&sTab[e], (unsigned long long)m);
                        if (s) atomicAdd(&sTab[CCSX_TR_STAY + e], (unsigned long long)s);
                    }
                    const int64_t d = ccsx_tr_fix(ccsx_tr_post(al, DLc[j], sB[(j + 1) * 64 + lane], inv));
                    if (d) atomicAdd(&sTab[CCSX_TR_DEL + kc / CCSX_NOBS], (unsigned long long)d);
                }
                if (lane == 0) {
                    sTab[CCSX_TR_NTAB] += (unsigned long long)ccsx_tr_loglik_fix(la, n);   // (two's complement: the sum is the signed sum)
                    sCnt[0] += 1; sCnt[2] += n;
                }
            } else if (lane == 0) sCnt[1] += 1;
            __syncthreads();                                  // sA / sB are free for the next pair
        }
    }
    __syncthreads();
    if (zcur >= 0) flush(zcur);
}

// The training stage of a CCSX_RUN_TRAIN batch on `st`: the slot's count buffers zeroed, then k_train over the window slots in groups of TR_WG_WIN, in launch
// pieces of at most max_blocks workgroups.  NULL, or the name of the call that failed.
const char *ccsx_train_launch(const KParams &P, hipStream_t st, long long max_blocks)
{
    if (!P.train_tab || !P.train_ll || !P.train_zi) return "k_train (no count buffers)";
    const size_t n = (size_t)(P.n_zmw > 0 ? P.n_zmw : 0);
    if (hipMemsetAsync(P.train_tab, 0, n * CCSX_TR_NTAB * 8, st) != hipSuccess) return "hipMemsetAsync";
    if (hipMemsetAsync(P.train_ll, 0, n * 8, st) != hipSuccess) return "hipMemsetAsync";
    if (hipMemsetAsync(P.train_zi, 0, n * 3 * 4, st) != hipSuccess) return "hipMemsetAsync";
    const long long groups = (P.total_wslots + TR_WG_WIN - 1) / TR_WG_WIN;
    if (max_blocks < 1) max_blocks = 1;
    for (long long g0 = 0; g0 < groups; g0 += max_blocks) {
        const long long nb = groups - g0 < max_blocks ? groups - g0 : max_blocks;
        hipLaunchKernelGGL(k_train, dim3((unsigned)nb), dim3(64), 0, st, P, g0);
        if (hipGetLastError() != hipSuccess) return "k_train";
    }
    return nullptr;
}

// train_core.h — the counting rule of the model training (DESIGN.md §2 "Model training"), one statement for the host and the device.
//
// A pair = (window of a ZMW, pass).  The full (n + 1) x (J + 1) forward and backward matrices of the pass's segment against the window template are filled with
// the SPEC v8 recurrences (no band), the pair is gated, and the posterior probability of every match, stay and deletion event of the core columns is converted
// once to 2^-32 fixed point and summed as an integer.  What is here:
//   - the per-ZMW tables as k_setup leaves them (ccsx_tr_tables_ctx: its arithmetic, operation for operation; every translation unit that includes this header
//     is compiled with -ffp-contract=off, so host and device agree bit for bit);
//   - the cell formulas, the gate and the fixed-point conversion (CCSX_TR_HD inlines: k_train in ccsx_train.hip and the host share them);
//   - ccsx_tr_pair_host: one pair on the calling thread, cell by cell (the body of ccsx_train_pair_host; k_train's sweep visits the same cells in another order,
//     and a cell's value depends on its three inputs only).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "ccsx.h"

#if defined(__HIPCC__)
#define CCSX_TR_HD __host__ __device__
#else
#define CCSX_TR_HD
#endif

#define CCSX_TR_TINY   1e-30f   /* alpha(n,J) and beta(0,0) of a counted pair lie above it */
#define CCSX_TR_AB_TOL 0.01f    /* ... and their log2 agree within it                      */
#define CCSX_TR_NTAB   400      /* int64 words of a ZMW's table: match[16][12], stay[16][12], del[16] */
#define CCSX_TR_STAY   192
#define CCSX_TR_DEL    384

// ---- float arithmetic both sides evaluate alike: IEEE division, one fused multiply-add, bit casts
CCSX_TR_HD inline float ccsx_tr_div(float a, float b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(a, b);
#else
    return a / b;
#endif
}
CCSX_TR_HD inline uint32_t ccsx_tr_bits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }
CCSX_TR_HD inline float ccsx_tr_float(uint32_t u) { float x; memcpy(&x, &u, 4); return x; }

// det_log2f of ccsx_kernels.hip (DESIGN.md §SPEC "det math"), restated
CCSX_TR_HD inline float ccsx_tr_log2(float x)
{
    const uint32_t u = ccsx_tr_bits(x);
    if ((int32_t)u < 0x00800000) return -127.0f;
    int e = (int)(u >> 23) - 127;
    float f = ccsx_tr_float((u & 0x007fffffu) | 0x3f800000u);
    if (f > 1.41421356f) { f = f * 0.5f; e = e + 1; }
    const float t = f - 1.0f;
    const float s = ccsx_tr_div(t, 2.0f + t);
    const float z = s * s;
    float p = z * 0.111111111f;
    p = p + 0.142857143f;
    p = p * z;
    p = p + 0.2f;
    p = p * z;
    p = p + 0.333333333f;
    p = p * z;
    p = p + 1.0f;
    const float ln = (2.0f * s) * p;
    return (float)e + ln * 1.44269504f;
}

CCSX_TR_HD inline int ccsx_tr_ctx(int prev, int cur) { if (prev > 3) prev = (cur + 2) & 3; return prev * 4 + cur; }

// ---- the per-ZMW tables: context k of k_setup, the x4 range shift included
struct ccsx_tr_tables {
    float ME[CCSX_NCTX * CCSX_NOBS], INS[CCSX_NCTX * CCSX_NOBS], DL[CCSX_NCTX];
    float MU[CCSX_NCTX], VAR[CCSX_NCTX];     /* z-score parameters (tabZ) */
};

CCSX_TR_HD inline void ccsx_tr_tables_ctx(const ccsx_model *m, const float snr[4], int k, ccsx_tr_tables *T)
{
    const int cur = k & 3;
    float s = snr[cur];
    if (s < m->snr_lo) s = m->snr_lo;
    if (s > m->snr_hi) s = m->snr_hi;
    float w[3];
    for (int mv = 0; mv < 3; ++mv) {
        const float *c = m->trans_poly[k][mv];
        float t = c[3] * s;
        t = t + c[2];
        t = t * s;
        t = t + c[1];
        t = t * s;
        t = t + c[0];
        if (t < 1e-6f) t = 1e-6f;
        w[mv] = t;
    }
    float den = 1.0f + w[0];
    den = den + w[1];
    den = den + w[2];
    const float pM = ccsx_tr_div(1.0f, den), pB = ccsx_tr_div(w[0], den), pS = ccsx_tr_div(w[1], den), pD = ccsx_tr_div(w[2], den);
    for (int o = 0; o < CCSX_NOBS; ++o) {
        const int b = o / 3, pwb = o % 3;
        T->ME[k * CCSX_NOBS + o] = (pM * m->em_match[k][o]) * 4.0f;
        if (b == cur) T->INS[k * CCSX_NOBS + o] = (pB * m->em_branch[k][pwb]) * 4.0f;
        else          T->INS[k * CCSX_NOBS + o] = ((pS * m->em_stick[k][pwb]) * 0.333333333f) * 4.0f;
    }
    T->DL[k] = pD;
    const float pA = pM + pD, pI = pB + pS;
    const float lM = ccsx_tr_log2(pM), lD = ccsx_tr_log2(pD), lB = ccsx_tr_log2(pB), lS = ccsx_tr_log2(pS * 0.333333333f);
    float e1m = 0.0f, e2m = 0.0f, e1b = 0.0f, e2b = 0.0f, e1s = 0.0f, e2s = 0.0f;
    for (int o = 0; o < CCSX_NOBS; ++o) { const float p = m->em_match[k][o], l = ccsx_tr_log2(p), t = p * l; e1m = e1m + t; e2m = e2m + t * l; }
    for (int b = 0; b < 3; ++b) { const float p = m->em_branch[k][b], l = ccsx_tr_log2(p), t = p * l; e1b = e1b + t; e2b = e2b + t * l; }
    for (int b = 0; b < 3; ++b) { const float p = m->em_stick[k][b], l = ccsx_tr_log2(p), t = p * l; e1s = e1s + t; e2s = e2s + t * l; }
    const float a1 = ccsx_tr_div(pM * (lM + e1m) + pD * lD, pA);
    const float a2 = ccsx_tr_div(pM * ((lM * lM + (2.0f * lM) * e1m) + e2m) + pD * (lD * lD), pA);
    const float s1 = ccsx_tr_div(pB * (lB + e1b) + pS * (lS + e1s), pI);
    const float s2 = ccsx_tr_div(pB * ((lB * lB + (2.0f * lB) * e1b) + e2b) + pS * ((lS * lS + (2.0f * lS) * e1s) + e2s), pI);
    const float vA = a2 - a1 * a1, vS = s2 - s1 * s1;
    const float EN = ccsx_tr_div(pI, pA), VN = ccsx_tr_div(pI, pA * pA);
    T->MU[k] = EN * s1 + a1;
    T->VAR[k] = (EN * vS + VN * (s1 * s1)) + vA;
}

// ---- the cells (SPEC v8).  g0 of column 0: 1 for row 0, else 0.  A neighbour outside the matrix is an exact 0, so its term adds nothing.
CCSX_TR_HD inline float ccsx_tr_gamma(float left, float dl, float diag, float me) { return fmaf(left, dl, diag * me); }
CCSX_TR_HD inline float ccsx_tr_alpha(float up, float ins, float gamma) { return fmaf(up, ins, gamma); }                /* not in column J: alpha = gamma there */
CCSX_TR_HD inline float ccsx_tr_beta(float dl, float right, float ins, float down, float me, float diag) { return fmaf(dl, right, fmaf(ins, down, me * diag)); }
// an event's posterior: ((alpha . transition) . beta) . inv, inv = 1 / alpha(n,J)
CCSX_TR_HD inline float ccsx_tr_post(float a, float p, float b, float inv) { return ((a * p) * b) * inv; }
CCSX_TR_HD inline int64_t ccsx_tr_fix(float x) { return (int64_t)floor((double)x * 4294967296.0 + 0.5); }
CCSX_TR_HD inline int64_t ccsx_tr_loglik_fix(float log2_alpha, int n) { return (int64_t)floor(((double)log2_alpha - 2.0 * (double)n) * 65536.0 + 0.5); }

// the gate: 1 = counted (log2 alpha(n,J) in *la).  M, V: the window template's z-score sums on the pass's strand, in column order (min_zscore != 0 only)
CCSX_TR_HD inline int ccsx_tr_gate(float aL, float b0, int n, float min_zscore, float M, float V, float *la)
{
    if (!(aL > CCSX_TR_TINY && b0 > CCSX_TR_TINY)) return 0;
    const float l = ccsx_tr_log2(aL), lb = ccsx_tr_log2(b0);
    float df = l - lb; if (df < 0.0f) df = -df;
    if (df > CCSX_TR_AB_TOL) return 0;
    if (min_zscore != 0.0f) {
        const float zd = (l - (float)(2 * n)) - M;
        if (zd < 0.0f && zd * zd > (min_zscore * min_zscore) * V) return 0;
    }
    *la = l;
    return 1;
}

// ---- one pair on the host.  tpl: the window template in the pass's orientation, J columns, left_flank 0..3 or 4 = none, core [cs, ce); obs: n codes 0..11.
// Adds to match[192], stay[192], del[16], *loglik; 1 counted, 0 gated.  The arguments are the caller's to check (ccsx_train_pair_host does).
inline int ccsx_tr_pair_host(const ccsx_tr_tables &T, const uint8_t *tpl, int J, int left_flank, int cs, int ce, const uint8_t *obs, int n, float min_zscore,
                             int64_t *match, int64_t *stay, int64_t *del, int64_t *loglik)
{
    static_assert(CCSX_JMAX == 31 && CCSX_IMAX == 63, "matrix sizes");
    float A[CCSX_IMAX + 2][CCSX_JMAX + 2], B[CCSX_IMAX + 2][CCSX_JMAX + 2];
    int K[CCSX_JMAX + 1];
    float M = 0.0f, V = 0.0f;
    for (int j = 0; j < J; ++j) {
        K[j] = ccsx_tr_ctx(j > 0 ? tpl[j - 1] : left_flank, tpl[j]);
        M = M + T.MU[K[j]]; V = V + T.VAR[K[j]];
    }
    for (int j = 0; j <= J; ++j)
        for (int i = 0; i <= n; ++i) {
            float g = (i == 0 && j == 0) ? 1.0f : 0.0f;
            if (j > 0) g = ccsx_tr_gamma(A[i][j - 1], T.DL[K[j - 1]], i > 0 ? A[i - 1][j - 1] : 0.0f, i > 0 ? T.ME[K[j - 1] * CCSX_NOBS + obs[i - 1]] : 0.0f);
            A[i][j] = (j < J && i > 0) ? ccsx_tr_alpha(A[i - 1][j], T.INS[K[j] * CCSX_NOBS + obs[i - 1]], g) : g;
        }
    for (int j = J; j >= 0; --j)
        for (int i = n; i >= 0; --i) {
            if (j == J) { B[i][j] = i == n ? 1.0f : 0.0f; continue; }
            const int k = K[j];
            B[i][j] = i < n ? ccsx_tr_beta(T.DL[k], B[i][j + 1], T.INS[k * CCSX_NOBS + obs[i]], B[i + 1][j], T.ME[k * CCSX_NOBS + obs[i]], B[i + 1][j + 1])
                            : ccsx_tr_beta(T.DL[k], B[i][j + 1], 0.0f, 0.0f, 0.0f, 0.0f);
        }
    float la = 0.0f;
    if (!ccsx_tr_gate(A[n][J], B[0][0], n, min_zscore, M, V, &la)) return 0;
    const float inv = ccsx_tr_div(1.0f, A[n][J]);
    for (int j = cs; j < ce; ++j) {
        const int k = K[j];
        for (int i = 0; i <= n; ++i) {
            if (i < n) {
                const int e = k * CCSX_NOBS + obs[i];
                match[e] += ccsx_tr_fix(ccsx_tr_post(A[i][j], T.ME[e], B[i + 1][j + 1], inv));
                stay[e] += ccsx_tr_fix(ccsx_tr_post(A[i][j], T.INS[e], B[i + 1][j], inv));
            }
            del[k] += ccsx_tr_fix(ccsx_tr_post(A[i][j], T.DL[k], B[i][j + 1], inv));
        }
    }
    *loglik += ccsx_tr_loglik_fix(la, n);
    return 1;
}

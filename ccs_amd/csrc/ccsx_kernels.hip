// ccsx_kernels.hip — hand-written gfx950 (CDNA4, wave64) kernels of the CCS per-ZMW consensus hot path.
//
//   k_setup       A0    per-ZMW Arrow parameter tables + z-score parameters              (docs/how-does-ccs-work.md:90-94)
//   k_poa_init    D3    pass selection, backbone chain (cascade pass 2: the draft itself)   (docs/how-does-ccs-work.md:34-51,
//   k_poa_dp      D1/D2 banded POA DP of one pass, FOUR graphs per wave64 (16-lane DPP rows)   docs/faq/accuracy-vs-passes.md:41-46)
//   k_poa_thread  D3    gate, traceback, threading of the pass, column records of the next DP
//   k_poa_finish  D3    heaviest path, draft, window bounds (step 4)
//   k_align16     step3 subread -> draft, 16-row band, FOUR passes per wave; band-saturation trigger (SPEC v5)
//   k_align       step3 the 64-row retry of the alignment cascade                            (docs/how-does-ccs-work.md:53-55)
//   k_rescue      step3/6 split / double-split alignment, partial passes                     (docs/how-does-ccs-work.md:74-78)
//   k_post        A7    per-ZMW usable-pass accounting, draft-cascade marks                  (docs/faq/accuracy-vs-passes.md:37-39)
//   k_wmap(_fill) step4 the batch's windows in compact order (grid map of the polish stage)
//   k_polish      A1-A6 Arrow alpha/beta fill, candidate filter, mutation scoring, polish loop, QVs; one workgroup per window
//                                                                                            (docs/how-does-ccs-work.md:57-61,80-106)
//   k_kinetics    N4    HiFi kinetics of the converged windows                               (docs/faq/kinetics.md:8-18)
//                       and / or the pileup summary (sa sm sx) from the same alignment         (docs/faq/bam-output.md:25-27)
//   k_stitch      step10 concatenate window cores, rq / np / ec, status                      (docs/how-does-ccs-work.md:108-112)
//   k_pile_stitch       the pileup summary's per-base planes (only with a pileup request)
//   k_tile_select / k_tile_scan / k_tile_rows   the polisher hand-off: low-quality tiles as pass-by-column cells (only with a hand-off request)
//                                                                                            (docs/faq/revio.md:28-53)
//
// The arithmetic follows DESIGN.md §SPEC operation by operation (compiled with -ffp-contract=off, no
// fast-math) so that sequences are bit-identical to the CPU restatement.  No MFMA: the recurrences are
// 3-term stencils with data-dependent coefficients.  DP matrices live in LDS (polish) or registers
// (alignment); only the POA keeps score columns in HBM scratch because its DAG is irregular.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstdio>
#include <cstdlib>

#include "ccsx.h"
#include "ccsx_kernels.h"
#include "wave_ops.h"

// gfx950 counts global STORES in vmcnt like loads, and the counter retires in order: a wait for one load drains every store issued before it.  The compiler
// waits for a load at its first use; when a RARE branch loads a value that is used after the join, that wait sits on the common path and every
// iteration stalls until the stores of the previous iteration have been acknowledged (k_poa_dp: two such waits per column).  LANDED(x) makes x
// "used" right where it is written, so the wait stays inside the rare branch and the common path keeps its stores in flight.
#define LANDED(x) asm volatile("" : "+v"(x))

// ---- experiment switches (timing studies of DESIGN.md §8; every one of them computes WRONG results).  They compile only together with -DCCSX_EXPERIMENT,
// which the library reports through ccsx_build_flags() and which turns ccsx_spec_version() negative, so that such a build cannot pass for the product
// (tests/test_abi.py; tools/gpu_ab.sh adds the define itself).
#if (defined(CCSX_EXP_NO_FILL) || defined(CCSX_EXP_NO_SCORE) || defined(CCSX_EXP_ONE_ROUND) || defined(CCSX_EXP_ALL_VALID) || defined(CCSX_EXP_CHEAP_VALIDITY) || \
     defined(CCSX_EXP_NO_ROWS) || defined(CCSX_EXP_NO_SCORE_LOG) || defined(CCSX_EXP_SKIP_ROUND2_SCORE) || defined(CCSX_EXP_NO_QV_EXP) || defined(CCSX_EXP_REPEAT) || defined(CCSX_EXP_NO_BANDMASK) || \
     defined(CCSX_EXP_HOT_PROLOGUE) || defined(CCSX_EXIT_AFTER_PROLOGUE)) && !defined(CCSX_EXPERIMENT)
#error "CCSX_EXP_* / CCSX_EXIT_AFTER_PROLOGUE switches produce wrong results: build them with -DCCSX_EXPERIMENT (never ship such a library)"
#endif
#define CCSX_STR2(x) #x
#define CCSX_STR(x) CCSX_STR2(x)
int ccsx_kernel_is_experiment()
{
#ifdef CCSX_EXPERIMENT
    return 1;
#else
    return 0;
#endif
}
const char *ccsx_kernel_build_flags()
{
    return ""
#ifdef CCSX_EXPERIMENT
        " CCSX_EXPERIMENT"
#endif
#ifdef CCSX_EXP_NO_FILL
        " CCSX_EXP_NO_FILL"
#endif
#ifdef CCSX_EXP_NO_SCORE
        " CCSX_EXP_NO_SCORE"
#endif
#ifdef CCSX_EXP_ONE_ROUND
        " CCSX_EXP_ONE_ROUND"
#endif
#ifdef CCSX_EXP_ALL_VALID
        " CCSX_EXP_ALL_VALID"
#endif
#ifdef CCSX_EXP_CHEAP_VALIDITY
        " CCSX_EXP_CHEAP_VALIDITY"
#endif
#ifdef CCSX_EXP_NO_ROWS
        " CCSX_EXP_NO_ROWS"
#endif
#ifdef CCSX_EXP_NO_SCORE_LOG
        " CCSX_EXP_NO_SCORE_LOG"
#endif
#ifdef CCSX_EXP_SKIP_ROUND2_SCORE
        " CCSX_EXP_SKIP_ROUND2_SCORE"
#endif
#ifdef CCSX_EXP_NO_QV_EXP
        " CCSX_EXP_NO_QV_EXP"
#endif
#ifdef CCSX_EXP_NO_BANDMASK
        " CCSX_EXP_NO_BANDMASK"
#endif
#ifdef CCSX_EXP_HOT_PROLOGUE
        " CCSX_EXP_HOT_PROLOGUE"
#endif
#ifdef CCSX_EXP_REPEAT
        " CCSX_EXP_REPEAT=" CCSX_STR(CCSX_EXP_REPEAT)
#endif
#ifdef CCSX_EXIT_AFTER_PROLOGUE
        " CCSX_EXIT_AFTER_PROLOGUE"
#endif
#ifdef CCSX_PROFILE_PHASES
        " CCSX_PROFILE_PHASES"
#endif
#ifdef CCSX_DEBUG_CHECKS
        " CCSX_DEBUG_CHECKS"
#endif
#ifdef CCSX_EXTRA_FLAGS_STR                                  // (__graft_entry__.build(): whatever $CCSX_EXTRA_FLAGS held, e.g. tuning overrides of the PW_* defaults)
        " extra: " CCSX_EXTRA_FLAGS_STR
#endif
        ;
}
#define LANES 64
#define PW_MAXREADS_SPEC CCSX_MAX_PASSES      // passes of a ZMW the engine uses (k_polish / k_kinetics take them in groups of PW_MAXREADS)
#ifdef CCSX_PROFILE_PHASES
// (round 6: the phase times of wave 0 are summed in LDS (thread 0) and flushed ONCE per workgroup — the first version added a barrier and a global atomic per phase
// boundary, which made the instrumented kernel four times slower and every phase look alike)
#define PHASE_T0() __shared__ unsigned long long sPh[8]; unsigned long long ph_t = __builtin_readcyclecounter(); if (threadIdx.x < 8) sPh[threadIdx.x] = 0ull; (void)ph_t
#define PHASE(idx) do { unsigned long long n_ = __builtin_readcyclecounter(); if (threadIdx.x == 0) sPh[(idx)] += n_ - ph_t; ph_t = n_; } while (0)
#define PHASE_FLUSH() do { if (threadIdx.x == 0 && (blockIdx.x & 63u) == 0u) for (int q_ = 0; q_ < 8; ++q_) atomicAdd((unsigned long long *)P.phase + q_, sPh[q_]); } while (0)   /* one workgroup in 64: millions of atomics on eight addresses are a workload of their own */
#else
#define PHASE_T0() do { } while (0)
#define PHASE(idx) do { } while (0)
#define PHASE_FLUSH() do { } while (0)
#endif
#ifdef CCSX_PROFILE_PHASES                  // one-wave kernels: lane 0's cycle counter between phases, summed over the graphs
#define TPH_T0() unsigned long long tph_t = __builtin_readcyclecounter(); (void)tph_t
#define TPH(idx) do { if (threadIdx.x == 0) { unsigned long long n_ = __builtin_readcyclecounter(); atomicAdd((unsigned long long *)P.phase + (idx), n_ - tph_t); tph_t = n_; } } while (0)
#else
#define TPH_T0() do { } while (0)
#define TPH(idx) do { } while (0)
#endif
#ifdef CCSX_DEBUG_CHECKS
#ifndef CCSX_CHK_MASK
#define CCSX_CHK_MASK 0xff
#endif
#define CHK(cond, code) do { if (((CCSX_CHK_MASK >> ((code) - 101)) & 1) && !(cond)) { if (atomicCAS(P.debug, 0, (code)) == 0) { P.debug[1] = __LINE__; } return; } } while (0)
#else
#define CHK(cond, code) do { } while (0)
#endif
#define NEGV (-(1 << 28))
#define SC_MATCH 3
#define SC_MISMATCH (-5)
#define SC_INS (-4)
#define SC_DEL (-4)
#define MV_DIAG 0
#define MV_DEL 1
#define MV_INS 2
#define MUT_EPS 0.01f
#define MUT_SEP 5
#define MULTI_ROUNDS 2
#define JMIN_DEL 4
#define AB_TOL 0.01f
#define TINY_P 1e-30f
#define SKIP_MARGIN 6
#define SKIP_SPREAD 3
#define SCORE_BAND 5                  // SPEC: half width (read rows) of the mutation scoring band around the window diagonal
// (SPEC v7 / ABI v6: the smallest per-base error probability that is reported — also for a position the candidate filter skips — is P.perr_floor = 10^(-opts.max_qv/10),
// 1e-5 = Q50 by default: nothing measured supports a higher claim; max_qv 93 = the reference's documented range)
#define REP_NP0 10                    // SPEC v8: a CLOSED tract's floor (both ends inside the visible template) is scaled by (REP_NP0 / passes used)^2 beyond REP_NP0 passes
#define REP_ERRS 0.2f                 // SPEC v7 "repeat-count floor": a core base inside a period-p tandem tract of L >= REP_MINLEN(p) visible bases reports p_err >= REP_ERRS / L
#define FILL_MARGIN 2                 // SPEC v6 "banded fill": alpha / beta exist on the diagonals j - i in [min(0, J - I) - (Wr + 2), max(0, J - I) + (Wr + 2)] only
#define DQ_SCALE 65536.0f
#define DQ_CLAMP 100.0f

// ------------------------------------------------------------------------------------------------
// deterministic log2 / exp2 (DESIGN.md §SPEC "det math"): only +, *, / (IEEE, correctly rounded) and bit ops
__device__ __forceinline__ float det_log2f(float x)
{
    uint32_t u = __float_as_uint(x);
    if ((int32_t)u < 0x00800000) return -127.0f;
    int e = (int)(u >> 23) - 127;
    float f = __uint_as_float((u & 0x007fffffu) | 0x3f800000u);
    if (f > 1.41421356f) { f = f * 0.5f; e = e + 1; }
    float t = f - 1.0f;
    float s = __fdiv_rn(t, 2.0f + t);
    float z = s * s;
    float p = z * 0.111111111f;
    p = p + 0.142857143f;
    p = p * z;
    p = p + 0.2f;
    p = p * z;
    p = p + 0.333333333f;
    p = p * z;
    p = p + 1.0f;
    float ln = (2.0f * s) * p;
    return (float)e + ln * 1.44269504f;
}

__device__ __forceinline__ float det_exp2f(float x)
{
    if (x < -125.0f) x = -125.0f;
    if (x > 60.0f) x = 60.0f;
    float n = floorf(x + 0.5f);
    float f = (x - n) * 0.693147181f;
    float p = f * 1.98412698e-4f;
    p = p + 1.38888889e-3f;
    p = p * f;
    p = p + 8.33333333e-3f;
    p = p * f;
    p = p + 4.16666667e-2f;
    p = p * f;
    p = p + 0.166666667f;
    p = p * f;
    p = p + 0.5f;
    p = p * f;
    p = p + 1.0f;
    p = p * f;
    p = p + 1.0f;
    int ni = (int)n;
    return p * __uint_as_float((uint32_t)(ni + 127) << 23);
}

__device__ __forceinline__ int ctx_of(int prev, int cur) { if (prev > 3) prev = (cur + 2) & 3; return prev * 4 + cur; }
__device__ __forceinline__ int obs_of(int base, int pw) { int b = pw < 1 ? 1 : (pw > 3 ? 3 : pw); return (base & 3) * 3 + (b - 1); }   // only the low two bits of a base code count

__device__ __forceinline__ int wave_max_i32(int v)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) { int o = __shfl_xor(v, s); v = o > v ? o : v; }
    return v;
}
__device__ __forceinline__ int wave_min_i32(int v)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) { int o = __shfl_xor(v, s); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ float wave_max_f32(float v)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) { float o = __shfl_xor(v, s); v = o > v ? o : v; }
    return v;
}
__device__ __forceinline__ int bcast_i32(int v, int lane) { return __shfl(v, lane); }

// scalar min / max of wave-uniform values (the compiler otherwise moves such chains to the VALU for v_min3 and reads them back)
__device__ __forceinline__ int smin(int a, int b) { int r; asm("s_min_i32 %0, %1, %2" : "=s"(r) : "s"(a), "s"(b) : "scc"); return r; }
__device__ __forceinline__ int smax(int a, int b) { int r; asm("s_max_i32 %0, %1, %2" : "=s"(r) : "s"(a), "s"(b) : "scc"); return r; }
// band placement of a column from scalars (k_align, k_poa's chain step): same arithmetic as band_lo
__device__ __forceinline__ int band_lo_s(int lo_u, int bestrow_u, int hi /* max(I - 63, 0) */)
{
    return smax(smin(smin(smax(bestrow_u + 1 - CCSX_BAND / 2, lo_u), lo_u + 2), hi), 0);
}
__device__ __forceinline__ int band_lo(int lo_u, int bestrow_u, int I)
{
    int lo = bestrow_u + 1 - CCSX_BAND / 2;
    if (lo < lo_u) lo = lo_u;
    if (lo > lo_u + 2) lo = lo_u + 2;
    int hi = I - (CCSX_BAND - 1); if (hi < 0) hi = 0;
    if (lo > hi) lo = hi;
    if (lo < 0) lo = 0;
    return lo;
}

// ------------------------------------------------------------------------------------------------
// A0: per-ZMW parameter tables.  One thread per (zmw, ctx).
__global__ void k_setup(KParams P)
{
    int gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= P.n_zmw * CCSX_NCTX) return;
    int z = gid / CCSX_NCTX, k = gid % CCSX_NCTX;
    const ccsx_model *m = P.model;
    int cur = k & 3;
    float s = P.snr[z * 4 + cur];
    if (s < m->snr_lo) s = m->snr_lo;
    if (s > m->snr_hi) s = m->snr_hi;
    float w[3];
#pragma unroll
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
    float pM = __fdiv_rn(1.0f, den), pB = __fdiv_rn(w[0], den), pS = __fdiv_rn(w[1], den), pD = __fdiv_rn(w[2], den);
    float *ME = P.tabME + (size_t)z * 192, *INS = P.tabINS + (size_t)z * 192;
    for (int o = 0; o < CCSX_NOBS; ++o) {
        int b = o / 3, pwb = o % 3;
        ME[k * CCSX_NOBS + o] = (pM * m->em_match[k][o]) * 4.0f;
        if (b == cur) INS[k * CCSX_NOBS + o] = (pB * m->em_branch[k][pwb]) * 4.0f;
        else          INS[k * CCSX_NOBS + o] = ((pS * m->em_stick[k][pwb]) * 0.333333333f) * 4.0f;
    }
    P.tabDL[(size_t)z * 16 + k] = pD;
    // A7 z-score parameters (SPEC "z-score gate"; oracle orc_zparams, same operation order)
    {
        const float pA = pM + pD, pI = pB + pS;
        const float lM = det_log2f(pM), lD = det_log2f(pD), lB = det_log2f(pB), lS = det_log2f(pS * 0.333333333f);
        float e1m = 0.0f, e2m = 0.0f, e1b = 0.0f, e2b = 0.0f, e1s = 0.0f, e2s = 0.0f;
        for (int o = 0; o < CCSX_NOBS; ++o) { const float p = m->em_match[k][o], l = det_log2f(p), t = p * l; e1m = e1m + t; e2m = e2m + t * l; }
        for (int b = 0; b < 3; ++b) { const float p = m->em_branch[k][b], l = det_log2f(p), t = p * l; e1b = e1b + t; e2b = e2b + t * l; }
        for (int b = 0; b < 3; ++b) { const float p = m->em_stick[k][b], l = det_log2f(p), t = p * l; e1s = e1s + t; e2s = e2s + t * l; }
        const float a1 = __fdiv_rn(pM * (lM + e1m) + pD * lD, pA);
        const float a2 = __fdiv_rn(pM * ((lM * lM + (2.0f * lM) * e1m) + e2m) + pD * (lD * lD), pA);
        const float s1 = __fdiv_rn(pB * (lB + e1b) + pS * (lS + e1s), pI);
        const float s2 = __fdiv_rn(pB * ((lB * lB + (2.0f * lB) * e1b) + e2b) + pS * ((lS * lS + (2.0f * lS) * e1s) + e2s), pI);
        const float vA = a2 - a1 * a1, vS = s2 - s1 * s1;
        const float EN = __fdiv_rn(pI, pA), VN = __fdiv_rn(pI, pA * pA);
        P.tabZ[(size_t)z * 32 + k] = EN * s1 + a1;
        P.tabZ[(size_t)z * 32 + 16 + k] = (EN * vS + VN * (s1 * s1)) + vA;
    }
}

// ------------------------------------------------------------------------------------------------
// packed 2-bit oriented read in LDS (one wave owns it)
// mode bit 0: walk the bytes backwards, bit 1: complement.  0 = as stored, 3 = reverse complement (rev), 1 / 2 = those two read
// from their last base to their first (the reversed half of the split alignment)
// 16 consecutive bases of a read as one packed word.  A load under `if (i < L)` is waited for on the spot, so the plain form (still used for the words
// at the two ends of a read) costs sixteen DEPENDENT memory round trips per word (~ 1.5 us each under load: 0.2 ms per 2048-base chunk of k_poa_dp, with
// the other three graphs of the wave waiting at the barrier).  A word that lies inside the read issues its sixteen byte loads off ONE address
// (immediate offsets) before the first is used: one round trip.
// (NB = byte loads in flight at a time: 16, or 8 where the caller's loop is short of registers)
template <int NB>
__device__ __forceinline__ uint32_t pack16_bases(const uint8_t *bases, int L, int i0, bool backwards, bool complement)
{
    uint32_t v = 0;
    if (NB > 0 && i0 >= 0 && i0 + 15 < L) {
#pragma unroll
        for (int h = 0; h < 16; h += (NB > 0 ? NB : 16)) {
            uint32_t b[NB > 0 ? NB : 1];
            if (backwards) {
                const uint8_t *p = bases + (L - 1 - i0 - h);
#pragma unroll
                for (int k = 0; k < NB; ++k) b[k] = (uint32_t)p[-k];
            } else {
                const uint8_t *p = bases + i0 + h;
#pragma unroll
                for (int k = 0; k < NB; ++k) b[k] = (uint32_t)p[k];
            }
            if (NB < 16) asm volatile("" : "+v"(b[NB - 1]));    // (keeps the second batch from being hoisted above the first batch's use)
#pragma unroll
            for (int k = 0; k < NB; ++k) v |= (b[k] & 3u) << (2 * (h + k));
        }
        if (complement) v = ~v;                                 // 3 - b on every 2-bit field
    } else {
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int i = i0 + k;
            if (i >= 0 && i < L) { uint32_t b = (uint32_t)bases[backwards ? L - 1 - i : i]; if (complement) b = 3u - b; v |= (b & 3u) << (2 * k); }
        }
    }
    return v;
}
__device__ __forceinline__ void load_read_packed_mode(uint32_t *sread, const uint8_t *bases, int L, int mode, int lane)
{
    int nw = (L + 15) >> 4;
    for (int w = lane; w < nw; w += LANES) sread[w] = pack16_bases<16>(bases, L, w << 4, (mode & 1) != 0, (mode & 2) != 0);
}
__device__ __forceinline__ void load_read_packed(uint32_t *sread, const uint8_t *bases, int L, int rev, int lane)
{
    load_read_packed_mode(sread, bases, L, rev ? 3 : 0, lane);
}
// a CH16-base chunk [c0, c0 + CH16) of the oriented read, packed 2 bits per base into sread[0 .. CH16/16] (k_align16 keeps only the
// part of each pass its band can reach in LDS: 0.5 KB instead of the whole pass, so the kernel's occupancy is not LDS-bound)
#define CH16 2048
__device__ __forceinline__ void load_read_chunk(uint32_t *sread, const uint8_t *bases, int L, int rev, int c0, int lane)
{
    for (int w = lane; w <= CH16 / 16; w += LANES) sread[w] = pack16_bases<0>(bases, L, c0 + (w << 4), rev != 0, rev != 0);   // (plain form: k_align16 needs <= 64 VGPRs for its 8 waves per SIMD, which cover the latency)
}
__device__ __forceinline__ int read_base_packed(const uint32_t *sread, int i) { return (int)((sread[i >> 4] >> (2 * (i & 15))) & 3u); }
// the band's next read base, wave-uniform index: 64 packed words (1024 bases) of the read sit in one VGPR, lane = word, loaded
// at a point from which the band cannot advance past the window before the next load (<= 2 rows per column); a column takes
// its word with v_readlane into an SGPR (scalar shift / mask): no LDS access and no vector arithmetic in the column
struct BaseCursor { uint32_t vw; int w0; };
__device__ __forceinline__ void cursor_load(BaseCursor &c, const uint32_t *sread, int nwords, int t0, int lane)
{
    c.w0 = (t0 < 0 ? 0 : t0) >> 4;
    const int wi = c.w0 + lane;
    c.vw = sread[wi < nwords ? wi : (nwords > 0 ? nwords - 1 : 0)];
}
__device__ __forceinline__ int base_at(const BaseCursor &c, int t)
{
    return (int)(((uint32_t)__builtin_amdgcn_readlane((int)c.vw, ((t >> 4) - c.w0) & 63) >> (2 * (t & 15))) & 3u);
}

// ------------------------------------------------------------------------------------------------
// D2/D3: sparse POA (docs/how-does-ccs-work.md:34-51; SPEC: POA_BAND = 32 rows, a pass is threaded only if it passes the gate).
//
// Round 3: the POA is a pipeline of four kernels per threaded pass instead of one wave per graph doing everything —
//   k_poa_init    one wave per graph: pass selection, the backbone chain, the column records of the first DP
//   k_poa_dp      ONE WAVE = FOUR GRAPHS: the banded DP of one pass over four graphs in lockstep.  Each graph owns a 16-lane DPP
//                 row; a lane holds TWO band rows (2l, 2l+1), so the 32-row band's insertion chain is a lane-local step plus a
//                 4-step row scan, and the column maximum / best row one packed 4-step row scan.  Every column a graph finishes
//                 goes into an LDS ring (the last PRING columns + the START column, guard cells on both sides): in-edges read
//                 their source column from there at any band offset with plain ds_reads — no register shifting, no per-column
//                 branch on the edge type; only sources more than PRING positions back come from HBM (flagged by the prepass).
//                 Per column 32 move bytes + one 16-byte record go to HBM (round 2: 64 move bytes + the 256-byte score column
//                 of every column an in-edge skipped to + the record).
//   k_poa_thread  one wave per graph: the gate, traceback, threading of the pass into the graph (wave-parallel list insertion),
//                 and the prepass for the next DP: column records by topological position {base, in-edge count, positions of
//                 in-edges 0..2, "a far in-edge reads this column back"} — round 6: the threading itself produces them (see the layout note below)
//   k_poa_finish  heaviest path, draft, window bounds
// Round 6: a vertex IS its topological position.  Everything is laid out by position: crec {base | in-edges << 8 | flags | passes << 20, positions of
// in-edges 0..2} and px {positions of in-edges 3..6} (both ping-pong: threading a pass writes the next numbering while it reads the current one), kinfo {lo,
// colmax, bestrow, position of in-edge 0} and the move row mvK[32] of the current DP pass, M[32] for the far-read columns.  Until round 5 the graph lived by
// vertex ID (record, overflow in-edges, rank, passes-through) beside two order arrays, and every pass gathered / scattered all of them by id to produce the
// column records of the next DP: 8.5 MB of 4- and 16-byte gathers per ZMW.  Now a pass is threaded by ONE streaming merge: the records of the vertices that
// are not on the pass's path shift to their new positions, the path's elements write theirs (existing: in-edges remapped, passes + 1, the new edge; new: a
// fresh record), and the result IS the next DP's column records.
#define PB CCSX_POA_BAND              // rows of the POA band
#define PRING 8                       // columns of a graph the DP keeps in LDS (+ the START column in slot PRING)
#define PGS 40                        // words per ring column: 4 guards, 32 rows, 4 guards
#define CREC_NEED (1 << 16)            // column record: a far in-edge reads this column back from HBM
#define CREC_FAR0 (1 << 17)            //                in-edge 0 comes from more than PRING positions back
#define CREC_NREADS_SHIFT 20           //                bits 20..26: passes that go through the vertex (k_poa_finish)
enum { ST_N, ST_NADDED, ST_OK, ST_PAR, ST_KEND, ST_BS, ST_NPOA, ST_BB, ST_NREADS, ST_REV0, ST_LIVE, ST_WORDS = 16 };
struct PoaSlot {
    int32_t *st;                      // [ST_WORDS] per-graph state that travels between the kernels
    int4 *kinfo, *crec0, *crec1, *px0, *px1;
    int32_t *M, *bestK, *bpK, *pathv, *loK;
    uint8_t *mvK, *needK, *onpK;
};
#define POA_MV_BYTES (PB / 2)         // a column's moves: one nibble per band row (0..13 = in-edge slot * 2 + [deletion], 15 = insertion)
#define POA_BYTES_PER_VERTEX (PB * 4 + 16 * 5 + POA_MV_BYTES + 3 * 4 + 2)       // = 238 (the host sizes a slot with it: ccsx_kernels.h CCSX_POA_BYTES_PER_VERTEX)
static_assert(POA_BYTES_PER_VERTEX == CCSX_POA_BYTES_PER_VERTEX, "the host's slot size and the kernels' layout disagree");

__device__ __forceinline__ PoaSlot poa_slot(const KParams &P, int slot)
{
    PoaSlot s;
    const size_t vc = (size_t)P.vcap_max + 64;
    uint8_t *p = P.poa_scratch + (size_t)slot * P.poa_slot_bytes;
    s.st = (int32_t *)p;      p += 256;
    s.M = (int32_t *)p;       p += vc * PB * 4;
    s.kinfo = (int4 *)p;      p += vc * 16;
    s.crec0 = (int4 *)p;      p += vc * 16;     // column records, ping-pong (ST_PAR names the current one)
    s.crec1 = (int4 *)p;      p += vc * 16;
    s.px0 = (int4 *)p;        p += vc * 16;     // positions of in-edges 3..6, ping-pong like the records; an entry is meaningful only where the record counts more than three
    s.px1 = (int4 *)p;        p += vc * 16;
    s.mvK = p;                p += vc * POA_MV_BYTES;
    s.bestK = (int32_t *)p;   p += vc * 4;      // also the run-count / shift array while threading a read
    s.bpK = (int32_t *)p;     p += vc * 4;
    s.loK = (int32_t *)p;     p += vc * 4;      // band start of the column in the current DP pass (the traceback's half of kinfo)
    s.needK = p;              p += (vc + 3) & ~(size_t)3;   // 1 = some in-edge reaches this column from more than PRING positions ahead
    s.onpK = p;               p += (vc + 3) & ~(size_t)3;   // (while threading) 1 = the vertex is on the pass's path
    s.pathv = (int32_t *)p;
    return s;
}

__device__ __forceinline__ int imed3(int x, int lo, int hi) { x = x > lo ? x : lo; return x < hi ? x : hi; }   // clamp (v_med3_i32)
__device__ __forceinline__ int rl(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }
__device__ __forceinline__ int rfl(int v) { return __builtin_amdgcn_readfirstlane(v); }

__device__ __forceinline__ int int4_get(const int4 &v, int q) { return q == 0 ? v.x : (q == 1 ? v.y : (q == 2 ? v.z : v.w)); }
__device__ __forceinline__ void int4_set(int4 &v, int q, int x) { if (q == 0) v.x = x; else if (q == 1) v.y = x; else if (q == 2) v.z = x; else v.w = x; }

extern __shared__ uint32_t dyn_lds[];
#define TB_BLOCK 64                   // positions cached per traceback block (64 move rows of 32 bytes)

// zref[z]: bits 0-7 = backbone pass of the current draft, plus the state of the draft cascade (SPEC "fallback draft", "last resort")
#define ZREF_RETRY 256                  // k_post: this ZMW's first draft failed or most passes do not map to it
#define ZREF_DONE 512                   // the fallback draft (pass 1) has been made
#define ZREF_RETRY2 1024                // k_post: the fallback draft failed as well (bits 0-5: its backbone)
#define ZREF_DONE2 2048                 // the last-resort draft (pass 2: the backbone pass itself) has been made
#define ZREF_PASSBIT(pass) ((pass) == 1 ? ZREF_DONE : ZREF_DONE2)

// step 4: window bounds of a draft of Ld bases (one wave); returns the number of windows
__device__ __forceinline__ int poa_windows(const KParams &P, int z, int Ld, int lane)
{
    int nw = 0;
    {
        // step 4 windows.  SPEC: a break nb is bad when for some period p in 1..4 the p-mer before it equals the p-mer
        // after it ("avoid breaking windows at simple repeats", docs/how-does-ccs-work.md:58-60); the target cur+22 moves by
        // 0,+1,-1,+2,-2,+3,-3 to the first good position.  Lane l holds draft[cur+14+l]; E_p = ballot(d[i] == d[i+p]).
        const uint8_t *d = P.draft + P.seq_off[z];
        int32_t *b = P.wbounds + P.wb_off[z];
        int cur = 0;
        if (lane == 0) b[0] = 0;
        while (cur < Ld) {
            int nb;
            if (Ld - cur <= CCSX_WIN_CORE + 6) nb = Ld;
            else {
                const int base = cur + CCSX_WIN_CORE - 8;                 // positions base .. base+15 cover every p-mer examined
                const int pos = base + lane;
                const int x = (lane < 16 && pos < Ld) ? (int)d[pos] : 8 + lane;
                unsigned e[4];
#pragma unroll
                for (int p = 1; p <= 4; ++p) e[p - 1] = (unsigned)__ballot(x == __shfl(x, (lane + p) & 63)) & 0xffffu;
                nb = cur + CCSX_WIN_CORE;
                const int offs[7] = {0, 1, -1, 2, -2, 3, -3};
#pragma unroll
                for (int k = 6; k >= 0; --k) {                            // last assignment wins: scan the preference order backwards
                    const int c = 8 + offs[k];                            // bit index of the candidate break
                    bool bad = false;
#pragma unroll
                    for (int p = 1; p <= 4; ++p) bad |= ((e[p - 1] >> (c - p)) & ((1u << p) - 1u)) == ((1u << p) - 1u);
                    if (!bad) nb = cur + CCSX_WIN_CORE + offs[k];
                }
            }
            ++nw;
            if (lane == 0) b[nw] = nb;
            cur = nb;
        }
    }
    return nw;
}

// ---- k_poa_init: which passes, the backbone chain, the first column records.  One wave per graph (slot = block).
__global__ __launch_bounds__(64) void k_poa_init(KParams P, int z0, int pass, int b0)
{
    const int bx = (int)blockIdx.x + b0;                // (b0: the launch's first workgroup — the POA stage runs as two half-batches on two streams)
    const int lane = threadIdx.x;
    uint32_t *sread = dyn_lds;
    PoaSlot g = poa_slot(P, bx);
    if (z0 + bx >= P.n_zmw) return;
    const int z = rfl(P.zmw_perm[z0 + bx]);     // longest ZMWs first
    if (lane < ST_WORDS) g.st[lane] = 0;                // (ST_LIVE = 0: the other kernels skip this graph unless it is set below)
    __threadfence_block();
    const int r0 = rfl(P.read_off[z]);
    int nreads = rfl(P.read_off[z + 1]) - r0;
    {   // SPEC v5: at most CCSX_MAX_PASSES = 255 passes are used (--top-passes 0 = all of them)
        const int top = ccsx_top_passes(P.opts.top_passes);
        if (nreads > top) nreads = top;
    }
    // SPEC "partial passes" (flag bit 1; they follow the ZMW's full-length passes): not in the draft, not counted as passes
    const int nall = nreads;
    {
        int nf = 0;
        for (int b0 = 0; b0 < nall; b0 += LANES) nf += __popcll(__ballot(b0 + lane < nall && !(P.flags[r0 + (b0 + lane < nall ? b0 + lane : 0)] & 2)));
        nreads = rfl(nf);
    }
    // SPEC "fallback draft" (docs/faq/accuracy-vs-passes.md:41-46: a cascade from fast to robust draft generators): pass 1
    // (only for ZMWs k_post marked) takes the pass whose length is closest to the median as backbone and threads twice as
    // many passes, starting at the backbone and wrapping around
    // SPEC "last resort" (pass 2, only for ZMWs whose fallback draft failed too): the pass closest to the median among the passes
    // that have not been a backbone yet is the draft itself, no POA; the polish repairs its errors
    int bb = 0;
    if (pass >= 1) {
        const int zr = rfl(P.zref[z]);
        if (!(zr & (pass == 1 ? ZREF_RETRY : ZREF_RETRY2))) return;
        const int bb1 = pass == 2 ? (zr & 255) : -1;
        // up to CCSX_MAX_PASSES = 255 full-length passes: their lengths go to LDS, a lane ranks the passes lane, lane + 64, ...
        int32_t *slen = (int32_t *)sread;
        for (int q = lane; q < nreads; q += LANES) slen[q] = (int)(P.base_off[r0 + q + 1] - P.base_off[r0 + q]);
        __syncthreads();
        int medl = 0x7fffffff;                          // the length whose rank (ties by index) is nreads / 2
        for (int i = lane; i < nreads; i += LANES) {
            const int len = slen[i];
            int rank = 0;
            for (int q = 0; q < nreads; ++q) { const int lq = slen[q]; rank += (lq < len || (lq == len && q < i)) ? 1 : 0; }
            if (rank == nreads / 2) medl = len;
        }
        const int med = rfl(wave_min_i32(medl));
        int key = 0x7fffffff;
        for (int i = lane; i < nreads; i += LANES) {
            int dist = slen[i] - med; dist = dist < 0 ? -dist : dist;
            const bool cand = !(pass == 2 && ((i == bb1 && nreads > 1) || (i == 0 && nreads > 2)));   // not a backbone that failed
            const int k = ((dist > 0x3fffff ? 0x3fffff : dist) << 8) | i;
            if (cand && k < key) key = k;
        }
        bb = rfl(wave_min_i32(key)) & 255;
        __syncthreads();                                // (sread is loaded with the backbone below)
    }
    if (lane == 0) { P.nreads_used[z] = nall; P.nfull[z] = nreads; P.draft_len[z] = 0; P.nwin[z] = 0; P.zref[z] = bb | (pass ? ZREF_PASSBIT(pass) : 0); }
    // a new draft invalidates the partial passes' alignments of the previous generator (k_align16 resets the full-length passes it
    // realigns; the partial ones are aligned by k_rescue, which only looks at passes that are not valid)
    for (int q = nreads + lane; q < nall; q += LANES) { P.avalid[r0 + q] = 0; P.ascore[r0 + q] = NEGV; }
    const bool enough = !(nreads < P.opts.min_passes || nreads < 1);
    if (!enough) { if (lane == 0) P.zstat[z] = CCSX_TOO_FEW_PASSES; return; }
    const int cov = pass ? 2 * P.opts.max_poa_cov : P.opts.max_poa_cov;
    const int npoa = nreads < cov ? nreads : cov;
    const int vcap = rfl(P.vcap[z]);
    const int rev0 = rfl(P.flags[r0 + bb] & 1);
    const int r = r0 + bb;
    const uint8_t *rb = P.bases + P.base_off[r];
    const int I = rfl((int)(P.base_off[r + 1] - P.base_off[r]));
    if (pass == 2) {                                    // the backbone pass is the draft
        int Ld = I <= P.dcap[z] ? I : 0, nw = 0, stat = -1;
        uint8_t *draft = P.draft + P.seq_off[z];
        for (int q = lane; q < Ld; q += LANES) draft[q] = rb[q] & 3;
        __threadfence_block();
        if (Ld <= 0) stat = CCSX_DRAFT_FAILURE;
        else if (Ld < P.opts.min_length) stat = CCSX_TOO_SHORT;
        else if (Ld > P.opts.max_length) stat = CCSX_TOO_LONG;
        else nw = poa_windows(P, z, Ld, lane);
        if (lane == 0) { P.draft_len[z] = Ld; P.nwin[z] = (stat < 0) ? nw : 0; P.zstat[z] = (stat < 0) ? CCSX_SUCCESS : stat; }
        return;
    }
    load_read_packed(sread, rb, I, 0, lane);
    __syncthreads();
    int ok = 1, n = 0;
    if (I > vcap) ok = 0;
    else {                                              // first read: backbone chain; its column records are trivial
        for (int i = lane; i < I; i += LANES) {
            const int b = read_base_packed(sread, i);
            g.crec0[i] = make_int4(b | ((i > 0 ? 1 : 0) << 8) | (1 << CREC_NREADS_SHIFT), i - 1, -1, -1);
            g.needK[i] = 0;                               // (a chain has no far in-edge)
        }
        n = I;
    }
    __threadfence_block();
    if (lane == 0) {
        g.st[ST_N] = n; g.st[ST_NADDED] = 1; g.st[ST_OK] = ok; g.st[ST_PAR] = 0; g.st[ST_KEND] = -1; g.st[ST_BS] = NEGV;
        g.st[ST_NPOA] = npoa; g.st[ST_BB] = bb; g.st[ST_NREADS] = nreads; g.st[ST_REV0] = rev0; g.st[ST_LIVE] = 1;
    }
}

// ---- k_draft_in: the polish seam (ccsx_polish_batch, docs/img/ccs-impl.png "Polish Stage" fed by a host-side draft generator; docs/faq/revio.md:35-53: Arrow
// run again for QVs on a sequence made elsewhere).  The caller's drafts are in P.draft already; one wave per ZMW sets what the draft generators leave behind:
// passes used / full-length passes, the orientation reference, status by length, window bounds.  No cascade follows: the alignment's outcome is final.
__global__ __launch_bounds__(64) void k_draft_in(KParams P)
{
    const int lane = threadIdx.x, z = blockIdx.x;
    if (z >= P.n_zmw) return;
    const int r0 = rfl(P.read_off[z]);
    int nreads = rfl(P.read_off[z + 1]) - r0;
    {
        const int top = ccsx_top_passes(P.opts.top_passes);
        if (nreads > top) nreads = top;
    }
    const int nall = nreads;
    {
        int nf = 0;
        for (int b0 = 0; b0 < nall; b0 += LANES) nf += __popcll(__ballot(b0 + lane < nall && !(P.flags[r0 + (b0 + lane < nall ? b0 + lane : 0)] & 2)));
        nreads = rfl(nf);
    }
    int bb = rfl(P.din_bb[z]);
    if (bb < 0 || bb >= (nall > 0 ? nall : 1)) bb = 0;
    int Ld = rfl(P.din_len[z]);
    if (Ld < 0 || Ld > P.dcap[z]) Ld = 0;                  // (a draft that does not fit its slot is no draft)
    int stat = -1, nw = 0;
    if (nreads < P.opts.min_passes || nreads < 1) stat = CCSX_TOO_FEW_PASSES;
    else if (Ld <= 0) stat = CCSX_DRAFT_FAILURE;
    else if (Ld < P.opts.min_length) stat = CCSX_TOO_SHORT;
    else if (Ld > P.opts.max_length) stat = CCSX_TOO_LONG;
    uint8_t *draft = P.draft + P.seq_off[z];
    for (int q = lane; q < Ld; q += LANES) draft[q] = draft[q] & 3;     // only the low two bits of a base code count, as for the subreads
    __threadfence_block();
    if (stat < 0) nw = poa_windows(P, z, Ld, lane);
    for (int q = lane; q < nall; q += LANES) { P.avalid[r0 + q] = 0; P.ascore[r0 + q] = NEGV; }
    if (lane == 0) {
        P.nreads_used[z] = nall; P.nfull[z] = nreads; P.zref[z] = bb;
        P.draft_len[z] = (stat == CCSX_TOO_FEW_PASSES) ? 0 : Ld; P.nwin[z] = (stat < 0) ? nw : 0; P.zstat[z] = (stat < 0) ? CCSX_SUCCESS : stat;
    }
}

// a CH16-base chunk of the oriented read for one 16-lane group, packed 2 bits per base, shifted by ONE base: word w holds the bases
// c0 - 1 + 16 w .. (index -1 = a dummy), so that the base of row i - 1 for row i = c0 + x sits at packed position x
__device__ __forceinline__ void load_read_chunk_m1(uint32_t *sread, const uint8_t *bases, int L, int rev, int c0, int l16)
{
    for (int w = l16; w <= CH16 / 16 + 1; w += 16) sread[w] = pack16_bases<8>(bases, L, c0 - 1 + (w << 4), rev != 0, rev != 0);
}

// ---- k_poa_dp: the banded DP of pass rr over FOUR graphs per wave (see the header of this section)
// (branch layout: a taken branch costs the wave ~ 20 cycles of instruction fetch and this kernel runs two waves per SIMD, so the conditions of the rare blocks
// below carry __builtin_expect(., 0) — the blocks move out of line and the common column falls through.  The "two or more in-edges" blocks (43 % of the
// wave's columns) carry none: either hint measured slower, profiles/r04_poa_dp_vmcnt.txt)
__global__ __launch_bounds__(64) void k_poa_dp(KParams P, int z0, int pass, int rr, int b0)
{
    const int bx = (int)blockIdx.x + b0;                // (b0: the launch's first workgroup — the POA stage runs as two half-batches on two streams)
    __shared__ __attribute__((aligned(16))) int32_t sRing[4][PRING + 1][PGS];
    __shared__ __attribute__((aligned(16))) int4 sKin[4][PRING + 1];
    __shared__ __attribute__((aligned(16))) int4 sCrec[4][16];
    __shared__ uint32_t sRead[4][CH16 / 16 + 2];
    const int lane = threadIdx.x, gq = lane >> 4, l = lane & 15;
    const int zi = z0 + 4 * bx + gq;
    const bool have = zi < P.n_zmw && 4 * bx + gq < P.poa_slots;
    const PoaSlot G = poa_slot(P, have ? 4 * bx + gq : 4 * bx);   // per lane, uniform inside a 16-lane group
    int32_t *st = G.st;
    int32_t *Mcol = G.M;
    int4 *kinfo = G.kinfo;
    const int par_ = have ? st[ST_PAR] : 0;
    const int4 *crec = par_ ? G.crec1 : G.crec0;        // the current numbering's column records / overflow in-edges (ST_PAR)
    const int32_t *pxw = (const int32_t *)(par_ ? G.px1 : G.px0);
    const uint8_t *needK = G.needK;
    uint8_t *mvK = G.mvK;
    bool live = have && st[ST_LIVE] && st[ST_OK] && rr < st[ST_NPOA];
    if (!__any(live)) return;
    const int z = have ? P.zmw_perm[zi] : 0;
    const int r0 = P.read_off[z];
    const int n0 = live ? st[ST_N] : 0;
    int I = 0, rev = 0;
    const uint8_t *rb = P.bases;
    if (live) {
        const int bb = st[ST_BB], nr = st[ST_NREADS];
        const int r = r0 + (bb + rr < nr ? bb + rr : bb + rr - nr);
        rb = P.bases + P.base_off[r];
        I = (int)(P.base_off[r + 1] - P.base_off[r]);
        rev = ((P.flags[r] & 1) != st[ST_REV0]) ? 1 : 0;
    }
    // ---- LDS: guards and unused cells = NEGV, the START column M[l] = l * INS (l <= I), its record (lo 0, colmax 0, best row 0)
    for (int e = l; e < (PRING + 1) * PGS; e += 16) (&sRing[gq][0][0])[e] = NEGV;
    __syncthreads();
    sRing[gq][PRING][4 + 2 * l] = (2 * l <= I) ? 2 * l * SC_INS : NEGV;
    sRing[gq][PRING][5 + 2 * l] = (2 * l + 1 <= I) ? (2 * l + 1) * SC_INS : NEGV;
    if (l == 0) sKin[gq][PRING] = make_int4(0, 0, 0, 0);
    int c0 = 0;                                         // first base of the group's read chunk in LDS
    load_read_chunk_m1(sRead[gq], rb, I, rev, 0, l);
    __syncthreads();
    const int hiI = I - (PB - 1) > 0 ? I - (PB - 1) : 0;
    const int nmax = wave_max_i32(n0);
    int bs = NEGV, kend = -1;
    // per-lane constants of the column step
    const int l2 = 2 * l, l8 = 8 * l;
    const int kRow0 = 63 - 2 * l, kRow1 = 62 - 2 * l;
    typedef int32_t __attribute__((address_space(3))) *lds_i32;
    const uint32_t ringBase = (uint32_t)(uintptr_t)(lds_i32)&sRing[gq][0][0];      // 32-bit LDS addresses
    const uint32_t readBase = (uint32_t)(uintptr_t)(lds_i32)(int32_t *)&sRead[gq][0];
    const int bcastAddr = (lane | 15) << 2;                                        // ds_bpermute: the row's last lane
    // running per-lane output pointers (one 64-bit add per column instead of an index multiply)
    uint8_t *mvp = mvK + l;                             // one byte per lane and column: the nibbles of rows 2l and 2l+1
    int4 *kip = kinfo;
    int32_t *lop = G.loK;
    int32_t *Mp = Mcol + 2 * l;
    int4 recN = make_int4(0, -1, -1, -1);               // the NEXT block of 16 column records (lane l: column kb + 16 + l) and its
    int needN = 0;                                      // "a far in-edge reads this column" byte: merged at the hand-off, 16 columns after the loads were issued
    recN = crec[l < n0 ? l : 0];                        // (unconditional, clamped, masked at the hand-off: a load under a lane mask is copied into the
    needN = needK[l < n0 ? l : 0];                      //  loop-carried register at once, i.e. waited for)
#define LDS_I32(addr) (*(lds_i32)(uintptr_t)(addr))
    // wave masks of per-lane conditions straight from the compare (a bool that goes through ballot costs two extra VALU ops)
#define M_NE0(a) __builtin_amdgcn_uicmp((unsigned)(a), 0u, 33)
#define M_SLT(a, b) __builtin_amdgcn_sicmp((int)(a), (int)(b), 40)
#define M_SGT(a, b) __builtin_amdgcn_sicmp((int)(a), (int)(b), 38)
#define M_UGT(a, b) __builtin_amdgcn_uicmp((unsigned)(a), (unsigned)(b), 34)
    const uint32_t kinBase = (uint32_t)(uintptr_t)(lds_i32)(int32_t *)&sKin[gq][0];
    const unsigned long long livem = M_NE0(live ? 1 : 0);
    for (int k = 0; k < nmax; ++k, mvp += POA_MV_BYTES, ++kip, ++lop, Mp += PB) {
        if (__builtin_expect((k & 15) == 0, 0)) {       // hand the prefetched block to LDS, start fetching the one after it
            { int4 r = recN; if (needN) r.x |= CREC_NEED; sCrec[gq][l] = (k + l < n0) ? r : make_int4(0, -1, -1, -1); }
            { const int kn = k + 16 + l < n0 ? k + 16 + l : 0; recN = crec[kn]; needN = needK[kn]; }
            __syncthreads();
        }
        const unsigned long long actm = livem & M_SLT(k, n0);
        const int4 rec = sCrec[gq][k & 15];
        const int vb = rec.x & 3;
        const int p0 = rec.y;
        const unsigned long long multim = actm & M_NE0(rec.x & 0xe00);         // two or more in-edges
        const unsigned long long far0m = actm & M_NE0(rec.x & CREC_FAR0);      // in-edge 0 comes from more than PRING positions back
        // ---- band placement: from the in-edge column with the largest column maximum (first on ties); START for a source
        const uint32_t slot0 = p0 < 0 ? PRING : (uint32_t)(p0 & (PRING - 1));
        int k0x, k0y, k0z;
        { const uint32_t ka = kinBase + slot0 * 16; k0x = LDS_I32(ka); k0y = LDS_I32(ka + 4); k0z = LDS_I32(ka + 8); }
        if (__builtin_expect(far0m != 0ull, 0)) { if (rec.x & CREC_FAR0) { const int4 t = kinfo[p0]; k0x = t.x; k0y = t.y; k0z = t.z; } LANDED(k0x); LANDED(k0y); LANDED(k0z); }
        int ulo = k0x, ubr = k0z;
        int plo1 = 0, plo2 = 0;
        if (multim) {
            const int np = (rec.x >> 8) & 15;
            const bool act = live && k < n0;
            int bestcm = k0y;
            for (int q = 1; q < CCSX_MAXPRED; ++q) {
                if ((actm & M_SGT(np, q)) == 0ull) break;
                int pq = q == 1 ? rec.z : rec.w;
                if (q >= 3) {                           // in-edges 3..6 (rare): the overflow record of the column
                    if (act && np > q) pq = pxw[(size_t)k * 4 + (q - 3)];
                    LANDED(pq);
                }
                const bool on = act && np > q;
                const bool farq = on && k - pq > PRING;
                const uint32_t ka = kinBase + (on ? (uint32_t)(pq & (PRING - 1)) : (uint32_t)PRING) * 16;
                int qx = LDS_I32(ka), qy = LDS_I32(ka + 4), qz = LDS_I32(ka + 8);
                if (__builtin_expect(M_NE0(farq ? 1 : 0) != 0ull, 0)) { if (farq) { const int4 t = kinfo[pq]; qx = t.x; qy = t.y; qz = t.z; } LANDED(qx); LANDED(qy); LANDED(qz); }
                if (q == 1) plo1 = qx; else if (q == 2) plo2 = qx;
                if (on && qy > bestcm) { bestcm = qy; ulo = qx; ubr = qz; }
            }
        }
        int lo = imed3(ubr + (1 - PB / 2), ulo, ulo + 2);                        // clamp(best row + 1 - 16, ulo, ulo + 2)
        lo = lo < hiI ? lo : hiI;
        lo = lo > 0 ? lo : 0;
        // ---- the read bases of rows r0 - 1 and r0 (r0 = lo + 2l): the chunk follows the band
        if (__builtin_expect((actm & M_UGT(lo - c0, CH16 - PB - 2)) != 0ull, 0)) {
            __syncthreads();
            if (live && k < n0 && (unsigned)(lo - c0) > (unsigned)(CH16 - PB - 2)) {
                c0 = lo - 128 > 0 ? lo - 128 : 0;
                load_read_chunk_m1(sRead[gq], rb, I, rev, c0, l);
            }
            __syncthreads();
        }
        const int r0w = lo + l2;
        int s0, s1;
        {
            const uint32_t idx = (uint32_t)(r0w - c0) & (CH16 - 1);              // (inactive groups: any in-range index)
            const uint32_t wa = readBase + ((idx >> 4) << 2);
            const uint32_t wlo = (uint32_t)LDS_I32(wa), whi = (uint32_t)LDS_I32(wa + 4);
            const uint32_t t = __builtin_amdgcn_alignbit(whi, wlo, (idx & 15u) << 1);
            s0 = (vb == (int)(t & 3u)) ? SC_MATCH : SC_MISMATCH;
            s1 = (vb == (int)((t >> 2) & 3u)) ? SC_MATCH : SC_MISMATCH;
        }
        // ---- in-edge 0 (or START): diagonal then deletion; three consecutive rows of the source column at the band offset
        int b0, b1, m0, m1;
        {
            const int w = imed3(r0w - k0x + 3, 1, PGS - 3);   // word of row (r0 - plo) - 1 behind the 4 guard words
            const uint32_t src = ringBase + slot0 * (PGS * 4) + ((uint32_t)w << 2);
            int x0 = LDS_I32(src), y0 = LDS_I32(src + 4), y1 = LDS_I32(src + 8);
            if (__builtin_expect(far0m != 0ull, 0)) {
                if (rec.x & CREC_FAR0) {                // the source column comes from HBM
                    const int32_t *Mu = Mcol + (size_t)p0 * PB;
                    const int o = r0w - k0x - 1;
                    x0 = (unsigned)o < (unsigned)PB ? Mu[o] : NEGV;
                    y0 = (unsigned)(o + 1) < (unsigned)PB ? Mu[o + 1] : NEGV;
                    y1 = (unsigned)(o + 2) < (unsigned)PB ? Mu[o + 2] : NEGV;
                }
                LANDED(x0); LANDED(y0); LANDED(y1);
            }
            const int d0 = x0 + s0, e0 = y0 + SC_DEL, d1 = y0 + s1, e1 = y1 + SC_DEL;
            const bool t0 = e0 > d0, t1 = e1 > d1;              // move codes (a nibble): in-edge slot * 2 + [deletion], 15 = insertion
            b0 = t0 ? e0 : d0; m0 = t0 ? 1 : 0;
            b1 = t1 ? e1 : d1; m1 = t1 ? 1 : 0;
        }
        if (multim) {                                    // further in-edges, in list order: a later candidate wins only if strictly greater
            const int np = (rec.x >> 8) & 15;
            const bool act = live && k < n0;
            for (int q = 1; q < CCSX_MAXPRED; ++q) {
                if ((actm & M_SGT(np, q)) == 0ull) break;
                const bool on = act && np > q;
                int pq = q == 1 ? rec.z : rec.w, plo = q == 1 ? plo1 : plo2;
                if (q >= 3) {
                    if (on) {
                        pq = pxw[(size_t)k * 4 + (q - 3)];
                        if (k - pq > PRING) plo = kinfo[pq].x; else plo = LDS_I32(kinBase + (uint32_t)(pq & (PRING - 1)) * 16);
                    }
                    LANDED(pq); LANDED(plo);
                }
                const bool farq = on && k - pq > PRING;
                const int off = r0w - plo;
                const int w = imed3(off + 3, 1, PGS - 3);
                const uint32_t src = ringBase + (on ? (uint32_t)(pq & (PRING - 1)) : (uint32_t)PRING) * (PGS * 4) + ((uint32_t)w << 2);
                int x0 = LDS_I32(src), y0 = LDS_I32(src + 4), y1 = LDS_I32(src + 8);
                if (__builtin_expect(M_NE0(farq ? 1 : 0) != 0ull, 0)) {
                    if (farq) {
                        const int32_t *Mu = Mcol + (size_t)pq * PB;
                        const int o = off - 1;
                        x0 = (unsigned)o < (unsigned)PB ? Mu[o] : NEGV;
                        y0 = (unsigned)(o + 1) < (unsigned)PB ? Mu[o + 1] : NEGV;
                        y1 = (unsigned)(o + 2) < (unsigned)PB ? Mu[o + 2] : NEGV;
                    }
                    LANDED(x0); LANDED(y0); LANDED(y1);
                }
                const int mq = q << 1;
                int c;
                c = x0 + s0;     if (on && c > b0) { b0 = c; m0 = mq; }
                c = y0 + SC_DEL; if (on && c > b0) { b0 = c; m0 = mq | 1; }
                c = y0 + s1;     if (on && c > b1) { b1 = c; m1 = mq; }
                c = y1 + SC_DEL; if (on && c > b1) { b1 = c; m1 = mq | 1; }
            }
        }
        // ---- insertion chain x_i = max(c_i, x_{i-1} + INS) over the 32 rows: lane-local (row 2l -> 2l+1), an exclusive 4-step
        // row scan of the lanes' outgoing values, then the incoming value applied to both rows
        { const int c = b0 + SC_INS; if (c > b1) { b1 = c; m1 = 15; } }
        {
            const int S = row_scan_max_i32(b1 + l8);
            const int Sp = __builtin_amdgcn_update_dpp(-(1 << 30), S, DPP_ROW_SHR(1), 0xf, 0xf, false);
            const int c0v = Sp - (l8 - 8 - SC_INS);     // (final value of row 2l - 1) + INS ; lane 0: very negative
            const int c1v = Sp - (l8 - 8 - 2 * SC_INS);
            if (c0v > b0) { b0 = c0v; m0 = 15; }
            if (c1v > b1) { b1 = c1v; m1 = 15; }
        }
        if (r0w > I || b0 < NEGV / 2) b0 = NEGV;
        if (r0w >= I || b1 < NEGV / 2) b1 = NEGV;
        // ---- column maximum and the first row that attains it: one packed row scan (value << 6 | 63 - row).  A column without a
        // valid cell reports -2^24 as its maximum (it loses every comparison a valid column takes part in, like the SPEC's NEG)
        int cm, br;
        {
            const int f = -(1 << 24);
            const int k0_ = ((b0 > f ? b0 : f) * 64) | kRow0, k1_ = ((b1 > f ? b1 : f) * 64) | kRow1;
            const int key = row_allmax_i32(k0_ > k1_ ? k0_ : k1_);       // (an all-reduce by row rotations: no ds_bpermute broadcast on the chain that places the next band)
            cm = key >> 6; br = (lo + 63) - (key & 63);
        }
        // ---- the read's last row: best end cell over all columns (first in topological order)
        if (__builtin_expect((actm & M_SGT(lo + PB, I)) != 0ull, 0)) {
            const int e = r0w == I ? b0 : (r0w + 1 == I ? b1 : NEGV);
            const int ev = __builtin_amdgcn_ds_bpermute(bcastAddr, row_scan_max_i32(e));
            if (live && k < n0 && ev > NEGV / 2 && ev > bs) { bs = ev; kend = k; }
        }
        // ---- out: ring (LDS), moves + column record (HBM), the score column if a far in-edge will read it
        if (live && k < n0) {
            *(int2 *)&sRing[gq][k & (PRING - 1)][4 + l2] = make_int2(b0, b1);
            *mvp = (uint8_t)(m0 | (m1 << 4));
            if (l == 0) {
                sKin[gq][k & (PRING - 1)] = make_int4(lo, cm, br, 0);
                *lop = lo;                                  // all the traceback needs of a column (in-edge 0's position is in its record)
            }
            if (__builtin_expect((rec.x & CREC_NEED) != 0, 0)) {   // a far in-edge will read this column back: its scores and its record
                *(int2 *)Mp = make_int2(b0, b1);
                if (l == 0) *kip = make_int4(lo, cm, br, p0);
            }
        }
    }
#undef M_NE0
#undef M_SLT
#undef M_SGT
#undef M_UGT
#undef LDS_I32
    __threadfence_block();
    if (live && l == 0) { st[ST_KEND] = kend; st[ST_BS] = bs; }
}

// ---- k_poa_thread: gate, traceback and threading of pass rr, then the column records of the next DP.  One wave per graph.
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_poa_thread(KParams P, int z0, int pass, int rr, int b0)
{
    const int bx = (int)blockIdx.x + b0;                // (b0: the launch's first workgroup — the POA stage runs as two half-batches on two streams)
    __shared__ __attribute__((aligned(16))) uint8_t sMv[TB_BLOCK * POA_MV_BYTES];   // move rows (a nibble per cell) of the traceback's current block
    const int lane = threadIdx.x;
    uint32_t *sread = dyn_lds;
    PoaSlot g = poa_slot(P, bx);
    if (z0 + bx >= P.n_zmw) return;
    if (!g.st[ST_LIVE] || !g.st[ST_OK] || rr >= g.st[ST_NPOA]) return;
    TPH_T0();
    const int z = rfl(P.zmw_perm[z0 + bx]);
    const int r0 = rfl(P.read_off[z]);
    const int bb = rfl(g.st[ST_BB]), nreads = rfl(g.st[ST_NREADS]), npoa = rfl(g.st[ST_NPOA]);
    const int r = r0 + (bb + rr < nreads ? bb + rr : bb + rr - nreads);
    const uint8_t *rb = P.bases + P.base_off[r];
    const int I = rfl((int)(P.base_off[r + 1] - P.base_off[r]));
    const int kend = rfl(g.st[ST_KEND]), bsc = rfl(g.st[ST_BS]);
    // SPEC "POA gate": a pass is threaded only if its alignment reaches the read's last row with a score of at least 1.0 per base
    // the POA log (ccsx_poa_log; a null pointer otherwise): one record per (ZMW, generator, pass), written by lane 0 wherever the pass ends
    int32_t *const plog = (P.poa_log && pass < 2 && rr < P.poa_log_stride) ? P.poa_log + ((size_t)(2 * z + pass) * P.poa_log_stride + rr) * CCSX_POA_LOG_WORDS : nullptr;
    auto log_pass = [&](int threaded, int nv) { if (plog && lane == 0) { plog[0] = I; plog[1] = bsc; plog[2] = kend; plog[3] = threaded; plog[4] = nv; } };
    if (kend < 0 || bsc < I) { log_pass(0, g.st[ST_N]); return; }
    const int rev = rfl(((P.flags[r] & 1) != g.st[ST_REV0]) ? 1 : 0);
    const int vcap = rfl(P.vcap[z]);
    const int n0 = rfl(g.st[ST_N]);
    const int par = rfl(g.st[ST_PAR]);
    const int4 *crec = par ? g.crec1 : g.crec0, *pxc = par ? g.px1 : g.px0;      // the current numbering ...
    int4 *crec_nx = par ? g.crec0 : g.crec1, *px_nx = par ? g.px0 : g.px1;       // ... and the one this pass writes
    load_read_packed(sread, rb, I, rev, lane);
    __syncthreads();
    TPH(8);
    // ---- traceback: lane 0 walks, the block of TB_BLOCK positions it is in is cached in LDS.  Round 3: the per-position words come
    // from the DP's column record (base, in-edge count and the positions of in-edges 0..2 by position: no vertex-record gather), and
    // the NEXT block (the walk goes down the positions) is fetched into registers while the current one is walked.  Round 6: the path
    // holds POSITIONS (of the current numbering; -1 = a new vertex)
    {
        int k = kend, i = I;
        int4 kiN = make_int4(0, 0, 0, -1), crN = make_int4(0, -1, -1, -1);
        int kbN = -1;
        uint4 mvN0 = make_uint4(0, 0, 0, 0);
        auto fetch = [&](int kb_) {
            const int kk = kb_ + lane;
            kbN = kb_;
            kiN = make_int4(0, 0, 0, -1); crN = make_int4(0, -1, -1, -1);
            if (kb_ >= 0) {
                if (kk < n0) { crN = crec[kk]; kiN = make_int4(g.loK[kk], 0, 0, crN.y); }
                mvN0 = ((const uint4 *)(g.mvK + (size_t)kb_ * POA_MV_BYTES))[lane];     // 64 columns x 16 bytes
            }
        };
        fetch((k / TB_BLOCK) * TB_BLOCK);
        while (k >= 0) {
            const int kb = (k / TB_BLOCK) * TB_BLOCK;
            if (kbN != kb) fetch(kb);                          // (an in-edge that skipped a whole block: rare)
            __syncthreads();
            // block cache: the TB_BLOCK move rows go to LDS, the per-position words (band start, position of in-edge 0,
            // vertex id, record words) stay in lane registers and are handed out with v_readlane
            const int4 kiL = kiN, crL = crN;
            const int metaL = crN.x;
            ((uint4 *)sMv)[lane] = mvN0;
            fetch(kb - TB_BLOCK);                              // in flight while this block is walked
            __syncthreads();
            while (k >= kb) {                                  // uniform walk: every lane follows the same (k, i)
                int kl = k - kb;
                int mknown;                                    // the move of the cell the walk stands on after the run, if a lane has read it already (255: no)
                {
                    // a run of plain DIAG steps along the chain (in-edge 0 is the previous position): lane s tests
                    // step s of the run, one ballot gives its length, the path entries are stored by the lanes
                    const int kls = kl - lane;
                    const int src = kls & 63;
                    const int lo_s = __shfl(kiL.x, src), pp_s = __shfl(kiL.w, src);
                    const int off = i - lane - lo_s;
                    const bool inb = kls >= 0 && i - lane >= 1 && (unsigned)off < (unsigned)PB;
                    const int m_s = inb ? ((sMv[kls * POA_MV_BYTES + (off >> 1)] >> ((off & 1) << 2)) & 15) : 255;
                    const unsigned long long simple = __ballot(m_s == 0 && pp_s == k - lane - 1);
                    const int R = (simple == ~0ull) ? 64 : __ffsll((long long)~simple) - 1;
                    if (R > 0) {
                        const int meta_s = __shfl(metaL, src);
                        if (lane < R) {
                            const int ir = i - lane - 1;
                            g.pathv[ir] = ((meta_s & 3) == read_base_packed(sread, ir)) ? k - lane : -1;
                        }
                        k -= R; i -= R;
                        if (R >= 64 || k < kb) continue;
                        kl = k - kb;
                    }
                    // the cell that ended the run (or the very first one, R = 0) is lane R's cell: its move is in that lane's register already, so the step
                    // below needs neither another detection pass (two ds_bpermute + a byte read + a ballot per run before) nor a second LDS read
                    mknown = rl(m_s, R);
                }
                const int lo_k = rl(kiL.x, kl);
                CHK(i - lo_k >= 0 && i - lo_k < PB && i >= 0, 101);
                const int mo = i - lo_k;
                const int m = mknown != 255 ? mknown : rfl((sMv[kl * POA_MV_BYTES + (mo >> 1)] >> ((mo & 1) << 2)) & 15);
                const int t = m == 15 ? MV_INS : (m & 1), slot = m >> 1;   // (MV_DIAG = 0, MV_DEL = 1)
                CHK(i >= 1 || t == MV_DEL, 102);
                if (t == MV_INS) { if (lane == 0) g.pathv[i - 1] = -1; --i; continue; }
                const int meta = rl(metaL, kl);
                const int np = (meta >> 8) & 15;
                int up;
                if (np == 0) up = -1;
                else if (slot == 0) up = rl(kiL.w, kl);
                else if (slot == 1) up = rl(crL.z, kl);
                else if (slot == 2) up = rl(crL.w, kl);
                else up = rfl(((const int32_t *)pxc)[(size_t)k * 4 + (slot - 3)]);
                if (t == MV_DIAG) {
                    if (lane == 0) g.pathv[i - 1] = ((meta & 3) == read_base_packed(sread, i - 1)) ? k : -1;
                    --i;
                }
                CHK(up < k && up >= -1, 103);
                k = up;
            }
            k = rfl(k); i = rfl(i);
        }
        for (int q = lane; q < i; q += LANES) g.pathv[q] = -1;     // leading insertions at START
    }
    __threadfence_block();
    TPH(9);
    // ---- thread the read into the graph (wave-parallel; identical result to the serial list insertion).  Round 6: ONE streaming merge by position.
    //   A  runs of new vertices: the last element of a run records the run's length at its anchor (the path vertex before it; list head if none), path
    //      vertices are flagged;                                   B  prefix sum: S[q] = how far position q moves to the right;
    //   C  the vertices that are NOT on the path shift (in-edges remapped p -> p + S[p], far flags recomputed);
    //   D  the path's elements write their records at their new positions — an existing vertex: its record remapped, passes + 1, the edge from the path
    //      vertex before it (unless present / the in-edge cap is hit); a new vertex: a fresh record — and that IS the next DP's column records.
    int32_t *cnt = g.bestK;
    // the new position of the vertex at (current) position q; the record of the current numbering at q carried over to the next one
    auto newpos = [&](int q) -> int { return q + cnt[q]; };
    for (int q = lane; q <= n0; q += LANES) { cnt[q] = 0; g.onpK[q] = 0; }
    __threadfence_block();
    TPH(10);
    int lastEx = -1, nnew = 0;
    for (int c0 = 0; c0 < I; c0 += 2 * LANES) {                    // A: run lengths at the anchors, path flags (two blocks of loads in flight)
        int w[2], wn[2], ex[2];
        bool valid[2], isnew[2], lastOfRun[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int i = c0 + u * LANES + lane;
            valid[u] = i < I;
            const int ic = valid[u] ? i : I - 1;
            w[u] = g.pathv[ic];
            wn[u] = g.pathv[ic + 1 < I ? ic + 1 : ic];
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int i = c0 + u * LANES + lane;
            isnew[u] = valid[u] && w[u] < 0;
            nnew += __popcll(__ballot(isnew[u]));
            const int incl = wave_scan_max_i32((valid[u] && !isnew[u]) ? i : -1);
            int e = wave_shr1_i32(incl, -1);
            e = e > lastEx ? e : lastEx;                           // last existing path element before i
            ex[u] = e;
            const int li = rl(incl, 63);
            lastEx = li > lastEx ? li : lastEx;
            lastOfRun[u] = isnew[u] && ((i + 1 >= I) || (wn[u] >= 0));
        }
        int av[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) av[u] = g.pathv[(lastOfRun[u] && ex[u] >= 0) ? ex[u] : 0];     // the anchor's position
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int i = c0 + u * LANES + lane;
            if (valid[u] && !isnew[u]) g.onpK[w[u]] = 1;           // (a vertex is on the path once: one writer)
            if (lastOfRun[u]) {
                const int ap = ex[u] >= 0 ? av[u] : -1;
                CHK(ap >= -1 && ap < n0, 106);
                cnt[ap + 1] = i - ex[u];                           // (distinct runs have distinct anchors: one writer)
            }
        }
    }
    nnew = rfl(nnew);
    if (n0 + nnew > vcap) { if (lane == 0) g.st[ST_OK] = 0; log_pass(0, n0); return; }
    __threadfence_block();
    TPH(11);
    int carry = 0;
    for (int c0 = 0; c0 <= n0; c0 += 4 * LANES) {                  // B: inclusive prefix sum of the run counts
        int cv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { const int q = c0 + u * LANES + lane; cv[u] = cnt[q <= n0 ? q : n0]; }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int q = c0 + u * LANES + lane;
            const int incl = wave_scan_add_i32(q <= n0 ? cv[u] : 0);
            if (q <= n0) cnt[q] = carry + incl;
            carry += rl(incl, 63);
        }
    }
    const int n = n0 + nnew;
    for (int q = lane; q < n; q += LANES) g.needK[q] = 0;
    __threadfence_block();
    // the record at current position q in the next numbering (position kn): in-edges remapped, the far flags of the DP recomputed
    auto carry_over = [&](int q, int kn, int4 rec, int4 &pxr) -> int4 {
        const int np = (rec.x >> 8) & 15;
        rec.x &= ~CREC_FAR0;
        if (np > 0) { rec.y = newpos(rec.y); if (kn - rec.y > PRING) { g.needK[rec.y] = 1; rec.x |= CREC_FAR0; } }
        if (np > 1) { rec.z = newpos(rec.z); if (kn - rec.z > PRING) g.needK[rec.z] = 1; }
        if (np > 2) { rec.w = newpos(rec.w); if (kn - rec.w > PRING) g.needK[rec.w] = 1; }
        if (np > 3) {
            pxr = pxc[q];
            for (int e = 3; e < np; ++e) { const int pn = newpos(int4_get(pxr, e - 3)); int4_set(pxr, e - 3, pn); if (kn - pn > PRING) g.needK[pn] = 1; }
        }
        return rec;
    };
    for (int q0 = 0; q0 < n0; q0 += 2 * LANES) {                   // C: the vertices off the path shift right
        int4 rec[2]; int kn[2]; bool go[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int q = q0 + u * LANES + lane;
            go[u] = q < n0 && !g.onpK[q < n0 ? q : 0];
            rec[u] = make_int4(0, -1, -1, -1); kn[u] = 0;
            if (go[u]) { rec[u] = crec[q]; kn[u] = newpos(q); }
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) if (go[u]) {
            const int q = q0 + u * LANES + lane;
            int4 pxr = make_int4(-1, -1, -1, -1);
            const int4 r = carry_over(q, kn[u], rec[u], pxr);
            CHK(kn[u] >= 0 && kn[u] < n, 105);
            crec_nx[kn[u]] = r;
            if (((r.x >> 8) & 15) > 3) px_nx[kn[u]] = pxr;
        }
    }
    TPH(12);
    lastEx = -1;
    int prevP = -1;                                                // new position of the path element before the block's first one
    for (int c0 = 0; c0 < I; c0 += LANES) {                        // D: the path's elements
        const int i = c0 + lane;
        const bool valid = i < I;
        const int w = g.pathv[valid ? i : I - 1];
        const bool isnew = valid && w < 0;
        const int incl = wave_scan_max_i32((valid && !isnew) ? i : -1);
        int ex = wave_shr1_i32(incl, -1);
        ex = ex > lastEx ? ex : lastEx;
        { const int li = rl(incl, 63); lastEx = li > lastEx ? li : lastEx; }
        const int av = g.pathv[(isnew && ex >= 0) ? ex : 0];       // a new vertex: the position of its run's anchor
        int4 rec = make_int4(0, -1, -1, -1);
        if (valid && !isnew) rec = crec[w];
        const int qa = valid ? (isnew ? (ex >= 0 ? av : 0) : w) : 0;
        int P = newpos(qa);                                        // existing: its own new position; new: the anchor's ...
        if (isnew) P = (ex >= 0 ? P + 1 : 0) + (i - ex - 1);       // ... + its place in the run (list head: the run starts at position 0)
        if (!valid) P = -1;
        int Pp = wave_shr1_i32(P, prevP);                          // new position of the path element before this one (-1: none)
        prevP = rl(P, 63);
        if (valid) {
            CHK(P >= 0 && P < n, 104);
            int4 pxr = make_int4(-1, -1, -1, -1);
            bool pxdirty = false;
            if (isnew) rec = make_int4(read_base_packed(sread, i) | ((Pp >= 0 ? 1 : 0) << 8) | (1 << CREC_NREADS_SHIFT), Pp, -1, -1);
            else {
                rec = carry_over(w, P, rec, pxr);
                rec.x += 1 << CREC_NREADS_SHIFT;                   // one more pass goes through the vertex
                if (Pp >= 0) {                                      // SPEC: the edge is appended unless present or the in-edge cap (7) is hit
                    const int np = (rec.x >> 8) & 15;
                    bool found = false;
                    if (np > 0) found |= rec.y == Pp;
                    if (np > 1) found |= rec.z == Pp;
                    if (np > 2) found |= rec.w == Pp;
                    for (int e = 3; e < np; ++e) found |= int4_get(pxr, e - 3) == Pp;
                    if (!found && np < CCSX_MAXPRED) {
                        if (np == 0) rec.y = Pp; else if (np == 1) rec.z = Pp; else if (np == 2) rec.w = Pp; else { int4_set(pxr, np - 3, Pp); pxdirty = true; }
                        rec.x += 1 << 8;
                        if (P - Pp > PRING) { g.needK[Pp] = 1; if (np == 0) rec.x |= CREC_FAR0; }
                    }
                }
            }
            crec_nx[P] = rec;
            if (((rec.x >> 8) & 15) > 3 || pxdirty) px_nx[P] = pxr;
        }
    }
    __threadfence_block();
    if (lane == 0) { g.st[ST_N] = n; g.st[ST_NADDED] += 1; g.st[ST_PAR] ^= 1; }
    log_pass(1, n);
    (void)npoa;
    TPH(13);
}

// ---- k_poa_finish: consensus (heaviest path), draft, window bounds.  One wave per graph.
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_poa_finish(KParams P, int z0, int pass, int b0)
{
    const int bx = (int)blockIdx.x + b0;                // (b0: the launch's first workgroup — the POA stage runs as two half-batches on two streams)
    const int lane = threadIdx.x;
    PoaSlot g = poa_slot(P, bx);
    if (z0 + bx >= P.n_zmw) return;
    if (!g.st[ST_LIVE]) return;
    const int z = rfl(P.zmw_perm[z0 + bx]);
    const int ok = rfl(g.st[ST_OK]), n = rfl(g.st[ST_N]), nadded = rfl(g.st[ST_NADDED]);
    const int4 *crec = g.st[ST_PAR] ? g.crec1 : g.crec0;
    const int32_t *pxw = (const int32_t *)(g.st[ST_PAR] ? g.px1 : g.px0);
    // ---- consensus: heaviest path (uniform walk).  The column records of the last prepass give every column's base, pass count and the
    // topological positions of its in-edges 0..2 by position: one coalesced load per 64 columns, no order -> vertex record -> rank
    // chain of dependent gathers (round 3; in-edges 3..7 still go through the vertex id)
    int Ld = 0, nw = 0, stat = -1;
    if (ok && n > 0) {
        int kbest = -1, sb = NEGV, best_prev = 0;
        // Forward pass, 64 columns at a time.  Most columns continue a chain (one in-edge, from the position before): along a chain the
        // heaviest-path weight is a prefix sum of the columns' own weights.  So a block needs ONE wave scan of the weights, a serial
        // (wave-uniform) resolution of its chain HEADS only — columns with no / several in-edges or an in-edge from elsewhere —
        // and two ds_bpermute to hand every column its head's value.  Integer arithmetic: the same numbers as the column-by-column walk.
        for (int kb = 0; kb < n; kb += LANES) {
            const int kkL = kb + lane;
            int4 cL = make_int4(0, -1, -1, -1);
            if (kkL < n) cL = crec[kkL];
            const int nblk = (n - kb) < LANES ? (n - kb) : LANES;
            const int npL = (cL.x >> 8) & 15;
            const int wL = kkL < n ? 2 * ((cL.x >> CREC_NREADS_SHIFT) & 127) - nadded : 0;
            const int Pw = wave_scan_add_i32(wL);                                  // inclusive prefix sum of the block's weights
            const bool headL = kkL < n && (lane == 0 || npL != 1 || cL.y != kkL - 1);
            unsigned long long heads = __ballot(headL);
            const unsigned long long headmask = heads;
            int hb = 0, bpv = kkL - 1;                                             // lane h: value / back pointer of head h (chain columns: the position before)
            while (heads) {
                const int j = (int)__ffsll((long long)heads) - 1;
                heads &= heads - 1;
                const int k = kb + j;
                const int np = rl(npL, j);
                int b = 0, p = -1;
                for (int q = 0; q < np; ++q) {
                    int pu;
                    if (q < 3) pu = q == 0 ? rl(cL.y, j) : (q == 1 ? rl(cL.z, j) : rl(cL.w, j));
                    else pu = rfl(pxw[(size_t)k * 4 + (q - 3)]);
                    CHK(pu >= 0 && pu < k, 108);
                    int bu;
                    if (pu >= kb) {                                                // inside the block: its head's value + the weights since
                        const int pj = pu - kb;
                        const int hd = 63 - __clzll((long long)(headmask & ((2ull << pj) - 1ull)));
                        bu = rl(hb, hd) + rl(Pw, pj) - rl(Pw, hd);
                    } else bu = pu == kb - 1 ? best_prev : rfl(g.bestK[pu]);
                    if (bu > b) { b = bu; p = pu; }
                }
                const int bv = b + rl(wL, j);
                if (lane == j) { hb = bv; bpv = p; }
            }
            const int hdL = 63 - __clzll((long long)(headmask & ((2ull << lane) - 1ull)));   // (lanes past the block: any head)
            int myBest = __shfl(hb, hdL) + Pw - __shfl(Pw, hdL);
            // a path never continues from a non-positive value (it starts anew: "b = max(0, ...)"), which breaks the prefix sum of a
            // chain: only where a graph begins or is junk.  Such a block is walked column by column.
            const unsigned long long nonpos = __ballot(kkL < n && myBest <= 0);
            if ((nonpos << 1) & ~headmask & (nblk == 64 ? ~0ull : (1ull << nblk) - 1ull)) {
                int myBp = -1; myBest = 0;
                int bprev = best_prev;
                for (int j = 0; j < nblk; ++j) {
                    const int k = kb + j;
                    const int np = rl(npL, j);
                    int b = 0, p = -1;
                    for (int q = 0; q < np; ++q) {
                        int pu;
                        if (q < 3) pu = q == 0 ? rl(cL.y, j) : (q == 1 ? rl(cL.z, j) : rl(cL.w, j));
                        else pu = rfl(pxw[(size_t)k * 4 + (q - 3)]);
                        const int bu = pu == k - 1 ? bprev : ((pu >= kb) ? rl(myBest, pu - kb) : rfl(g.bestK[pu]));
                        if (bu > b) { b = bu; p = pu; }
                    }
                    const int bv = b + rl(wL, j);
                    if (lane == j) { myBest = bv; myBp = p; }
                    bprev = bv;
                }
                bpv = myBp;
            }
            if (kkL < n) { g.bestK[kkL] = myBest; g.bpK[kkL] = bpv; }
            // the block's maximum, first position on ties (the walk's "bv > sb" in position order)
            const int key = wave_max_i32(kkL < n ? myBest * 64 + (63 - lane) : INT32_MIN);
            const int bmax = key >> 6;
            if (bmax > sb) { sb = bmax; kbest = kb + 63 - (key & 63); }
            best_prev = rl(myBest, nblk - 1);
            __threadfence_block();
        }
        // backtrack (uniform), bases collected in reverse into scratch
        uint8_t *tmp = (uint8_t *)g.pathv;
        int len = 0, k = kbest;
        while (k >= 0) {
            const int kb = (k >> 6) << 6;
            const int kk = kb + lane;
            const int bpL = kk < n ? g.bpK[kk] : -1;
            const int bL = kk < n ? (crec[kk].x & 255) : 0;
            // whole runs per step: `chain` marks the positions whose back pointer is the position before; from kl the path takes every position down to the
            // highest one at or below kl whose bit is clear (t), each lane stores its own base, and the walk continues at t's back pointer (one position per
            // step and a lane-0 store before: ~ 10 k dependent steps per graph)
            const unsigned long long chain = __ballot(kk < n && bpL == kk - 1);
            while (k >= kb) {
                const int kl = k - kb;
                const unsigned long long inv = ~chain & ((2ull << kl) - 1ull);
                const int t = inv ? 63 - __clzll((long long)inv) : 0;
                CHK(len + kl - t < n, 107);
                if (lane >= t && lane <= kl) tmp[len + (kl - lane)] = (uint8_t)bL;
                len += kl - t + 1;
                k = inv ? rl(bpL, t) : kb - 1;
            }
        }
        __threadfence_block();
        if (len <= P.dcap[z]) {
            uint8_t *draft = P.draft + P.seq_off[z];
            for (int q = lane; q < len; q += LANES) draft[q] = tmp[len - 1 - q];
            Ld = len;
        }
        __threadfence_block();
    }
    if (Ld <= 0) stat = CCSX_DRAFT_FAILURE;
    else if (Ld < P.opts.min_length) stat = CCSX_TOO_SHORT;
    else if (Ld > P.opts.max_length) stat = CCSX_TOO_LONG;
    else {
        nw = poa_windows(P, z, Ld, lane);
    }
    if (lane == 0) { P.draft_len[z] = Ld; P.nwin[z] = (stat < 0) ? nw : 0; P.zstat[z] = (stat < 0) ? CCSX_SUCCESS : stat; }
}

// ------------------------------------------------------------------------------------------------
// step 3: subread -> draft, global, adaptive 64-row band, one wave per read; the previous column lives
// in registers.  Instead of storing moves and tracing back every cell, each cell carries the row at which
// its best path ENTERED the most recent window-edge column ("origin"); at every window-edge column the
// propagated origins are saved (64 x int32), and the entry rows are recovered by hopping edge to edge.
// window-edge column of needed-column index k (k_align's list: 0, b1-2, b1+2, b2-2, ..., Ld)
__device__ __forceinline__ int need_col(const int32_t *wb, int nw, int Ld, int k)
{
    return k == 0 ? 0 : (k == 2 * nw - 1 ? Ld : wb[(k + 1) >> 1] + ((k & 1) ? -CCSX_WIN_OVERHANG : CCSX_WIN_OVERHANG));
}
struct AlignEnd { int M, O, lo; unsigned K; };
// the column loop of step 3 over one oriented read in LDS (REV: the draft is walked backwards, the window-edge columns are
// mirrored: the suffix-against-suffix half of the split alignment).  Saves (origin, dirty) of every cell, the band start and the
// best cell (score, row, entry row) at every window-edge column.
template <int REV>
__device__ __forceinline__ AlignEnd align_pass(const KParams &P, const uint32_t *sread, int I, const uint8_t *d, int Ld, const int32_t *wb, int nw,
                                               int32_t *Osave, int lane)
{
    const int nneed = 2 * nw;                           // needed columns: 0, b1-2, b1+2, ..., Ld
    int32_t *lo_need = Osave + (size_t)P.need_max * 128;
    int32_t *cm_need = lo_need + P.need_max + 64, *br_need = cm_need + P.need_max, *eb_need = br_need + P.need_max;   // best cell of every window-edge column (split alignment)
    int2 *OMsave = (int2 *)Osave;                      // per window-edge column and cell: (origin row at the previous edge, dirty bits)
    int kk = 1;                                         // next needed column index
    auto need_at = [&](int k) { return REV ? Ld - need_col(wb, nw, Ld, nneed - 1 - k) : need_col(wb, nw, Ld, k); };
    int next_need = rfl(need_at(1));
    // column 0 = START
    int Mprev = (lane <= I) ? lane * SC_INS : NEGV;
    int Oprev = 0;                                      // entry row at column 0 is 0 for every cell
    // candidate-filter pile-up (SPEC "dirty masks"): every cell carries the dirty bits of the draft positions its best path has
    // passed since the last window-edge column e: bit (j - e - 1) = position j-1 (column j) was not passed by a matching DIAG
    // step.  Leading insertions dirty position 0.  Bit 31: an insertion right at the edge column (dirties the LAST position of
    // the previous interval, patched in the epilogue).
    unsigned Kprev = (lane >= 1) ? 1u : 0u;
    int ecol = 0;                                       // last window-edge column
    int lo = 0, br = 0;
    int rbv = (lane >= 1 && lane <= I) ? read_base_packed(sread, lane - 1) : 4;   // base of row lo + lane (minus one), band at lo = 0
    const int hiI = I - (CCSX_BAND - 1) > 0 ? I - (CCSX_BAND - 1) : 0;
    BaseCursor bcur; bcur.w0 = 0; bcur.vw = 0u;
    const int nwords = (I + 15) >> 4;
    for (int jb = 0; jb < Ld; jb += LANES) {            // draft bases: one coalesced load per 64 columns
        const int dL = (jb + lane < Ld) ? d[REV ? Ld - 1 - (jb + lane) : jb + lane] : 0;
        cursor_load(bcur, sread, nwords, lo + 61, lane);  // the next 64 columns fetch their band-top bases from this window
        asm volatile("" :: "v"(dL), "v"(bcur.vw));       // wait for the block loads here, not inside the column loop
        const int nblk = (Ld - jb) < LANES ? (Ld - jb) : LANES;
        // two columns per loop iteration (round 4, as in k_align16): the carried cells rotate between two register sets
        auto column = [&](const int jj) {
            const int j = jb + jj + 1;
            const int plo = lo;
            lo = rfl(band_lo_s(plo, br, hiI));           // scalar unit; the readfirstlane tells the compiler the result is wave-uniform
            const int sh = lo - plo;                    // 0..2
            const int i = lo + lane;
            const int vb = rl(dL, jj);
            // the read base of row i-1 travels with the band: a band shift moves it one lane down and only the top lane(s)
            // fetch a new base (4 = no base: rows 0 and > I)
            int x, y, ox, oy;
            unsigned kx, ky;
            // (origins and dirty bits shift with a hardware zero fill: bound_ctrl, no register pre-loaded with the fill value)
            if (sh == 0) { x = wave_shr1_i32(Mprev, NEGV); y = Mprev; ox = wave_shr1_i32_z(Oprev); oy = Oprev; kx = (unsigned)wave_shr1_i32_z((int)Kprev); ky = Kprev; }
            else {
                const int top = lo + 62;                                // read index of lane 63's base
                if (sh == 1) {
                    const int nb = top < I ? base_at(bcur, top) : 4;
                    x = Mprev; y = wave_shl1_i32(Mprev, NEGV); ox = Oprev; oy = wave_shl1_i32_z(Oprev);
                    kx = Kprev; ky = (unsigned)wave_shl1_i32_z((int)Kprev);
                    rbv = wave_shl1_i32(rbv, nb);
                } else {
                    x = wave_shl1_i32(Mprev, NEGV); y = wave_shl1_i32(x, NEGV); ox = wave_shl1_i32_z(Oprev); oy = wave_shl1_i32_z(ox);
                    kx = (unsigned)wave_shl1_i32_z((int)Kprev); ky = (unsigned)wave_shl1_i32_z((int)kx);
                    const int nb1 = top - 1 < I ? base_at(bcur, top - 1) : 4;
                    const int nb = top < I ? base_at(bcur, top) : 4;
                    rbv = wave_shl1_i32(wave_shl1_i32(rbv, nb1), nb);
                }
            }
            // invalid cells (outside the band, row 0 for the diagonal) carry NEGV and simply lose every comparison; rows > I and
            // anything below NEGV/2 are reset to NEGV at the end of the column, so nothing accumulates
            const unsigned bitj = 1u << (j - ecol - 1);
            const bool match = (vb == rbv);
            int best = x + (match ? SC_MATCH : SC_MISMATCH), org = ox;
            unsigned kd = match ? kx : (kx | bitj);
            { const int c = y + SC_DEL; if (c > best) { best = c; org = oy; kd = ky | bitj; } }
            const bool need = (j == next_need);
            unsigned insbits = bitj | (bitj << 1);      // an insertion in column j dirties positions j-1 and j
            if (need) {
                // origin (previous edge) of the cell's entry move + dirty bits of the interval that ends here
                OMsave[(size_t)kk * 64 + lane] = make_int2(org, (int)kd);
                if (lane == 0) lo_need[kk] = lo;
                org = i;                                // reset: this column is the new edge
                kd = 0u; insbits = 0x80000001u; ecol = j;
            }
            // insertion chain with origin: the winner of lane l is the highest lane k <= l that attains the prefix maximum of
            // d = c + 4*lane (ties keep the higher lane, as the SPEC's serial chain does).  ONE max-scan finds value and lane
            // together: the key is (d << 6) | lane, with d clamped at -2^24 so that it fits (cells of valid paths are above
            // -2^19; anything below -2^22 is an invalid cell and is reset to NEGV at the end of the column).
            const int d0 = best + 4 * lane;
            const int dc = d0 > -(1 << 24) ? d0 : -(1 << 24);
            const int key = wave_scan_max_i32((dc << 6) | lane);
            const int xi = (key >> 6) - 4 * lane;
            const int ksl = key & 63;
            const int osrc = __shfl(org, ksl);                                   // origin / dirty bits of the cell the insertion run starts from
            const unsigned ksrc = (unsigned)__shfl((int)kd, ksl);
            if (xi > best) { best = xi; org = osrc; kd = ksrc | insbits; }
            if (i > I || best < -(1 << 22)) best = NEGV;
            const int cm = wave_reduce_max_i32(best);
            const unsigned long long bal = __ballot(best == cm);
            br = lo + (__ffsll((long long)bal) - 1);
            Mprev = best; Oprev = org; Kprev = kd;
            if (need) {
                const int ebest = rl(org, br - lo);          // row at which the best cell's path entered this column
                if (lane == 0) { cm_need[kk] = cm; br_need[kk] = br; eb_need[kk] = ebest; }
                ++kk;
                next_need = (kk >= nneed) ? -1 : rfl(need_at(kk));
            }
        };
        { int jj = 0; for (; jj + 2 <= nblk; jj += 2) { column(jj); column(jj + 1); } if (jj < nblk) column(jj); }
    }
    AlignEnd out; out.M = Mprev; out.O = Oprev; out.K = Kprev; out.lo = lo;
    return out;
}

// ------------------------------------------------------------------------------------------------
// step 3, first attempt of the alignment cascade (SPEC "alignment cascade"): FOUR passes of one ZMW per wave, each in a 16-row band
// that lives in one 16-lane DPP row — row shifts, the insertion-chain scan and the column maximum are native row operations
// (row_shr / row_shl with the hardware's fill, 4-step scans), the band position is a per-lane value that is uniform inside a row.
// The band follows the best row, so this finds the path of the 64-row band unless an insertion run of more than 5 or a deleted stretch
// of 6 or more bases occurs (tests/align_lab.py; bit-identical consensus on the test sets); a pass that is not valid here goes on a list for the 64-row retry (k_align), and
// from there to the split alignment.  Same cell recurrence as align_pass.
// Round 5 (second session): the cells no longer carry (origin, dirty bits) through the DP — three values to shift, select and permute per cell instead of one.
// Every cell's MOVE goes to HBM instead (2 bits: diagonal match / diagonal mismatch / deletion / insertion; a lane shifts the two predicate masks of a column into a
// register with two v_addc and stores it every 16 columns, 4 bytes per pass and column), plus the band's step per column (2 bits), and k_align16_tb — ONE LANE PER
// PASS, 64 passes per wave — walks the moves back and writes the entry rows and dirty masks of the window-edge columns: the same path (the moves are the forward
// pass's own decisions), so the same entries and masks, for a third fewer instructions in the kernel that saturates the VALU and half of its HBM writes.
#define AB16 16
#define NEG16 (-(1 << 23))           // k_align16's internal "minus infinity" (see the kernel)
#define AB16_ABOVE 6
#define AB16_SAT_ROWS 1               // SPEC v5 "band saturation": best row within the last AB16_SAT_ROWS rows of a band that can still move down
#define AB16_SAT_GAIN 1               //   ... or a window's worth of columns (edge k-2 -> edge k) without this much gain of the column maximum
#define AVALID_TB 2                   // avalid: valid in the 16-row band, entries / masks not yet traced back (k_align16 -> k_align16_tb, same stream)
// scratch of a quad (one k_align16 workgroup): per pass h [blocks of 16 columns][16 band rows] move words, then [blocks] (band steps, edge flags): 2 bits per column each,
// column j at bits 2 * (15 - ((j - 1) & 15)); edge flag of column j = "column j - 1 is a window-edge column" (the trace-back then needs no window bounds); then the four final band starts
__device__ __forceinline__ int tb_blocks(int Ld) { return ccsx_tb_blocks(Ld); }
__device__ __forceinline__ int tb_stride(int Ld) { return ccsx_tb_stride(Ld); }                  // (ccsx_kernels.h: shared with the host's slot size)
// acc * 2 + (the lane's bit of the wave mask m): one v_addc
__device__ __forceinline__ unsigned shift_in(unsigned acc, unsigned long long m)
{
    unsigned r; unsigned long long co;
    asm("v_addc_co_u32_e64 %0, %1, %2, %2, %3" : "=v"(r), "=s"(co) : "v"(acc), "s"(m));
    return r;
}
__device__ __forceinline__ int sel_i32(unsigned long long m, int a, int b)      // m ? a : b per lane, the mask already in scalar registers
{
    int r;
    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(b), "v"(a), "s"(m));
    return r;
}
__global__ __launch_bounds__(64) void k_align16(KParams P, int qbase, int pass, int region)
{
    const int lane = threadIdx.x, h = lane >> 4, l = lane & 15, rowb = lane & 48;
    uint32_t *sread = dyn_lds;
    uint32_t *Osave = (uint32_t *)(P.align_scratch + ((size_t)region * P.align16_slots + blockIdx.x) * P.align16_slot_i32);
    if (qbase + (int)blockIdx.x >= P.n_quads) return;
    const int qd = rfl(P.quads[qbase + blockIdx.x]);    // (first pass << 2) | (passes - 1): up to four consecutive passes of one ZMW
    const int rfirst = qd >> 2, nq = (qd & 3) + 1;
    const int z = rfl(P.read_zmw[rfirst]);
    const int r0 = rfl(P.read_off[z]);
    const int zr = rfl(P.zref[z]);
    if (pass && !(zr & ZREF_PASSBIT(pass))) return;    // later passes: only the ZMWs whose draft was redone in that pass
    const bool live = h < nq;
    const int r = rfirst + (live ? h : 0);
    if (live && l == 0) { P.avalid[r] = 0; P.ascore[r] = NEGV; }
    if (P.zstat[z] != CCSX_SUCCESS) return;
    const int nused = rfl(P.nreads_used[z]);
    if (rfirst - r0 >= nused) return;
    const bool use = live && (r - r0 < nused);
    if (P.opts.disable_heuristics || (P.tflag && (rfl(P.tflag[z]) & 2))) {   // SPEC v5: --disable-heuristics (or a tandem repeat: DESIGN.md §2) aligns every pass with the 64-row band at once
        if (l == 0 && use) { const int idx = atomicAdd(&P.align_retry[0], 1); P.align_retry[16 + idx] = r; }
        return;
    }
    const int Ld = rfl(P.draft_len[z]), nw = rfl(P.nwin[z]);
    const uint8_t *d = P.draft + P.seq_off[z];
    const int32_t *wb = P.wbounds + P.wb_off[z];
    const int wstride = CH16 / 16 + 3;                  // LDS words per pass: one guard word (the base "before" the chunk: row 0 of a band at 0 looks there),
                                                        // then one chunk of the pass at a time
    const int fl0 = rfl(P.flags[r0 + (zr & 255)] & 1);
    for (int hh = 0; hh < nq; ++hh) {
        const int rr = rfirst + hh;
        const int Ih = rfl((int)(P.base_off[rr + 1] - P.base_off[rr]));
        load_read_chunk(sread + hh * wstride + 1, P.bases + P.base_off[rr], Ih, rfl(((P.flags[rr] & 1) != fl0) ? 1 : 0), 0, lane);
    }
    if (lane < 4) sread[lane * wstride] = 0u;           // the guard words
    __syncthreads();
    int c0 = 0;                                         // first base of the row's chunk in LDS (per lane, uniform inside a row)
    int bi = l - 1;                                     // chunk index of the base of row i - 1 (the band starts at row 0)
    const int I = use ? (int)(P.base_off[r + 1] - P.base_off[r]) : 0;
    const uint32_t *myread = sread + h * wstride + 1;
    const int nneed = 2 * nw;
    const int tbs = tb_stride(Ld);
    uint32_t *mvL = Osave + (size_t)h * tbs + l;                        // the lane's move word of the current block of 16 columns
    uint32_t *shL = Osave + (size_t)h * tbs + tb_blocks(Ld) * 16;       // the pass's (band steps, edge flags) of the block (stored by lane 0 of the row)
    unsigned mvacc = 0u, shacc = 0u, edgeacc = 0u;
    bool prev_edge = false;                             // column j - 1 is a window-edge column other than column 0 (scalar)
    int kk = 1;
    // window-edge columns ahead: lane q holds column kkb + q of the list, refilled every 64 edges (a load + wait per edge otherwise)
    int kkb = 1;
    int needv = need_col(wb, nw, Ld, (kkb + lane < nneed) ? kkb + lane : nneed - 1);
    int next_need = rl(needv, 0);
    // (round 4) inside this kernel an invalid cell is NEG16 = -2^23 instead of NEGV = -2^28: still below every cell of a valid path (> -2^19) and below the
    // -2^22 threshold that resets a cell
    int Mprev = (l <= I) ? l * SC_INS : NEG16;
    int lo = 0, br = 0;                                  // per lane, uniform inside a row
    const int hiI = I - (AB16 - 1) > 0 ? I - (AB16 - 1) : 0;
    const int lane4 = 4 * lane;
    // the band never leaves the read (lo <= hiI = I - 15) unless the read is shorter than the band: only then can a row lie beyond the read and must be kept out of
    // the column maximum (wave-uniform: two VALU per column that ordinary passes do not need)
    const bool tiny = __any(use && I < AB16 - 1);
    // SPEC v5 "band saturation": the narrow band's answer is not trusted (-> 64-row retry) when the best row reaches the band's last row
    // before the band has reached the read's end, or when the column maximum gains less than AB16_SAT_GAIN between two window-edge
    // columns one window apart (cmE0 / cmE1: the maxima two edges / one edge back; edge 0 is column 0 with maximum 0)
    int satf = 0, cmE0 = 0, cmE1 = 0;
    unsigned long long satm = 0ull;
    for (int jb = 0; jb < Ld; jb += LANES) {
        const int dL = (jb + lane < Ld) ? d[jb + lane] : 0;
        asm volatile("" :: "v"(dL));
        // the 64 draft bases of the block as two wave masks: a column takes its base with scalar shifts (round 4: a v_readlane per column before — 6 cycles of the
        // VALU this kernel saturates)
        const unsigned long long dB0 = __ballot(dL & 1), dB1 = __ballot(dL & 2);
        const int nblk = (Ld - jb) < LANES ? (Ld - jb) : LANES;
        auto column = [&](const int jj) {
            const int j = jb + jj + 1;
            const int plo = lo;
            {   // band_lo with 16 rows, per row (the SPEC's final max(., 0) cannot bind: plo >= 0 and hiI >= plo)
                int t = br + 1 - AB16_ABOVE;              // 6 rows above the best row, 9 below: insertion bursts push the path down
                t = t > plo ? t : plo;
                t = t < plo + 2 ? t : plo + 2;
                lo = t < hiI ? t : hiI;
            }
            const int sh = lo - plo;                    // 0..2, per row
            bi += sh;                                   // index of base i - 1 in the row's chunk (no clamps: index -1 is the guard word, indices beyond the read
                                                        // hold zero bits; neither can reach a valid cell)
            shacc = (shacc << 2) | (unsigned)sh;
            edgeacc = (edgeacc << 2) | (prev_edge ? 1u : 0u);
            prev_edge = j == next_need;
            const int vb = (int)((dB0 >> jj) & 1ull) | ((int)((dB1 >> jj) & 1ull) << 1);
            // (every ~2000 columns per pass) the band reaches the end of a chunk: next chunk.  Looked at every 8th column only — the band moves at most two rows
            // per column, so 16 rows of margin cover the columns in between (the chunk holds CH16 + 32 bases)
            if ((jj & 7) == 0 && __any(lo + AB16 + 2 + 16 > c0 + CH16)) {
                for (int hh = 0; hh < nq; ++hh) {
                    const int src = hh << 4;
                    if (rl(lo, src) + AB16 + 2 + 16 > rl(c0, src) + CH16) {
                        const int rr = rfirst + hh;
                        const int Ih = rfl((int)(P.base_off[rr + 1] - P.base_off[rr]));
                        const int nc0 = rl(lo, src) - 16 > 0 ? rl(lo, src) - 16 : 0;
                        __syncthreads();
                        load_read_chunk(sread + hh * wstride + 1, P.bases + P.base_off[rr], Ih, rfl(((P.flags[rr] & 1) != fl0) ? 1 : 0), nc0, lane);
                        __syncthreads();
                        if (h == hh) { c0 = nc0; bi = lo + l - 1 - nc0; }
                    }
                }
            }
            // the read base of row i-1: an unconditional (clamped) LDS read issued here, consumed after the shifts below
            const uint32_t bw = myread[bi >> 4];
            // rows of the previous column in the new band position.  x = cell (i - 1) of the previous column is the previous column shifted by sh - 1 lanes (one
            // of three variants, selected per row — none at all when all four bands move down by one row, the common column); y = cell i is x shifted up by one
            // more lane, except for a band that did not move (its last lane keeps its own cell)
            // (no "no base" code for rows 0 and > I: row 0 has no diagonal source — its x is the shift's fill — and a row beyond the read is reset below, so
            // whatever base the clamped index fetches there cannot reach a valid cell)
            const int rbv = (int)((bw >> (2 * (bi & 15))) & 3u);
            const unsigned long long matchm = __builtin_amdgcn_uicmp((unsigned)vb, (unsigned)rbv, 32 /* eq */);
            int x, y;
            if (__all(sh == 1)) {                         // every band moves down by one row: no selects
                x = Mprev; y = row_shl1_i32(Mprev, NEG16);
            } else {
                const int mR = row_shr1_i32(Mprev, NEG16), m1 = row_shl1_i32(Mprev, NEG16);
                const bool s0 = sh == 0, s1 = sh == 1;
                x = s0 ? mR : (s1 ? Mprev : m1);
                const int yu = row_shl1_i32(x, NEG16);
                y = s0 ? Mprev : yu;
            }
            // the cell: diagonal, then deletion if strictly better, then the insertion chain inside the row (x_i = max(c_i, x_{i-1} + INS): one max-scan of
            // value + 4 * lane) if strictly better — the three decisions are the move
            const int dg = x + sel_i32(matchm, SC_MATCH, SC_MISMATCH);
            const int dl = y + SC_DEL;
            const unsigned long long delm = __builtin_amdgcn_sicmp(dl, dg, 38 /* gt */);
            int best = dl > dg ? dl : dg;
            const int xi = row_scan_max_i32(best + lane4) - lane4;
            const unsigned long long insm = __builtin_amdgcn_sicmp(xi, best, 38 /* gt */);
            best = xi > best ? xi : best;
            // move code of the cell: 0 diagonal match, 1 diagonal mismatch, 2 deletion, 3 insertion
            mvacc = shift_in(mvacc, delm | insm);
            mvacc = shift_in(mvacc, insm | ~(delm | matchm));
            if ((jj & 15) == 15) {                       // 16 columns of moves per lane, 16 band steps per row
                *mvL = mvacc; mvL += 16;
                if (l == 0) *(uint2 *)shL = make_uint2(shacc, edgeacc);
                shL += 2;
            }
            if (tiny && lo + l > I) best = NEG16;        // (a row beyond the read must not take part in the column maximum; an invalid cell inside the read may keep
                                                         // whatever it has below -2^22: it loses every comparison and cannot drift far in 65 k columns)
            // column maximum of the row and the lowest row that attains it, in every lane of the row: ONE all-reduce of (value * 16 + 15 - row) by four row rotations
            // (second session of round 5; before: a prefix scan, a ds_bpermute broadcast — an LDS round trip on the chain that places the next column's band —, a
            // ballot, a 64-bit shift and a find-first)
            const int ck = row_allmax_i32((best << 4) | (15 - l));
            const int cm = ck >> 4, brl = 15 - (ck & 15);
            br = lo + brl;
            satm |= __builtin_amdgcn_sicmp(brl, AB16 - AB16_SAT_ROWS, 39 /* >= */) & __builtin_amdgcn_sicmp(lo, hiI, 40 /* < */);   // (wave masks: two compares, the rest scalar)
            Mprev = best;
            if (j == next_need) {
                if (kk >= 2 && cm - cmE0 < AB16_SAT_GAIN) satf = 1;       // cmE0 = the maximum two edges back, cmE1 = one edge back (a rotation: an
                cmE0 = cmE1; cmE1 = cm;                                   // index kk & 1 made the compiler put the pair into scratch memory)
                ++kk;
                if (kk - kkb >= LANES) { kkb = kk; needv = need_col(wb, nw, Ld, (kkb + lane < nneed) ? kkb + lane : nneed - 1); }
                next_need = (kk >= nneed) ? -1 : rl(needv, kk - kkb);
            }
        };
        { int jj = 0; for (; jj + 2 <= nblk; jj += 2) { column(jj); column(jj + 1); } if (jj < nblk) column(jj); }
    }
    if (Ld & 15) {                                        // the last, partial block: its columns to the top of the word, like a full one
        const int s2 = 2 * (16 - (Ld & 15));
        *mvL = mvacc << s2;
        if (l == 0) *(uint2 *)shL = make_uint2(shacc << s2, edgeacc << s2);
    }
    const int oe = I - lo;
    const bool inr = oe >= 0 && oe < AB16;
    const int srcl = rowb + (inr ? oe : 0);
    const int scv = __shfl(Mprev, srcl);
    satf |= (int)((satm >> lane) & 1ull);
    const int sc = (inr && scv > -(1 << 22)) ? scv : NEGV;     // (an invalid end cell is reported as the SPEC's NEG)
    const int valid = (sc > NEGV / 2 && sc >= Ld && !satf) ? 1 : 0;
    if (l == 0 && use) {
        P.ascore[r] = sc;
        if (valid) {
            Osave[4 * (size_t)tbs + h] = (uint32_t)lo;          // where the trace-back starts: the band of the last column
            P.avalid[r] = AVALID_TB;
        } else {
            P.avalid[r] = 0;
            const int idx = atomicAdd(&P.align_retry[0], 1);        // -> the 64-row retry
            P.align_retry[16 + idx] = r;
        }
    }
}

// The trace-back of k_align16's passes: one LANE per pass, 64 passes per wave.  Walks the stored moves from (I, Ld) to (0, 0) and writes, for every window-edge
// column, the row at which the path ENTERS it (ent) and the dirty bits of the draft positions between two edge columns (dmask) — exactly what the cells used to
// carry forward (align_pass still does): bit (j - e - 1) of an interval that starts after edge column e for a mismatch or deletion at column j, bits of columns j
// and j + 1 for an insertion after column j; an insertion in an edge column itself belongs to the NEXT interval (bit 0) and dirties the last position of its own.
// The walk comes from above, so it collects an interval's bits counted from the interval's UPPER edge (bit eH - j) and reverses them when it reaches the lower one.
// The walk is a dependent chain per lane and its 64 lanes are 64 different passes, so (1) nothing in it may wait for HBM and (2) every per-lane global access is a
// fully divergent instruction — 64 cache lines, ~ 256 cycles of the address unit each (a first version with the loads in the walk took 20 ms per 16384 ZMWs, one
// with per-lane window bounds and 4-byte entry stores 12).  The wave therefore works in EPOCHS of TBE blocks of 16 draft columns: per epoch it copies every pass's
// move words of those columns to LDS with full-width loads (16 bytes per lane, a pass's 128 bytes contiguous), each lane fetches its band steps and edge flags with
// ONE 16-byte load, the walk itself touches LDS only, and the entries go out four at a time (16-byte stores at multiples of four edge columns).
#define TBE 2                          // blocks of 16 draft columns per epoch
#define TB_LSTRIDE (TBE * 16 + 2 * TBE + 1)             // words per lane: odd, so the lanes' rows sit in different banks
__global__ __launch_bounds__(64) void k_align16_tb(KParams P, int qbase, int nslots, int region)
{
    __shared__ uint32_t sS[64 * TB_LSTRIDE];
    __shared__ unsigned long long sOff[64];             // word offset of the pass's first staged move word in the alignment scratch
    __shared__ int sCnt[64];                            // move words of the pass in this epoch (0: none)
    const int lane = threadIdx.x;
    const int t = (int)blockIdx.x * 64 + lane;
    const int s = t >> 2, h = t & 3;
    bool act = s < nslots;
    int r = 0;
    if (act) {
        const int qd = P.quads[qbase + s];
        const int rfirst = qd >> 2, nq = (qd & 3) + 1;
        act = h < nq;
        r = rfirst + (act ? h : 0);
        act = act && P.avalid[r] == AVALID_TB;
    }
    if (!__any(act)) return;
    const int z = act ? P.read_zmw[r] : 0;
    const int Ld = act ? P.draft_len[z] : 0, nw = act ? P.nwin[z] : 1;
    const int I = act ? (int)(P.base_off[r + 1] - P.base_off[r]) : 0;
    const int tbs = tb_stride(Ld), nb = tb_blocks(Ld);
    const size_t sbase = ((size_t)region * P.align16_slots + s) * P.align16_slot_i32;
    const size_t moff = sbase + (size_t)h * tbs;
    const uint32_t *As = (const uint32_t *)P.align_scratch;
    const uint32_t *shw = As + moff + (size_t)nb * 16;
    int lo = act ? (int)As[sbase + 4 * (size_t)tbs + h] : 0;
    int32_t *ent = P.ent + P.ent_off[r];                // (ent_off is a multiple of 4: the 16-byte stores below)
    uint32_t *dm = P.dmask + P.ent_off[r];
    const int nneed = 2 * nw;
    uint32_t *my = sS + lane * TB_LSTRIDE;              // [0, 16 TBE) moves, then TBE (band steps, edge flags)
    uint32_t *mySh = my + TBE * 16;
    uint32_t e0 = 0u, e1 = 0u, e2r = 0u, e3 = 0u, d0 = 0u, d1 = 0u, d2 = 0u, d3 = 0u;   // the last four entry rows / dirty masks, newest first
    int i = I, j = act ? Ld : 0, K = nneed - 1;         // interval K = columns (eL, eH] between the edge columns K - 1 and K
    int eH = Ld;
    unsigned mk = 0u, pend = 0u;                        // dirty bits of interval K counted from eH / of interval K + 1 (final form) until the insertions of edge column K are known
    bool atedge = true;                                 // the walk has just arrived at column eH
    int bhi = nb;                                       // the next epoch covers the blocks [b0, bhi), b0 even
    while (__any(j > 0)) {
        const bool on = j > 0;
        const int b0 = bhi > 0 ? (bhi - 1) & ~1 : 0;          // (a lane that has finished stays at j = 0 = its jstop)
        sOff[lane] = on ? (unsigned long long)(moff + (size_t)b0 * 16) : 0ull;
        sCnt[lane] = on ? (bhi - b0) * 16 : 0;
        // (every load of the epoch is issued before the first is used — unconditional, from a clamped address: a load under a branch is waited for at once, and
        // nine dependent round trips per epoch were what the second version spent its time on)
        const uint4 vs = *(const uint4 *)(on ? shw + 2 * b0 : As);
        __syncthreads();
        // the moves: 16 bytes per lane, TBE * 4 lanes per pass
        uint4 vm[TBE * 4];
#pragma unroll
        for (int q = 0; q < TBE * 4; ++q) {
            const int rd = q * (16 / TBE) + lane / (TBE * 4), part = lane % (TBE * 4);
            vm[q] = *(const uint4 *)(As + sOff[rd] + (part * 4 < sCnt[rd] ? part * 4 : 0));
        }
        mySh[0] = vs.x; mySh[1] = vs.y; mySh[2] = vs.z; mySh[3] = vs.w;
#pragma unroll
        for (int q = 0; q < TBE * 4; ++q) {
            const int rd = q * (16 / TBE) + lane / (TBE * 4), part = lane % (TBE * 4);
            if (part * 4 < sCnt[rd]) {
                uint32_t *dst = sS + rd * TB_LSTRIDE + part * 4;
                dst[0] = vm[q].x; dst[1] = vm[q].y; dst[2] = vm[q].z; dst[3] = vm[q].w;
            }
        }
        __syncthreads();
        const int jstop = b0 * 16;                      // column j lives in block (j - 1) >> 4
        // (the 64 lanes are 64 different passes, so every branch of the step is taken by some lane in nearly every iteration: the step is written with selects,
        // the last four entry rows / masks live in registers that shift at every edge column, and only the 16-byte stores are under a branch)
        while (j > jstop) {
            const int blk = ((j - 1) >> 4) - b0, o = (i - lo) & 15;
            int sft = 2 * (15 - ((j - 1) & 15));
            const uint32_t Wm = my[blk * 16 + o], Ws = mySh[2 * blk], We = mySh[2 * blk + 1];
            if (!atedge) {
                // Round 6: a RUN of plain matches per iteration.  A diagonal match with a band step of 1 keeps the band row (i - lo), so the run's moves are consecutive
                // 2-bit fields of the SAME move word, and its band steps / edge flags consecutive fields of the block's two other words: the run ends at the first
                // field that is not (move 0, step 1, no edge) — the fields shifted in above the word's last column read as "step 0", i.e. end it too.  Matches
                // touch neither the dirty bits nor the entry rows, so i, j and the band start just move by the run's length (one move per iteration before:
                // ~ 12 k iterations of a 64-way divergent walk per 10 kb pass, now ~ one per mismatch / indel / word)
                uint32_t bad = (Wm >> sft) | ((Ws >> sft) ^ 0x55555555u) | ((We >> sft) & 0x55555555u);
                bad = (bad | (bad >> 1)) & 0x55555555u;
                const int k = bad ? (__ffs((int)bad) - 1) >> 1 : 16;
                if (k > 0) {
                    i -= k; j -= k; lo -= k; sft += 2 * k;
                    if (i < 0) { j = 0; continue; }     // (cannot happen on a valid path: never spin on corrupt moves)
                    if (sft >= 32) continue;            // the run reached the word's last column: the next word at the loop's head
                }
            }
            const int code = (int)(Wm >> sft) & 3;
            const unsigned w2 = Ws >> sft, e2 = We >> sft;
            const bool ins = code == 3;
            // dirty bits: an insertion after column j = columns j and j + 1 (in an edge column: the next interval's first position and this one's last);
            // a mismatch or deletion = column j
            const unsigned bj = 1u << ((eH - j) & 31);
            mk |= ins ? (atedge ? 1u : bj | (bj >> 1)) : (code != 0 ? bj : 0u);
            if (ins && atedge) pend |= 1u;
            const bool emit = !ins && atedge;           // the path enters edge column K at row i
            if (emit) {
                e3 = e2r; e2r = e1; e1 = e0; e0 = (uint32_t)i;
                if ((K & 3) == 0) *(uint4 *)(ent + K) = make_uint4(e0, e1, e2r, e3);
                if (K + 1 < nneed) {
                    d3 = d2; d2 = d1; d1 = d0; d0 = pend & 0x7fffffffu;
                    if (((K + 1) & 3) == 0) *(uint4 *)(dm + K + 1) = make_uint4(d0, d1, d2, d3);
                }
                atedge = false;
            }
            if (code != 2) --i;
            if (ins) { if (i < 0) j = 0; continue; }    // (i < 0 cannot happen on a valid path: never spin on corrupt moves)
            lo -= (int)(w2 & 3u);                       // the band of column j - 1
            --j;
            if (e2 & 1u) {                              // column j is an edge column: next interval down, the finished one's bits counted from its lower edge
                const int len = eH - j < 32 ? eH - j : 32;
                pend = __brev(mk) >> (32 - len); mk = 0u; --K;
                eH = j;
                atedge = true;
            }
        }
        bhi = b0;
        __syncthreads();
    }
    if (act) {
        // column 0: the bits of interval 1; rows above the path's start are insertions before the first column (its bit 0).  The last edge column entered was 1.
        const int len = eH < 32 ? eH : 32;
        unsigned m1 = len > 0 ? __brev(mk) >> (32 - len) : 0u;
        if (i > 0) m1 |= 1u;
        *(uint4 *)ent = make_uint4(0u, e0, e1, e2r);
        *(uint4 *)dm = make_uint4(0u, m1 & 0x7fffffffu, d0, d1);
        P.avalid[r] = 1;
    }
}

// The 64-row retry of the alignment cascade: the passes k_align16 could not align in its 16-row band (a list it appended to),
// one wave per pass over a grid-stride loop.
__global__ __launch_bounds__(64) void k_align(KParams P, int pass)
{
    const int lane = threadIdx.x;
    uint32_t *sread = dyn_lds;
    int32_t *Osave = P.retry_scratch + (size_t)blockIdx.x * P.align_slot_i32;   // [need][64] then lo_need[need]
    const int nretry = rfl(P.align_retry[0]);
    for (int it = blockIdx.x; it < nretry; it += gridDim.x) {
    const int r = rfl(P.align_retry[16 + it]);
    const int z = rfl(P.read_zmw[r]);
    const int r0 = rfl(P.read_off[z]);
    const int zr = rfl(P.zref[z]);
    __syncthreads();
    const int Ld = rfl(P.draft_len[z]), nw = rfl(P.nwin[z]);
    const uint8_t *d = P.draft + P.seq_off[z];
    const int32_t *wb = P.wbounds + P.wb_off[z];
    const int I = rfl((int)(P.base_off[r + 1] - P.base_off[r]));
    const int rev = rfl(((P.flags[r] & 1) != (P.flags[r0 + (zr & 255)] & 1)) ? 1 : 0);
    load_read_packed(sread, P.bases + P.base_off[r], I, rev, lane);
    __syncthreads();
    const AlignEnd ae = align_pass<0>(P, sread, I, d, Ld, wb, nw, Osave, lane);
    const int lo = ae.lo, Mprev = ae.M, Oprev = ae.O; const unsigned Kprev = ae.K;
    const int nneed = 2 * nw;
    int32_t *lo_need = Osave + (size_t)P.need_max * 128;
    int2 *OMsave = (int2 *)Osave;
    const int oe = I - lo;
    int sc = NEGV, eLast = 0;
    unsigned kLast = 0u;
    if (oe >= 0 && oe < LANES) { sc = rl(Mprev, oe); eLast = rl(Oprev, oe); kLast = (unsigned)rl((int)Kprev, oe); }
    const int valid = (sc > NEGV / 2 && sc >= Ld) ? 1 : 0;
    __threadfence_block();
    if (lane == 0) {
        P.ascore[r] = sc; P.avalid[r] = (uint8_t)valid;
        if (valid) {
            int32_t *ent = P.ent + P.ent_off[r];
            uint32_t *dm = P.dmask + P.ent_off[r];
            int e = eLast;
            ent[nneed - 1] = e;
            // interval k2 = columns col(k2-1)+1 .. col(k2); a set bit 31 in interval k2+1 (insertion while sitting on edge k2)
            // dirties the last position of interval k2
            unsigned carry = kLast >> 31;               // trailing insertions after the last draft position
            for (int k2 = nneed - 1; k2 >= 1; --k2) {
                const int cell = e - lo_need[k2];
                const int2 om = OMsave[(size_t)k2 * 64 + cell];
                unsigned mk = (unsigned)om.y;
                const int cend = (k2 == nneed - 1) ? Ld : wb[(k2 + 1) >> 1] + ((k2 & 1) ? -CCSX_WIN_OVERHANG : CCSX_WIN_OVERHANG);
                const int cbeg = (k2 == 1) ? 0 : wb[k2 >> 1] + (((k2 - 1) & 1) ? -CCSX_WIN_OVERHANG : CCSX_WIN_OVERHANG);
                if (carry) mk |= 1u << (cend - cbeg - 1);
                carry = mk >> 31;
                dm[k2] = mk & 0x7fffffffu;
                if (k2 >= 2) { e = om.x; ent[k2 - 1] = e; }
            }
            ent[0] = 0; dm[0] = 0u;
        }
    }
    }
}

// SPEC "split alignment": a pass that failed step 3 and is more than RESCUE_MIN_EXCESS bases longer than the draft is tried as
// prefix + ONE large insertion + suffix ("spurious sequencing activity", docs/how-does-ccs-work.md:74-78; the 64-row band cannot
// follow an insertion run of more than ~31 rows).  The forward pass and the pass over the reversed read and draft each leave the
// best cell of every window-edge column; the split is the interior edge column with the largest sum of the two scores whose rows do
// not overlap.  Entry rows left of it come from the forward origins, right of it from the mirrored reverse origins; every position
// counts as dirty.  One wave per read over a grid-stride loop (rare reads: most iterations end at the first test); two scratch slots.
#define RESCUE_MIN_EXCESS 24
__global__ __launch_bounds__(64) void k_rescue(KParams P, int pass)
{
    const int lane = threadIdx.x;
    uint32_t *sread = dyn_lds;
    int32_t *OsF = P.retry_scratch + (size_t)(2 * blockIdx.x) * P.align_slot_i32, *OsR = OsF + P.align_slot_i32;
    for (int rbase = blockIdx.x * LANES; rbase < P.n_reads; rbase += gridDim.x * LANES) {
      // 64 passes per look: nearly all of them aligned
      unsigned long long todo = __ballot(rbase + lane < P.n_reads && !P.avalid[P.read_perm[rbase + lane < P.n_reads ? rbase + lane : 0]]);
      while (todo) {
        const int rp = rbase + (int)__ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int r = rfl(P.read_perm[rp]);
        const int z = rfl(P.read_zmw[r]);
        const int r0 = rfl(P.read_off[z]);
        const int zr = rfl(P.zref[z]);
        if (pass && !(zr & ZREF_PASSBIT(pass))) continue;
        if (P.zstat[z] != CCSX_SUCCESS || r - r0 >= P.nreads_used[z] || P.avalid[r]) continue;
        const int Ld = rfl(P.draft_len[z]), nw = rfl(P.nwin[z]);
        const int I = rfl((int)(P.base_off[r + 1] - P.base_off[r]));
        const int nneed = 2 * nw;
        const uint8_t *d = P.draft + P.seq_off[z];
        const int32_t *wb = P.wbounds + P.wb_off[z];
        const int fl = rfl((int)P.flags[r]);
        const int rev = rfl(((fl & 1) != (P.flags[r0 + (zr & 255)] & 1)) ? 1 : 0);
        if (fl & 2) {
            // SPEC "partial passes": anchored at one end of the draft (flag bit 2 = the adapter is at the pass's end; in draft orientation
            // that is the draft's end iff the pass is on the draft's strand).  The column loop runs from the anchored end; the pass covers
            // the draft up to the window-edge column with the largest column maximum (first on ties), valid iff that score reaches 1.0 per
            // covered base; uncovered edges get entry rows that give every window touching them a negative segment length
            if (nneed < 2) continue;
            const int from_end = ((fl >> 2) & 1) ^ rev;
            __syncthreads();
            load_read_packed_mode(sread, P.bases + P.base_off[r], I, from_end ? (rev ? 2 : 1) : (rev ? 3 : 0), lane);
            __syncthreads();
            if (from_end) (void)align_pass<1>(P, sread, I, d, Ld, wb, nw, OsF, lane);
            else (void)align_pass<0>(P, sread, I, d, Ld, wb, nw, OsF, lane);
            __threadfence_block();
            const int32_t *loF = OsF + (size_t)P.need_max * 128, *cmF = loF + P.need_max + 64, *ebF = cmF + 2 * P.need_max;
            int best = NEGV, bk = 1 << 30;
            for (int k = 1 + lane; k < nneed; k += LANES) {          // edge columns in the direction of the DP
                const int cf = cmF[k];
                if (cf > NEGV / 2 && cf > best) { best = cf; bk = k; }
            }
            const int wbest = rfl(wave_max_i32(best));
            const int ks = rfl(wave_min_i32(best == wbest ? bk : (1 << 30)));
            if (wbest <= NEGV / 2) continue;
            const int scol = from_end ? Ld - need_col(wb, nw, Ld, nneed - 1 - ks) : need_col(wb, nw, Ld, ks);   // covered draft columns
            if (scol <= 0 || wbest < scol) continue;
            if (lane == 0) {
                int32_t *ent = P.ent + P.ent_off[r];
                uint32_t *dm = P.dmask + P.ent_off[r];
                const int2 *OM = (const int2 *)OsF;
                int e = ebF[ks];
                if (!from_end) {
                    ent[ks] = e;
                    for (int k2 = ks; k2 >= 2; --k2) { e = OM[(size_t)k2 * 64 + (e - loF[k2])].x; ent[k2 - 1] = e; }
                    ent[0] = 0;
                    for (int k2 = ks + 1; k2 < nneed; ++k2) ent[k2] = -(1 << 20) - 64 * k2;
                } else {
                    ent[nneed - 1 - ks] = I - e;
                    for (int kq = ks; kq >= 1; --kq) {
                        e = (kq >= 2) ? OM[(size_t)kq * 64 + (e - loF[kq])].x : 0;
                        ent[nneed - kq] = I - e;
                    }
                    for (int k2 = 0; k2 < nneed - 1 - ks; ++k2) ent[k2] = (1 << 20) + 64 * (nneed - k2);
                }
                dm[0] = 0u;
                for (int k2 = 1; k2 < nneed; ++k2) dm[k2] = 0x7fffffffu;
                P.avalid[r] = 1; P.ascore[r] = wbest;
            }
            continue;
        }
        if (I - Ld <= RESCUE_MIN_EXCESS || nneed < 3) continue;
        __syncthreads();
        load_read_packed_mode(sread, P.bases + P.base_off[r], I, rev ? 3 : 0, lane);
        __syncthreads();
        (void)align_pass<0>(P, sread, I, d, Ld, wb, nw, OsF, lane);
        __syncthreads();
        load_read_packed_mode(sread, P.bases + P.base_off[r], I, rev ? 2 : 1, lane);     // the oriented read, last base first
        __syncthreads();
        (void)align_pass<1>(P, sread, I, d, Ld, wb, nw, OsR, lane);
        __threadfence_block();
        const int32_t *loF = OsF + (size_t)P.need_max * 128, *cmF = loF + P.need_max + 64, *brF = cmF + P.need_max, *ebF = brF + P.need_max;
        const int32_t *loR = OsR + (size_t)P.need_max * 128, *cmR = loR + P.need_max + 64, *brR = cmR + P.need_max, *ebR = brR + P.need_max;
        // the split: interior edge column k (mirror index nneed-1-k) with the largest score sum, rows not overlapping; ties: smallest k
        int best = NEGV, bk = 1 << 30;
        for (int k = lane; k < nneed; k += LANES) {              // k = 0 / nneed-1: an empty half (score 0, no rows): a block at the very start / end
            const int kr = nneed - 1 - k;
            const int cf = k ? cmF[k] : 0, cr = kr ? cmR[kr] : 0, a = k ? brF[k] : 0, b = kr ? brR[kr] : 0;
            if (cf > NEGV / 2 && cr > NEGV / 2 && a + b <= I) { const int tot = cf + cr; if (tot > best) { best = tot; bk = k; } }
        }
        const int wbest = rfl(wave_max_i32(best));
        const int ks = rfl(wave_min_i32(best == wbest ? bk : (1 << 30)));
        if (wbest <= NEGV / 2 || wbest < Ld) {
            // SPEC "double split" (v4): no single split column carries the pass (two insertions the band cannot follow).  It is used
            // as a prefix up to the edge column with the largest forward column maximum and a suffix from the edge column with the
            // largest reverse one (first on ties in the direction of each DP, as for partial passes), iff there are edge columns in
            // between, the parts share no read rows and each scores at least 1.0 per covered base; the edges in between get entry
            // rows that make every window touching them unusable for this pass (negative, or longer than the pass)
            int bF = NEGV, kF = 1 << 30, bR = NEGV, kR = 1 << 30;
            for (int k = 1 + lane; k < nneed; k += LANES) {
                const int cf = cmF[k], cr = cmR[k];
                if (cf > NEGV / 2 && cf > bF) { bF = cf; kF = k; }
                if (cr > NEGV / 2 && cr > bR) { bR = cr; kR = k; }
            }
            const int wF = rfl(wave_max_i32(bF)), wR = rfl(wave_max_i32(bR));
            if (wF <= NEGV / 2 || wR <= NEGV / 2) continue;
            const int k1 = rfl(wave_min_i32(bF == wF ? kF : (1 << 30))), kr = rfl(wave_min_i32(bR == wR ? kR : (1 << 30)));
            const int k2 = nneed - 1 - kr;
            const int s1 = need_col(wb, nw, Ld, k1), s2r = Ld - need_col(wb, nw, Ld, k2);
            if (!(k1 < k2 && s1 > 0 && s2r > 0 && wF >= s1 && wR >= s2r && brF[k1] + brR[kr] <= I)) continue;
            if (lane == 0) {
                int32_t *ent = P.ent + P.ent_off[r];
                uint32_t *dm = P.dmask + P.ent_off[r];
                const int2 *OMF = (const int2 *)OsF, *OMR = (const int2 *)OsR;
                int e = ebF[k1];
                ent[k1] = e;
                for (int kq = k1; kq >= 2; --kq) { e = OMF[(size_t)kq * 64 + (e - loF[kq])].x; ent[kq - 1] = e; }
                ent[0] = 0;
                int er = ebR[kr];
                ent[k2] = I - er;
                for (int kq = kr; kq >= 1; --kq) {
                    er = (kq >= 2) ? OMR[(size_t)kq * 64 + (er - loR[kq])].x : 0;
                    ent[nneed - kq] = I - er;
                }
                for (int kq = k1 + 1; kq < k2; ++kq) ent[kq] = -(1 << 20) - 64 * kq;
                dm[0] = 0u;
                for (int kq = 1; kq < nneed; ++kq) dm[kq] = 0x7fffffffu;
                P.avalid[r] = 1; P.ascore[r] = wF + wR;
            }
            continue;
        }
        if (lane == 0) {
            int32_t *ent = P.ent + P.ent_off[r];
            uint32_t *dm = P.dmask + P.ent_off[r];
            const int2 *OMF = (const int2 *)OsF, *OMR = (const int2 *)OsR;
            int e = ks ? ebF[ks] : 0;
            ent[ks] = e;
            for (int k2 = ks; k2 >= 2; --k2) { e = OMF[(size_t)k2 * 64 + (e - loF[k2])].x; ent[k2 - 1] = e; }
            ent[0] = 0;
            const int ksr = nneed - 1 - ks;                         // the same column in the mirrored list
            // reverse entries of the mirrored columns below ksr are the forward entries of the columns above ks: I - entry
            int er = ksr ? ebR[ksr] : 0;
            for (int kq = ksr; kq >= 1; --kq) {
                er = (kq >= 2) ? OMR[(size_t)kq * 64 + (er - loR[kq])].x : 0;
                ent[nneed - kq] = I - er;
            }
            dm[0] = 0u;
            for (int k2 = 1; k2 < nneed; ++k2) dm[k2] = 0x7fffffffu;
            P.avalid[r] = 1; P.ascore[r] = wbest;
        }
      }
    }
}

// per-ZMW: count usable reads, raise TOO_MANY_UNUSABLE (docs/faq/accuracy-vs-passes.md:37-39)
__global__ void k_post(KParams P, int pass)
{
    int z = blockIdx.x * blockDim.x + threadIdx.x;
    if (z >= P.n_zmw) return;
    const int zr = P.zref[z];
    if (pass && !(zr & ZREF_PASSBIT(pass))) return;
    // the draft cascade: a failed draft, or one most passes do not map to, is retried — pass 0 -> the fallback draft (pass 1), pass 1 ->
    // the last resort (pass 2); the last attempt's outcome is final
    const bool may_retry = !P.opts.no_fallback_draft && pass < 2;
    const int retry = pass == 0 ? ZREF_RETRY : ((zr & 255) | ZREF_RETRY2);
    if (P.zstat[z] != CCSX_SUCCESS) {
        P.np[z] = 0; P.out_fn[z] = 0; P.out_rn[z] = 0;
        if (may_retry && P.zstat[z] == CCSX_DRAFT_FAILURE) P.zref[z] = retry;
        return;
    }
    int r0 = P.read_off[z], nr = P.nfull[z], np = 0, rn = 0;     // full-length passes only: partial passes are not passes
    const int f0 = P.flags[r0 + (zr & 255)];
    for (int r = 0; r < nr; ++r) {
        const int v = P.avalid[r0 + r];
        np += v;
        if (v && ((P.flags[r0 + r] ^ f0) & 1)) ++rn;
    }
    P.np[z] = np; P.out_fn[z] = np - rn; P.out_rn[z] = rn;
    if (2 * np <= nr) {
        if (may_retry) P.zref[z] = retry;                  // try the next draft generator before giving up
        else { P.zstat[z] = CCSX_TOO_MANY_UNUSABLE; P.nwin[z] = 0; }
    }
}

// The windows of the batch in compact order (after the last k_post: nwin[z] is final).  The polish / kinetics grids used to cover every window SLOT
// (capacity: 1.25 x the longest pass / 19 + 4 per ZMW, a host-built map) — 31 % of the workgroups found no window and left, each after holding a workgroup's
// LDS for two dependent loads.  One workgroup: exclusive scan of nwin over the ZMWs, then the map (window index -> ZMW).
__global__ __launch_bounds__(1024) void k_wmap(KParams P)
{
    __shared__ int sTot[16], sCarry;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) sCarry = 0;
    __syncthreads();
    for (int z0 = 0; z0 < P.n_zmw; z0 += 1024) {
        const int z = z0 + tid;
        const int v = z < P.n_zmw ? P.nwin[z] : 0;
        const int incl = wave_scan_add_i32(v);
        if (lane == 63) sTot[wv] = incl;
        __syncthreads();
        int base = sCarry;
        for (int q = 0; q < wv; ++q) base += sTot[q];
        if (z < P.n_zmw) P.wstart[z] = base + incl - v;
        __syncthreads();
        if (tid == 1023) sCarry = base + incl;
        __syncthreads();
    }
    if (tid == 0) P.wstart[P.n_zmw] = sCarry;
}
__global__ __launch_bounds__(256) void k_wmap_fill(KParams P)     // one wave per ZMW: the map entries of its windows
{
    const int z = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (z >= P.n_zmw) return;
    const int a = P.wstart[z], nw = P.nwin[z];
    for (int w = lane; w < nw; w += LANES) P.wslot_zmw[a + w] = z;
}

// ------------------------------------------------------------------------------------------------
// A1-A7 + step 7: Arrow polish of one window per workgroup (PW_THREADS = 4 waves).
//
// v4 (round 3; tables: round 6).  LDS holds: sCTX[obs][ctx] = (ME, INS) as float2, 17 entries per observation row (16 contexts, one zero entry;
// row 12 = all zeros): the scoring's table; per-column entries (DL, offset of the column's context in a row of sCTX) for a long read's sweep (sColJ);
// the quad fill's per-column table sTC[strand][obs][column] + sDLC (see TC_LO below); gamma/beta of one chunk of up to EIGHT reads
// (sGB, even row stride: the fill's lane = row stores step by S - 1 words from lane to lane, the scoring's lane = column loads by 1:
// both conflict free).  Fill: lane = read row, anti-diagonal sweep, neighbours via DPP wave shifts; two short reads per wave (lanes
// 0-31 / 32-63); a chunk's two pair tasks run as four alpha-only / beta-only sweeps, one per wave.  Candidate filter
// (docs/how-does-ccs-work.md:80-83): the step-3 alignments' dirty bits give a per-position pile-up margin; unambiguous
// non-homopolymer positions enumerate no mutations.  Scoring: a pool of (64 compacted mutation lanes) x (usable read) units over the
// waves, serial over read rows exactly as the SPEC orders the operations; per-read gains are summed in 2^-16 fixed point with LDS
// integer atomics, so the sum does not depend on which wave scored which read.
#ifndef PW_THREADS
#define PW_THREADS 256                // 4 waves.  Round 2 (ms per 2048 ZMWs, 10 x 10 kb): 256 threads x 3 workgroups/CU 95, 512 x 2 (all ten reads in one
#endif                                //   LDS chunk) 101-103, 256 x 2 141, 320 x 2 208.  Round 3 (ms per 8192): 256 x 4 155, 384 x 3 225, 384 x 2 234-255, 512 x 2 229-260
#ifndef PW_MINWAVES
#define PW_MINWAVES 4
#endif
#define PW_WAVES (PW_THREADS / 64)
#ifndef PW_CHUNK_READS
#define PW_CHUNK_READS 8              // reads per gamma/beta chunk (0: as many as fit).  A chunk costs one fill sweep + one scoring pass however many
                                      // reads it holds (ms of k_polish per 8192 ZMWs: 2 reads per chunk 234, 4 reads 169.5, as many as fit = 4-5 reads 175.7):
                                      // four reads = two pair tasks = four alpha-only / beta-only units = every wave busy for ONE sweep, a fifth read
                                      // adds a task and turns the units into full alpha+beta sweeps on three waves.  Eight-wave workgroups with 8 / 10
                                      // reads per chunk (2 per CU, 80 KB each) ran 260 / 229 ms: profiles/r03_polish_fill_variants.txt
#endif
#ifndef PW_MAXREADS
#define PW_MAXREADS 32                // passes per GROUP: the per-read arrays, observations and chunk plan of k_polish / k_kinetics describe one group.  Round 4
                                      // (profiles/r04_group_size.txt, ms of k_polish at 10 passes / the configs[4] mix / 30 passes x 20 kb): 64 157 / 311 / 861 with 16-bit
                                      // observation codes; one byte per observation: 32 156 / 254 / 705, 16 156 / 258 / 755, 12 155 / 260 / 763
#endif
#ifndef PW_LDS_BYTES
#define PW_LDS_BYTES 40960            // static + dynamic LDS of one workgroup: FOUR workgroups per CU fill its 160 KB exactly.  Round 3 sweep (ms of
                                      // k_polish per 8192 ZMWs 10 x 10 kb, alone / under the draft stage of the next batch): 52992 (3 per CU) 217.9 / 305.3,
                                      // 40960 184.6 / 264.8, 40448 189.6 / 273.3, 38912 195.0 / 279.3, 36864 199.7 / 281.1, 32256 (5 per CU) 225.6 / 307.8
#endif
#ifndef CTXS
#define CTXS 17                       // entries per observation row of sCTX: 16 contexts + one zero entry (odd stride: (obs + ctx) mod 16 spreads the scoring's look-ups over the bank pairs)
#endif
#define FILL16_MAXBW 24               // widest band (diagonals) of a read that shares a wave with three others (k_polish's quad sweep)
// Round 6: the quad fill's per-COLUMN table.  sTC[strand][obs][column] = (ME, INS) of the column's context for that observation (row 12 and the columns from
// J on: zeros) — the lane of a quad unit (a read row: fixed observation, a new column every step) reads it with ONE ds_read_b64 at a running address + immediate;
// the 16 lanes of a DPP row are on 16 CONSECUTIVE columns, so whatever their observations they hit 16 different bank pairs (row stride 32 entries).  Until round 5 a
// lane took the column's context offset from a staggered per-column entry and then the pair from its observation's row of sCTX[obs][ctx]: two dependent LDS reads,
// the second at (obs + ctx) mod 16 — 42 % of the kernel's LDS cycles were bank conflicts.  sDLC[strand][column] = DL of the column's context (1 outside 0 .. J-1).
// A lane forms column indices from TC_LO .. 31 + TC_HI while it is off the band; what it reads there is never used but has to be FINITE (0 * x), so the tables sit
// between guards of finite floats: [sDL, sZP, padding] in front, sDLC behind.
#define TC_LO 56                      // columns below 0 / above 31 a quad lane may form: alpha -27 .. 67, beta -53 .. 62 (a read much shorter than its quad's longest keeps
#define TC_HI 38                      // stepping after its own last column), DL one column lower
#define TC_ROW 32                     // entries per observation row
#define TC_STRAND ((CCSX_NOBS + 1) * TC_ROW)                 // entries per strand
#define DLC_S (33 + TC_LO)            // sDLC: [TC_LO pad | strand 0: columns 0 .. 32 | TC_LO pad | strand 1 | TC_HI pad] — the middle pad serves both strands
#define DLC_TOTAL (TC_LO + DLC_S + 33 + TC_HI)
#define TAB_TAIL (2 * TC_HI - 48)     // floats of padding behind sDL / sZP, which with them are the guard behind sTC
#define OBS_TC(o) ((o) * (TC_ROW * 8))         // the byte offset of observation o's row in a strand of sTC
#define OBS_CODE(o) ((o) * (CTXS * 8))        // the byte offset of observation o's row in sCTX (sObs holds the 8-bit observation itself)

struct LaneMut {                     // per-lane constants of one mutation on one strand
    int c, q, kA, kB, isdel, fin;    // kA / kB index a row of sCTX; 16 = the zero entry (see lane_mut)
    int qoff;                        // q - c - 1 (0: insertion, 1: substitution / deletion): how far beta(i+1, q) sits above gamma(i, c) in diagonals (SPEC v8 joint band test)
    float dlA, dlL;
};

__device__ __forceinline__ LaneMut lane_mut(int type, int c, int x, const uint8_t *t, int J, int lf, const float *sDL)
{
    // branch-free: both template neighbours are loaded unconditionally (clamped indices; sT has 32 entries), then selected
    LaneMut L;
    const int tm1 = t[c > 0 ? c - 1 : 0];
    const int nidx = (type == 2) ? c : c + 1;
    const int tn = t[nidx < 31 ? nidx : 31];
    const int fin = (type == 2) ? (c == J) : (c + 1 == J);
    const int nx = fin ? 0 : tn;                             // the template base after the mutated column (0 when there is none)
    int pA = (c > 0) ? tm1 : lf;
    const int xA = (type == 1) ? nx : x;
    if (pA > 3) pA = (xA + 2) & 3;
    const int kA = pA * 4 + xA, kB = (type == 1) ? kA : xA * 4 + nx;
    const int q = (type == 2) ? c + 1 : c + 2;
    L.c = c; L.q = q > J ? J : q; L.isdel = (type == 1); L.fin = fin; L.qoff = (type == 2) ? 0 : 1;
    L.dlA = sDL[kA]; L.dlL = sDL[kB];
    // the SPEC's "no stay move" cases read the ZERO entry of the observation's row: a deletion whose extension is the final column (INS[kA] is unused and
    // b = a, so ME[kA] is not needed either), and any extension that reaches the final column (INS[kB] unused; ME[kB] only feeds the link, which such a lane does
    // not report).  Until round 5 the table carried a second half of (ME, 0) copies for them: 1.6 KB of LDS
    L.kA = (type == 1 && fin) ? (CTXS - 1) : kA;
    L.kB = fin ? (CTXS - 1) : kB;
    return L;
}

// 32-bit LDS pointers (address space 3): they survive being made opaque to the optimiser as LDS pointers (ds_read, not flat)
typedef const float __attribute__((address_space(3))) *lds_cf;
typedef const char __attribute__((address_space(3))) *lds_cc;

typedef const uint8_t __attribute__((address_space(3))) *lds_cu8;
struct ScoreChain {                  // running state of one (lane, read) mutation evaluation
    float ap, bp, acc, b, bq;
    float2 pA, pB;
    lds_cf g, be;                    // gamma(i, c) and beta(i+1, q) of the row about to be processed: both advance by the read's pitch per row
    lds_cu8 op;                      // observation of that row (0..11, 12 = none)
    unsigned w0, w1, w2;             // the observation bytes of the block's rows still to come, byte 0 of w0 = the row about to be loaded (obs_words)
    int dg;                          // SPEC v6/v8: gamma's diagonal relative to the read's band, c - i - dlo; the row's two cells are on the band iff 0 <= dg <= bw - 1 - (q - c - 1)
};

// v in the lanes of the wave mask m, 0 elsewhere: one v_cndmask on a mask that already sits in scalar registers
__device__ __forceinline__ float lanes_or_zero(unsigned long long m, float v)
{
    float r;
    asm("v_cndmask_b32_e64 %0, 0, %1, %2" : "=v"(r) : "v"(v), "s"(m));
    return r;
}

// What a wave keeps of a mutation lane ACROSS units (both strands, the whole round): the seven small integers of LaneMut in one word, and the two DL factors.
// A unit unpacks its strand's word with a handful of v_bfe; the scoring rows then have 12 VGPRs more than when both strands' LaneMut stayed unpacked.
struct LanePk { int pk; float dlA, dlL; };   // pk = c | q << 5 | kA << 10 | kB << 15 | isdel << 20 | fin << 21 | qoff << 22
__device__ __forceinline__ LanePk lane_pack(const LaneMut &L)
{
    LanePk k;
    k.pk = L.c | L.q << 5 | L.kA << 10 | L.kB << 15 | L.isdel << 20 | L.fin << 21 | L.qoff << 22;
    k.dlA = L.dlA; k.dlL = L.dlL;
    return k;
}
__device__ __forceinline__ LaneMut lane_unpack(const LanePk &k)
{
    LaneMut L;
    const unsigned p = (unsigned)k.pk;
    L.c = p & 31; L.q = (p >> 5) & 31; L.kA = (p >> 10) & 31; L.kB = (p >> 15) & 31; L.isdel = (p >> 20) & 1; L.fin = (p >> 21) & 1; L.qoff = (p >> 22) & 1;
    L.dlA = k.dlA; L.dlL = k.dlL;
    return L;
}

// ---- one row of the extend+link recursion = one ROW-STEP: its loads (rs_load) and its arithmetic (rs_compute).  tA / tB = the lane's columns of
// sCTX (context kA / kB).  Every lane walks its own rows (the SPEC's band around the window diagonal starts at a per-lane row), so every lane has its own
// observation code per row; row I of a read carries code 12 = the all-zero row of sCTX ("no base left": the SPEC's i < I cases become exact +0 products).
// SPEC v6: gamma / beta are stored on the read's band only; a scoring band that is clamped into a corner of the window reads cells outside it, which are zeros
// (the address of such a cell aliases a neighbouring row's: the value is replaced, never used).
// The rows run as a two-deep pipeline (profiles/polish_scoring_loads.txt).  A row-step's six LDS words — gamma(i, c), beta(i+1, q) and the two table pairs — depend on
// nothing the rows compute: the addresses run with the row, and the row's observation byte comes from REGISTERS (obs_words: the chain's next twelve bytes of sObs[r],
// loaded once as aligned words and shifted into place per lane).  So a row-step's loads are issued while the row-step before it computes, into registers of their
// own (RowLoads), and the wait in front of its arithmetic finds them there.  Until then a row waited three times in series: for its observation byte, for the table
// pairs behind it, and for gamma / beta, which shared one temporary register with the next load.
#define SCORE_OBS_ROWS 12             // rows per block of observation bytes: twelve bytes from any residue of the first row's address lie in four aligned words
typedef const unsigned __attribute__((address_space(3))) *lds_cu32;
struct RowLoads { float g, be; unsigned long long va, vb; };

// the chain's observation bytes of rows i .. i + 11 (op = &sObs[r][i]) into w0 .. w2, byte 0 of w0 = row i.  The words behind the row's own 68 bytes belong to the
// next row or to the gamma/beta area: their bytes are shifted in and never used
__device__ __forceinline__ void obs_words(ScoreChain &s, lds_cu8 op)
{
    const unsigned sh = (unsigned)(unsigned long long)op & 3u;
    lds_cu32 w = (lds_cu32)(op - sh);
    const unsigned d0 = w[0], d1 = w[1], d2 = w[2], d3 = w[3];
    s.w0 = __builtin_amdgcn_alignbyte(d1, d0, sh);
    s.w1 = __builtin_amdgcn_alignbyte(d2, d1, sh);
    s.w2 = __builtin_amdgcn_alignbyte(d3, d2, sh);
}

__device__ __forceinline__ void rs_load(ScoreChain &s, RowLoads &r, lds_cc tA, lds_cc tB, int pitch)
{
    typedef const unsigned long long __attribute__((address_space(3))) *lds_cu64;
    r.g = *s.g; r.be = *s.be;
    const int o256 = __mul24((int)(s.w0 & 255u), CTXS * 8);   // byte offset of the observation's row in sCTX
    r.va = *(lds_cu64)(tA + o256); r.vb = *(lds_cu64)(tB + o256);   // one ds_read_b64 each
    s.g += pitch; s.be += pitch;
    s.w0 = __builtin_amdgcn_alignbit(s.w1, s.w0, 8); s.w1 = __builtin_amdgcn_alignbit(s.w2, s.w1, 8); s.w2 >>= 8;
}

__device__ __forceinline__ void rs_compute(ScoreChain &s, const LaneMut &L, const RowLoads &r, unsigned lim)
{
    // SPEC v8 "joint band test": gamma(i, c) and beta(i+1, q) of the row sit q - c - 1 diagonals apart; both are zeros unless both are on the band — one compare
    // (lim = bw - 1 - (q - c - 1)) whose mask serves both selects (v7: a test per cell)
#ifndef CCSX_EXP_NO_BANDMASK                                // experiment (timing only, wrong results in the corners of a window): what the band test costs
    const unsigned long long on = __builtin_amdgcn_uicmp((unsigned)s.dg, lim, 37 /* ule */);
    const float gmm = lanes_or_zero(on, r.g);
    const float bqn = lanes_or_zero(on, r.be);
#else
    const float gmm = r.g, bqn = r.be;
#endif
    const float2 nA = make_float2(__uint_as_float((unsigned)r.va), __uint_as_float((unsigned)(r.va >> 32)));
    const float2 nB = make_float2(__uint_as_float((unsigned)r.vb), __uint_as_float((unsigned)(r.vb >> 32)));
    s.dg -= 1;
    const float insA = s.pA.y, meA = s.pA.x, insB = s.pB.y;
    // SPEC v8 "fused recurrences": every multiply-add is one fma, nested as written in DESIGN.md §2
    const float a = __builtin_fmaf(s.ap, insA, gmm);
    float b;
    if (L.isdel) b = a;
    else b = __builtin_fmaf(s.bp, insB, __builtin_fmaf(a, L.dlA, s.ap * meA));
    s.acc = __builtin_fmaf(b, __builtin_fmaf(L.dlL, s.bq, nB.x * bqn), s.acc);
    s.ap = a; s.bp = b; s.b = b; s.pA = nA; s.pB = nB; s.bq = bqn;
    asm volatile("" : "+v"(s.acc), "+v"(s.bp));              // the arithmetic stays HERE, between its fences: sunk behind the later loads it would keep every RowLoads alive at once
}
#define RS_FENCE() __builtin_amdgcn_sched_barrier(0)   // nothing moves across: a row-step's loads stay in front of the arithmetic they overlap

// first row of a lane's scoring band: floor((2 c I + J) / (2 J)) - Wr, clamped so that nrows rows fit into 0..I (SPEC "banded link");
// the quotient through a float reciprocal with an exact remainder correction (all values < 2^12)
__device__ __forceinline__ int band_row0(int c, int I, int J2, float invJ2, int J, int Wr, int nrows)
{
    const int num = __mul24(2 * c, I) + J;
    int q = (int)((float)num * invJ2);
    const int r = num - __mul24(q, J2);
    q += (r >= J2 ? 1 : 0) - (r < 0 ? 1 : 0);
    int i0 = q - Wr;
    i0 = i0 < 0 ? 0 : i0;
    const int hi = I + 1 - nrows;
    return i0 > hi ? hi : i0;
}

// fixed-point image of one read's log2-likelihood gain (SPEC "integer sum over reads")
__device__ __forceinline__ int dq_fix(float d)
{
    if (d < -DQ_CLAMP) d = -DQ_CLAMP;
    if (d > DQ_CLAMP) d = DQ_CLAMP;
    return (int)floorf(d * DQ_SCALE + 0.5f);
}

// error probability reported for a position the candidate filter skipped (pile-up margin g = clean - dirty)
__device__ __forceinline__ float skip_perr(int g, float floor_)
{
    if (g < 0) g = 0;
    if (g > 12) g = 12;
    const float p = 8.0f * det_exp2f(-3.0f * (float)g);
    return p < floor_ ? floor_ : p;                          // SPEC v7: the pile-up supports no claim beyond Q50 (opts.max_qv)
}

// SPEC v7 "repeat-count floor": lane x's longest period-p tandem tract among the visible window bases, from the wave mask m (bit k: v[k] == v[k+p]); 0 = none
// (SPEC v8: bit 8 of the result = the tract is OPEN, i.e. runs into an end of the visible template of nvis bases; on equal lengths the flags are ORed)
__device__ __forceinline__ int tract_len(unsigned long long m, int x, int p, int nvis)
{
    const int lo = x - p < 0 ? 0 : x - p;
    const unsigned long long cand = m & ((2ull << x) - 1ull) & ~((1ull << lo) - 1ull);      // the runs that reach x start their last equality at k in [x - p, x]
    if (!cand) return 0;
    int best = 0;
#pragma unroll
    for (int which = 0; which < 2; ++which) {                // the lowest and the highest such k: the same run, or the two runs that touch x
        const int k = which ? 63 - __clzll((long long)cand) : __ffsll((long long)cand) - 1;
        const unsigned long long zb = ~m & ((1ull << k) - 1ull);
        const int i = zb ? 64 - __clzll((long long)zb) : 0;
        const int j = k + (__ffsll((long long)(~m >> k)) - 1);
        const int L = j - i + p, op = ((i == 0) || (j + p >= nvis)) ? 256 : 0;
        if (L > (best & 255)) best = L | op; else if (L == (best & 255)) best |= op;
    }
    return best;
}


// SPEC v6 "banded fill": the diagonals d = j - i on which alpha / beta of a (read, window) pair exist (exact zeros elsewhere), and how gamma / beta are laid out in
// LDS.  A band narrower than a matrix row is stored BY DIAGONAL: cell (i, j) at i * (BWp - 1) + (j - dlo), BWp = BW | 1 floats per row (odd: the fill's lane stride
// BWp - 2 and the scoring lanes' ~ BWp are then conflict free) — 15 floats per row instead of 28 at I = J, so a chunk holds twice the reads.  A band that wide or wider
// (|I - J| >= 5: rare) keeps the row layout i * S + j.  Both are "org + i * pitch + j".
struct FillBand { int dlo, dhi, bw, pitch, org, rowsz; };
__device__ __forceinline__ FillBand fill_band_of(int I, int J, int S)
{
    FillBand b;
    const int dIJ = I > J ? I - J : J - I;
    const int W = SCORE_BAND + FILL_MARGIN + (dIJ > 2 ? dIJ - 2 : 0);
    const int lo = (J - I < 0 ? J - I : 0) - W, hi = (J - I > 0 ? J - I : 0) + W;
    b.dlo = lo < -I ? -I : lo; b.dhi = hi > J ? J : hi;
    b.bw = b.dhi - b.dlo + 1;
    const int bwp = b.bw | 1;
    const bool diag = bwp < S;
    b.rowsz = diag ? bwp : S; b.pitch = diag ? bwp - 1 : S; b.org = diag ? -b.dlo : 0;
    return b;
}

// the windows a launch piece covers, and the XCD-contiguous order of its blocks: block b -> the (b / 8)-th window of the (b % 8)-th eighth; -1 = no window
__device__ __forceinline__ int polish_piece_windows(int total, int slot0, int grid) { const int c = total - slot0; return c < 0 ? 0 : (c > grid ? grid : c); }
__device__ __forceinline__ int xcd_contiguous(unsigned b, int count)
{
    const int per = (count + 7) >> 3;
    const int k = (int)(b >> 3), r = (int)(b & 7u) * per + k;
    return (k < per && r < count) ? r : -1;
}

// PWT threads, PWMIN workgroups' worth of waves per SIMD, PWCH reads per gamma/beta chunk: ONE instantiation is shipped, 256 x 4 x 4.  Round 4 measured
// the 512-thread shape (2 workgroups of 80 KB per CU, 8 reads per chunk) at 14 / 18 / 24 passes and on the configs[4] mix: 2.2 / 2.3 / 1.8 / 1.7 times
// SLOWER than this one (profiles/r04_c4_shapes.txt; its apparent 2.4x win at 30 passes x 20 kb came from a grid of more than 2^32 threads that covered 23 % of the windows).
template <int PWT, int PWMIN, int PWCH>
__global__ __launch_bounds__(PWT, PWMIN) void k_polish_t(KParams P, int slot0)
{
    // [obs][ctx] = (ME, INS); entry 16 of a row and row 12 = zeros ("no base").  Odd row stride: with the banded link every lane looks up its OWN
    // observation row, and with an even stride all lanes of one context hit the same bank pair whatever their rows (35 % of the LDS cycles were bank
    // conflicts in round 2); 17 spreads them by (obs + ctx) mod 16
    __shared__ float2 sCTX[(CCSX_NOBS + 1) * CTXS];
    // one float array: [sDLC] [sTC: 2 strands x 13 observation rows x 32 columns x (ME, INS)] [sDL 16 | sZP 32 | padding] — the first and the last part
    // double as the finite guards of sTC (see TC_LO): 2 TC_LO floats in front, 2 TC_HI behind
    static_assert(DLC_TOTAL >= 2 * TC_LO && TAB_TAIL >= 0 && (DLC_TOTAL & 1) == 0, "sTab: guards / alignment of sTC");
    __shared__ __attribute__((aligned(16))) float sTab[DLC_TOTAL + 2 * TC_STRAND * 2 + 48 + TAB_TAIL];
    float *const sDLC = sTab;
    float2 *const sTC = (float2 *)(sTab + DLC_TOTAL);
    float *const sDL = sTab + DLC_TOTAL + 2 * TC_STRAND * 2, *const sZP = sDL + 16;         // sZP: z-score MU[16], VAR[16]
    __shared__ uint8_t sT[2][32];                            // template: [0] forward, [1] reverse complement
    __shared__ uint8_t sTd[32];                              // the draft's window as it was (the large-insertion trim of a reloaded group compares with it)
    // dynamic LDS: observation codes of the batch's largest ZMW ([reads][68]: 63 codes + look-ahead slack), then gamma/beta.
    // One BYTE per read row (round 3 stored the 16-bit byte offset of the observation's sCTX row: at 30 passes those 4 KB left room for only three
    // reads per gamma/beta chunk; the extra multiply per row is not measurable).  The scoring takes a chain's bytes as aligned WORDS, twelve rows at a time (obs_words):
    // rows of 68 bytes keep every row 4-byte aligned.
    uint8_t (*sObs)[68] = (uint8_t (*)[68])dyn_lds;
    float *sGB = (float *)((uint8_t *)dyn_lds + P.pw_obs_bytes);
    const int GB_FLOATS = P.pw_gb_floats;
    __shared__ int sI[PW_MAXREADS], sGoff[PW_MAXREADS], sBoff[PW_MAXREADS];   // segment length; where gamma / beta (i, j) = sGB[off + i * pitch + j] of the chunk's reads start
    __shared__ int sBand[PW_MAXREADS];                       // the read's band and layout (SPEC v6): pitch | rowsz << 8 | bw << 16 | (dlo + 128) << 24
    __shared__ unsigned sDirty[PW_MAXREADS];                 // window-relative pile-up dirty bits of each read
    __shared__ uint8_t sStrand[PW_MAXREADS], sRend[PW_MAXREADS];   // sRend[first read of a chunk] = the chunk's end (see plan_chunks)
    __shared__ unsigned sZdrop[(CCSX_MAX_PASSES + 32) / 32]; // z-score gate, one BIT per pass (all groups; a group is one word): decided on the draft window (round 0), then kept
    __shared__ float sBase[PW_MAXREADS], sB00[PW_MAXREADS];   // alpha(I,J) / beta(0,0) of the chunk's reads (the fill's two halves meet here)
    __shared__ short2 sTask[PW_MAXREADS];                    // .x: the fill tasks of a chunk (a read each: long units, then quad members), listed from the chunk's first read on;
                                                             // .y at a chunk's first read: its long units | quad members << 8
    __shared__ int sDeltaI[256];                             // fixed-point sums of the per-read gains (converted in registers at the round's end, never in place)
    __shared__ uint8_t sMvalid[256];
    __shared__ int sCtl[12];                                 // 0:J 1:cs 2:ce 3:nacc 7:ev bits
    __shared__ float sZS[4];                                 // z-score sums: M fwd, V fwd, M rev, V rev
    __shared__ float sPskip[36];                             // error probability of a position if it is skipped (travels with the base)
    __shared__ uint8_t sList[256];                           // compacted valid mutation lanes (a lane index < 256)

    const int tid = threadIdx.x, lane = tid & 63, wave = rfl(tid >> 6);      // wave-uniform values are made scalar explicitly (rfl):
    // loop counters, read indices and observation codes then live in SGPRs and cost no vector instructions
    PHASE_T0();
    // ---- locate (zmw, window).  The prologue is a chain of dependent global loads; every level issues all of its
    // loads before the first use (clamped indices instead of branches), so the chain is 4 round trips deep
    // (z-level scalars -> window bounds + per-read metadata + tables -> entry rows -> segments), not one per array.
    // XCD-aware order: block b runs on XCD b % 8 (observed, a speed matter only), every XCD has its own L2, and neighbouring windows of a ZMW share the lines of
    // their entry rows, dirty masks and read segments — so XCD x takes the x-th CONTIGUOUS eighth of the windows there are, not every eighth window
    // (slot0: a batch of more than 2^24 - 256 window slots is launched in pieces, see ccsx_launch_all; the grid covers the slot capacity, a multiple of 8,
    // the map only the windows there are)
    const int nwin_here = polish_piece_windows(P.wstart[P.n_zmw], slot0, (int)gridDim.x);
#ifdef CCSX_EXP_HOT_PROLOGUE                                // experiment (timing only, wrong results): every workgroup takes one of the same 4096 windows, so the
    const int bid_ = slot0 + xcd_contiguous(blockIdx.x, nwin_here);   // prologue's loads come from the L2 — what its HBM latency costs the whole kernel
    const int bid = bid_ < slot0 ? bid_ : slot0 + ((bid_ - slot0) & 4095);
#else
    const int bid = slot0 + xcd_contiguous(blockIdx.x, nwin_here);
#endif
    if (bid < slot0) return;
    const int z = P.wslot_zmw[bid];                         // device-built compact map (k_wmap): no dependent search
    const int wbo = P.wb_off[z], nw = P.nwin[z], Ld = P.draft_len[z];
    const int r0 = P.read_off[z], nreads = P.nreads_used[z];
    const int64_t so = P.seq_off[z];
    const int w = bid - P.wstart[z];
    const int32_t *wb = P.wbounds + wbo;
    const uint8_t *draft = P.draft + so;
    const int wb0 = wb[w], wb1 = wb[w + 1];
    const int64_t bo_r0 = P.base_off[r0];
    const int fl0 = P.flags[r0 + (P.zref[z] & 255)] & 1;    // orientation of the draft = that of its backbone pass
    int ws = wb0 - CCSX_WIN_OVERHANG; if (ws < 0) ws = 0;
    int we = wb1 + CCSX_WIN_OVERHANG; if (we > Ld) we = Ld;
    const int idx_ws = (w == 0) ? 0 : 2 * w - 1, idx_we = (w == nw - 1) ? 2 * nw - 1 : 2 * (w + 1);
    const int lfv = draft[ws > 0 ? ws - 1 : 0], rfv = draft[we < Ld ? we : Ld - 1];
    const int lf = ws > 0 ? lfv : 4, rf = we < Ld ? rfv : 4;
    // the (at most three) alignment intervals this window spans: start columns relative to ws and lengths
    const int c1 = need_col(wb, nw, Ld, idx_ws + 1), c2 = (idx_ws + 2 <= idx_we) ? need_col(wb, nw, Ld, idx_ws + 2) : we;
    const int maxins = P.opts.max_insertion_size == 0 ? 30 : P.opts.max_insertion_size;
    {
        // level 2: everything that needs only z / r0 / the window bounds
        const int e0 = tid < CCSX_NOBS * 16 ? tid : 0;      // (observation e0 >> 4, context e0 & 15)
        const size_t tz = (size_t)z * 192;
        const int i0 = (e0 & 15) * CCSX_NOBS + (e0 >> 4);
        const float me0 = P.tabME[tz + i0], in0 = P.tabINS[tz + i0];
        const float dl = P.tabDL[(size_t)z * 16 + (tid & 15)];
        const float zp = P.tabZ[(size_t)z * 32 + (tid & 31)];
        const int tcl = tid < we - ws ? tid : we - ws - 1;
        const uint8_t dr = draft[ws + tcl];
        if (tid < CCSX_NOBS * 16) sCTX[(e0 >> 4) * CTXS + (e0 & 15)] = make_float2(me0, in0);
        if (tid < CTXS) sCTX[CCSX_NOBS * CTXS + tid] = make_float2(0.0f, 0.0f);
        if (tid < CCSX_NOBS) sCTX[tid * CTXS + (CTXS - 1)] = make_float2(0.0f, 0.0f);     // (the zero entry of every row)
        if (tid < TAB_TAIL) sZP[32 + tid] = 0.0f;            // (the padding behind sZP: part of the guard behind sTC)
        if (tid < 16) sDL[tid] = dl;
        if (tid < 32) sZP[tid] = zp;
        if (tid < we - ws) { sT[0][tid] = dr; sTd[tid] = dr; }
        if (tid == 0) { sCtl[0] = we - ws; sCtl[1] = wb0 - ws; sCtl[2] = wb1 - ws; }
    }
    // SPEC v5: a ZMW's passes (up to CCSX_MAX_PASSES = 255) are taken in GROUPS of PW_MAXREADS = 32: the per-read arrays below, the observation
    // codes and the chunk plan always describe one group (local read index = pass - g0).  A ZMW of at most 32 passes — most — loads
    // its one group here and never again; larger ones reload group after group in every round (rare, so the reload is not optimised).
    const int ngroups = (nreads + PW_MAXREADS - 1) / PW_MAXREADS;
    // levels 2 + 3 of the prologue for the reads g0 .. g0 + ng - 1: metadata, entry rows of the window's two edge columns, dirty masks
    auto load_meta = [&](int g0, int ng) -> int {
        int trimflag = 0;
        const int rcl = tid < ng ? tid : ng - 1;
        const int rr = r0 + g0 + rcl;
        const int64_t bo0 = P.base_off[rr], bo1 = P.base_off[rr + 1], eo = P.ent_off[rr];
        const int flr = P.flags[rr] & 1, av = P.avalid[rr];
        // level 3: entry rows of the window's two edge columns (in bounds for every read; ignored unless the read mapped)
        const int a = P.ent[eo + idx_ws], b = P.ent[eo + idx_we];
        const unsigned m1 = P.dmask[eo + idx_ws + 1];
        const unsigned m2 = (idx_ws + 2 <= idx_we) ? P.dmask[eo + idx_ws + 2] : 0u;
        const unsigned m3 = (idx_ws + 3 <= idx_we) ? P.dmask[eo + idx_ws + 3] : 0u;
        if (tid < ng) {
            const int L = (int)(bo1 - bo0);
            const int st = flr != fl0 ? 1 : 0;
            int n = -1, na = 0;
            if (av) {
                n = b - a;
                if (n > L) n = -1;                           // (entry rows are rows of this pass: anything else is not a segment)
                // SPEC "trim large insertions": a segment more than max_insertion_size bases longer than the window is cut down
                // to the window's length below (sBoff keeps the full length until the chunk plan re-uses it)
                if (n >= 0 && maxins > 0 && n > (we - ws) + maxins) { trimflag = 1; sBoff[tid] = n; n = we - ws; }
                else { sBoff[tid] = 0; if (n < 0 || n > CCSX_IMAX) n = -1; }
                na = st ? L - b : a;
            } else sBoff[tid] = 0;
            sI[tid] = n; sStrand[tid] = (uint8_t)st;
            sGoff[tid] = (int)(bo0 - bo_r0) + na;            // segment start relative to the ZMW's first base (sGoff is re-planned later)
            // interval k covers draft positions col(k-1) .. col(k)-1: bit (p - col(k-1))
            sDirty[tid] = av ? (m1 | (m2 << (c1 - ws)) | (m3 << (c2 - ws))) : 0u;
        }
        return trimflag;
    };
    // (the LAST group first: the candidate filter below walks the groups from the last to the first, so every group is loaded once and group 0 is the one that is
    // resident when the rounds begin — ADVICE r04: a ZMW of 33-64 passes used to load group 0 twice here and once more in round 0)
    const int glast = (ngroups > 1 ? ngroups - 1 : 0) * PW_MAXREADS;
    const int ng0 = nreads - glast < PW_MAXREADS ? nreads - glast : PW_MAXREADS;
    const int trimflag = load_meta(glast, ng0);
    int resident = glast;                                   // the group whose per-read arrays and observation codes are in LDS (wave-uniform)
    if (tid < (CCSX_MAX_PASSES + 32) / 32) sZdrop[tid] = 0u;
    // level 4 for the group's ng reads: the read segments (native orientation), four reads per wave in flight; then the rare trim
    auto load_obs = [&](int ng, int tflag) {
    const int anytrim = __syncthreads_or(tflag);
    for (int rb = 0; rb < ng; rb += 4 * (PWT / 64)) {
        uint8_t bq[4], pq[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = rb + (PWT / 64) * q + wave;
            const int n = r < ng ? sI[r] : -1;
            const int64_t p = bo_r0 + ((lane < n) ? sGoff[r] + lane : 0);
            bq[q] = P.bases[p]; pq[q] = P.pw[p];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = rb + (PWT / 64) * q + wave;
            if (r < ng) {
                const int n = sI[r];
                sObs[r][lane] = (lane < n) ? (uint8_t)obs_of(bq[q], pq[q]) : (uint8_t)(lane == n ? CCSX_NOBS : 0);   // row n: "no base"
                if (lane < 4) sObs[r][64 + lane] = 0;
            }
        }
    }
    if (anytrim) {
        // rare: cut over-long segments down to J bases = their first s and last J - s bases, s = the split with the most diagonal
        // matches of prefix and suffix against the window in read orientation (ties: the smallest s).  The main loop above has
        // already stored the first J codes; the same wave owns the read here.
        const int J0 = we - ws;
        for (int r = wave; r < ng; r += (PWT / 64)) {
            const int nfull = rfl(sBoff[r]);
            if (nfull == 0) continue;
            const int st = rfl((int)sStrand[r]);
            const int64_t p0 = bo_r0 + sGoff[r];
            const bool in = lane < J0;
            const int bp = in ? P.bases[p0 + lane] : 0;
            const int bs = in ? P.bases[p0 + nfull - J0 + lane] : 0, ps = in ? P.pw[p0 + nfull - J0 + lane] : 0;
            const int T = in ? (st ? 3 - (int)sTd[J0 - 1 - lane] : (int)sTd[lane]) : 9;
            const unsigned long long mp = __ballot(in && (bp & 3) == T), ms = __ballot(in && (bs & 3) == T);
            const int tot = (lane <= J0) ? __popcll(mp & ((1ull << lane) - 1ull)) + __popcll(ms >> lane) : -1;
            const int sb = 63 - (rfl(wave_max_i32((tot << 6) | (63 - lane))) & 63);
            if (in && lane >= sb) sObs[r][lane] = (uint8_t)obs_of(bs, ps);
        }
    }
    };
    load_obs(ng0, trimflag);
    // ---- step 7, candidate filter: pile-up margin of every window position over the reads with a usable segment (of every group: a ZMW
    // of more than 32 passes (PW_MAXREADS) walks its groups from the last to the first here, so that group 0 is the one loaded when the rounds begin)
    {
        int nuse = 0, nd = 0;                                 // (wave 0)
        for (int g0 = (ngroups - 1) * PW_MAXREADS; g0 >= 0; g0 -= PW_MAXREADS) {
            const int ng = nreads - g0 < PW_MAXREADS ? nreads - g0 : PW_MAXREADS;
            if (g0 != resident) {
                __syncthreads();
                const int tf = load_meta(g0, ng);
                load_obs(ng, tf);
                __syncthreads();
                resident = g0;
            }
            if (wave == 0) {
                const int vIr = lane < ng ? sI[lane] : -1;                      // lane = read: one load each, then v_readlane per read
                const unsigned vDr = lane < ng ? sDirty[lane] : 0u;
                for (int r = 0; r < ng; ++r) if (rl(vIr, r) >= 0) { ++nuse; nd += (int)(((unsigned)rl((int)vDr, r) >> (lane & 31)) & 1u); }
            }
        }
        if (wave == 0) {
            const int J0 = we - ws;
            const int margin = nuse - 2 * nd;
            const bool inw = lane < J0;
            const unsigned neg = (unsigned)__ballot(inw && margin < 0);
            // positions within SKIP_SPREAD of a dirty majority are polished too
            const unsigned nearneg = neg | (neg << 1) | (neg << 2) | (neg << 3) | (neg >> 1) | (neg >> 2) | (neg >> 3);
            const bool noheur = P.opts.disable_heuristics || (P.tflag && (P.tflag[z] & 2));   // (a flagged tandem repeat: DESIGN.md §2)
            const bool ok = inw && !noheur && margin >= SKIP_MARGIN && !((nearneg >> lane) & 1u);
            const unsigned ev = (unsigned)__ballot(ok);
            if (lane == 0) sCtl[7] = (int)ev;
            if (lane < 36) sPskip[lane] = inw ? skip_perr(margin, P.perr_floor) : 0.0f;
        }
    }
    const int half = lane >> 5, hrow = lane & 31;          // fill: which read of the pair, row within it
    PHASE(0);
#ifdef CCSX_EXIT_AFTER_PROLOGUE                             // experiment: what the prologue alone costs in kernel time
    __syncthreads();
    if (tid == 0) P.wsum[(size_t)(P.wb_off[z] - z) + w] = (float)sI[0] + (float)sObs[0][0] + sPskip[0] + sCTX[5].x;
    return;
#endif
#ifdef CCSX_EXP_REPEAT                                      // experiment: the compute of a window CCSX_EXP_REPEAT times after ONE prologue
    __syncthreads();                                        // (T(R=2) - T(R=1) = a window's compute without the memory latency at its head)
    const int xr_t = sT[0][tid & 31], xr_c0 = sCtl[0], xr_c1 = sCtl[1], xr_c2 = sCtl[2], xr_c7 = sCtl[7];
    const float xr_p = sPskip[tid < 36 ? tid : 0];
    for (int xrep = 0; xrep < CCSX_EXP_REPEAT; ++xrep) {
    __syncthreads();
    if (tid < 32) sT[0][tid] = (uint8_t)xr_t;
    if (tid < 36) sPskip[tid] = xr_p;
    if (tid < (CCSX_MAX_PASSES + 32) / 32) sZdrop[tid] = 0u;
    if (tid == 0) { sCtl[0] = xr_c0; sCtl[1] = xr_c1; sCtl[2] = xr_c2; sCtl[7] = xr_c7; }
    __syncthreads();
#endif
    // ---- the chunk plan of the resident group (lane = read), made by ONE wave, once per round and after every reload of a group inside a round: its inputs are
    // sI[], J, S and the LDS budget, all known when the round's J is.  The greedy walk — a chunk takes reads while their gamma/beta fit the budget, at most
    // PWCH of them — runs over all chunks by prefix sum and ballots and leaves, per read: sGoff / sBoff / sBand (sGoff = -1: no segment); per chunk, at its first
    // read rb: the end sRend[rb], the fill tasks sTask[rb ..].x (a read is in exactly one chunk, so the slices never overlap) and their counts in sTask[rb].y.
    // The barrier that opens every chunk publishes the plan; the other waves only read it.  (Until round 6 every wave recomputed the plan of every chunk.)
    // sGoff / sBoff hold the segment start / the untrimmed length until here: the caller has a barrier between load_obs and the plan.
    auto plan_chunks = [&](int ng, int J, int S) {
        int r = lane;
        asm volatile("" : "+v"(r));                          // (opaque: what the plan derives from the lane is formed here, not hoisted out of the rounds into registers that spill)
        const int n0 = r < ng ? sI[r] : -1;
        const FillBand fb = fill_band_of(n0 >= 0 ? n0 : 0, J, S);
        const int need0 = (2 * n0 + 3) * fb.rowsz;                       // gamma rows 0..n, beta rows 0..n+1 (row n+1: zeros)
        // a short segment whose band leaves a lane time to change rows (see the quad sweep) shares a wave with three others; the rest — more than
        // 31 bases, or |I - J| >= 5 — takes a wave of its own (rare)
        const bool qd0 = n0 <= 31 && fb.bw <= FILL16_MAXBW;
        const unsigned long long lower = (1ull << r) - 1ull;
        for (int rb = 0; rb < ng;) {
            const bool cand = n0 >= 0 && r >= rb;
            const int need = cand ? need0 : 0;
            const int incl = wave_scan_add_i32(need);
            const unsigned long long bcand = __ballot(cand);
            const unsigned long long over = __ballot(cand && (incl > GB_FLOATS || (PWCH > 0 && __popcll(bcand & lower) >= PWCH)));
            const int rend_ = over ? (int)__ffsll((long long)over) - 1 : ng;                 // the first read that does not fit any more
            if (r >= rb && r < rend_) {
                if (!cand) sGoff[r] = -1;
                else {
                    const int off = incl - need;
                    sGoff[r] = off + fb.org; sBoff[r] = off + (n0 + 1) * fb.rowsz + fb.org;
                    sBand[r] = fb.pitch | (fb.rowsz << 8) | (fb.bw << 16) | ((fb.dlo + 128) << 24);
                }
            }
            const bool inchunk = cand && r < rend_;
            const bool qd = inchunk && qd0, lng = inchunk && !qd0;
            const unsigned long long bl = __ballot(lng), bs = __ballot(qd);
            const int nl_ = __popcll(bl);
            if (lng) sTask[rb + __popcll(bl & lower)].x = (short)r;
            if (qd) sTask[rb + nl_ + __popcll(bs & lower)].x = (short)r;
            if (r == rb) { sRend[rb] = (uint8_t)rend_; sTask[rb].y = (short)(nl_ | (__popcll(bs) << 8)); }
            rb = rfl(rend_);
        }
    };
    int iters = 0, nonconv = 0;
    unsigned skmask = 0;                                     // positions skipped in the current round (wave-uniform)
    int nvalid_last = 0, nvfull_last = 0;                    // usable reads of the last round: all / full-length passes only
    const int nfull = P.nfull[z];
    for (int it = 0; it < CCSX_MAX_ITER; ++it) {
        // ---- the round set-up, from registers.  Everything up to the chunk-opening barrier depends on the window template (32 bytes) and two control words: every lane
        // loads its column's base, J and the evidence bits ONCE and takes the neighbours, the reverse complement and both strands' contexts from its own wave's lanes
        // (DPP shifts, one ds_bpermute); nothing the set-up writes is read back by the set-up, so no barrier stands inside it: three went (the one behind sT[1],
        // the two of the lane compaction), two remain — this one in front of it and the chunk-opening one, which publishes what it wrote
        // (profiles/polish_round_setup.txt).  Who wrote each word last, who reads it next, which barrier lies between:
        //   sT[0], sCtl[0 / 7]    written by the prologue or by wave 0's selection of the round before, in front of this barrier; read here by every wave
        //   sT[1]                 written here by wave 0; read by lane_mut in the scoring, behind the chunk-opening barrier (its readers of the round before: in front of
        //                         the barrier that ends the round).  The tables and the z-score sums used to take their bases from it and needed a barrier behind it
        //   sMvalid, sDeltaI,     written here, every entry by its own thread, every wave for its own 64-lane slice.  Read by the scoring (sList, the atomicAdd into
        //   sList                 sDeltaI) behind the chunk-opening barrier, by every wave behind the round's last barrier (the round's end, the QV terms); their readers
        //                         of the round before: in front of the barrier behind the selection.  Every wave evaluates the validity of all four slices (same column,
        //                         slots 2 q + (lane >> 5)): its base offset and the round's lane count are popcounts of its own ballots — no counts through LDS, none of
        //                         the compaction's two barriers
        //   sTC, sDLC             written here, four entries + one per thread, from sCTX / sDL (prologue); read by the fill behind the chunk-opening barrier (the fill of
        //                         the round before: in front of its own barrier)
        //   sZS                   written here in round 0 by waves 0 and 1; read by the validity step behind the fill's barrier
        // (Round 4 had measured the round without three of these barriers while every wave still walked the LDS chains between them: no gain then.  Measured with this
        // set-up and not kept: the four z-score sums as four chains on wave 2, + 3.8 ms of 270; this barrier folded into the one behind the selection in later rounds —
        // nothing is written between the two — + 0.5 ms.)
        __syncthreads();
        const int J = rfl(sCtl[0]);
        const unsigned evb = (unsigned)rfl(sCtl[7]);         // evidence bits of the candidate filter (wave-uniform)
        int tl = tid;
        asm volatile("" : "+v"(tl));                         // (opaque: what the set-up derives from the thread index is formed here, not hoisted out of the rounds into registers that spill)
        const int ll = tl & 63;
        const int c = tl & 31;                               // the lane's column: PWT is a multiple of 32, so it is the column of the thread's mutation lane and of its table entries too
        const int tc = (int)sT[0][c];                        // (columns from J on: stale bytes, never used)
        const float invJ2 = 1.0f / (float)(2 * J);           // band_row0's reciprocal
        const int S = (J + 2) & ~1;                          // EVEN row stride >= J+1: in the fill lane = row writes column t - row, so the
                                                             // lane-to-lane address stride is S - 1, which must be odd to be bank-conflict free
        const int lfr = (rf < 4) ? 3 - rf : 4;
        // (the wave shifts and both ds_bpermute below take their values from other lanes and need ALL 64 lanes of the wave active: an inactive source lane gives
        // the fill value / 0, not its base.  They stand in workgroup-uniform control flow; keep them out of any `if (tid < ...)`)
        const int tm1 = wave_shr1_i32(tc, 0), tp1 = wave_shl1_i32(tc, 0);                    // t[c-1], t[c+1] (lanes 0 / 32 and 31 / 63: not a neighbour; c > 0 and c + 1 < J guard them)
        const int rcc = 3 - __builtin_amdgcn_ds_bpermute(((J - 1 - c) & 31) << 2, tc);      // reverse complement: column c of strand 1 is 3 - t[J-1-c]
        const int rm1 = wave_shr1_i32(rcc, 0);
        if (tl < J) sT[1][tl] = (uint8_t)rcc;               // (lane_mut and the scoring read it, behind the chunk-opening barrier)
        // the contexts of column c on both strands; from J on: entry 16 of a row of sCTX, the exact zero pair
        const int fctx = c < J ? ctx_of(c > 0 ? tm1 : lf, tc) : CTXS - 1;
        const int rctx = c < J ? ctx_of(c > 0 ? rm1 : lfr, rcc) : CTXS - 1;
        // the chunk plan of the round, when the round's first group is the one in LDS (nearly always: a ZMW of more than PW_MAXREADS passes ends a round on its
        // last group and plans after the reload below).  The last wave: it has no share in the z-score sums of round 0
        if (wave == (PWT / 64) - 1 && resident == 0) plan_chunks(nreads < PW_MAXREADS ? nreads : PW_MAXREADS, J, S);
        // z-score expectation of the window template on each strand, summed in column order (SPEC); the gate is decided in round 0
        // only.  Lane j holds column j's terms, the ordered sums take them with v_readlane (no chain of dependent LDS loads).
        // No loop: CCSX_JMAX steps with immediate lane indices.  The lanes from J on contribute + 0.0f (their context CTXS - 1 = 16 reads sZP[16] and sZP[32], a variance
        // and the first float of the zeroed padding behind sZP: replaced), and a sum that starts at + 0.0f cannot become - 0.0f under round-to-nearest, so the added
        // zeros change no bit; the order of the real terms is the column order.  (A loop of J steps — a v_readlane with a scalar index, the dependent add and the branch
        // per step — kept waves 2 and 3 waiting at the chunk-opening barrier for longer; one chain per wave on all four waves was measured and is slower than two
        // chains on each of waves 0 and 1: profiles/polish_round_end.txt)
        if (it == 0 && wave < 2 && P.opts.min_zscore != 0.0f) {
            static_assert(CTXS == 17 && TAB_TAIL >= 1 && CCSX_JMAX < 32, "the z-score terms of a column from J on are read at sZP[CTXS - 1] and sZP[16 + CTXS - 1]");
            const int k = wave ? rctx : fctx;
            const float t0 = sZP[k], t1 = sZP[16 + k];
            const float mu = ll < J ? t0 : 0.0f, va = ll < J ? t1 : 0.0f;
            float M = 0.0f, V = 0.0f;
#pragma unroll
            for (int q = 0; q < CCSX_JMAX; ++q) {
                M = M + __int_as_float(rl(__float_as_int(mu), q));
                V = V + __int_as_float(rl(__float_as_int(va), q));
            }
            if (lane == 0) { sZS[2 * wave] = M; sZS[2 * wave + 1] = V; }
        }
        // positions skipped this round: evidence bit set and not inside a homopolymer of the CURRENT template
        {
            const int tcv = c < J ? tc : 9;
            const int prev = c > 0 ? (c - 1 < J ? tm1 : 8) : lf, next = c + 1 < J ? tp1 : rf;
            const bool hp = (prev == tcv) || (next == tcv);
            skmask = (unsigned)__ballot(ll < J && ((evb >> c) & 1u) && !hp);
        }
        // valid mutation lanes of this round, compacted: lane m = slot*32 + c is valid iff the SPEC enumerates it;
        // thread t then scores the t-th valid lane, so unused lanes cost nothing
        auto lane_valid = [&](int sl) -> int {               // slot sl (0 .. 7) of the lane's column
            int v;
            if (sl < 3) v = c < J;
            else if (sl == 3) v = c < J && !(c > 0 && tm1 == tc);
            else v = c <= J && !(c > 0 && tm1 == sl - 4);
            const int cc = c < J ? c : J - 1;               // candidate filter (insertions after the last column follow J-1)
            if (v && ((skmask >> cc) & 1u)) v = 0;
            // a quiet position inside a homopolymer keeps only the mutations that change the run's LENGTH: deletion of the
            // run's first base, insertion of the run's base before it (the enumeration admits both at run starts only)
            else if (v && ((evb >> cc) & 1u) && !(c < J && (sl == 3 || (sl >= 4 && sl - 4 == tc)))) v = 0;
            return v;
        };
        int nvm = 0;
        {
            static_assert(PWT == 256, "the set-up: eight slots of 32 columns, two per wave");
            unsigned long long mine = 0ull;
            int basew = 0;
#pragma unroll
            for (int q = 0; q < (PWT / 64); ++q) {
                const unsigned long long b = __ballot(lane_valid(2 * q + (ll >> 5)));
                const int n = __popcll(b);
                if (q < wave) basew += n;
                if (q == wave) mine = b;
                nvm += n;
            }
            const int v0 = (int)((mine >> ll) & 1ull);
            sMvalid[tl] = (uint8_t)v0; sDeltaI[tl] = 0;
            if (v0) sList[basew + __popcll(mine & ((1ull << ll) - 1ull))] = (uint8_t)tid;
        }
        // the fill's per-column tables of this round's template.  sTC[strand][obs][column]: the pair of the column's context in
        // the observation's row of sCTX — zeros from column J on ("no stay in the final column") and for observation 12 ("no base": the zero row);
        // sDLC[strand][column]: DL of the column's context, 1 outside 0 .. J-1 (beta's start value passes through column J as 1 * beta).  Boundary cells are data,
        // not control: the sweeps are branch-free.
        {
            static_assert(PWT == 256 && TC_ROW == 32 && 2 * TC_STRAND <= 4 * PWT && DLC_TOTAL <= PWT, "the set-up: four sTC entries and one sDLC entry per thread");
            // entry tid + 256 k is row (tl >> 5) + 8 k of the 26 (strand, observation) rows, column c: one sCTX read per entry, all reads before the stores
            const int row0 = tl >> 5;
            const int ej = tl - TC_LO - (tl >= TC_LO + 33 ? DLC_S : 0);                   // the column of the thread's sDLC entry: its contexts sit in lane ej & 31
            const int both = __builtin_amdgcn_ds_bpermute((ej & 31) << 2, fctx | (rctx << 8));
            float2 v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int r = row0 + 8 * k, sd = r >= CCSX_NOBS + 1 ? 1 : 0, o = r - sd * (CCSX_NOBS + 1);
                v[k] = sCTX[r < 2 * (CCSX_NOBS + 1) ? o * CTXS + (sd ? rctx : fctx) : 0];
            }
            const bool inw = ej >= 0 && ej < J;
            const float dv = sDL[inw ? (tl >= TC_LO + 33 ? both >> 8 : both & 255) : 0];
#pragma unroll
            for (int k = 0; k < 4; ++k) if (row0 + 8 * k < 2 * (CCSX_NOBS + 1)) sTC[tl + PWT * k] = v[k];
            // (the entry right in front of sTC is column -1 of strand 0's observation row 0: row 1's lane reads it at step 0 while row 0's start value 1 is still in its
            // neighbour, so its ME has to be an exact zero like column 31 of the row before every other observation row — no lane uses a DL that far out)
            if (tl < DLC_TOTAL) sDLC[tl] = tl >= DLC_TOTAL - 2 ? 0.0f : (inw ? dv : 1.0f);
        }
        const int nblk = (nvm + 63) >> 6;
        PHASE(1);
        int nvalid = 0, nvfull = 0;
        int curblk = -1;                                     // the block whose lane constants this wave holds (they survive the chunks of a round)
        LanePk LF, LR;
        int myM = 0; bool mval = false;
        // ---- groups of PW_MAXREADS passes (one group for nearly every ZMW), and in a group: chunks of reads whose gamma/beta fit the LDS budget
        for (int g0 = 0; g0 < nreads; g0 += PW_MAXREADS) {
        const int ng = nreads - g0 < PW_MAXREADS ? nreads - g0 : PW_MAXREADS;
        if (g0 != resident) {                                // (the per-read arrays and observation codes of the group; one group only: never reloaded)
            __syncthreads();
            const int tf = load_meta(g0, ng);
            load_obs(ng, tf);
            resident = g0;
            __syncthreads();                                 // (load_obs read the segment starts and untrimmed lengths that the plan overwrites)
            if (wave == (PWT / 64) - 1) plan_chunks(ng, J, S);
        }
        int rbeg = 0;
        while (rbeg < ng) {
            __syncthreads();                                 // (publishes the chunk plan, too)
            const int rend = rfl((int)sRend[rbeg]), ntasks = rfl((int)sTask[rbeg].y), nlong = ntasks & 255, nshort = ntasks >> 8;
            const short2 *const cTask = sTask + rbeg;        // the chunk's fill tasks
            PHASE(2);
            // ---- A1/A2: fill (SPEC v6: on the band of diagonals only).  Work units, one wave each, every unit ONE anti-diagonal sweep:
            //   quad units — FOUR short reads per wave, one per 16-lane DPP row, alpha and beta of a quad on different waves;
            //   long units — one read per wave (lane = row), alpha and beta on different waves.
            // alpha(I,J) / beta(0,0) of a read meet in LDS, and every wave derives the reads' validity from them after the barrier (lane = read; identical values
            // in every wave: no second barrier).  Eight short reads = two quads = four units: every wave runs one sweep per chunk.
#ifdef CCSX_EXP_NO_FILL                                     // experiment (timing only, wrong results)
            const int nquad = 0, nunit_f = 0, rpq = 4;
#else
            // (reads per quad unit: always four.  Spreading a small chunk — three passes, the tail chunk of ten — over all the waves, two reads or one per unit, was
            // measured and is SLOWER: k_polish 313.9 against 301.6 ms at 10 passes, 95.8 against 92.4 at 3 — the kernel is bound by its instruction count, and a
            // sweep costs the same instructions whatever it holds)
            const int rpq = 4;
            const int nquad = (nshort + rpq - 1) / rpq, nunit_f = 2 * nquad + 2 * nlong;
#endif
            for (int fu = wave; fu < nunit_f; fu += (PWT / 64)) {
              if (fu < 2 * nquad) {
                // ---- quad unit.  Lane l of a DPP row owns read rows l and l + 16 (a short segment has at most 32 rows): row i is on the band for the 15-or-so
                // steps t = i + j in [2 i + dlo, 2 i + dhi], row i + 16 exactly 32 steps later, so with a band of at most FILL16_MAXBW = 24 diagonals the lane is
                // idle for at least 8 steps in between and changes rows there.  The neighbour row's cell comes by a ROTATION inside the DPP row (row_ror: lane 0
                // takes lane 15, whose row 15 precedes lane 0's row 16; while lane 0 is on row 0, lane 15 has not started and holds a zero).  A lane that is not on
                // the band holds a zero running cell, which is what its neighbours must read past the band's edge.  Look-ups run four steps ahead: slot k holds DL and the
                // (ME, INS) pair of the step's column — read from the per-column tables sDLC / sTC at a running pointer + immediate — and is refilled right after use.  The row
                // change therefore happens in two parts: the look-up side (observation row of sTC, 16 columns back) at the first iteration whose look-ups no longer
                // serve the old row, the compute side (activity window, store pointer) one iteration later.
                const int quad = fu >> 1, isb = fu & 1;
                const int g4 = lane >> 4, l16 = lane & 15;
                const int qi = rpq * quad + g4;
                const bool have = g4 < rpq && qi < nshort;
                const int myr = cTask[nlong + (have ? qi : rpq * quad)].x;
                const int I = sI[myr], sd = sStrand[myr], band = sBand[myr];
                const int pitch = band & 255, rowsz = (band >> 8) & 255, bdlo = (int)((unsigned)band >> 24) - 128, bdhi = bdlo + ((band >> 16) & 255) - 1;
                const int row0 = l16, row1 = l16 + 16;
                const bool ok0 = have && row0 <= I, ok1 = have && row1 <= I;
                const int jlo0 = (row0 + bdlo > 0) ? row0 + bdlo : 0, jhi0 = (row0 + bdhi < J) ? row0 + bdhi : J;
                const int jlo1 = (row1 + bdlo > 0) ? row1 + bdlo : 0, jhi1 = (row1 + bdhi < J) ? row1 + bdhi : J;
                int Tmax = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) { const int iq = rfl(sI[rfl((int)cTask[nlong + ((q < rpq && rpq * quad + q < nshort) ? rpq * quad + q : rpq * quad)].x)]); Tmax = iq > Tmax ? iq : Tmax; }
                Tmax += J;
                const int NEVER = 1 << 20;
#define LDPR(ROWP, OFF) (*(const float2 *)((ROWP) + (OFF)))
                if (!isb) {
                    // alpha: row 0 first.  Step t: the lane's row i computes column j = t - i
                    const int obA0 = OBS_TC((row0 >= 1 && ok0) ? (int)sObs[myr][row0 - 1] : 12);       // o_{i-1}; 12 = no base: row 0 has no diagonal / stay
                    const int obA1 = OBS_TC(ok1 ? (int)sObs[myr][row1 - 1] : 12);
                    // tA[x] (bytes: 8 x) = the pair of column x - row in the lane's observation row of sTC; dA[x] = DL of column x - row - 1.  Both run with t; the
                    // look-up side changes rows (observation row, 16 columns back) one iteration before the compute side
                    const char *tA = (const char *)(sTC + sd * TC_STRAND) + obA0 - 8 * row0;
                    const int dtA = obA1 - obA0 - 8 * 16;
                    const float *dA = sDLC + sd * DLC_S + (TC_LO - 1 - row0);
                    const int tA0 = ok0 ? row0 + jlo0 : NEVER, tA1 = row1 + jlo1;
                    unsigned uJ = ok0 ? (unsigned)(jhi0 - jlo0) : 0u;
                    const unsigned uJ1 = (unsigned)(jhi1 - jlo1);
                    const int tsw = ok1 ? ((row0 + jhi0) & ~3) : NEVER;          // = the first multiple of 4 >= (last step of row i) - 3
                    float *gA = sGB + sGoff[myr] + row0 * pitch - row0;               // gA[x] = gamma(row, x - row)
                    const int dgA = 16 * (pitch - 1), dcnt = tA0 - tA1;
                    float acur = (ok0 && row0 == 0) ? 1.0f : 0.0f, mnext = 0.0f;     // mnext = alpha(i-1, j-1) * ME(j-1) of the next step, formed a step ahead
#define CCSX_A_INIT(K) float dl##K = dA[K]; float2 p##K = LDPR(tA, 8 * (K));
                    CCSX_A_INIT(0) CCSX_A_INIT(1) CCSX_A_INIT(2) CCSX_A_INIT(3)
#undef CCSX_A_INIT
                    int cnt = -tA0;
#define CCSX_A_STEP(K)                                                                                                     \
                    {                                                                                                      \
                        const float up = row_ror1_f32(acur);         /* alpha(i-1, j) */                                     \
                        const float gmm = __builtin_fmaf(acur, dl##K, mnext);   /* SPEC v8: fused */                      \
                        const unsigned long long on = __builtin_amdgcn_uicmp((unsigned)(cnt + (K)), uJ, 37 /* ule */);    \
                        if (__builtin_amdgcn_inverse_ballot_w64(on)) gA[(K)] = gmm;                                        \
                        acur = lanes_or_zero(on, __builtin_fmaf(up, p##K.y, gmm));   /* row 0 and column J read zero entries: + 0.  (ONE compare: the mask serves the store's exec and the select) */ \
                        mnext = up * p##K.x;                                                                               \
                        p##K = LDPR(tA, 8 * ((K) + 4));              /* the slot's next use: four steps on */              \
                        dl##K = dA[(K) + 4];                                                                               \
                    }
                    for (int t = 0; t <= Tmax; t += 4, tA += 32, dA += 4, gA += 4, cnt += 4) {
                        if (t == tsw) { tA += dtA; dA -= 16; }
                        if (t - 4 == tsw) { uJ = uJ1; cnt += dcnt; gA += dgA; }
                        CCSX_A_STEP(0) CCSX_A_STEP(1) CCSX_A_STEP(2) CCSX_A_STEP(3)
                    }
#undef CCSX_A_STEP
                    // (a lane's running cell is zero once its row has left the band: alpha(I,J) = gamma(I,J) — no stay in the final column — is read back from LDS)
                    if (have && l16 == 0) sBase[myr] = sGB[sGoff[myr] + I * pitch + J];
                } else {
                    // beta: row I first.  Step t: the lane's row i computes column j = J - (t - (I - i)); a lane with two rows starts on row l + 16
                    const int rowF = ok1 ? row1 : row0, jloF = ok1 ? jlo1 : jlo0, jhiF = ok1 ? jhi1 : jhi0;
                    const int obB0 = OBS_TC((ok0 && row0 < I) ? (int)sObs[myr][row0] : 12);             // o_i; 12 = no base: row I emits nothing more
                    const int obBF = ok1 ? OBS_TC(row1 < I ? (int)sObs[myr][row1] : 12) : obB0;
                    // tB[-x] (bytes: -8 x) = the pair of column J + I - row - x in the lane's observation row of sTC; dB[-x] = DL of that column
                    const char *tB = (const char *)(sTC + sd * TC_STRAND) + obBF + 8 * (J + I - rowF);
                    const int dtB = obB0 - obBF + 8 * 16;
                    const float *dB = sDLC + sd * DLC_S + (TC_LO + J + I - rowF);
                    const int tB0 = ok0 ? I - rowF + J - jhiF : NEVER, tB1 = I - row0 + J - jhi0;
                    unsigned uJ = ok0 ? (unsigned)(jhiF - jloF) : 0u;
                    const unsigned uJ1 = (unsigned)(jhi0 - jlo0);
                    const int tsw = ok1 ? ((I - row1 + J - jlo1) & ~3) : NEVER;
                    float *bE = sGB + sBoff[myr] + rowF * pitch + (J + I - rowF);     // bE[-x] = beta(row, J + I - row - x)
                    const int dbE = -16 * (pitch - 1), dcnt = tB0 - tB1;
                    float bcur = (ok0 && rowF == I) ? 1.0f : 0.0f, t1next = 0.0f;    // t1next = ME(j) * beta(i+1, j+1) of the next step
#define CCSX_B_INIT(K) float dk##K = dB[-(K)]; float2 q##K = LDPR(tB, -8 * (K));
                    CCSX_B_INIT(0) CCSX_B_INIT(1) CCSX_B_INIT(2) CCSX_B_INIT(3)
#undef CCSX_B_INIT
                    int cnt = -tB0;
#define CCSX_B_STEP(K, KN)                                                                                                 \
                    {                                                                                                      \
                        const float dn = row_rol1_f32(bcur);         /* beta(i+1, j) */                                    \
                        const float bv = __builtin_fmaf(dk##K, bcur, __builtin_fmaf(q##K.y, dn, t1next));   /* SPEC v8: fused */ \
                        const unsigned long long on = __builtin_amdgcn_uicmp((unsigned)(cnt + (K)), uJ, 37 /* ule */);    \
                        if (__builtin_amdgcn_inverse_ballot_w64(on)) bE[-(K)] = bv;                                        \
                        bcur = lanes_or_zero(on, bv);                                                                      \
                        t1next = q##KN.x * dn;                       /* (slot KN holds the pair of the next step's column) */ \
                        q##K = LDPR(tB, -8 * ((K) + 4));                                                                   \
                        dk##K = dB[-(K) - 4];                                                                              \
                    }
                    for (int t = 0; t <= Tmax; t += 4, tB -= 32, dB -= 4, bE -= 4, cnt += 4) {
                        if (t == tsw) { tB += dtB; dB += 16; }
                        if (t - 4 == tsw) { uJ = uJ1; cnt += dcnt; bE += dbE; }
                        CCSX_B_STEP(0, 1) CCSX_B_STEP(1, 2) CCSX_B_STEP(2, 3) CCSX_B_STEP(3, 0)
                    }
#undef CCSX_B_STEP
                    // zero row I+1 of beta; beta(0,0)
                    const int org_ = pitch == S ? 0 : -bdlo;
                    if (have) for (int x = l16; x < rowsz; x += 16) sGB[sBoff[myr] - org_ + (I + 1) * rowsz + x] = 0.0f;
                    if (have && l16 == 0) sB00[myr] = sGB[sBoff[myr]];
                }
#undef LDPR
              } else {
                // ---- long unit: one read per wave, lane = row, the plain loop (alpha-only or beta-only)
                const int tk = (fu - 2 * nquad) >> 1, mode = 1 + ((fu - 2 * nquad) & 1);      // 1: alpha only, 2: beta only
                const int myr = rfl((int)cTask[tk].x);
                const int row = lane;
                const int I = rfl(sI[myr]);
                const int Tmax = I + J;
                const int sd = sStrand[myr];
                const float *dlcol = sDLC + sd * DLC_S + TC_LO;      // DL by column (1 at column J)
                const bool rowok = row <= I;
                // SPEC v6: the columns of this lane's row that lie on the read's band, jlo .. jhi; the cells outside are zeros and are neither computed nor stored
                const int band = sBand[myr];
                const int pitch = band & 255, rowsz = (band >> 8) & 255, bdlo = (int)((unsigned)band >> 24) - 128, bdhi = bdlo + ((band >> 16) & 255) - 1;
                const int jlo = (row + bdlo > 0) ? row + bdlo : 0, jhi = (row + bdhi < J) ? row + bdhi : J;
                // the lane's observation rows of the per-column table sTC
                const int op = OBS_TC((row >= 1 && rowok) ? (int)sObs[myr][row - 1] : 12);     // o_{i-1}; 12 = no base: row 0 has no diagonal / stay
                const int oc = OBS_TC((row < I) ? (int)sObs[myr][row] : 12);                    // o_i;     12 = no base: row I emits nothing more
                const float2 *rowA = (const float2 *)((const char *)(sTC + sd * TC_STRAND) + op), *rowB = (const float2 *)((const char *)(sTC + sd * TC_STRAND) + oc);
                // activity windows: alpha computes column j = t - row for t in [row + jlo, row + jhi]; beta computes column
                // jb = J - (t - (I - row)) for t in [I - row + J - jhi, I - row + J - jlo]
                const int tA0 = rowok ? row + jlo : (1 << 20), tB0 = rowok ? I - row + J - jhi : (1 << 20);
                const float one0 = (row == 0) ? 1.0f : 0.0f, oneI = (row == I) ? 1.0f : 0.0f;
                float *gA = sGB + sGoff[myr] + row * pitch - row;
                float *bB = sGB + sBoff[myr] + row * pitch + (J + I - row - 1);
                // start values chosen so that the general recurrence yields the boundary cells: gamma(i,0) = 0*x + one0*1,
                // beta(i,J) = (0 + 0) + 1*oneI (column J of the tables is zero with DL = 1)
                float acur = one0, updiag = 0.0f, mePrev = 0.0f, dlPrev = 1.0f;
                float bcur = oneI, dndiag = 0.0f;
                // a lane whose step is not on the band holds a ZERO running cell (SPEC v6: its neighbours read the cell past the band's edge as zero); row 0 / row I
                // keep their start value until their first step, which is the sweep's first
                const unsigned uJ = rowok ? (unsigned)(jhi - jlo) : 0u;   // (a lane beyond the read's rows: tA0 / tB0 keep it off; its jlo .. jhi may be an empty, i.e. negative, range)
                const int tAc = rowok ? row : (1 << 20);             // (the loop carries ME / DL of the previous column from column 0 on)
                const unsigned uJc = (unsigned)J;
                if (mode == 1) {
                    for (int t = 0; t <= Tmax; t += 2, gA += 2) {
#define CCSX_LA_STEP(T, AOFF)                                                                                         \
                        {                                                                                                  \
                            const float up = wave_shr1_f32_z(acur);  /* all rows of the read shift together (full exec) */ \
                            float nv = 0.0f;                                                                               \
                            if ((unsigned)((T) - tAc) <= uJc) {      /* alpha, column j = T - row of the window */        \
                                const float2 pr = rowA[(T) - row];                                                         \
                                const float dlc = dlcol[(T) - row];                                                        \
                                const float gmm = __builtin_fmaf(acur, dlPrev, updiag * mePrev);                           \
                                if ((unsigned)((T) - tA0) <= uJ) { gA[(AOFF)] = gmm; nv = __builtin_fmaf(up, pr.y, gmm); }   /* ... on the band; row 0 and column J read zero entries: + 0 */ \
                                mePrev = pr.x; dlPrev = dlc;                                                               \
                            }                                                                                              \
                            acur = nv;                                                                                     \
                            updiag = up;                                                                                   \
                        }
                        CCSX_LA_STEP(t, 0)
                        CCSX_LA_STEP(t + 1, 1)
#undef CCSX_LA_STEP
                    }
                    if (lane == 0) sBase[myr] = sGB[sGoff[myr] + I * pitch + J];   // (alpha(I,J) = gamma(I,J): no stay in the final column)
                } else {
                    for (int t = 0; t <= Tmax; t += 2, bB -= 2) {
#define CCSX_LB_STEP(T, BOFF)                                                                                         \
                        {                                                                                                  \
                            const float dn = wave_shl1_f32_z(bcur);                                                        \
                            float nv = 0.0f;                                                                               \
                            if ((unsigned)((T) - tB0) <= uJ) {       /* beta, column jb = J - (T - (I - row)), on the band */ \
                                const int jb = J + I - row - (T);    /* the column the step computes */                   \
                                const float2 pr = rowB[jb];                                                                \
                                const float bv = __builtin_fmaf(dlcol[jb], bcur, __builtin_fmaf(pr.y, dn, pr.x * dndiag)); \
                                bB[(BOFF)] = bv;                                                                           \
                                nv = bv;                                                                                   \
                            }                                                                                              \
                            bcur = nv;                                                                                     \
                            dndiag = dn;                                                                                   \
                        }
                        CCSX_LB_STEP(t, 1)
                        CCSX_LB_STEP(t + 1, 0)
#undef CCSX_LB_STEP
                    }
                    const int org_ = pitch == S ? 0 : -bdlo;      // (row layout: no origin shift)
                    if (row < rowsz) sGB[sBoff[myr] - org_ + (I + 1) * rowsz + row] = 0.0f;
                    if (lane == 0) sB00[myr] = sGB[sBoff[myr]];
                }
              }
            }
            __syncthreads();
            PHASE(3);
            // read validity (lane = read; every wave computes the same values): alpha/beta agreement, the z-score gate of round 0.  The two logarithms are repeated
            // in every wave on purpose: taking them once, in the fill unit's lane that holds the value, and loading them here was measured at -0.2 ms of 291 alone and
            // + 1.8 ms on top of the once-per-round chunk plan (profiles/polish_once_per_round.txt): nothing
            int vOk = 0; float vLa = 0.0f;
            if (lane >= rbeg && lane < rend && sGoff[lane] >= 0) {
                const float aIJ = sBase[lane], b00 = sB00[lane];
                const int I = sI[lane], sd = sStrand[lane];
                if (aIJ > TINY_P && b00 > TINY_P) {
#ifdef CCSX_EXP_CHEAP_VALIDITY                              // experiment (timing only, wrong results): what the two logarithms of the validity step cost
                    vLa = aIJ; const float lb = b00 - (b00 - aIJ);
#else
                    vLa = det_log2f(aIJ); const float lb = det_log2f(b00);
#endif
                    float df = vLa - lb; if (df < 0.0f) df = -df;
                    vOk = !(df > AB_TOL);
                    if ((sZdrop[g0 >> 5] >> lane) & 1u) vOk = 0;       // (g0 is a multiple of PW_MAXREADS = 32, lane < 32 here)
                    else if (vOk && it == 0 && P.opts.min_zscore != 0.0f) {   // A7 z-score gate, round 0 only (x4 per emitted base = 2 bits per read base)
                        const float zd = (vLa - (float)(2 * I)) - sZS[2 * sd];
                        const float zm = P.opts.min_zscore;
                        if (zd < 0.0f && zd * zd > (zm * zm) * sZS[2 * sd + 1]) { vOk = 0; atomicOr(&sZdrop[g0 >> 5], 1u << lane); }   // (every wave sets the same bit)
                    }
                }
            }
#ifdef CCSX_EXP_ALL_VALID                                   // experiment (timing only): every read with a segment counts as usable, whatever the fill produced
            vOk = (lane >= rbeg && lane < rend && sGoff[lane] >= 0) ? 1 : 0;
#endif
            // usable reads of the chunk, in read order: every wave builds the list in a register (lane k = the k-th usable read) with one
            // ds_permute (valid lane r sends r to lane rank(r), the others fill the remaining lanes): no LDS list, no second barrier
            int vRlist, nv_chunk;
            {
                const bool v = vOk != 0;
                const unsigned long long bv = __ballot(v), lower = (1ull << lane) - 1ull;
                nv_chunk = rfl(__popcll(bv));
                nvfull += __popcll(bv & (nfull - g0 >= 64 ? ~0ull : (nfull - g0 <= 0 ? 0ull : (1ull << (nfull - g0)) - 1ull)));   // (partial passes sit behind the full ones)
                const int dest = v ? __popcll(bv & lower) : nv_chunk + __popcll(~bv & lower);
                vRlist = __builtin_amdgcn_ds_permute(dest << 2, lane);
            }
            PHASE(7);
            // ---- A3/A4: work pool.  A unit = (block of 64 compacted mutation lanes) x (one usable read), numbered block-major; every
            // wave takes an equal contiguous share and walks it two reads at a time (two independent chains per lane) while the
            // block stays the same — 2 blocks x 5 reads are 3+3+2+2 units, not 2+2+1+1 pair tasks.  Gains are added to sDeltaI in
            // fixed point (order independent).
            {
#ifdef CCSX_EXP_SKIP_ROUND2_SCORE
                const int nv = nv_chunk, nunits = (it == 0) ? nblk * nv : 0;   // experiment: upper bound of what neighbourhood-only rescoring could save
#elif defined(CCSX_EXP_NO_SCORE)
                const int nv = nv_chunk, nunits = 0;
#else
                const int nv = nv_chunk, nunits = nblk * nv;
#endif
                nvalid += nv;
                // per-read scalars of the chunk's usable reads, one read per lane: a unit takes them with v_readlane (no chain of
                // dependent LDS loads at the start of every unit)
                int vR, vI, vSt, vG, vB, vBd; float vBase;
                {
                    vR = lane < nv ? vRlist : rl(vRlist, 0);
                    vI = sI[vR]; vSt = (int)sStrand[vR]; vG = sGoff[vR]; vB = sBoff[vR]; vBd = sBand[vR]; vBase = __shfl(vLa, vR);
                }
                const int u_end = ((wave + 1) * nunits) / (PWT / 64);
                for (int u = (wave * nunits) / (PWT / 64); u < u_end;) {
                    int blk = 0, k0 = u;                                     // u = blk * nv + k0 (a window has one or two blocks of lanes: no integer division)
                    while (k0 >= nv) { k0 -= nv; ++blk; }
                    const bool two = (u + 1 < u_end) && (k0 + 1 < nv);       // the next unit is mine and in the same block
                    u += two ? 2 : 1;
                    if (blk != curblk) {
                        curblk = blk;
                        const int li = blk * 64 + lane;
                        mval = li < nvm;
                        myM = mval ? sList[li] : 0;
                        const int slot = myM >> 5, cpos = myM & 31;
                        int type, x = 0;
                        const uint8_t *t = sT[0];
                        if (slot < 3) { type = 0; x = (t[cpos < J ? cpos : 0] + 1 + slot) & 3; }
                        else if (slot == 3) type = 1;
                        else { type = 2; x = slot - 4; }
                        if (mval) {
                            LF = lane_pack(lane_mut(type, cpos, x, sT[0], J, lf, sDL));
                            LR = lane_pack(lane_mut(type, (type == 2) ? J - cpos : J - 1 - cpos, 3 - x, sT[1], J, lfr, sDL));
                        } else { LF = lane_pack(lane_mut(0, 0, 0, sT[0], J, lf, sDL)); LR = LF; }
                    }
                    int dq;
                    if (!two) {
                        // a single unit (the usual case with four reads per chunk and one block of lanes): one chain, and none of the
                        // second chain's set-up
                        const int ra = rl(vR, k0), Ia = rl(vI, k0);
                        LanePk Ka = rl(vSt, k0) ? LR : LF;
                        asm volatile("" : "+v"(Ka.pk));                       // (unpacked HERE, per unit: hoisted out of the unit loop the fields would be live across it again)
                        const LaneMut La = lane_unpack(Ka);
                        const int gA_ = rl(vG, k0), bA_ = rl(vB, k0), bdA = rl(vBd, k0);
                        const int pA = bdA & 255, dloA = (int)((unsigned)bdA >> 24) - 128; const unsigned bwA = (unsigned)(bdA >> 16) & 255u;
                        const int dA = Ia > J ? Ia - J : J - Ia, WrA = SCORE_BAND + (dA > 2 ? dA - 2 : 0);
#ifdef CCSX_EXP_NO_ROWS                                     // experiment (timing only): a unit without its rows
                        const int nrA = 0;
#else
                        const int nrA = (Ia < 2 * WrA ? Ia : 2 * WrA) + 1;
#endif
                        const int i0a = band_row0(La.c, Ia, 2 * J, invJ2, J, WrA, nrA);
                        lds_cc tAa = (lds_cc)(sCTX + La.kA), tBa = (lds_cc)(sCTX + La.kB);
                        ScoreChain ca;
                        ca.ap = ca.bp = ca.acc = ca.b = 0.0f; ca.pA = ca.pB = make_float2(0.f, 0.f);
                        ca.g = (lds_cf)(sGB + gA_ + __mul24(i0a, pA) + La.c); ca.be = (lds_cf)(sGB + bA_ + __mul24(i0a, pA) + La.q);
                        ca.dg = La.c - i0a - dloA;
                        ca.bq = *ca.be; if ((unsigned)(La.q - i0a - dloA) >= bwA) ca.bq = 0.0f;   // beta(i0, q): the first row's own cell, a zero off the band
                        ca.be += pA;
                        const unsigned limA = bwA - 1u - (unsigned)La.qoff;
                        ca.op = (lds_cu8)(&sObs[ra][0] + i0a);
                        asm volatile("" : "+v"(ca.g), "+v"(ca.be), "+v"(tAa), "+v"(tBa), "+v"(ca.op));
                        // one chain: the loads of row i + 1 are issued in front of row i's arithmetic (X and Y take turns)
                        for (int k = 0; k < nrA; k += SCORE_OBS_ROWS) {
                            const int na = nrA - k < SCORE_OBS_ROWS ? nrA - k : SCORE_OBS_ROWS;
                            obs_words(ca, ca.op + k);
                            RowLoads X, Y;
                            int ia = 0;
                            rs_load(ca, X, tAa, tBa, pA);
                            for (; ia + 3 <= na; ia += 2) {                    // (two rows with a third behind them)
                                rs_load(ca, Y, tAa, tBa, pA); RS_FENCE();
                                rs_compute(ca, La, X, limA); RS_FENCE();
                                rs_load(ca, X, tAa, tBa, pA); RS_FENCE();
                                rs_compute(ca, La, Y, limA); RS_FENCE();
                            }
                            if (ia + 2 <= na) {                                // the block's last two rows
                                rs_load(ca, Y, tAa, tBa, pA); RS_FENCE();
                                rs_compute(ca, La, X, limA); RS_FENCE();
                                rs_compute(ca, La, Y, limA);
                            } else rs_compute(ca, La, X, limA);
                        }
                        const float res = La.fin ? ca.b : ca.acc;
#ifdef CCSX_EXP_NO_SCORE_LOG                                // experiment (timing only): a unit without its logarithm and fixed-point conversion
                        dq = __float_as_int(res) >> 20;
#else
                        dq = dq_fix(det_log2f(res) - __int_as_float(rl(__float_as_int(vBase), k0)));
#endif
                    } else {
                    const int k1 = k0 + 1;
                    const int ra = rl(vR, k0), rb = rl(vR, k1);
                    const int Ia = rl(vI, k0), Ib = rl(vI, k1);
                    LanePk Ka = rl(vSt, k0) ? LR : LF, Kb = rl(vSt, k1) ? LR : LF;
                    asm volatile("" : "+v"(Ka.pk), "+v"(Kb.pk));
                    const LaneMut La = lane_unpack(Ka), Lb = lane_unpack(Kb);
                    const int gA_ = rl(vG, k0), bA_ = rl(vB, k0), gB_ = rl(vG, k1), bB_ = rl(vB, k1), bdA = rl(vBd, k0), bdB = rl(vBd, k1);
                    const int pA = bdA & 255, dloA = (int)((unsigned)bdA >> 24) - 128; const unsigned bwA = (unsigned)(bdA >> 16) & 255u;
                    const int pB = bdB & 255, dloB = (int)((unsigned)bdB >> 24) - 128; const unsigned bwB = (unsigned)(bdB >> 16) & 255u;
                    // SPEC "banded link": every lane scores the rows around its column's point on the window diagonal only
                    const int dA = Ia > J ? Ia - J : J - Ia, WrA = SCORE_BAND + (dA > 2 ? dA - 2 : 0);
                    const int nrA = (Ia < 2 * WrA ? Ia : 2 * WrA) + 1;
                    const int dB = Ib > J ? Ib - J : J - Ib, WrB = SCORE_BAND + (dB > 2 ? dB - 2 : 0);
                    const int nrB = (Ib < 2 * WrB ? Ib : 2 * WrB) + 1;
                    const int i0a = band_row0(La.c, Ia, 2 * J, invJ2, J, WrA, nrA);
                    const int i0b = band_row0(Lb.c, Ib, 2 * J, invJ2, J, WrB, nrB);
                    lds_cc tAa = (lds_cc)(sCTX + La.kA), tBa = (lds_cc)(sCTX + La.kB);
                    lds_cc tAb = (lds_cc)(sCTX + Lb.kA), tBb = (lds_cc)(sCTX + Lb.kB);
                    ScoreChain ca, cb;
                    ca.ap = ca.bp = ca.acc = ca.b = 0.0f; ca.pA = ca.pB = make_float2(0.f, 0.f);
                    cb.ap = cb.bp = cb.acc = cb.b = 0.0f; cb.pA = cb.pB = make_float2(0.f, 0.f);
                    ca.g = (lds_cf)(sGB + gA_ + __mul24(i0a, pA) + La.c); ca.be = (lds_cf)(sGB + bA_ + __mul24(i0a, pA) + La.q);
                    cb.g = (lds_cf)(sGB + gB_ + __mul24(i0b, pB) + Lb.c); cb.be = (lds_cf)(sGB + bB_ + __mul24(i0b, pB) + Lb.q);
                    ca.dg = La.c - i0a - dloA; cb.dg = Lb.c - i0b - dloB;
                    ca.bq = *ca.be; if ((unsigned)(La.q - i0a - dloA) >= bwA) ca.bq = 0.0f;
                    cb.bq = *cb.be; if ((unsigned)(Lb.q - i0b - dloB) >= bwB) cb.bq = 0.0f;
                    ca.be += pA; cb.be += pB;
                    const unsigned limA = bwA - 1u - (unsigned)La.qoff, limB = bwB - 1u - (unsigned)Lb.qoff;
                    ca.op = (lds_cu8)(&sObs[ra][0] + i0a); cb.op = (lds_cu8)(&sObs[rb][0] + i0b);
                    // opaque to the optimiser from here: the running pointers hold complete LDS addresses (otherwise the
                    // dynamic-LDS base is re-added at every use)
                    asm volatile("" : "+v"(ca.g), "+v"(ca.be), "+v"(cb.g), "+v"(cb.be), "+v"(tAa), "+v"(tBa), "+v"(tAb), "+v"(tBb), "+v"(ca.op), "+v"(cb.op));
                    // both chains, row-steps in the order a, b, a, b: the loads of a row-step are issued in front of the arithmetic of the row-step before it, which is the
                    // other chain's (X: chain a's loads, Y: chain b's)
                    const int nmax = nrA > nrB ? nrA : nrB;
                    for (int k = 0; k < nmax; k += SCORE_OBS_ROWS) {
                        int na = nrA - k, nb = nrB - k;                        // the block's rows of each chain (0: the chain has ended)
                        na = na < 0 ? 0 : (na < SCORE_OBS_ROWS ? na : SCORE_OBS_ROWS); nb = nb < 0 ? 0 : (nb < SCORE_OBS_ROWS ? nb : SCORE_OBS_ROWS);
                        if (na > 0) obs_words(ca, ca.op + k);
                        if (nb > 0) obs_words(cb, cb.op + k);
                        const int nmin = na < nb ? na : nb;
                        RowLoads X, Y;
                        bool xl = false, yl = false;                           // X / Y hold the loads of the chain's next row
                        int i = 0;
                        if (nmin >= 2) {
                            rs_load(ca, X, tAa, tBa, pA);
                            for (; i + 4 <= nmin; i += 2) {                    // (a row pair with another behind it: straight-line, no test in front of chain a's next loads)
                                rs_load(cb, Y, tAb, tBb, pB); RS_FENCE();
                                rs_compute(ca, La, X, limA); RS_FENCE();
                                rs_load(ca, X, tAa, tBa, pA); RS_FENCE();
                                rs_compute(cb, Lb, Y, limB); RS_FENCE();
                                rs_load(cb, Y, tAb, tBb, pB); RS_FENCE();
                                rs_compute(ca, La, X, limA); RS_FENCE();
                                rs_load(ca, X, tAa, tBa, pA); RS_FENCE();
                                rs_compute(cb, Lb, Y, limB); RS_FENCE();
                            }
                            rs_load(cb, Y, tAb, tBb, pB); RS_FENCE();          // the last pair the two chains share
                            rs_compute(ca, La, X, limA); RS_FENCE();
                            rs_load(ca, X, tAa, tBa, pA); RS_FENCE();
                            rs_compute(cb, Lb, Y, limB); RS_FENCE();
                            rs_load(cb, Y, tAb, tBb, pB); RS_FENCE();
                            rs_compute(ca, La, X, limA); RS_FENCE();
                            i += 2;
                            xl = i < na;
                            if (xl) rs_load(ca, X, tAa, tBa, pA);
                            RS_FENCE();
                            rs_compute(cb, Lb, Y, limB); RS_FENCE();
                        }
                        // the tails (and a block with fewer than two shared rows) carry no fences on purpose: chain b's Y is issued ahead of chain a's tail, and the compiler may
                        // sink it — a block ends with at most one odd row per chain at the usual eleven rows, nothing to measure
                        if (i < nb) { rs_load(cb, Y, tAb, tBb, pB); yl = true; }
                        for (int ia = i; ia < na; ++ia) { if (!xl) rs_load(ca, X, tAa, tBa, pA); xl = false; rs_compute(ca, La, X, limA); }
                        for (int ib = i; ib < nb; ++ib) { if (!yl) rs_load(cb, Y, tAb, tBb, pB); yl = false; rs_compute(cb, Lb, Y, limB); }
                    }
                    {
                        const float res = La.fin ? ca.b : ca.acc;
                        dq = dq_fix(det_log2f(res) - __int_as_float(rl(__float_as_int(vBase), k0)));
                    }
                    {
                        const float res = Lb.fin ? cb.b : cb.acc;
                        dq += dq_fix(det_log2f(res) - __int_as_float(rl(__float_as_int(vBase), k1)));
                    }
                    }
                    if (mval) atomicAdd(&sDeltaI[myM], dq);
                }
            }
            rbeg = rend;
            PHASE(4);
        }
        }
        ++iters;
        nvalid_last = nvalid; nvfull_last = nvfull;
        // ---- the end of a round, behind ONE barrier.  Every wave loads the gains and validity bytes of all 256 mutation lanes, four per lane (entries lane + 64 k),
        // and converts the gains in registers: whether any mutation is favourable is then the wave's own ballot — the same 256 words in every wave, nobody writes them
        // between this barrier and the next, so the value is wave-uniform and identical in all four waves and every wave takes the exits below by itself.  The
        // selection (wave 0) uses these registers; the QV step behind the loop loads the thread's own entry again.  Nothing is converted in place: sDeltaI stays
        // integer until the next round's set-up zeroes it.  Who wrote each word last, who reads it next, which barrier lies between:
        //   sDeltaI               zeroed by the round's set-up (own thread), summed by the scoring's atomicAdd, in front of this barrier; read here by every wave and, entry tid, behind the loop.  Next
        //                         writer: the next round's set-up, behind the barrier that follows the selection and the round's top barrier
        //   sMvalid               written by the round's set-up, in front of the chunk-opening barrier; read here by every wave and, entry tid, behind the loop (the QV step itself reads
        //                         none: the terms of lanes that are not enumerated are stored as exact zeros).  Next writer: as sDeltaI
        //   sGB[0 .. PWT-1]       gamma/beta of the round's last chunk, last read by the scoring in front of this barrier: dead behind it.  Written behind the loop by
        //                         every thread (its own QV term), read by the core positions' threads behind the barrier in front of the QV step
        //   sCtl[0 .. 3, 7],      written by the prologue or by wave 0's selection; read by every wave behind the barrier that follows the selection (sCtl[3]), behind the
        //   sT[0], sPskip         round's top barrier (the set-up) or behind the barrier in front of the QV step.  While wave 0 selects, the other waves wait at the
        //                         barrier behind the selection and read none of them: their last reads of the round (sT[1] is the scoring's) lie in front of this barrier
        __syncthreads();
        float dk[4];                                         // the lane's four gains
        int candmask = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int m = lane + 64 * k;
            const int mvk = sMvalid[m];
            dk[k] = (float)sDeltaI[m] * (1.0f / DQ_SCALE);
            if (mvk && dk[k] > MUT_EPS) candmask |= 1 << k;
        }
        const int anyfav = __ballot(candmask != 0) != 0ull;
#ifdef CCSX_EXP_ONE_ROUND                                   // experiment (timing only): exactly one round per window whatever the gains say, so that variants which
        break;                                              // corrupt the gains (rows / logarithm compiled out) do not change the control flow they are compared under
#endif
        if (!anyfav || P.qv_only) break;                    // (CCSX_QV_ONLY: the gains of the sequence as given are all that is wanted)
        if (it == CCSX_MAX_ITER - 1) { nonconv = 1; break; }
        // ---- A5: greedy selection (wave 0; lane l owns m = l, l+64, l+128, l+192 which share position l&31)
        if (wave == 0) {
            int Jn = J, nacc = 0;
            unsigned accpos = 0;                             // positions of the accepted mutations (at most one per position: they are >= MUT_SEP apart)
            int accm = 0;                                    // lane c (< 32): the mutation accepted at position c
            for (;;) {
                float bd = -1.0f; int bm = 1 << 20;
#pragma unroll
                for (int k = 0; k < 4; ++k) if (candmask & (1 << k)) { const int m = lane + 64 * k; const float dv = dk[k]; if (dv > bd) { bd = dv; bm = m; } }
                const float wmax = wave_max_f32(bd);
                if (!(wmax > 0.0f)) break;
                const int msel = wave_min_i32((bd == wmax) ? bm : (1 << 20));
                if (lane == (msel & 63)) candmask &= ~(1 << (msel >> 6));
                const int sl = msel >> 5, c = msel & 31;
                if (sl >= 4 && Jn >= CCSX_JMAX) continue;
                if (sl == 3 && Jn <= JMIN_DEL + 1) continue;
                if (sl >= 4) ++Jn; else if (sl == 3) --Jn;
                if (lane == c) accm = msel;
                accpos |= 1u << c;
                ++nacc;
                if (it >= MULTI_ROUNDS) break;
                int dc = (lane & 31) - c; if (dc < 0) dc = -dc;
                if (dc < MUT_SEP) candmask = 0;
            }
            {
                // apply in descending position order.  lane = column: the template base and the skip probability of every column sit in a register
                // and an insertion / deletion is one lane shift (round 3 walked both arrays in LDS on lane 0, a dependent load -> store per column)
                int Jc = J, cs = sCtl[1], ce = sCtl[2];
                unsigned ev = (unsigned)sCtl[7];
                int tb = lane < 32 ? (int)sT[0][lane] : 0;
                float ps = lane < 36 ? sPskip[lane] : 0.0f;
                while (accpos) {
                    const int c = 31 - __clz((int)accpos);
                    accpos &= ~(1u << c);
                    const int m = rl(accm, c), sl = m >> 5;
                    if (sl < 3) { if (lane == c) tb = (tb + 1 + sl) & 3; }
                    else if (sl >= 4) {
                        const int tu = __shfl_up(tb, 1);
                        const float pu = __shfl_up(ps, 1);
                        tb = lane < c ? tb : (lane == c ? sl - 4 : tu);
                        if (lane < 32) ps = lane < c ? ps : (lane == c ? 0.0f : pu);      // (entries 32 .. 35 stay, as in the column-by-column walk)
                        ++Jc;
                        if (c < cs) { ++cs; ++ce; } else if (c < ce) ++ce;
                        // the evidence bit and the skip probability travel with their base; an inserted base is a candidate
                        const unsigned lowm = (1u << c) - 1u;
                        ev = (ev & lowm) | ((ev & ~lowm) << 1);
                    } else {
                        const int td = __shfl_down(tb, 1);
                        const float pd = __shfl_down(ps, 1);
                        if (lane >= c) tb = td;
                        if (lane >= c && lane < 31) ps = pd;
                        --Jc;
                        if (c < cs) { --cs; --ce; } else if (c < ce) --ce;
                        const unsigned lowm = (1u << c) - 1u;
                        ev = (ev & lowm) | ((ev >> 1) & ~lowm);
                    }
                    // re-open the neighbourhood of the applied mutation for the following rounds
                    for (int q = c - SKIP_SPREAD; q <= c + SKIP_SPREAD; ++q) if (q >= 0 && q < 32) ev &= ~(1u << q);
                }
                if (lane < 32) sT[0][lane] = (uint8_t)tb;
                if (lane < 36) sPskip[lane] = ps;
                if (lane == 0) { sCtl[0] = Jc; sCtl[1] = cs; sCtl[2] = ce; sCtl[3] = nacc; sCtl[7] = (int)ev; }
            }
        }
        __syncthreads();
        if (sCtl[3] == 0) break;
    }
    PHASE(5);
    // ---- A6: QVs of the core positions from the last scoring round
    // every mutation lane's term exp2(min(delta, 20)) is computed by the lane's own thread (all waves at once; the core threads below used to
    // evaluate their 8 - 12 exponentials one after the other while three waves waited), then summed per position in the SPEC's order.  The terms go to the
    // first PWT floats of the gamma/beta area, which nobody reads any more (see the table at the round's last barrier; ccsx_polish_lds guarantees the area
    // holds that many): no barrier in front of the stores, unlike an image written in place over sDeltaI, which slower waves may still be reading.  A lane
    // that is not enumerated stores an exact zero
    {
        const int vmine = sMvalid[tid];                      // (the thread's own lane, reloaded: held in registers since the round's end it costs a spill in the scoring loop)
        float dv = (float)sDeltaI[tid] * (1.0f / DQ_SCALE);
        if (dv > 20.0f) dv = 20.0f;
#ifndef CCSX_EXP_NO_QV_EXP                                  // (experiment, timing only: the QV exponentials compiled out)
        dv = det_exp2f(dv);
#endif
        sGB[tid] = vmine ? dv : 0.0f;
    }
    __syncthreads();
    const int J = sCtl[0], cs = sCtl[1], ce = sCtl[2];
    const size_t wi = (size_t)(P.wb_off[z] - z) + w;
    // SPEC v7 "repeat-count floor": tandem tracts (period 1..4) of the converged template with its flanks, as wave masks (the core's threads sit in wave 0)
    unsigned long long tm1 = 0, tm2 = 0, tm3 = 0, tm4 = 0;
    const int voff = lf < 4 ? 1 : 0;
    if (wave == 0) {
        const int nvis = J + voff + (rf < 4 ? 1 : 0);
        auto vat = [&](int i) -> int { return i < voff ? lf : (i - voff < J ? (int)sT[0][i - voff < 31 ? i - voff : 31] : rf); };
        const int vx = vat(lane);
        tm1 = __ballot(lane + 1 < nvis && vx == vat(lane + 1));
        tm2 = __ballot(lane + 2 < nvis && vx == vat(lane + 2));
        tm3 = __ballot(lane + 3 < nvis && vx == vat(lane + 3));
        tm4 = __ballot(lane + 4 < nvis && vx == vat(lane + 4));
    }
    // (wave-uniform masks: whether ANY tract is long enough to matter is scalar arithmetic — on ordinary sequence none is, and the per-base work is skipped)
    auto has_run = [](unsigned long long m, int n) -> bool { unsigned long long x = m; for (int i = 1; i < n; ++i) x &= m >> i; return x != 0; };
    const bool any_tract = has_run(tm1, 8 - 1) || has_run(tm2, 10 - 2) || has_run(tm3, 12 - 3) || has_run(tm4, 16 - 4);
    float pl = 0.0f;                                        // this position's error probability
    if (tid < ce - cs) {
        const int c = cs + tid;
        float p;
        if ((skmask >> c) & 1u) p = sPskip[c];              // skipped by the candidate filter: error probability from the pile-up margin
        else {
            float s = (((unsigned)sCtl[7] >> c) & 1u) ? sPskip[c] : 0.0f;   // quiet homopolymer position: its untested mutations
            // all loads of the position first, then the sum in the SPEC's slot order: a term that is not enumerated enters as + 0.0f, which leaves the
            // non-negative finite s as it is (a chain of eight to twelve dependent load pairs before)
            const bool lastc = c == J - 1;                   // the insertions after the last column follow it
            const int ce_ = lastc ? J : c;
            float dv[12];                                    // (the terms: exact zeros where the lane is not enumerated)
#pragma unroll
            for (int sl = 0; sl < 8; ++sl) dv[sl] = sGB[sl * 32 + c];
#pragma unroll
            for (int sl = 4; sl < 8; ++sl) dv[sl + 4] = sGB[sl * 32 + ce_];
#pragma unroll
            for (int q = 0; q < 12; ++q) s = s + ((q < 8 || lastc) ? dv[q] : 0.0f);
            p = __fdiv_rn(s, 1.0f + s);
        }
        if (any_tract) {
            const int x = c + voff;
            const int nvis_ = J + voff + (rf < 4 ? 1 : 0);
            const int T1 = tract_len(tm1, x, 1, nvis_), T2 = tract_len(tm2, x, 2, nvis_), T3 = tract_len(tm3, x, 3, nvis_), T4 = tract_len(tm4, x, 4, nvis_);
            // SPEC v8: a CLOSED tract (both ends inside the visible template) is resolved by the likelihood — its floor falls with the square of the passes used beyond REP_NP0
            const int npw = nvalid_last;
            const float closed_scale = npw > REP_NP0 ? __fdiv_rn((float)(REP_NP0 * REP_NP0), (float)(npw * npw)) : 1.0f;
            float fl = 0.0f;
#define CCSX_TRACT_FLOOR(TT, MINL) if (((TT) & 255) >= (MINL)) { float f = __fdiv_rn(REP_ERRS, (float)((TT) & 255)); if (!((TT) & 256) && npw > REP_NP0) f = f * closed_scale; fl = f > fl ? f : fl; }
            CCSX_TRACT_FLOOR(T1, 8) CCSX_TRACT_FLOOR(T2, 10) CCSX_TRACT_FLOOR(T3, 12) CCSX_TRACT_FLOOR(T4, 16)
#undef CCSX_TRACT_FLOOR
            if (p < fl) p = fl;
        }
        if (p < P.perr_floor) p = P.perr_floor;             // SPEC v7: no base claims more than Q50 (opts.max_qv)
        float qv = -3.01029996f * det_log2f(p);
        if (qv < 0.0f) qv = 0.0f;
        if (qv > 93.0f) qv = 93.0f;
        P.wseq[wi * 32 + tid] = sT[0][c];
        P.wqv[wi * 32 + tid] = qv;
        pl = p;
    }
    if (wave == 0) {                                         // the core positions (<= 32) all sit in wave 0: ordered sum by v_readlane
        float wsum = 0.0f;
        // (32 steps with immediate lane indices, no loop: pl is + 0.0f in the lanes from ce - cs on, and x + 0.0f is x for every value the sum holds — it starts
        // at + 0.0f and adds positive terms only)
#pragma unroll
        for (int k = 0; k < 32; ++k) wsum = wsum + __int_as_float(rl(__float_as_int(pl), k));
      if (tid == 0) {
        P.wsum[wi] = wsum;
        P.wmeta[wi] = make_int4(ce - cs, nvalid_last | (nvfull_last << 8), nonconv, iters);
        if (P.wtmeta) P.wtmeta[wi] = make_short2((short)J, (short)cs);
      }
    }
    if (P.wtpl && tid < J) P.wtpl[wi * 32 + tid] = sT[0][tid];
#ifdef CCSX_EXP_REPEAT
    }
#endif
    PHASE(6);
    PHASE_FLUSH();
}

// ------------------------------------------------------------------------------------------------
// N4: HiFi kinetics (docs/faq/kinetics.md:8-18; SPEC DESIGN.md §2.9).  One workgroup per window, one wave per read:
// lane = read row of a global alignment of the read's segment to the CONVERGED window template (read orientation),
// the insertion chain of a column is one fused DPP max-scan, the 2-bit moves of a row stay in the lane's registers
// (31 columns = 62 bits) and the traceback walks them with v_readlane on wave-uniform scalars — no DP matrix in
// memory at all.  Matching DIAG cells add the read base's decoded IPD / PW frames to integer LDS sums (order
// independent, so atomics keep the result deterministic); means are re-encoded with CodecV1.
__device__ __forceinline__ int codec_v1_decode(int c)
{
    return c < 64 ? c : (c < 128 ? 64 + (c - 64) * 2 : (c < 192 ? 192 + (c - 128) * 4 : 448 + (c - 192) * 8));
}
__device__ __forceinline__ int codec_v1_encode(int f)
{
    if (f < 64) return f;
    if (f < 192) return 64 + (f - 64 + 1) / 2;
    if (f < 448) return 128 + (f - 192 + 2) / 4;
    const int c = 192 + (f - 448 + 4) / 8;
    return c > 255 ? 255 : c;
}
__device__ __forceinline__ int kin_mean_code(unsigned sum, unsigned cnt)
{
    return cnt ? codec_v1_encode((int)((2u * sum + cnt) / (2u * cnt))) : 0;
}

// scalar traceback of one read: rows live in lanes base..base+n; bit c of (upm, lfm) in the lane of row i says the
// move of cell (i, c+1) is UP / LEFT (neither = DIAG).  Returns, for lane base+c, the read row matched (DIAG) to
// column c of the read-oriented template, or -1.
__device__ __forceinline__ int kin_traceback(int upm, int lfm, int n, int J, int base, int lane)
{
    int i = n, j = J, myrow = -1;
    while (i > 0 && j > 0) {                                 // DIAG needs both; the rest of the path is a straight edge
        const unsigned su = (unsigned)rl(upm, base + i) >> (j - 1), sl = (unsigned)rl(lfm, base + i) >> (j - 1);
        const int up = su & 1u, lf = sl & 1u;
        if (!(up | lf) && lane == base + j - 1) myrow = i - 1;
        i -= 1 - lf;
        j -= 1 - up;
    }
    return myrow;
}

// the same walk for segments of <= 31 bases, one iteration per DIAG RUN instead of per cell: nd = (up | left) << (32 - row)
// puts the cells of one diagonal (i - j constant) at the same bit position in every lane, so a single
// ballot lists the non-DIAG cells of the current diagonal and the highest one at or below row i ends the run.  A
// typical window has ~3 indels per read: ~4 iterations instead of ~30 steps.
__device__ __forceinline__ int kin_traceback_runs(int upm, unsigned long long nd, int n, int J, int base, int lane)
{
    int i = n, j = J, myrow = -1;
    const int c = lane - base;
    while (i > 0 && j > 0) {
        const int p = j + 31 - i;                            // bit of cell (i', j') on this diagonal: (j'-1) + 32 - i'
        const unsigned rows = (unsigned)(__ballot((int)((nd >> p) & 1ull)) >> base);
        const unsigned below = rows & (unsigned)((2ull << i) - 1ull);         // non-DIAG cells at rows <= i (row 0 always is one)
        const int istar = 31 - __builtin_clz(below | 1u);
        int run = i - istar;
        if (run > j) run = j;
        if (c >= j - run && c < j) myrow = c + i - j;        // DIAG cell (c + 1 + i - j, c + 1) matches read row c + i - j
        i -= run; j -= run;
        if (i > 0 && j > 0) {                                // (i, j) is UP or LEFT
            if (((unsigned)rl(upm, base + i) >> (j - 1)) & 1u) --i; else --j;
        }
    }
    return myrow;
}

// The kinetics alignment of one wave's task (k_kinetics_t, k_tile_rows): one segment of n > 31 bases in the wave's 64 lanes, or two of <= 31 in its halves
// (paired: lanes 0-31 the segment of nA bases, 32-63 that of nB).  The lane of row i = lane - base holds read base i - 1 (rbv; 0 beyond the segment) and the
// template's bit planes of the segment's strand (tlo, thi: bit c = column c).  Returns, for the lane of column c < J, the read row a DIAG cell puts on
// column c of the read-oriented template, or -1.
__device__ __forceinline__ int kin_align_rows(int rbv, unsigned tlo, unsigned thi, int J, bool paired, int half, int row, int nA, int nB, int lane)
{
    // bit c of mt: read base of this row == template column c (the two bit planes of the template come as ballots)
    const unsigned mt = ~((tlo ^ ((rbv & 1) ? ~0u : 0u)) | (thi ^ ((rbv & 2) ? ~0u : 0u)));
    // scores are kept shifted by +5 inside a column (h5 = h + 5): diag5 = x + 8*match, left5 = H + 1.  Rows beyond
    // the read compute garbage that no lower lane and no traceback step ever reads.
    const int c1 = 4 * row - 5;
    int H = row * SC_INS;
    int upm = 0, lfm = 0;
    for (int j = 1; j <= J; ++j) {
        int x = wave_shr1_i32(H, NEGV);
        if (row == 0) x = NEGV;                          // (lane 32 of a pair would otherwise see the other read)
        const int diag5 = x + (int)(((mt >> (j - 1)) & 1u) << 3);
        const int left5 = H + 1;
        const int h5 = diag5 >= left5 ? diag5 : left5;
        // insertion chain: v(i) = max_k<=i h(k) + (i-k)*SC_INS, one fused DPP max-scan (per half when paired)
        const int d0 = h5 + c1;
        const int v = (paired ? half_scan_max_i32(d0) : wave_scan_max_i32(d0)) - 4 * row;     // = v(i) exactly
        const unsigned bit = 1u << (j - 1);
        if (v + 5 > h5) upm |= bit;
        else if (diag5 < left5) lfm |= bit;
        H = v;
    }
    int myrow;
    if (nA <= 31) {
        const unsigned long long nd = (unsigned long long)(unsigned)(upm | lfm) << (32 - (row & 31));
        myrow = kin_traceback_runs(upm, nd, nA, J, 0, lane);
        if (paired) {
            const int rowB = kin_traceback_runs(upm, nd, nB, J, 32, lane);
            if (half) myrow = rowB;
        }
    } else myrow = kin_traceback(upm, lfm, nA, J, 0, lane);
    return myrow;
}

// the tasks of up to PW_MAXREADS segments (sN: their lengths, -1 = unusable), in segment order: two short segments share a wave (32 lanes each).  One thread
__device__ __forceinline__ int kin_plan_tasks(const int *sN, int ng, short2 *sTask)
{
    int nt = 0, pend = -1;
    for (int r = 0; r < ng; ++r) {
        const int n = sN[r];
        if (n < 0) continue;
        if (n > 31) sTask[nt++] = make_short2((short)r, (short)-1);
        else if (pend < 0) pend = r;
        else { sTask[nt++] = make_short2((short)pend, (short)r); pend = -1; }
    }
    if (pend >= 0) sTask[nt++] = make_short2((short)pend, (short)-1);
    return nt;
}

// KIN: the kinetics sums (--hifi-kinetics); PILE: the pileup summary (ccsx_consensus_pileup / ccsx_submit_pileup, DESIGN.md §2 "Pileup summary") — per core
// column the passes with a usable segment, and of those the DIAG cells whose bases agree / differ.  Both read the ONE alignment below; <1, 0> is the kinetics
// kernel as it always was.
template <int KIN, int PILE>
__global__ __launch_bounds__(256) void k_kinetics_t(KParams P, int slot0)
{
    __shared__ uint8_t sT[2][32];
    __shared__ unsigned sK[2][3][32];                       // [strand][ipd, pw, count][forward column]
    __shared__ unsigned sPM[2][32];                         // PILE: [match, mismatch][forward column]
    __shared__ int sCov;                                    // PILE: passes with a usable segment (over all groups)
    __shared__ int sN[PW_MAXREADS], sOff[PW_MAXREADS];      // segment length (-1 = unusable), offset of the segment in the read
    __shared__ uint8_t sSt[PW_MAXREADS];
    __shared__ short2 sTask[PW_MAXREADS];
    __shared__ int sNT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int bid = slot0 + xcd_contiguous(blockIdx.x, polish_piece_windows(P.wstart[P.n_zmw], slot0, (int)gridDim.x));   // (as k_polish)
    if (bid < slot0) return;
    const int z = P.wslot_zmw[bid];
    const int w = bid - P.wstart[z];
    const int nw = P.nwin[z];
    const size_t wi = (size_t)(P.wb_off[z] - z) + w;
    const short2 tm = P.wtmeta[wi];
    const int J = tm.x, cs = tm.y, ce = cs + P.wmeta[wi].x;
    const int r0 = P.read_off[z], nreads = P.nreads_used[z];
    const int idx_ws = (w == 0) ? 0 : 2 * w - 1, idx_we = (w == nw - 1) ? 2 * nw - 1 : 2 * (w + 1);
    if (tid < J) { const uint8_t b = P.wtpl[wi * 32 + tid]; sT[0][tid] = b; sT[1][J - 1 - tid] = (uint8_t)(3 - b); }
    if (KIN && tid < 192) (&sK[0][0][0])[tid] = 0u;
    if (PILE && tid < 64) (&sPM[0][0])[tid] = 0u;
    if (PILE && tid == 0) sCov = 0;
    // SPEC v5: up to CCSX_MAX_PASSES passes, taken in groups of PW_MAXREADS (the sums in sK run over all groups)
    for (int g0 = 0; g0 < nreads; g0 += PW_MAXREADS) {
    const int ng = nreads - g0 < PW_MAXREADS ? nreads - g0 : PW_MAXREADS;
    __syncthreads();
    if (tid < ng) {                                          // one lane per read: segment of the read inside this window
        const int rr = r0 + g0 + tid;
        int n = -1, off = 0;
        const int st = ((P.flags[rr] ^ P.flags[r0 + (P.zref[z] & 255)]) & 1) ? 1 : 0;
        if (P.avalid[rr]) {
            const int32_t *ent = P.ent + P.ent_off[rr];
            const int a = ent[idx_ws], b = ent[idx_we];
            n = b - a;
            if (n < 0 || n > CCSX_IMAX) n = -1;
            off = st ? (int)(P.base_off[rr + 1] - P.base_off[rr]) - b : a;
        }
        sN[tid] = n; sOff[tid] = off; sSt[tid] = (uint8_t)st;
    }
    __syncthreads();
    if (tid == 0) {                                          // tasks: two short segments share a wave (32 lanes each)
        sNT = kin_plan_tasks(sN, ng, sTask);
        if (PILE) { int nc = 0; for (int r = 0; r < ng; ++r) nc += sN[r] >= 0 ? 1 : 0; sCov += nc; }
    }
    __syncthreads();
    const int ntask = sNT;
    unsigned tlo[2], thi[2];                                 // template bit planes per strand: bit c = column c (wave-uniform)
    for (int sd = 0; sd < 2; ++sd) {
        const int b = lane < J ? sT[sd][lane] : 0;
        tlo[sd] = (unsigned)__ballot(b & 1); thi[sd] = (unsigned)__ballot(b & 2);
    }
    for (int tk = wave; tk < ntask; tk += 4) {
        const short2 task = sTask[tk];
        const bool paired = rfl((int)task.y) >= 0;
        const int half = (paired && lane >= 32) ? 1 : 0;
        const int base = half * 32, row = lane - base;
        const int myr = half ? task.y : task.x;
        const int n = sN[myr], st = sSt[myr];
        const int64_t p0 = P.base_off[r0 + g0 + myr] + sOff[myr];
        const int rbv = (row >= 1 && row <= n) ? (P.bases[p0 + row - 1] & 3) : 0;   // lane of row i holds read base i-1
        const uint8_t *t = sT[st];
        const int myrow = kin_align_rows(rbv, tlo[st], thi[st], J, paired, half, row, rfl(sN[task.x]), paired ? rfl(sN[task.y]) : 0, lane);
        if (row < J && myrow >= 0) {
            const int jf = st ? J - 1 - row : row;
            const int64_t p = p0 + myrow;
            if (jf >= cs && jf < ce) {
                const bool same = (P.bases[p] & 3) == t[row];
                if (KIN && same) {
                    atomicAdd(&sK[st][0][jf], (unsigned)codec_v1_decode(P.ipd[p]));
                    atomicAdd(&sK[st][1][jf], (unsigned)codec_v1_decode(P.pw[p]));
                    atomicAdd(&sK[st][2][jf], 1u);
                }
                if (PILE) atomicAdd(&sPM[same ? 0 : 1][jf], 1u);
            }
        }
    }
    }
    __syncthreads();
    if (tid < ce - cs) {
        const int c = cs + tid;
        if (KIN) {
            uchar4 k;
            k.x = (uint8_t)kin_mean_code(sK[0][0][c], sK[0][2][c]); k.y = (uint8_t)kin_mean_code(sK[0][1][c], sK[0][2][c]);
            k.z = (uint8_t)kin_mean_code(sK[1][0][c], sK[1][2][c]); k.w = (uint8_t)kin_mean_code(sK[1][1][c], sK[1][2][c]);
            P.wkin[wi * 32 + tid] = k;
        }
        if (PILE) P.wpile[wi * 32 + tid] = make_uchar4((uint8_t)sCov, (uint8_t)sPM[0][c], (uint8_t)sPM[1][c], 0);   // (<= CCSX_MAX_PASSES each)
    }
}

// ------------------------------------------------------------------------------------------------
// step 10: concatenate window cores; rq = 1 - mean(p_err); ec, np, status.  One wave per ZMW.
__global__ __launch_bounds__(64) void k_stitch(KParams P)
{
    __shared__ double sSum;
    __shared__ int sHist[256];                              // windows by number of passes used (0 .. CCSX_MAX_PASSES)
    __shared__ int sOff[LANES], sLen[LANES];                // a block of 64 windows: offset of each core in the block's output, its length
    __shared__ float sQ[LANES * 32];                        // ... the block's QVs and bases, compacted
    __shared__ uint8_t sS[LANES * 32];
    const int z = blockIdx.x, lane = threadIdx.x;
    int stat = P.zstat[z];
    const int nw = (stat == CCSX_SUCCESS) ? P.nwin[z] : 0;
    const size_t w0 = (size_t)(P.wb_off[z] - z);
    const int64_t so = P.seq_off[z], cap = P.seq_off[z + 1] - so;
    int run = 0, nvs = 0, its = 0, ncv = 0;
    if (lane == 0) sSum = 0.0;
    for (int q = lane; q < 256; q += LANES) sHist[q] = 0;
    __syncthreads();
    for (int wbase = 0; wbase < nw; wbase += LANES) {
        const int w = wbase + lane;
        int4 mt = make_int4(0, 0, 0, 0);
        if (w < nw) { mt = P.wmeta[w0 + w]; if ((unsigned)(mt.y >> 8) <= (unsigned)CCSX_MAX_PASSES) atomicAdd(&sHist[mt.y >> 8], 1); mt.y &= 255; }   // np: full-length passes; ec: all
        int pre = mt.x;                                     // inclusive scan of lengths
#pragma unroll
        for (int s = 1; s < LANES; s <<= 1) { int o = __shfl_up(pre, s); if (lane >= s) pre += o; }
        const int off = run + pre - mt.x;
        // The block's 64 window rows are read row-major (coalesced) and compacted in LDS, then written out position-major (coalesced).  Before, a lane copied its
        // own window base by base: 4-byte stores 88 bytes apart — the kernel wrote 1.3 MB per ZMW for 60 KB of results (PMC, profiles/r04_traffic.json).
        sOff[lane] = pre - mt.x; sLen[lane] = mt.x;
        __syncthreads();
        const int nrow = (nw - wbase < LANES ? nw - wbase : LANES) * 32;
        const size_t rowbase = (w0 + (size_t)wbase) * 32;
        for (int q0 = 0; q0 < nrow; q0 += 4 * LANES) {
            float fq[4]; uint8_t fs[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { const int q = q0 + u * LANES + lane; const int qc = q < nrow ? q : nrow - 1; fq[u] = P.wqv[rowbase + qc]; fs[u] = P.wseq[rowbase + qc]; }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int q = q0 + u * LANES + lane;
                if (q < nrow) { const int wl = q >> 5, k = q & 31; if (k < sLen[wl]) { const int d = sOff[wl] + k; sQ[d] = fq[u]; sS[d] = fs[u]; } }
            }
        }
        __syncthreads();
        const int tot = __shfl(pre, 63);
        for (int p0 = lane; p0 < tot; p0 += LANES) {
            if (run + p0 < cap) {
                const float qv = sQ[p0];
                P.out_seq[so + run + p0] = sS[p0];
                P.out_raw[so + run + p0] = qv;
                P.out_qual[so + run + p0] = (uint8_t)(qv + 0.5f);
            }
        }
        if (P.out_kin) {                                    // (--hifi-kinetics only: the four kinetics planes keep the window-by-window copy)
            for (int k = 0; k < mt.x; ++k) {
                if (off + k < cap) {
                    const uchar4 kk = P.wkin[(w0 + w) * 32 + k];
                    uint8_t *o = P.out_kin + so + off + k;
                    o[0] = kk.x; o[P.kin_plane] = kk.y; o[2 * P.kin_plane] = kk.z; o[3 * P.kin_plane] = kk.w;
                }
            }
        }
        run += tot;
        nvs += mt.y; ncv |= mt.z; its += mt.w;
        // fixed-order (window order) double sum of per-window float sums
        for (int k = 0; k < LANES; ++k) {
            float v = __shfl((w < nw) ? P.wsum[w0 + w] : 0.0f, k);
            if (lane == 0 && wbase + k < nw) sSum += (double)v;
        }
        __syncthreads();                                    // (the next block reuses sOff / sLen / sQ / sS)
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) { nvs += __shfl_xor(nvs, s); its += __shfl_xor(its, s); ncv |= __shfl_xor(ncv, s); }
    __syncthreads();
    // np = mode over windows of the passes used for polishing (docs/faq/accuracy-vs-passes.md:18-24); ties: the smaller count
    int npmode;
    {
        int key = 0;                                         // (windows << 8) | (255 - passes): the most windows, then the smaller count
        for (int v = lane; v < 256; v += LANES) { const int k = (sHist[v] << 8) | (255 - v); key = k > key ? k : key; }
        npmode = 255 - (wave_max_i32(key) & 255);
    }
    if (lane == 0) {
        if (stat == CCSX_SUCCESS) P.np[z] = npmode;
        int64_t len = run;
        const bool overflow = len > cap;                    // never a silently truncated HiFi read
        if (overflow) len = cap;
        float rq = 0.0f, ec = 0.0f;
        if (stat == CCSX_SUCCESS) {
            rq = len > 0 ? (float)(1.0 - sSum / (double)run) : 0.0f;
            ec = nw > 0 ? (float)((double)nvs / (double)nw) : 0.0f;
            if (overflow) { stat = CCSX_CAPACITY; len = 0; }
            else if (len == 0) stat = CCSX_EMPTY_WINDOW;
            else if (ncv) stat = CCSX_NON_CONVERGENT;
            else if (rq < P.opts.min_rq) stat = CCSX_LOW_RQ;
        } else len = 0;
        P.out_status[z] = stat; P.out_len[z] = (int32_t)len; P.out_rq[z] = rq; P.out_ec[z] = ec;
        P.out_iters[z] = its; P.out_nwin[z] = nw;
    }
}

// the pileup summary's planes (only with a pileup request; k_stitch itself is untouched): one wave per ZMW, the same windows and offsets as k_stitch —
// a ZMW whose status before stitching is not SUCCESS has none, and nothing is written at or beyond the ZMW's capacity
__global__ __launch_bounds__(64) void k_pile_stitch(KParams P)
{
    const int z = blockIdx.x, lane = threadIdx.x;
    const int nw = (P.zstat[z] == CCSX_SUCCESS) ? P.nwin[z] : 0;
    const size_t w0 = (size_t)(P.wb_off[z] - z);
    const int64_t so = P.seq_off[z], cap = P.seq_off[z + 1] - so;
    int64_t run = 0;
    for (int wbase = 0; wbase < nw; wbase += LANES) {
        const int w = wbase + lane;
        const int len = w < nw ? P.wmeta[w0 + w].x : 0;
        int pre = len;                                      // inclusive scan of the core lengths
#pragma unroll
        for (int s = 1; s < LANES; s <<= 1) { int o = __shfl_up(pre, s); if (lane >= s) pre += o; }
        const int64_t off = run + pre - len;
        for (int k = 0; k < len; ++k) {
            if (off + k < cap) {
                const uchar4 pp = P.wpile[(w0 + w) * 32 + k];
                uint8_t *o = P.out_pile + so + off + k;
                o[0] = pp.x; o[P.pile_plane] = pp.y; o[2 * P.pile_plane] = pp.z;
            }
        }
        run += __shfl(pre, 63);
    }
}

// ------------------------------------------------------------------------------------------------
// The polisher hand-off (ccsx_consensus_handoff / ccsx_submit_handoff; DESIGN.md §2 "Polisher hand-off").  Three kernels on the polish stream after the stitch:
//   k_tile_select  one wave per ZMW: the tiles of its consensus, their qual sums and selection flags, each selected tile's rank within the ZMW, the ZMW's counts,
//                  and every window's core offset in SEQ (k_pile_stitch's scan)
//   k_tile_scan    CCSX_TILE_SCAN_ZMWS ZMWs per workgroup: the exclusive scan of the counts (every workgroup sums the counts in front of it: integer sums, no
//                  atomics, so slot g of a tile depends on the batch alone), the batch's counts, the headers and row tables of the tiles within the capacity,
//                  the padding cells of a short last tile
//   k_tile_rows    one workgroup per window slot, in k_kinetics_t's launch pieces: the kinetics alignment of the row passes' segments, the cells of the
//                  window's core columns for all R rows.  Every cell has one writer
static_assert(PW_MAXREADS >= 32, "k_tile_rows keeps up to 32 rows (ccsx_handoff_opts.max_rows) in the per-group arrays");

__global__ __launch_bounds__(64) void k_tile_select(KParams P)
{
    const int z = blockIdx.x, lane = threadIdx.x;
    const int T = P.ho.tile_len, L = P.out_len[z];
    const int64_t so = P.seq_off[z], t0 = ccsx_handoff_tile_off(so, z, T);
    const int nt = (L + T - 1) / T;
    int nsel = 0;
    for (int tb = 0; tb < nt; tb += LANES) {
        const int t = tb + lane;
        int qsum = 0, len = 0;
        if (t < nt) {
            len = L - t * T < T ? L - t * T : T;
            const uint8_t *q = P.out_qual + so + (int64_t)t * T;
            for (int k = 0; k < len; ++k) qsum += q[k];
        }
        const bool sel = t < nt && qsum < P.ho.skip_above * len;
        const unsigned long long m = __ballot(sel);
        if (t < nt) { P.ho_tqsum[t0 + t] = qsum; P.ho_tslot[t0 + t] = sel ? nsel + __popcll(m & ((1ull << lane) - 1ull)) : -1; }
        nsel += __popcll(m);
    }
    if (lane == 0) { P.ho_zcnt[z] = nt; P.ho_zcnt[P.n_zmw + z] = nsel; }
    if (L <= 0) return;                                      // (a ZMW with a consensus was stitched from all its windows)
    const int nw = P.nwin[z];
    const size_t w0 = (size_t)(P.wb_off[z] - z);
    int run = 0;
    for (int wbase = 0; wbase < nw; wbase += LANES) {
        const int w = wbase + lane;
        const int len = w < nw ? P.wmeta[w0 + w].x : 0;
        int pre = len;                                      // inclusive scan of the core lengths
#pragma unroll
        for (int s = 1; s < LANES; s <<= 1) { int o = __shfl_up(pre, s); if (lane >= s) pre += o; }
        if (w < nw) P.ho_woff[w0 + w] = run + pre - len;
        run += __shfl(pre, 63);
    }
}

__global__ __launch_bounds__(256) void k_tile_scan(KParams P)
{
    __shared__ int sRed[2][4];
    __shared__ int sBase[CCSX_TILE_SCAN_ZMWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = P.n_zmw, zb = blockIdx.x * CCSX_TILE_SCAN_ZMWS;
    const int T = P.ho.tile_len, R = P.ho.max_rows, M = P.ho_max_tiles;
    int a = 0, s = 0;
    for (int z = tid; z < zb; z += 256) { a += P.ho_zcnt[z]; s += P.ho_zcnt[n + z]; }
    a = wave_reduce_add_i32(a); s = wave_reduce_add_i32(s);
    if (lane == 0) { sRed[0][wave] = a; sRed[1][wave] = s; }
    __syncthreads();
    if (wave == 0) {
        const int pre_all = sRed[0][0] + sRed[0][1] + sRed[0][2] + sRed[0][3], pre_sel = sRed[1][0] + sRed[1][1] + sRed[1][2] + sRed[1][3];
        const int z = zb + lane;
        const int c = z < n ? P.ho_zcnt[n + z] : 0, ta = z < n ? P.ho_zcnt[z] : 0;
        const int inc = wave_scan_add_i32(c), tot = wave_reduce_add_i32(ta);
        sBase[lane] = pre_sel + inc - c;
        if (lane == 63 && zb + CCSX_TILE_SCAN_ZMWS >= n) { P.ho_counts[0] = pre_all + tot; P.ho_counts[1] = pre_sel + inc; }   // the last workgroup: the batch's counts
    }
    __syncthreads();
    const int per = CCSX_TILE_SCAN_ZMWS / 4;
    for (int i = 0; i < per; ++i) {                          // one wave per ZMW
        const int zl = wave * per + i, z = zb + zl;
        if (z >= n) break;
        if (P.ho_zcnt[n + z] == 0) continue;
        const int g0 = sBase[zl], nt = P.ho_zcnt[z], L = P.out_len[z];
        const int64_t t0 = ccsx_handoff_tile_off(P.seq_off[z], z, T);
        // the ZMW's rows: row k = the k-th valid pass among those used, in batch order
        const int r0 = P.read_off[z], nreads = P.nreads_used[z];
        unsigned long long vm[4] = {0, 0, 0, 0};
        int nrows = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int p = c * 64 + lane;
            vm[c] = __ballot(p < nreads && P.avalid[r0 + p] != 0);
            nrows += __popcll(vm[c]);
        }
        if (nrows > R) nrows = R;
        int rp = 255, rs = 0;
        if (lane < nrows) {
            int rem = lane;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int pc = __popcll(vm[c]);
                if (rp == 255 && rem < pc) {
                    unsigned long long x = vm[c];
                    for (int q = 0; q < rem; ++q) x &= x - 1;
                    rp = c * 64 + __builtin_ctzll(x);
                }
                rem -= pc;
            }
            rs = (P.flags[r0 + rp] ^ P.flags[r0 + (P.zref[z] & 255)]) & 1;
        }
        for (int tb = 0; tb < nt; tb += LANES) {
            const int t = tb + lane;
            int g = -1;
            if (t < nt) {
                const int loc = P.ho_tslot[t0 + t];
                if (loc >= 0) {
                    g = g0 + loc < M ? g0 + loc : -1;
                    P.ho_tslot[t0 + t] = g;                  // from here on: the tile's slot, -1 beyond the capacity
                }
                if (g >= 0) {
                    P.ho_hdr[g] = z; P.ho_hdr[M + g] = t * T; P.ho_hdr[2 * (size_t)M + g] = L - t * T < T ? L - t * T : T;
                    P.ho_hdr[3 * (size_t)M + g] = P.ho_tqsum[t0 + t]; P.ho_hdr[4 * (size_t)M + g] = nrows;
                }
            }
            unsigned long long todo = __ballot(g >= 0);
            while (todo) {                                   // the row tables of each such tile, and the padding cells of a short one
                const int src = __builtin_ctzll(todo);
                todo &= todo - 1;
                const int gg = __shfl(g, src), tt = tb + src;
                if (lane < R) { P.ho_rows[(size_t)gg * R + lane] = (uint8_t)rp; P.ho_rows[((size_t)M + gg) * R + lane] = (uint8_t)rs; }
                const int len = L - tt * T < T ? L - tt * T : T, pad = T - len;
                for (int q = lane; q < R * pad; q += LANES)
                    P.ho_cells[((size_t)gg * R + q / pad) * T + len + q % pad] = make_uchar4(5, 0, 0, 0);
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_tile_rows(KParams P, int slot0)
{
    __shared__ uint8_t sT[2][32];
    __shared__ int sN[PW_MAXREADS], sOff[PW_MAXREADS], sPass[PW_MAXREADS];   // the rows' segments: length (-1 = unusable or no such row), offset in the pass, the pass
    __shared__ uint8_t sSt[PW_MAXREADS];
    __shared__ short2 sTask[PW_MAXREADS];
    __shared__ int sNT, sWc[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int bid = slot0 + xcd_contiguous(blockIdx.x, polish_piece_windows(P.wstart[P.n_zmw], slot0, (int)gridDim.x));   // (as k_polish)
    if (bid < slot0) return;
    const int z = P.wslot_zmw[bid];
    if (P.out_len[z] <= 0) return;                           // no consensus: no tiles
    const int w = bid - P.wstart[z];
    const int nw = P.nwin[z];
    const size_t wi = (size_t)(P.wb_off[z] - z) + w;
    const int nc = P.wmeta[wi].x;
    if (nc <= 0) return;
    const short2 tm = P.wtmeta[wi];
    const int J = tm.x, cs = tm.y, ce = cs + nc;
    const int T = P.ho.tile_len, R = P.ho.max_rows;
    // the tiles the core's columns fall into (<= 32 columns, tiles of >= 16: at most three) and their slots; none selected within the capacity: nothing to do
    const int woff = P.ho_woff[wi];
    const int64_t t0 = ccsx_handoff_tile_off(P.seq_off[z], z, T);
    const int tf = woff / T, tl = (woff + nc - 1) / T;
    const int g0 = P.ho_tslot[t0 + tf], g1 = tf + 1 <= tl ? P.ho_tslot[t0 + tf + 1] : -1, g2 = tf + 2 <= tl ? P.ho_tslot[t0 + tf + 2] : -1;
    if ((g0 & g1 & g2) < 0) return;
    uchar4 *const cells = P.ho_cells;                        // (captured by value: a reference to P would put the whole parameter block into scratch)
    auto put = [cells, woff, T, R, tf, g0, g1, g2](int k, int col, uchar4 v) {   // row k, core column col
        const int pos = woff + col, tq = pos / T - tf;
        const int g = tq == 0 ? g0 : (tq == 1 ? g1 : g2);
        if (g >= 0) cells[((size_t)g * R + k) * T + (pos - (tf + tq) * T)] = v;
    };
    const int r0 = P.read_off[z], nreads = P.nreads_used[z];
    const int idx_ws = (w == 0) ? 0 : 2 * w - 1, idx_we = (w == nw - 1) ? 2 * nw - 1 : 2 * (w + 1);
    if (tid < J) { const uint8_t b = P.wtpl[wi * 32 + tid]; sT[0][tid] = b; sT[1][J - 1 - tid] = (uint8_t)(3 - b); }
    if (tid < PW_MAXREADS) sN[tid] = -1;
    // the pass -> row map (at most CCSX_MAX_PASSES = 255 passes: one thread each)
    const bool valid = tid < nreads && P.avalid[r0 + tid] != 0;
    const unsigned long long vmask = __ballot(valid);
    if (lane == 0) sWc[wave] = __popcll(vmask);
    __syncthreads();
    int k = __popcll(vmask & ((1ull << lane) - 1ull));
    for (int q = 0; q < wave; ++q) k += sWc[q];
    int nrows = sWc[0] + sWc[1] + sWc[2] + sWc[3];
    if (nrows > R) nrows = R;
    if (valid && k < R) {                                    // the row's segment inside this window (k_kinetics_t's)
        const int rr = r0 + tid;
        const int st = ((P.flags[rr] ^ P.flags[r0 + (P.zref[z] & 255)]) & 1) ? 1 : 0;
        const int32_t *ent = P.ent + P.ent_off[rr];
        const int a = ent[idx_ws], b = ent[idx_we];
        int n = b - a;
        if (n < 0 || n > CCSX_IMAX) n = -1;
        sN[k] = n; sOff[k] = st ? (int)(P.base_off[rr + 1] - P.base_off[rr]) - b : a; sSt[k] = (uint8_t)st; sPass[k] = tid;
    }
    __syncthreads();
    if (tid == 0) sNT = kin_plan_tasks(sN, nrows, sTask);
    __syncthreads();
    const int ntask = sNT;
    unsigned tlo[2], thi[2];                                 // template bit planes per strand: bit c = column c (wave-uniform)
    for (int sd = 0; sd < 2; ++sd) {
        const int b = lane < J ? sT[sd][lane] : 0;
        tlo[sd] = (unsigned)__ballot(b & 1); thi[sd] = (unsigned)__ballot(b & 2);
    }
    for (int tk = wave; tk < ntask; tk += 4) {
        const short2 task = sTask[tk];
        const bool paired = rfl((int)task.y) >= 0;
        const int half = (paired && lane >= 32) ? 1 : 0;
        const int base = half * 32, row = lane - base;
        const int myr = half ? task.y : task.x;
        const int n = sN[myr], st = sSt[myr];
        const int64_t p0 = P.base_off[r0 + sPass[myr]] + sOff[myr];
        const int rbv = (row >= 1 && row <= n) ? (P.bases[p0 + row - 1] & 3) : 0;   // lane of row i holds read base i-1
        const int myrow = kin_align_rows(rbv, tlo[st], thi[st], J, paired, half, row, rfl(sN[task.x]), paired ? rfl(sN[task.y]) : 0, lane);
        // the DIAG column next to this one on the side that is LEFT in SEQ: a lower column of a forward pass, a higher one of a pass on the opposite strand
        const bool hit = row < J && myrow >= 0;
        const unsigned dm = (unsigned)(__ballot(hit) >> base);
        int nb = -1;
        if (row < 32) {
            if (!st) { const unsigned lo = dm & ((1u << row) - 1u); if (lo) nb = 31 - __builtin_clz(lo); }
            else { const unsigned hi = row < 31 ? dm >> (row + 1) : 0u; if (hi) nb = row + 1 + __builtin_ctz(hi); }
        }
        const int rnb = __shfl(myrow, base + (nb < 0 ? 0 : nb));
        if (row < J) {
            const int jf = st ? J - 1 - row : row;
            if (jf >= cs && jf < ce) {
                uchar4 v = make_uchar4(4, 0, 0, 0);
                if (myrow >= 0) {
                    const int64_t p = p0 + myrow;
                    const int b = P.bases[p] & 3;
                    const int ins = st ? (nb >= 0 ? rnb - myrow - 1 : n - 1 - myrow) : (nb >= 0 ? myrow - rnb - 1 : myrow);
                    v = make_uchar4((uint8_t)(st ? 3 - b : b), P.pw[p], P.ipd ? P.ipd[p] : (uint8_t)0, (uint8_t)ins);
                }
                put(myr, jf - cs, v);
            }
        }
    }
    for (int q = tid; q < R * nc; q += 256) {                // rows without a usable segment here, and the rows the ZMW does not have
        const int kk = q / nc;
        if (sN[kk] < 0) put(kk, q - kk * nc, make_uchar4(5, 0, 0, 0));
    }
}

// ------------------------------------------------------------------------------------------------
// The heteroduplex finder (ccsx_hd_batch; DESIGN.md §2 "Heteroduplex rule", §4).  Runs after the alignment cascade and the window map of the polish seam, on
// the same inputs k_polish gets (draft, window bounds, entry rows), before any insertion trim.  Three kernels:
//   k_hd_pile     a group of HD_WG_WIN consecutive windows per one-wave workgroup: the unit-cost edit DP of every (pass, window) segment against the window
//                 template, one segment per lane (the windows' segments are pooled, so at 10 passes the 64 lanes serve 6-7 windows at once), 2-bit moves in
//                 LDS, the trace-back's core-column outcomes counted per strand with LDS integer atomics (independent of which lane ran which segment), then the
//                 column test in the same workgroup: per window a site count, its lowest sites in column order and their smallest p
//   k_hd_indel    one wave per ZMW: the 1-3-window length excesses from the entry rows, events merged over adjacent windows, their Fisher tests
//   k_hd_verdict  one wave per ZMW: counts, the ordered site list (a merge of the per-window lists and the indel list: no global atomics) and the verdict
#define HD_WG_WIN 16

// two-sided Fisher exact p of [[a, nf - a], [c, nr - c]]: the tables with the same margins whose probability is <= p_obs (1 + 1e-7), summed in increasing
// order of the top-left cell; log k! from the host's table (tests/hd_ref.py restates it operation for operation)
__device__ double hd_fisher(const double *lf, int a, int nf, int c, int nr)
{
    const int m = a + c, N = nf + nr;
    const double base = lf[nf] + lf[nr] + lf[m] + lf[N - m] - lf[N];
    const double thr = exp(base - lf[a] - lf[nf - a] - lf[m - a] - lf[nr - m + a]) * (1.0 + 1e-7);
    const int lo = m - nr > 0 ? m - nr : 0, hi = nf < m ? nf : m;
    double p = 0.0;
    for (int x = lo; x <= hi; ++x) {
        const double px = exp(base - lf[x] - lf[nf - x] - lf[m - x] - lf[nr - m + x]);
        if (px <= thr) p += px;
    }
    return p < 1.0 ? p : 1.0;
}

// window w of a ZMW: template draft[ws, we) and the indices of its two entry rows (the same expressions as k_polish)
struct HdWin { int ws, we, iws, iwe; };
__device__ __forceinline__ HdWin hd_win(const int32_t *wb, int nw, int Ld, int w)
{
    HdWin g;
    g.ws = wb[w] - CCSX_WIN_OVERHANG; if (g.ws < 0) g.ws = 0;
    g.we = wb[w + 1] + CCSX_WIN_OVERHANG; if (g.we > Ld) g.we = Ld;
    g.iws = (w == 0) ? 0 : 2 * w - 1;
    g.iwe = (w == nw - 1) ? 2 * nw - 1 : 2 * (w + 1);
    return g;
}

__device__ __forceinline__ bool hd_site_less(const ccsx_hd_site &x, const ccsx_hd_site &y) { return x.column < y.column || (x.column == y.column && x.kind < y.kind); }

__global__ __launch_bounds__(64) void k_hd_pile(KParams P)
{
    __shared__ uint64_t sMv[CCSX_HD_IMAX * 64];               // [row - 1][lane]: 2-bit moves of columns 1 .. 31 (0 diagonal, 1 deletion, 2 insertion)
    __shared__ uint32_t sCnt[HD_WG_WIN][32][2][2];            // [window][column][strand]: A|C|G|T counts (a byte each), deletions
    __shared__ uint64_t sTpl[HD_WG_WIN];                      // window template, 2 bits per column
    __shared__ int sW[HD_WG_WIN][8];                          // z, ws, J, cs, ce, r0, fl0, iws | iwe << 16
    __shared__ int sOff[HD_WG_WIN + 1];                       // first task (pass) of each window
    const int lane = threadIdx.x;
    const int nwin_all = P.wstart[P.n_zmw];
    const int k0 = blockIdx.x * HD_WG_WIN;
    if (k0 >= nwin_all) return;
    for (int q = lane; q < HD_WG_WIN * 32 * 4; q += 64) (&sCnt[0][0][0][0])[q] = 0u;
    int np = 0;
    if (lane < HD_WG_WIN) {
        const int k = k0 + lane;
        if (k < nwin_all) {
            const int z = P.wslot_zmw[k], nw = P.nwin[z], Ld = P.draft_len[z], w = k - P.wstart[z];
            const int32_t *wb = P.wbounds + P.wb_off[z];
            const HdWin g = hd_win(wb, nw, Ld, w);
            const int J = g.we - g.ws;
            const uint8_t *d = P.draft + P.seq_off[z];
            uint64_t t = 0;
            for (int j = 0; j < J && j < 31; ++j) t |= (uint64_t)(d[g.ws + j] & 3) << (2 * j);
            const int r0 = P.read_off[z];
            sTpl[lane] = t;
            sW[lane][0] = z; sW[lane][1] = g.ws; sW[lane][2] = J; sW[lane][3] = wb[w] - g.ws; sW[lane][4] = wb[w + 1] - g.ws;
            sW[lane][5] = r0; sW[lane][6] = P.flags[r0 + (P.zref[z] & 255)] & 1; sW[lane][7] = g.iws | (g.iwe << 16);
            np = J <= 31 ? P.nreads_used[z] : 0;
        }
    }
    const int incl = wave_scan_add_i32(np);                   // (lanes 16..63 add 0)
    if (lane < HD_WG_WIN) sOff[lane + 1] = incl;
    if (lane == 0) sOff[0] = 0;
    __syncthreads();
    const int T = sOff[HD_WG_WIN];
    const int mi = P.hd.min_indel;
    for (int t = lane; t < T; t += 64) {
        int k = 0;
        while (k < HD_WG_WIN - 1 && sOff[k + 1] <= t) ++k;
        const int r = sW[k][5] + (t - sOff[k]);
        if (!P.avalid[r]) continue;
        const int64_t eo = P.ent_off[r], bo = P.base_off[r];
        const int L = (int)(P.base_off[r + 1] - bo);
        const int a = P.ent[eo + (sW[k][7] & 0xffff)], n = P.ent[eo + (sW[k][7] >> 16)] - a;
        const int J = sW[k][2];
        if (a < 0 || n < 0 || a + n > L || n > CCSX_HD_IMAX || n - J >= mi || J - n >= mi) continue;   // (rows of this pass only)
        const int st = (P.flags[r] & 1) ^ sW[k][6];
        // the segment in draft orientation, 2 bits per base (rows 1..32 in s0, 33..49 in s1)
        uint64_t s0 = 0, s1 = 0;
        for (int i = 0; i < n; ++i) {
            const int b = st ? 3 - (P.bases[bo + (L - 1 - a - i)] & 3) : (P.bases[bo + a + i] & 3);
            if (i < 32) s0 |= (uint64_t)b << (2 * i); else s1 |= (uint64_t)b << (2 * (i - 32));
        }
        const uint64_t tpl = sTpl[k];
        int D[32];
#pragma unroll
        for (int j = 0; j < 32; ++j) D[j] = j;
        for (int i = 1; i <= n; ++i) {
            const int rb = (int)((i <= 32 ? s0 >> (2 * (i - 1)) : s1 >> (2 * (i - 33))) & 3);
            int diag = D[0], left = i;
            D[0] = i;
            uint64_t mv = 0;
#pragma unroll
            for (int j = 1; j < 32; ++j) {                    // tie order diagonal < deletion < insertion (strict compares)
                const int up = D[j];
                const int dv = diag + (rb != (int)((tpl >> (2 * (j - 1))) & 3) ? 1 : 0);
                int best = dv, m = 0;
                if (left + 1 < best) { best = left + 1; m = 1; }
                if (up + 1 < best) { best = up + 1; m = 2; }
                mv |= (uint64_t)m << (2 * (j - 1));
                diag = up; D[j] = best; left = best;
            }
            sMv[(i - 1) * 64 + lane] = mv;
        }
        const int cs = sW[k][3], ce = sW[k][4];
        int i = n, j = J;
        while (i > 0 || j > 0) {
            const int m = i == 0 ? 1 : (j == 0 ? 2 : (int)((sMv[(i - 1) * 64 + lane] >> (2 * (j - 1))) & 3));
            if (m != 2) {
                const int c = j - 1;
                if (c >= cs && c < ce) {
                    if (m == 0) {
                        const int rb = (int)((i <= 32 ? s0 >> (2 * (i - 1)) : s1 >> (2 * (i - 33))) & 3);
                        atomicAdd(&sCnt[k][c][st][0], 1u << (8 * rb));
                    } else atomicAdd(&sCnt[k][c][st][1], 1u);
                }
                --j;
            }
            if (m != 1) --i;
        }
    }
    __syncthreads();
    // the column test: two windows per step, lane & 31 = the template column
    const int c = lane & 31;
    for (int k = lane >> 5; k < HD_WG_WIN; k += 2) {
        const int kg = k0 + k;
        bool site = false;
        ccsx_hd_site rec;
        rec.p = 1.0;
        if (kg < nwin_all && c >= sW[k][3] && c < sW[k][4]) {
            const uint32_t f4 = sCnt[k][c][0][0], r4 = sCnt[k][c][1][0];
            const int nf = (int)((f4 & 255) + ((f4 >> 8) & 255) + ((f4 >> 16) & 255) + (f4 >> 24) + sCnt[k][c][0][1]);
            const int nr = (int)((r4 & 255) + ((r4 >> 8) & 255) + ((r4 >> 16) & 255) + (r4 >> 24) + sCnt[k][c][1][1]);
            const int db = (int)((sTpl[k] >> (2 * c)) & 3);
            int alt = -1, best = 0;
            for (int b = 0; b < 4; ++b) {
                const int tot = (int)(((f4 >> (8 * b)) & 255) + ((r4 >> (8 * b)) & 255));
                if (b != db && tot > best) { best = tot; alt = b; }
            }
            if (alt >= 0 && nf >= P.hd.min_strand_passes && nr >= P.hd.min_strand_passes) {
                const int fa = (int)((f4 >> (8 * alt)) & 255), ra = (int)((r4 >> (8 * alt)) & 255);
                const double fr = (double)P.hd.min_alt_frac;
                if ((double)fa >= fr * (double)nf || (double)ra >= fr * (double)nr) {
                    rec.p = hd_fisher(P.hd_lf, fa, nf, ra, nr);
                    if (rec.p <= P.hd.max_pvalue) {
                        site = true;
                        rec.column = sW[k][1] + c; rec.kind = 0; rec.alt = (int8_t)alt;
                        rec.fwd_alt = (uint8_t)fa; rec.fwd_n = (uint8_t)nf; rec.rev_alt = (uint8_t)ra; rec.rev_n = (uint8_t)nr;
                        rec.pad_[0] = rec.pad_[1] = 0;
                    }
                }
            }
        }
        const unsigned long long ball = __ballot(site);
        const unsigned half = (unsigned)(ball >> (lane & 32));
        const int pos = __popc(half & ((1u << c) - 1u)), cnt = __popc(half);
        double mp = site ? rec.p : 1.0;
        for (int o = 16; o >= 1; o >>= 1) { const double q = __shfl_xor(mp, o, 32); mp = q < mp ? q : mp; }
        if (kg < nwin_all) {
            if (site && pos < CCSX_HD_WIN_SITES) P.hd_wrec[(size_t)kg * CCSX_HD_WIN_SITES + pos] = rec;
            if (c == 0) { P.hd_wcnt[kg] = cnt; P.hd_wminp[kg] = mp; }
        }
    }
}

__global__ __launch_bounds__(64) void k_hd_indel(KParams P)
{
    const int z = blockIdx.x, lane = threadIdx.x;
    if (z >= P.n_zmw) return;
    const int n = P.n_zmw;
    ccsx_hd_site *out = P.hd_isite + (size_t)z * CCSX_HD_MAX_SITES;
    const int nw = P.zstat[z] == CCSX_SUCCESS ? P.nwin[z] : 0;
    const int Ld = P.draft_len[z], r0 = P.read_off[z], np = P.nreads_used[z], mi = P.hd.min_indel;
    const int fl0 = P.flags[r0 + (P.zref[z] & 255)] & 1;
    const int32_t *wb = P.wbounds + P.wb_off[z];
    int n_ind = 0, listed = 0;
    double minp = 1.0;
    // per lane and group of 64 passes: event / coverage bits of the open insertion (bit 0, 1) and deletion (bit 2, 3) cluster
    int state[4] = {0, 0, 0, 0};
    int open_i = -1, open_d = -1;
    for (int w = 0; w <= nw; ++w) {
        int ev[4] = {0, 0, 0, 0};                              // bit 0 insertion event, bit 1 deletion event, bit 2 the one-window segment is valid
        int anyI = 0, anyD = 0;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int p = g * 64 + lane;
            if (w < nw && p < np && P.avalid[r0 + p]) {
                const int r = r0 + p;
                const int64_t eo = P.ent_off[r];
                const int L = (int)(P.base_off[r + 1] - P.base_off[r]);
                const HdWin g0 = hd_win(wb, nw, Ld, w);
                const int a = P.ent[eo + g0.iws];
                int e = 0;
                for (int s = 0; s < 3 && w + s < nw; ++s) {
                    const HdWin g1 = hd_win(wb, nw, Ld, w + s);
                    const int len = P.ent[eo + g1.iwe] - a;
                    if (len < 0 || len > L) continue;
                    const int ex = len - (g1.we - g0.ws);
                    if (s == 0) e |= 4;
                    if (ex >= mi) e |= 1;
                    if (-ex >= mi) e |= 2;
                }
                ev[g] = e;
            }
            anyI |= __ballot(ev[g] & 1) != 0ull;
            anyD |= __ballot(ev[g] & 2) != 0ull;
        }
        for (int sign = 0; sign < 2; ++sign) {
            const int any = sign ? anyD : anyI;
            int &open = sign ? open_d : open_i;
            const int eb = sign ? 2 : 1, sh = 2 * sign;
            if (any) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int e = (ev[g] & eb) ? 1 : 0, cv = (ev[g] & 4) ? 1 : 0;
                    const int old = (state[g] >> sh) & 3;
                    const int nv = open < 0 ? (e | (cv << 1)) : ((old & 1) | e) | ((old & 2) & (cv << 1));
                    state[g] = (state[g] & ~(3 << sh)) | (nv << sh);
                }
                if (open < 0) open = w;
            } else if (open >= 0) {                            // the cluster ended at w - 1: its Fisher table
                int fa = 0, fn = 0, ra = 0, rn = 0;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int p = g * 64 + lane;
                    const int sv = (state[g] >> sh) & 3;
                    const int st = p < np ? ((P.flags[r0 + p] & 1) ^ fl0) : 0;
                    const bool counted = p < np && sv != 0;
                    fa += __popcll(__ballot(counted && (sv & 1) && !st)); fn += __popcll(__ballot(counted && !st));
                    ra += __popcll(__ballot(counted && (sv & 1) && st));  rn += __popcll(__ballot(counted && st));
                }
                if (fn >= P.hd.min_strand_passes && rn >= P.hd.min_strand_passes) {
                    const double p = hd_fisher(P.hd_lf, fa, fn, ra, rn);
                    if (p <= P.hd.max_pvalue) {
                        ++n_ind;
                        minp = p < minp ? p : minp;
                        if (lane == 0) {
                            ccsx_hd_site s;
                            s.column = wb[open]; s.kind = (int8_t)(1 + sign); s.alt = -1;
                            s.fwd_alt = (uint8_t)fa; s.fwd_n = (uint8_t)fn; s.rev_alt = (uint8_t)ra; s.rev_n = (uint8_t)rn; s.pad_[0] = s.pad_[1] = 0; s.p = p;
                            // the CCSX_HD_MAX_SITES lowest (column, kind), sorted (clusters close out of column order only across the two signs)
                            int q = listed < CCSX_HD_MAX_SITES ? listed : CCSX_HD_MAX_SITES - 1;
                            if (listed < CCSX_HD_MAX_SITES || hd_site_less(s, out[q])) {
                                while (q > 0 && hd_site_less(s, out[q - 1])) { out[q] = out[q - 1]; --q; }
                                out[q] = s;
                            }
                        }
                        listed += listed < CCSX_HD_MAX_SITES ? 1 : 0;
                    }
                }
                open = -1;
            }
        }
    }
    if (lane == 0) { P.hd_zi[2 * (size_t)n + z] = n_ind; P.hd_zi[4 * (size_t)n + z] = listed; P.hd_minp[z] = minp; }
}

__global__ __launch_bounds__(64) void k_hd_verdict(KParams P)
{
    __shared__ ccsx_hd_site sL[2 * CCSX_HD_MAX_SITES];        // [0, 16): substitution sites in column order, [16, 32): the indel list
    const int z = blockIdx.x, lane = threadIdx.x;
    if (z >= P.n_zmw) return;
    const int n = P.n_zmw;
    const bool ok = P.zstat[z] == CCSX_SUCCESS;
    const int nw = ok ? P.nwin[z] : 0, a0 = P.wstart[z];
    int nsub = 0, ns = 0;
    double minp = P.hd_minp[z];
    for (int w0 = 0; w0 < nw; w0 += 64) {
        const int w = w0 + lane;
        const int cnt = w < nw ? P.hd_wcnt[a0 + w] : 0;
        double mp = w < nw ? P.hd_wminp[a0 + w] : 1.0;
        for (int o = 32; o >= 1; o >>= 1) { const double q = __shfl_xor(mp, o); mp = q < mp ? q : mp; }
        minp = mp < minp ? mp : minp;
        nsub += wave_reduce_add_i32(cnt);
        unsigned long long m = __ballot(cnt > 0);
        while (m && ns < CCSX_HD_MAX_SITES) {                  // windows with sites, in order: ordered compaction of their lists
            const int wl = __ffsll((long long)m) - 1;
            m &= m - 1;
            const int kg = a0 + w0 + wl;
            int c = P.hd_wcnt[kg];
            c = c < CCSX_HD_WIN_SITES ? c : CCSX_HD_WIN_SITES;
            c = c < CCSX_HD_MAX_SITES - ns ? c : CCSX_HD_MAX_SITES - ns;
            if (lane < c) sL[ns + lane] = P.hd_wrec[(size_t)kg * CCSX_HD_WIN_SITES + lane];
            ns += c;
        }
    }
    const int nind = ok ? P.hd_zi[2 * (size_t)n + z] : 0, ni = ok ? P.hd_zi[4 * (size_t)n + z] : 0;
    if (lane < ni) sL[CCSX_HD_MAX_SITES + lane] = P.hd_isite[(size_t)z * CCSX_HD_MAX_SITES + lane];
    __syncthreads();
    int listed = 0;
    if (lane == 0) {                                           // merge the two sorted lists: the CCSX_HD_MAX_SITES lowest (column, kind)
        ccsx_hd_site *out = P.hd_sites + (size_t)z * CCSX_HD_MAX_SITES;
        int x = 0, y = 0;
        while (listed < CCSX_HD_MAX_SITES && (x < ns || y < ni)) {
            const bool take_sub = y >= ni || (x < ns && !hd_site_less(sL[CCSX_HD_MAX_SITES + y], sL[x]));
            out[listed++] = take_sub ? sL[x++] : sL[CCSX_HD_MAX_SITES + y++];
        }
        const int fn = P.out_fn[z], rn = P.out_rn[z], msp = P.hd.min_strand_passes;
        const int verdict = !ok ? CCSX_HD_UNTESTED
                          : (nsub >= P.hd.min_sites || nind >= 1) ? CCSX_HD_HETERODUPLEX
                          : (fn >= msp && rn >= msp) ? CCSX_HD_DOUBLE_STRAND : CCSX_HD_UNTESTED;
        P.hd_zi[z] = verdict; P.hd_zi[(size_t)n + z] = ok ? nsub : 0; P.hd_zi[2 * (size_t)n + z] = nind; P.hd_zi[3 * (size_t)n + z] = listed;
        P.hd_zi[5 * (size_t)n + z] = P.zstat[z];
        P.hd_minp[z] = ok ? minp : 1.0;
        // the split (fused run, ccsx_hd_request.split): the ZMW leaves the polish stage here — no windows, so the rebuilt window map gives k_polish /
        // k_kinetics nothing of it and k_stitch reports the status with an empty consensus (fn / rn stay as k_post counted them).  Only this ZMW's words
        // are written, after every lane has read them.
        if (P.hd_split && verdict == CCSX_HD_HETERODUPLEX) { P.zstat[z] = CCSX_HETERODUPLEX; P.nwin[z] = 0; }
    }
}

// ------------------------------------------------------------------------------------------------
// launch wrappers (called from ccsx_api.cpp, which is plain C++)
// dynamic LDS of k_polish: [reads][68] observations (a byte each) for the largest ZMW of the batch (at most one group of PW_MAXREADS), the rest of the workgroup's
// budget holds gamma/beta of one chunk of reads
int ccsx_polish_lds(int max_reads, int *obs_bytes, int *gb_floats)
{
    hipFuncAttributes fa;                                  // per call: the attribute is per device, handles live on several
    const void *fn = (const void *)k_polish_t<PW_THREADS, PW_MINWAVES, PW_CHUNK_READS>;
    if (hipFuncGetAttributes(&fa, fn) != hipSuccess) return -1;
    const int static_bytes = (int)fa.sharedSizeBytes;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, PW_LDS_BYTES - static_bytes) != hipSuccess) return -1;
    if (max_reads > PW_MAXREADS) max_reads = PW_MAXREADS;
    if (max_reads < 1) max_reads = 1;
    *obs_bytes = ((max_reads * 68) + 15) & ~15;
    *gb_floats = (PW_LDS_BYTES - static_bytes - *obs_bytes) / 4;
    if (*gb_floats < PW_THREADS) return -1;                // (the kernel keeps a window's QV terms, one float per thread, at the head of the gamma/beta area)
    return 0;
}

// ---- k_sdust: tandem-repeat detection on a ZMW's deciding draft (DESIGN.md §2 "Tandem repeats").  One wave per ZMW, longest first.
// Symmetric DUST over triplets: for every end triplet e the suffixes [i, e] inside a window (e - i <= W - 3) are scored in order of growing length.
// [i, e] is a perfect interval when its score S / k (S = pairs of equal triplets, k = triplets - 1) exceeds T / 10 and is at least the score of every
// perfect interval inside it: the best perfect interval of every start with an earlier end (sBest) and the perfect suffixes of e found so far.  Lane l owns
// a contiguous range of ends and first replays the W - 3 ends before it without output, starting no interval before its warm-up's first triplet: whether
// an interval is perfect depends only on the intervals inside it, so the split is exact.  The masked bases of each end's perfect suffixes ([i_min, e + 2])
// merge into runs that are ORed into an LDS bit mask; a scan of the mask finds the longest run.  Exact gate: a suffix has at most the pairs S_w of the whole
// window [ilo, e], and a perfect one needs S > 2k, so only k < S_w / 2 is scored (about 14 of 61 suffixes on random sequence).  Per lane, in [slot][lane]
// LDS cells (no bank conflicts): the ring of the last 64 triplets (bytes), the window's triplet counts (bytes), the counts of the current end's suffix (words
// tagged with e, so nothing is cleared) and the best perfect interval per start (S << 8 | k, 0 = none).  tests/sdust_ref.py restates this operation for operation.
__global__ __launch_bounds__(64) void k_sdust(KParams P, int pass)
{
    const int lane = threadIdx.x;
    if ((int)blockIdx.x >= P.n_zmw) return;
    const int z = rfl(P.zmw_perm[blockIdx.x]);
    if (rfl(P.tflag[z])) return;                                    // decided on an earlier draft of this ticket
    if (pass && !(rfl(P.zref[z]) & ZREF_PASSBIT(pass))) return;     // later passes: only the ZMWs whose draft was redone
    if (rfl(P.zstat[z]) != CCSX_SUCCESS) return;                    // no draft that the cascade aligns in this pass
    uint32_t *sCnt = dyn_lds, *sBest = dyn_lds + 64 * 64, *sMask = dyn_lds + CCSX_SDUST_TABLE_BYTES / 4;
    uint8_t *sTri = (uint8_t *)(dyn_lds + 2 * 64 * 64), *sWin = sTri + 64 * 64;
    int Ld = rfl(P.draft_len[z]);
    if (Ld > 32 * P.sdust_words) Ld = 0;                            // (bounds guard: the mask covers opts.max_length, the longest draft with status SUCCESS)
    const int nwd = (Ld + 31) >> 5;
    for (int w = lane; w < nwd; w += LANES) sMask[w] = 0;
    __syncthreads();
    const uint8_t *d = P.draft + P.seq_off[z];
    const int nt = Ld - 2;                                          // triplets 0 .. nt - 1; ends 1 .. nt - 1
    const int ch = nt >= 2 ? (nt - 1 + LANES - 1) / LANES : 0;
    const int e0 = 1 + lane * ch, e1 = min(e0 + ch, nt);
    if (e0 < e1) {
        const int lo = e0 - (CCSX_SDUST_W - 3) > 0 ? e0 - (CCSX_SDUST_W - 3) : 0;   // the warm-up's first triplet
        for (int q = 0; q < 64; ++q) { sCnt[q * 64 + lane] = 0xffffffffu; sBest[q * 64 + lane] = 0u; sWin[q * 64 + lane] = 0; }
        int t = ((d[lo] & 3) << 4) | ((d[lo + 1] & 3) << 2) | (d[lo + 2] & 3);
        sTri[(lo & 63) * 64 + lane] = (uint8_t)t;
        sWin[t * 64 + lane] = 1;
        uint32_t Sw = 0;                                            // pairs of equal triplets in the window [ilo, e]
        int rs = -1, re = -2;                                       // the run of masked bases being merged
        auto flush = [&](int a, int b) {                            // OR bases [a, b] into the mask
            if (a < 0) return;
            for (int w = a >> 5; w <= (b >> 5); ++w) {
                const int lb = a - 32 * w > 0 ? a - 32 * w : 0, hb = b - 32 * w < 31 ? b - 32 * w : 31;
                atomicOr(&sMask[w], (0xffffffffu >> (31 - hb)) & (0xffffffffu << lb));
            }
        };
        for (int e = lo + 1; e < e1; ++e) {
            t = ((t << 2) | (d[e + 2] & 3)) & 63;
            if (e - (CCSX_SDUST_W - 2) >= lo) {                     // triplet e - 62 leaves the window
                const int to = sTri[((e - (CCSX_SDUST_W - 2)) & 63) * 64 + lane];
                const uint32_t co = sWin[to * 64 + lane] - 1u;
                sWin[to * 64 + lane] = (uint8_t)co;
                Sw -= co;
            }
            {
                const uint32_t cn = sWin[t * 64 + lane];
                sWin[t * 64 + lane] = (uint8_t)(cn + 1u);
                Sw += cn;
            }
            sTri[(e & 63) * 64 + lane] = (uint8_t)t;
            sBest[(e & 63) * 64 + lane] = 0u;                       // (the slot of start e - 64: out of every window from here on)
            const uint32_t tag = (uint32_t)e << 8;
            sCnt[t * 64 + lane] = tag | 1u;
            int ilo = e - (CCSX_SDUST_W - 3) > lo ? e - (CCSX_SDUST_W - 3) : lo;
            const int kmax = Sw > 0 ? (int)((Sw - 1u) >> 1) : 0;    // (the gate: longer suffixes cannot score above 2)
            ilo = e - kmax > ilo ? e - kmax : ilo;
            uint32_t S = 0, M = 0;
            int imn = -1;
            for (int i = e - 1; i >= ilo; --i) {
                const uint32_t k = (uint32_t)(e - i);
                const uint32_t ti = sTri[(i & 63) * 64 + lane];
                const uint32_t w = sCnt[ti * 64 + lane];
                const uint32_t c = (w & ~255u) == tag ? (w & 255u) : 0u;
                S += c;
                sCnt[ti * 64 + lane] = tag | (c + 1u);
                const uint32_t b = sBest[(i & 63) * 64 + lane];
                if (b && (!M || (b >> 8) * (M & 255u) > (M >> 8) * (b & 255u))) M = b;
                if (S * 10u > (uint32_t)CCSX_SDUST_T * k && (!M || S * (M & 255u) >= (M >> 8) * k)) {
                    M = (S << 8) | k;
                    sBest[(i & 63) * 64 + lane] = M;
                    imn = i;
                }
            }
            if (e >= e0 && imn >= 0) {
                if (rs >= 0 && imn <= re + 1) { rs = imn < rs ? imn : rs; re = e + 2; }
                else { flush(rs, re); rs = imn; re = e + 2; }
            }
        }
        flush(rs, re);
    }
    __syncthreads();
    // the longest run: every lane summarises a contiguous range of bases, lane 0's loop joins the ranges in order
    const int cb = (Ld + LANES - 1) / LANES;
    const int p0 = min(lane * cb, Ld), p1 = min(p0 + cb, Ld);
    int pre = 0, cur = 0, inner = 0, full = 1;
    for (int p = p0; p < p1; ++p) {
        if ((sMask[p >> 5] >> (p & 31)) & 1u) ++cur;
        else { if (full) { pre = cur; full = 0; } inner = cur > inner ? cur : inner; cur = 0; }
    }
    if (full) pre = cur;
    inner = cur > inner ? cur : inner;
    int best = 0, run = 0;
    for (int j = 0; j < LANES; ++j) {
        const int pj = rl(pre, j);
        if (rl(full, j)) run += pj;
        else { best = imax(best, imax(run + pj, rl(inner, j))); run = rl(cur, j); }
    }
    best = imax(best, run);
    if (lane == 0) { P.tlen[z] = best; P.tflag[z] = 1 | ((P.min_tandem > 0 && best >= P.min_tandem) ? 2 : 0); }
}

// ---- k_fold: adapter palindromes on a ZMW's final draft (DESIGN.md §2 "Adapter palindromes").  One 256-thread workgroup per ZMW, longest first.
// Thread t owns a contiguous range of k-mer positions and rolls the forward and reverse-complement codes over it; every scan below re-reads the draft, so no
// per-sample state outlives a pass.  (1) The sampled positions are counted per thread; a scan of the counts finds the last position that enters (the NS_MAX-th
// sample).  (2) The samples are split by their hash into passes (normally one): per pass an open-addressing LDS table counts every canonical code of the pass
// (integer atomics), a second scan links the positions of the kept codes (count <= max_occ) into per-code lists, and every kept position walks its code's list
// for the earlier positions of the other orientation: each hit's anti-diagonal bin is counted in the LDS histogram.  A pass with more than CCSX_FOLD_CAP distinct
// codes or kept positions restarts the vote with twice the passes, so no sample is ever dropped.  (3) The winning pair of bins, a max-reduction over (H, -b).
// (4) The hits again (the table is kept when there is one pass), now reducing min / max of D, i and j over the winning bins.  Counts, minima and maxima only:
// the result does not depend on thread order.  tests/fold_ref.py restates the rule.
//
// What the three draft screens (k_fold, k_adapter, k_control) share.  screen_zmw: the workgroup's ZMW (z < 0: none), its final draft's length and number of
// 15-mer positions, and whether the cascade left it SUCCESS; a kernel tests the ZMW when that holds and its own LDS bound does.
struct ScreenZmw { int z, L, npos; bool success; };
__device__ __forceinline__ ScreenZmw screen_zmw(const KParams &P)
{
    if ((int)blockIdx.x >= P.n_zmw) return {-1, 0, 0, false};
    const int z = rfl(P.zmw_perm[blockIdx.x]), L = rfl(P.draft_len[z]);
    return {z, L, L >= CCSX_FOLD_K ? L - CCSX_FOLD_K + 1 : 0, rfl(P.zstat[z]) == CCSX_SUCCESS};
}

// one row of a report of [k][n] planes: out = plane 0's entry of the ZMW
template <class... V> __device__ __forceinline__ void put_planes(int32_t *out, size_t n, V... v) { size_t j = 0; ((out[j++ * n] = (int32_t)v), ...); }

// thread tid's contiguous share [p0, p1) of `count` positions split over nt threads (the last shares are short or empty)
__device__ __forceinline__ void thread_share(int count, int nt, int tid, int &p0, int &p1) { const int ch = (count + nt - 1) / nt; p0 = min(tid * ch, count); p1 = min(p0 + ch, count); }

// fn(i, F, R) for the K-mer (the screens' 15-mer) at every position i of [p0, e) of the draft d: F its code, R its reverse complement's, both rolled (a K - 1-base
// warm-up first)
template <int K = CCSX_FOLD_K, class Fn> __device__ __forceinline__ void kmer_scan(const uint8_t *d, int p0, int e, Fn fn)
{
    constexpr uint32_t KMASK = (1u << (2 * K)) - 1u;
    if (p0 >= e) return;
    uint32_t F = 0u, R = 0u;
    for (int t = 0; t < K - 1; ++t) { const uint32_t b = d[p0 + t] & 3u; F = (F << 2) | b; R = (R >> 2) | ((3u - b) << (2 * K - 2)); }
    for (int i = p0; i < e; ++i) {
        const uint32_t b = d[i + K - 1] & 3u;
        F = ((F << 2) | b) & KMASK;
        R = (R >> 2) | ((3u - b) << (2 * K - 2));
        fn(i, F, R);
    }
}

// q* = argmax over the pairs of adjacent bins q in [0, nq) of their hits pair(q), ties to the smallest q: returns q* and H = its hits, or -1 and 0 when no pair
// has a hit.  A max-reduction over (H, -q) through *sBest, which the workgroup has zeroed before its last barrier.  It holds a __syncthreads():
// every thread of the workgroup calls it, in uniform control flow, and every thread gets the same value.
template <class Pair> __device__ __forceinline__ int best_pair(unsigned long long *sBest, int nq, int nt, Pair pair, int &H)
{
    unsigned long long best = 0ull;
    for (int q = (int)threadIdx.x; q < nq; q += nt) {
        const unsigned long long key = ((unsigned long long)pair(q) << 32) | (0xffffffffu - (uint32_t)q);
        best = key > best ? key : best;
    }
    if (best >> 32) atomicMax(sBest, best);
    __syncthreads();
    H = (int)(*sBest >> 32);
    return H ? (int)(0xffffffffu - (uint32_t)(*sBest & 0xffffffffull)) : -1;
}

__global__ __launch_bounds__(CCSX_FOLD_THREADS) void k_fold(KParams P)
{
    constexpr int K = CCSX_FOLD_K, NT = CCSX_FOLD_THREADS, T = CCSX_FOLD_SLOTS, CAP = CCSX_FOLD_CAP;
    constexpr uint32_t NIL = 0xffffu;
    static_assert((T & (T - 1)) == 0 && T == 2048 && CAP < T && CAP < (int)NIL, "k_fold: the slot hash takes the top 11 bits");
    __shared__ uint32_t sKey[T];          // canonical code + 1 (0 = empty)
    __shared__ uint32_t sCnt[T];          // samples of the pass with that code
    __shared__ uint32_t sHead[T];         // first linked position of the code (NIL = none)
    __shared__ uint32_t sMem[CAP];        // linked position: i << 1 | (F != C)
    __shared__ uint16_t sNext[CAP], sSlot[CAP];
    __shared__ uint32_t sScan[NT];
    __shared__ int sV[10];                // 0 codes, 1 linked, 2 overflow, 3 last position that enters, 4..9 min D, max D, min i, max i, min j, max j
    __shared__ unsigned long long sBest;
    uint32_t *sHist = dyn_lds;            // [fold_bins] hits per anti-diagonal bin
    const int tid = threadIdx.x;
    const ScreenZmw zm = screen_zmw(P);
    if (zm.z < 0) return;
    const int L = zm.L, npos = zm.npos;
    const int nb = npos > 0 ? ((2 * L - K - 1) >> 6) + 1 : 0;       // bins of this draft's anti-diagonals
    const size_t n = (size_t)P.n_zmw;
    int32_t *out = P.fold_zi + zm.z;
    if (!zm.success || nb + 1 > P.fold_bins) {                       // untested (the second: a bounds guard, the histogram covers opts.max_length)
        if (tid == 0) put_planes(out, n, CCSX_FOLD_UNTESTED, -1, 0, 0);
        return;
    }
    const uint8_t *d = P.draft + P.seq_off[zm.z];
    int p0, p1;
    thread_share(npos, NT, tid, p0, p1);
    // fn(i, F, C, h) for every sampled position i of this thread's range up to `last`
    auto scan = [&](int last, auto fn) {
        kmer_scan(d, p0, min(p1, last + 1), [&](int i, uint32_t F, uint32_t R) {
            const uint32_t C = F < R ? F : R, h = ccsx_fmix32(C);
            if ((h & 7u) == 0u) fn(i, F, C, h);
        });
    };
    // (1) the last position that enters
    int cnt = 0;
    scan(npos - 1, [&](int, uint32_t, uint32_t, uint32_t) { ++cnt; });
    sScan[tid] = (uint32_t)cnt;
    if (tid == 0) { sV[3] = npos - 1; sBest = 0ull; }
    __syncthreads();
    for (int o = 1; o < NT; o <<= 1) {
        const uint32_t v = tid >= o ? sScan[tid - o] : 0u;
        __syncthreads();
        sScan[tid] += v;
        __syncthreads();
    }
    const int incl = (int)sScan[tid], excl = incl - cnt, total = (int)sScan[NT - 1];
    if (excl < CCSX_FOLD_NS_MAX && incl >= CCSX_FOLD_NS_MAX) {        // this range holds the NS_MAX-th sample
        int k = CCSX_FOLD_NS_MAX - excl;
        scan(npos - 1, [&](int i, uint32_t, uint32_t, uint32_t) { if (--k == 0) sV[3] = i; });
    }
    __syncthreads();
    const int last = sV[3];
    const int ns = min(total, CCSX_FOLD_NS_MAX);
    const uint32_t max_occ = (uint32_t)P.fold.max_occ;
    // (2) pass p of nparts (a power of two): the table and the linked positions; false (for every thread) when it overflowed
    auto build = [&](int p, int nparts) -> bool {
        for (int s = tid; s < T; s += NT) { sKey[s] = 0u; sCnt[s] = 0u; sHead[s] = NIL; }
        if (tid == 0) { sV[0] = 0; sV[1] = 0; sV[2] = 0; }
        __syncthreads();
        scan(last, [&](int, uint32_t, uint32_t C, uint32_t h) {
            if ((int)((h >> 3) & (uint32_t)(nparts - 1)) != p) return;
            const uint32_t key = C + 1u;
            int s = (int)(h >> 21);
            for (int probe = 0; probe < T; ++probe, s = (s + 1) & (T - 1)) {
                uint32_t k = sKey[s];
                if (k == 0u) {
                    k = atomicCAS(&sKey[s], 0u, key);
                    if (k == 0u) { if (atomicAdd(&sV[0], 1) >= CAP) sV[2] = 1; k = key; }
                }
                if (k == key) { atomicAdd(&sCnt[s], 1u); return; }
            }
            sV[2] = 1;                                              // (the table is full)
        });
        __syncthreads();
        if (sV[2]) { __syncthreads(); return false; }
        scan(last, [&](int i, uint32_t F, uint32_t C, uint32_t h) {
            if ((int)((h >> 3) & (uint32_t)(nparts - 1)) != p) return;
            const uint32_t key = C + 1u;
            int s = (int)(h >> 21);
            while (sKey[s] != key) s = (s + 1) & (T - 1);           // (inserted above)
            if (sCnt[s] > max_occ) return;
            const int m = atomicAdd(&sV[1], 1);
            if (m >= CAP) { sV[2] = 1; return; }
            sMem[m] = ((uint32_t)i << 1) | (F != C ? 1u : 0u);
            sSlot[m] = (uint16_t)s;
            sNext[m] = (uint16_t)atomicExch(&sHead[s], (uint32_t)m);
        });
        __syncthreads();
        const bool ok = sV[2] == 0;
        __syncthreads();
        return ok;
    };
    // fn(i, j, D) for every hit of the current pass, counted by its later position j
    auto hits = [&](auto fn) {
        const int nm = sV[1];
        for (int m = tid; m < nm; m += NT) {
            const uint32_t vj = sMem[m];
            const int j = (int)(vj >> 1);
            for (uint32_t q = sHead[sSlot[m]]; q != NIL; q = sNext[q]) {
                const uint32_t vi = sMem[q];
                const int i = (int)(vi >> 1);
                if (((vi ^ vj) & 1u) && i + K <= j) fn(i, j, i + j + K - 1);
            }
        }
    };
    int nparts = 1;
    while (nparts * CAP < ns) nparts <<= 1;
    for (;;) {
        for (int b = tid; b <= nb; b += NT) sHist[b] = 0u;
        bool ok = true;
        for (int p = 0; p < nparts && ok; ++p) {
            ok = build(p, nparts);
            if (ok) { hits([&](int, int, int D) { atomicAdd(&sHist[D >> 6], 1u); }); __syncthreads(); }
        }
        if (ok) break;
        nparts <<= 1;
    }
    // (3) b* = argmax over b of H(b) = hist[b] + hist[b + 1], ties to the smallest b
    int H;
    const int bs = best_pair(&sBest, nb, NT, [&](int b) { return sHist[b] + sHist[b + 1]; }, H);
    if (H == 0) {
        if (tid == 0) put_planes(out, n, CCSX_FOLD_NONE, -1, 0, 0);
        return;
    }
    // (4) the extent of the winning hits
    if (tid == 0) { sV[4] = 0x7fffffff; sV[5] = -1; sV[6] = 0x7fffffff; sV[7] = -1; sV[8] = 0x7fffffff; sV[9] = -1; }
    __syncthreads();
    auto extent = [&](int i, int j, int D) {
        if ((D >> 6) != bs && (D >> 6) != bs + 1) return;
        atomicMin(&sV[4], D); atomicMax(&sV[5], D); atomicMin(&sV[6], i); atomicMax(&sV[7], i); atomicMin(&sV[8], j); atomicMax(&sV[9], j);
    };
    if (nparts == 1) hits(extent);
    else for (int p = 0; p < nparts; ++p) { (void)build(p, nparts); hits(extent); __syncthreads(); }
    __syncthreads();
    if (tid == 0) {
        const ccsx_fold_opts &o = P.fold;
        const int fold = (sV[4] + sV[5]) / 4;
        const int span = min(sV[7] - sV[6], sV[9] - sV[8]) + K;
        const int shorter = min(fold, L - fold);
        const bool reach = fold <= L - fold ? sV[6] <= o.end_slack : sV[9] + K >= L - o.end_slack;
        const bool pal = H >= o.min_hits && span >= o.min_arm && 10 * span >= o.min_span_tenths * shorter && reach;
        put_planes(out, n, pal ? CCSX_FOLD_PALINDROME : CCSX_FOLD_NONE, fold, H, span);
    }
}

// ---- k_control: the control screen on a ZMW's final draft (DESIGN.md §2 "Control screen").  One 256-thread workgroup per ZMW, longest first.  The workgroup
// copies the control's index (ccsx_kernels.h: sorted codes, their positions, a prefilter bitmap; 28 KiB, L2-resident for the whole launch) into LDS.  Thread t owns a
// contiguous range of k-mer positions and rolls F and R over it as k_fold's scan does; each code passes the prefilter bit, then a 12-step lower bound over the
// padded code array, and every index entry with exactly that code is a hit (a kept code has at most max_occ entries).  (1) Every hit's diagonal bin is counted in
// one of two LDS histograms.  (2) The winning (orientation, pair of bins), a max-reduction over (H, orientation 0 first, -b).  (3) The hits again, now only the
// winning ones: their control positions set bits of an LDS bitmap (matched = its population count, the control extent its first and last bit), the draft extent is
// a per-thread min / max joined by one atomic each.  Counts, minima, maxima and a bitmap only: the result does not depend on thread order.  tests/control_ref.py
// restates the rule.
__global__ __launch_bounds__(CCSX_CONTROL_THREADS) void k_control(KParams P)
{
    constexpr int K = CCSX_FOLD_K, NT = CCSX_CONTROL_THREADS, CAP = CCSX_CONTROL_MAX_LEN;
    static_assert((CAP & (CAP - 1)) == 0 && CAP <= 65536 && CCSX_CONTROL_INDEX_WORDS % 4 == 0, "k_control: a power-of-two code array, 16-bit positions, 16-byte copies");
    __shared__ __attribute__((aligned(16))) uint32_t sIdx[CCSX_CONTROL_INDEX_WORDS];
    __shared__ uint32_t sSeen[CAP / 32];  // bit j: control position j is among the winning hits
    __shared__ int sV[5];                 // 0 min i, 1 max i, 2 matched, 3 min j, 4 max j
    __shared__ unsigned long long sBest;
    const int tid = threadIdx.x, M = P.ctl_len, bins = P.ctl_bins;
    const ScreenZmw zm = screen_zmw(P);
    if (zm.z < 0) return;
    const int L = zm.L, npos = zm.npos;
    const int nb = npos > 0 ? ((L - K + M - K) >> 6) + 1 : 0;       // bins of this draft's diagonals
    const bool tested = zm.success && nb + 1 <= bins;               // (the second: a bounds guard, the histograms cover opts.max_length)
    const size_t n = (size_t)P.n_zmw;
    int32_t *out = P.ctl_zi + zm.z;
    if (!tested || npos == 0) {                                      // (npos == 0: too short for one 15-mer)
        if (tid == 0) put_planes(out, n, tested ? CCSX_CONTROL_NONE : CCSX_CONTROL_UNTESTED, -1, 0, 0, 0, 0, 0, 0);
        return;
    }
    uint32_t *sHist = dyn_lds;            // [2][bins] hits per diagonal bin of orientation 0, 1
    {
        const uint4 *src = reinterpret_cast<const uint4 *>(P.ctl_index);
        uint4 *dst = reinterpret_cast<uint4 *>(sIdx);
        for (int w = tid; w < CCSX_CONTROL_INDEX_WORDS / 4; w += NT) dst[w] = src[w];
    }
    for (int b = tid; b < 2 * bins; b += NT) sHist[b] = 0u;
    for (int w = tid; w < CAP / 32; w += NT) sSeen[w] = 0u;
    if (tid == 0) { sV[0] = 0x7fffffff; sV[1] = -1; sV[2] = 0; sV[3] = 0x7fffffff; sV[4] = -1; sBest = 0ull; }
    __syncthreads();
    const uint32_t *sCode = sIdx, *sFilt = sIdx + CCSX_CONTROL_FILTER_WORD;
    const uint16_t *sPos = reinterpret_cast<const uint16_t *>(sIdx + CCSX_CONTROL_POS_WORD);
    const uint8_t *d = P.draft + P.seq_off[zm.z];
    int p0, p1;
    thread_share(npos, NT, tid, p0, p1);
    // fn(o, i, j, dg) for every hit of this thread's range: orientation, draft position, control position, diagonal
    auto scan = [&](auto fn) {
        auto lookup = [&](uint32_t code, int o, int i, int u) {
            const uint32_t h = ccsx_fmix32(code) & (uint32_t)(CCSX_CONTROL_FILTER_BITS - 1);
            if (!((sFilt[h >> 5] >> (h & 31u)) & 1u)) return;
            int lo = 0;
            for (int s = CAP >> 1; s > 0; s >>= 1) lo += sCode[lo + s - 1] < code ? s : 0;   // entries below `code` (the padding is above every code)
            for (int e = lo; sCode[e] == code; ++e) { const int j = (int)sPos[e]; fn(o, i, j, u - j + (M - K)); }
        };
        kmer_scan(d, p0, p1, [&](int i, uint32_t F, uint32_t R) { lookup(F, 0, i, i); lookup(R, 1, i, (L - K) - i); });
    };
    // (1) the vote
    scan([&](int o, int, int, int dg) { atomicAdd(&sHist[o * bins + (dg >> 6)], 1u); });
    __syncthreads();
    // (2) (o*, b*) = argmax of H(o, b) = hist[o][b] + hist[o][b + 1], ties to orientation 0, then to the smallest b
    // (as one index q = o * nb + b: the smallest q of a tie is orientation 0's, then the smallest b)
    int H;
    const int qs = best_pair(&sBest, 2 * nb, NT, [&](int q) { const int w = q >= nb ? q - nb + bins : q; return sHist[w] + sHist[w + 1]; }, H);
    if (H == 0) {
        if (tid == 0) put_planes(out, n, CCSX_CONTROL_NONE, -1, 0, 0, 0, 0, 0, 0);
        return;
    }
    const int os = qs >= nb ? 1 : 0, bs = qs - os * nb;
    // (3) the winning hits: distinct control positions and the two extents
    int imin = 0x7fffffff, imax = -1;
    scan([&](int o, int i, int j, int dg) {
        if (o != os || ((dg >> 6) != bs && (dg >> 6) != bs + 1)) return;
        atomicOr(&sSeen[j >> 5], 1u << (j & 31));
        imin = i < imin ? i : imin; imax = i > imax ? i : imax;
    });
    if (imax >= 0) { atomicMin(&sV[0], imin); atomicMax(&sV[1], imax); }
    __syncthreads();
    for (int w = tid; w < CAP / 32; w += NT) {
        const uint32_t m = sSeen[w];
        if (m) { atomicAdd(&sV[2], __popc(m)); atomicMin(&sV[3], w * 32 + __ffs((int)m) - 1); atomicMax(&sV[4], w * 32 + 31 - __clz((int)m)); }
    }
    __syncthreads();
    if (tid == 0) {
        const ccsx_control_opts &o = P.ctl;
        const int cs = sV[3], ce = sV[4] + K, ds = sV[0], de = sV[1] + K;
        const bool found = sV[2] >= o.min_matched && 10 * (ce - cs) >= o.min_ctl_tenths * M && 10ll * (de - ds) >= (long long)o.min_draft_tenths * L;
        put_planes(out, n, found ? CCSX_CONTROL_FOUND : CCSX_CONTROL_NONE, os, H, sV[2], cs, ce, ds, de);
    }
}

// ---- k_orient: the orientation of the passes flagged CCSX_PASS_STRAND_UNKNOWN against their ZMW's anchor pass (DESIGN.md §2 "Pass orientation"), first kernel of
// the draft stage.  CCSX_ORIENT_MAX_WGS 256-thread workgroups at most, each with its own table in the handle's scratch; a workgroup walks the ZMWs blockIdx.x,
// blockIdx.x + gridDim.x, ... of the launch order (longest first).  A ZMW without a flagged pass gets its report rows (GIVEN) and is left at once.  Otherwise the
// workgroup (1) clears the table's ccsx_orient_slots(M) words and the LDS prefilter and inserts the forward code of every 13-mer position of the anchor: thread t owns
// a contiguous range and rolls F over it as k_fold's scan does; atomicCAS on the code's slot, linear probing (load <= 1/2: a probe ends), so the table holds the SET
// of codes whatever the order of insertion; (2) per flagged pass rolls F and R over the pass the same way, looks each up — the prefilter bit, which may only
// reject, then the probe sequence up to the code or an empty slot: membership is exact — and sums the two counts of positions; (3) thread 0 calls the pass and
// writes its report row and its flags byte (bit 0 resolved, bit 3 cleared).  Every access of the table is an L2 atomic (clear, insert, look-up), so no look-up can
// be served a line this CU's L1 kept from an earlier ZMW.  Counts only: the result does not depend on thread order.  tests/orient_ref.py restates the rule.
__global__ __launch_bounds__(CCSX_ORIENT_THREADS) void k_orient(KParams P)
{
    constexpr int K = CCSX_ORIENT_K, NT = CCSX_ORIENT_THREADS, FW = CCSX_ORIENT_FILTER_BITS / 32, SH = CCSX_ORIENT_FILTER_SHIFT;
    constexpr uint32_t EMPTY = CCSX_ORIENT_EMPTY;
    static_assert(2 * K <= 30 && (32 - SH) == 18 && CCSX_ORIENT_FILTER_BITS == (1 << 18), "k_orient: a code is below EMPTY, the prefilter takes the hash's top 18 bits");
    __shared__ uint32_t sFilt[FW];
    __shared__ int sV[2];                 // v_same, v_opp of the current pass
    const int tid = threadIdx.x;
    const size_t R = (size_t)P.n_reads;
    uint32_t *tab = P.orient_tab + (size_t)blockIdx.x * (size_t)P.orient_tab_words;
    uint8_t *flags = P.orient_flags, *o_strand = P.orient_rep8, *o_call = P.orient_rep8 + R;
    int32_t *o_same = P.orient_votes, *o_opp = P.orient_votes + R;
    auto put = [&](int r, int f, int strand, int call, int vs, int vo) {
        o_strand[r] = (uint8_t)strand; o_call[r] = (uint8_t)call; o_same[r] = vs; o_opp[r] = vo;
        flags[r] = (uint8_t)((f & ~(CCSX_PASS_STRAND_UNKNOWN | 1)) | strand);
    };
    for (int zi = (int)blockIdx.x; zi < P.n_zmw; zi += (int)gridDim.x) {
        const int z = rfl(P.zmw_perm[zi]), r0 = rfl(P.read_off[z]), nr = rfl(P.read_off[z + 1]) - r0;
        int any = 0;
        for (int q = tid; q < nr; q += NT) {
            const int f = flags[r0 + q];
            if (f & CCSX_PASS_STRAND_UNKNOWN) any = 1;
            else { o_strand[r0 + q] = (uint8_t)(f & 1); o_call[r0 + q] = CCSX_ORIENT_GIVEN; o_same[r0 + q] = 0; o_opp[r0 + q] = 0; }
        }
        if (!__syncthreads_or(any)) continue;
        const int a = rfl(P.orient_anchor[z]);
        if (a < 0 || a >= nr) {                                       // no full-length pass: the caller's bits stay
            for (int q = tid; q < nr; q += NT) { const int f = flags[r0 + q]; if (f & CCSX_PASS_STRAND_UNKNOWN) put(r0 + q, f, f & 1, CCSX_ORIENT_NO_ANCHOR, 0, 0); }
            continue;
        }
        const int M = rfl((int)(P.base_off[r0 + a + 1] - P.base_off[r0 + a]));
        const int slots = ccsx_orient_slots(M);
        const int nposA = (M >= K && slots <= P.orient_tab_words) ? M - K + 1 : 0;   // (the second: a bounds guard, the host sizes the tables for the longest anchor)
        const int anchor_rev = rfl(flags[r0 + a] & 1);
        const uint32_t mask = (uint32_t)slots - 1u;
        if (nposA > 0) {                                              // (1) the anchor's set
            for (int w = tid; w < FW; w += NT) sFilt[w] = 0u;
            for (int s = tid; s < slots; s += NT) __hip_atomic_store(tab + s, EMPTY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __threadfence();
            __syncthreads();
            int p0, p1;
            thread_share(nposA, NT, tid, p0, p1);
            kmer_scan<K>(P.bases + P.base_off[r0 + a], p0, p1, [&](int, uint32_t F, uint32_t) {
                const uint32_t h = ccsx_fmix32(F), b = h >> SH;
                atomicOr(&sFilt[b >> 5], 1u << (b & 31u));
                for (uint32_t s = h & mask;; s = (s + 1u) & mask) {
                    uint32_t k = __hip_atomic_load(tab + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (k == EMPTY) k = atomicCAS(tab + s, EMPTY, F);
                    if (k == EMPTY || k == F) break;
                }
            });
            __threadfence();
            __syncthreads();
        }
        auto member = [&](uint32_t code) -> int {
            const uint32_t h = ccsx_fmix32(code), b = h >> SH;
            if (!((sFilt[b >> 5] >> (b & 31u)) & 1u)) return 0;
            for (uint32_t s = h & mask;; s = (s + 1u) & mask) {
                const uint32_t k = __hip_atomic_load(tab + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (k == code) return 1;
                if (k == EMPTY) return 0;
            }
        };
        for (int q = 0; q < nr; ++q) {                                // (2), (3) the flagged passes, one after the other
            const int f = rfl(flags[r0 + q]);
            if (!(f & CCSX_PASS_STRAND_UNKNOWN)) continue;
            if (q == a) { if (tid == 0) put(r0 + q, f, f & 1, CCSX_ORIENT_ANCHOR, 0, 0); continue; }
            const int N = rfl((int)(P.base_off[r0 + q + 1] - P.base_off[r0 + q]));
            if (tid == 0) { sV[0] = 0; sV[1] = 0; }
            __syncthreads();
            int cs = 0, co = 0;
            if (nposA > 0 && N >= K) {
                int p0, p1;
                thread_share(N - K + 1, NT, tid, p0, p1);
                kmer_scan<K>(P.bases + P.base_off[r0 + q], p0, p1, [&](int, uint32_t F, uint32_t Rc) { cs += member(F); co += member(Rc); });
            }
            cs = wave_reduce_add_i32(cs); co = wave_reduce_add_i32(co);
            if ((tid & 63) == 0 && (cs | co)) { atomicAdd(&sV[0], cs); atomicAdd(&sV[1], co); }
            __syncthreads();
            if (tid == 0) {
                const int vs = sV[0], vo = sV[1], mv = P.orient.min_votes, ra = P.orient.ratio;
                int call = CCSX_ORIENT_UNDETERMINED, strand = f & 1;  // (undetermined: the caller's bit, a prior)
                if (vs >= mv && vs >= ra * vo) { call = CCSX_ORIENT_SAME; strand = anchor_rev; }
                else if (vo >= mv && vo >= ra * vs) { call = CCSX_ORIENT_OPPOSITE; strand = anchor_rev ^ 1; }
                put(r0 + q, f, strand, call, vs, vo);
            }
        }
        __syncthreads();                                              // (the next ZMW clears the prefilter)
    }
}

// ---- k_adapter: the adapter screen on a ZMW's final draft (DESIGN.md §2 "Adapter screen").  One 256-thread workgroup per ZMW, longest first.  Myers' bit-vector
// column update, one 64-bit word per search.  A lane owns one (search, chunk of CCSX_ADAPTER_CHUNK draft bases): it starts from the all-ones vertical state m + k
// bases before its chunk (after that warm-up every value <= k is exact and so is the predicate E <= k: a fresh start can only over-estimate, and a match of distance
// <= k spans at most m + k draft bases) and owns the runs that START inside its chunk, following such a run past the chunk's end until it closes, so every hit is
// found by exactly one lane.  The hit's start is the owning lane's second pass: the reversed pattern against the reversed draft, anchored at the end.  Aggregates
// are LDS atomic add / min / max / or (counts, minima, maxima and a bitmap of the union: nothing depends on lane order).  The list: every hit's key (end, search,
// dist, length) goes to an LDS buffer; when the buffer overflows (a draft made of adapters) the pass is repeated for the hits that end at or before the 16th set
// bit of a bitmap of the ends (at most 16 ends x 16 searches, so that pass cannot overflow).  The 16 smallest keys are selected by rank.  tests/adapter_ref.py
// restates the rule.
// (MyersCol / myers_step: barcode_core.h, shared with k_barcode)
__global__ __launch_bounds__(CCSX_ADAPTER_THREADS) void k_adapter(KParams P)
{
    constexpr int NT = CCSX_ADAPTER_THREADS, CH = CCSX_ADAPTER_CHUNK, CAP = CCSX_ADAPTER_BUF, MAXS = 2 * CCSX_ADAPTER_MAX_PATTERNS, NH = CCSX_ADAPTER_MAX_HITS;
    __shared__ unsigned long long sPeq[MAXS][4], sPeqR[MAXS][4];   // match masks of every search, and of its reversed pattern
    __shared__ unsigned long long sBuf[CAP];                       // hit keys: end << 32 | search << 24 | dist << 16 | end - start
    __shared__ int sSeg[NT][3];                                    // the zero-run scan's segments: leading zeros, trailing zeros, longest inner run
    __shared__ int sM[MAXS];                                       // pattern lengths
    __shared__ int sV[8];                                          // 0 n_hits, 1 first_start, 2 last_end, 3 min_dist, 4 covered, 5 buffered keys, 6 bound on the ends
    const int tid = threadIdx.x;
    const ScreenZmw zm = screen_zmw(P);
    if (zm.z < 0) return;
    const int z = zm.z, L = zm.L, words = (L + 31) >> 5;
    const size_t n = (size_t)P.n_zmw;
    int32_t *out = P.adapt_zi + z;
    int32_t *list = P.adapt_hits + (size_t)z * NH * 3;
    if (!zm.success || words > P.adapt_words) {                      // untested (the second: a bounds guard, the bitmaps cover opts.max_length)
        if (tid == 0) put_planes(out, n, 0, 0, 0, 0, 0, 0, -1, -1, 255);
        if (tid < NH * 3) list[tid] = 0;
        return;
    }
    uint32_t *sUnion = dyn_lds, *sEnds = dyn_lds + P.adapt_words;   // bit b: draft base b is inside a hit / a hit ends at b + 1
    const uint8_t *d = P.draft + P.seq_off[z];
    const int S = 2 * P.adapt_n;
    if (tid < S * 4) {
        const int s = tid >> 2, code = tid & 3, a = s >> 1, m = P.adapt_len[a];
        unsigned long long f = 0ull, r = 0ull;
        for (int i = 0; i < m; ++i) {
            const int q = (s & 1) ? m - 1 - i : i;
            int b = (int)((P.adapt_seq[a][q >> 4] >> (2 * (q & 15))) & 3u);
            if (s & 1) b = 3 - b;
            if (b == code) { f |= 1ull << i; r |= 1ull << (m - 1 - i); }
        }
        sPeq[s][code] = f; sPeqR[s][code] = r;
        if (code == 0) sM[s] = m;
    }
    for (int w = tid; w < words; w += NT) { sUnion[w] = 0u; sEnds[w] = 0u; }
    if (tid == 0) { sV[0] = 0; sV[1] = 0x7fffffff; sV[2] = -1; sV[3] = 255; sV[4] = 0; sV[5] = 0; sV[6] = 0x7fffffff; }
    __syncthreads();
    const int nchunks = (L + CH - 1) / CH;
    // every hit of this thread's (search, chunk) items that ends at or before `bound`: fn(start, end, search, dist)
    auto scan = [&](int bound, auto fn) {
        for (int it = tid; it < nchunks * S; it += NT) {
            const int c = it / S, s = it - c * S;
            const int lo = c * CH, hi = min(L, lo + CH);
            if (lo >= bound) continue;                               // (its hits end beyond lo)
            const int m = sM[s], k = m * P.adapt.max_dist_pct / 100;
            const unsigned long long top = 1ull << (m - 1);
            const unsigned long long e0 = sPeq[s][0], e1 = sPeq[s][1], e2 = sPeq[s][2], e3 = sPeq[s][3];
            MyersCol col{~0ull, 0ull, m};
            bool prev = false, own = false, done = false;
            int best = 0, end = 0;
            // a closed run of this lane: its start by the anchored second pass
            auto emit = [&]() {
                if (end > bound) return;
                MyersCol rc{~0ull, 0ull, m};
                const int xmax = min(end, m + best);
                int x = 0;
                while (x < xmax) {
                    const int b = d[end - 1 - x] & 3;
                    ++x;
                    myers_step(rc, sPeqR[s][b], top, 1ull);
                    if (x >= m - best && rc.score == best) break;
                }
                fn(end - x, end, s, best);
            };
            int j = max(0, lo - (m + k));
            while (j < L && !done) {
                const int nb = min(8, L - j);
                uint8_t ch[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) ch[q] = q < nb ? d[j + q] : (uint8_t)0;
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    if (q >= nb || done) continue;
                    const int b = ch[q] & 3;
                    myers_step(col, b == 0 ? e0 : b == 1 ? e1 : b == 2 ? e2 : e3, top, 0ull);
                    const int jj = j + q + 1;                       // E[jj] = col.score
                    const bool ok = col.score <= k;
                    if (jj > lo) {
                        if (ok && !prev) { own = true; best = col.score; end = jj; }          // (jj <= hi: the lane stops at hi outside an owned run)
                        else if (ok && own && col.score < best) { best = col.score; end = jj; }
                        else if (!ok && prev && own) { emit(); own = false; }
                        if (jj >= hi && !own) done = true;
                    }
                    prev = ok;
                }
                j += nb;
            }
            if (own) emit();                                         // (the run reaches the draft's end)
        }
    };
    scan(0x7fffffff, [&](int start, int end, int s, int dist) {
        atomicAdd(&sV[0], 1); atomicMin(&sV[1], start); atomicMax(&sV[2], end); atomicMin(&sV[3], dist);
        for (int w = start >> 5; w <= (end - 1) >> 5; ++w) {
            const int b0 = max(start, w << 5) & 31, b1 = min(end, (w + 1) << 5) - (w << 5);   // bits [b0, b1) of word w
            atomicOr(&sUnion[w], (b1 == 32 ? 0xffffffffu : (1u << b1) - 1u) & ~((1u << b0) - 1u));
        }
        atomicOr(&sEnds[(end - 1) >> 5], 1u << ((end - 1) & 31));
        const int i = atomicAdd(&sV[5], 1);
        if (i < CAP) sBuf[i] = ((unsigned long long)end << 32) | ((unsigned long long)s << 24) | ((unsigned long long)dist << 16) | (unsigned long long)(end - start);
    });
    __syncthreads();
    const int n_hits = sV[0];
    if (n_hits > CAP) {                                              // the buffer overflowed: again, for the hits up to the 16th end
        if (tid == 0) {
            int seen = 0, bound = L;
            for (int w = 0; w < words && seen < NH; ++w)
                for (uint32_t v = sEnds[w]; v && seen < NH; v &= v - 1u)
                    if (++seen == NH) bound = (w << 5) + __builtin_ctz(v) + 1;
            sV[6] = bound; sV[5] = 0;
        }
        __syncthreads();
        scan(sV[6], [&](int start, int end, int s, int dist) {
            const int i = atomicAdd(&sV[5], 1);
            if (i < CAP) sBuf[i] = ((unsigned long long)end << 32) | ((unsigned long long)s << 24) | ((unsigned long long)dist << 16) | (unsigned long long)(end - start);
        });
        __syncthreads();
    }
    // the list: the keys of rank < 16
    const int nk = min(sV[5], CAP), n_listed = min(n_hits, NH);
    for (int i = tid; i < nk; i += NT) {
        const unsigned long long key = sBuf[i];
        int rank = 0;
        for (int q = 0; q < nk && rank < NH; ++q) rank += sBuf[q] < key ? 1 : 0;
        if (rank < NH) {
            const int end = (int)(key >> 32);
            list[rank * 3] = end - (int)(key & 0xffffu); list[rank * 3 + 1] = end; list[rank * 3 + 2] = (int)((key >> 24) & 0xffu) | ((int)((key >> 16) & 0xffu) << 8);
        }
    }
    if (tid < NH && tid >= n_listed) { list[tid * 3] = 0; list[tid * 3 + 1] = 0; list[tid * 3 + 2] = 0; }
    // covered and max_gap from the union
    int cov = 0;
    for (int w = tid; w < words; w += NT) cov += __popc(sUnion[w]);
    if (cov) atomicAdd(&sV[4], cov);
    {
        int a, b;
        thread_share(L, NT, tid, a, b);
        int lead = -1, run = 0, inner = 0;
        for (int i = a; i < b; ++i) {
            if ((sUnion[i >> 5] >> (i & 31)) & 1u) { if (lead < 0) lead = run; inner = max(inner, run); run = 0; }
            else ++run;
        }
        sSeg[tid][0] = lead < 0 ? b - a : lead; sSeg[tid][1] = run; sSeg[tid][2] = lead < 0 ? -1 : inner;   // (-1: the segment has no covered base)
    }
    __syncthreads();
    if (tid == 0) {
        int run = 0, gap = 0;
        for (int t = 0; t < NT; ++t) {
            if (sSeg[t][2] < 0) { run += sSeg[t][0]; continue; }
            gap = max(gap, max(run + sSeg[t][0], sSeg[t][2]));
            run = sSeg[t][1];
        }
        gap = max(gap, run);
        const ccsx_adapter_opts &o = P.adapt;
        const int first = n_hits ? sV[1] : -1, last = sV[2];
        int v = 0;
        if (n_hits >= o.min_copies && gap <= o.max_insert) v |= CCSX_ADAPTER_CONCAT;
        if (n_hits >= 1 && (first <= o.end_slack || last >= L - o.end_slack)) v |= CCSX_ADAPTER_NEAR_END;
        put_planes(out, n, 1, v, n_hits, n_listed, sV[4], gap, first, last, sV[3]);
    }
}

// ---- the coverage screen (DESIGN.md §2 "Coverage rule"; include/ccsx.h ccsx_coverage_*).  k_coverage: one wave per ZMW, longest first, on the draft stream after
// the draft screens.  Lanes stride over the windows of the final draft; a lane walks the ZMW's passes and takes the segment between the window's two edge
// columns from the entry rows exactly as k_polish's prologue does (before the 63-base limit, before trimming).  Per pass an LDS flag says "missed some window":
// every lane that sets it stores the same 1, so the AND over the windows does not depend on lane order.  Windows by clean count go into an LDS histogram, from
// which drop_windows is a sum once cov_max is known.  Counts, maxima, minima and integer sums only: nothing depends on the order in which lanes ran.
__global__ __launch_bounds__(64) void k_coverage(KParams P)
{
    __shared__ int sLen[CCSX_MAX_PASSES + 1];               // pass r: its length, or -1 when it did not align (avalid)
    __shared__ uint8_t sMiss[CCSX_MAX_PASSES + 1];          // pass r does not reach some window
    __shared__ int sHist[CCSX_MAX_PASSES + 1];              // windows with clean_w = c
    if ((int)blockIdx.x >= P.n_zmw) return;
    const int lane = threadIdx.x;
    const int z = rfl(P.zmw_perm[blockIdx.x]);
    const size_t n = (size_t)P.n_zmw;
    int32_t *out = P.cov_zi + z;
    if (rfl(P.zstat[z]) != CCSX_SUCCESS) {                  // UNTESTED: every plane 0
        if (lane < CCSX_COVERAGE_PLANES) out[(size_t)lane * n] = 0;
        return;
    }
    const int nw = rfl(P.nwin[z]), Ld = rfl(P.draft_len[z]);
    const int r0 = rfl(P.read_off[z]);
    int nreads = rfl(P.nreads_used[z]), nfull = rfl(P.nfull[z]);
    if (nreads > CCSX_MAX_PASSES) nreads = CCSX_MAX_PASSES; // (never: the engine uses at most that many)
    if (nfull > nreads) nfull = nreads;
    const int32_t *wb = P.wbounds + P.wb_off[z];
    const size_t w0 = (size_t)(P.wb_off[z] - z);
    const int block = P.cov.block;
    for (int r = lane; r <= CCSX_MAX_PASSES; r += LANES) {
        sLen[r] = (r < nreads && P.avalid[r0 + r]) ? (int)(P.base_off[r0 + r + 1] - P.base_off[r0 + r]) : -1;
        sMiss[r] = 0; sHist[r] = 0;
    }
    __syncthreads();
    int cmax = 0, rsum = 0, key = 0x7fffffff;               // key = clean_w << 16 | w: its minimum is the FIRST window among those with the fewest clean passes
    for (int w = lane; w < nw; w += LANES) {
        int ws = wb[w] - CCSX_WIN_OVERHANG; if (ws < 0) ws = 0;
        int we = wb[w + 1] + CCSX_WIN_OVERHANG; if (we > Ld) we = Ld;
        const int idx_ws = (w == 0) ? 0 : 2 * w - 1, idx_we = (w == nw - 1) ? 2 * nw - 1 : 2 * (w + 1);
        const int lim = (we - ws) + block;
        int reach = 0, lng = 0;
        for (int r = 0; r < nreads; ++r) {
            const int L = sLen[r];                          // (uniform over the lanes: no divergence)
            if (L < 0) continue;
            const int64_t eo = P.ent_off[r0 + r];
            const int nseg = P.ent[eo + idx_we] - P.ent[eo + idx_ws];
            if (nseg >= 0 && nseg <= L) { ++reach; lng += nseg > lim ? 1 : 0; }
            else sMiss[r] = 1;
        }
        P.cov_reach[w0 + w] = (uint8_t)reach;
        const int clean = reach - lng;
        atomicAdd(&sHist[clean], 1);
        cmax = reach > cmax ? reach : cmax; rsum += reach;
        const int k = (clean << 16) | (w & 0xffff);
        key = k < key ? k : key;
    }
    __syncthreads();
    int npa = 0, spans = 0;
    for (int r = lane; r < nfull; r += LANES) if (sLen[r] >= 0) { ++npa; spans += sMiss[r] ? 0 : 1; }
    npa = wave_reduce_add_i32(npa); spans = wave_reduce_add_i32(spans);
    cmax = wave_reduce_max_i32(cmax); rsum = wave_reduce_add_i32(rsum);
    key = -wave_reduce_max_i32(-key);
    const int thr = P.cov.drop_percent * cmax;
    int drops = 0;
    for (int c = lane; c <= CCSX_MAX_PASSES; c += LANES) if (c * 100 <= thr) drops += sHist[c];
    drops = wave_reduce_add_i32(drops);
    if (lane == 0) {
        const int clean_min = nw > 0 ? key >> 16 : 0, drop_window = nw > 0 ? key & 0xffff : 0;
        const int verdict = npa < P.opts.min_passes ? CCSX_COVERAGE_DRAFT_TOO_DIFFERENT
                          : spans < P.cov.min_spans ? CCSX_COVERAGE_INSUFFICIENT_SPANS
                          : drops >= 1 ? CCSX_COVERAGE_COVERAGE_DROPS : CCSX_COVERAGE_NONE;
        put_planes(out, n, verdict, npa, spans, cmax, clean_min, drop_window, drops, rsum, 0, 0);
        // the gate: the ZMW leaves the polish stage here, as a split heteroduplex does (k_hd_verdict) — no windows, so the rebuilt window map gives k_polish
        // nothing of it and k_stitch reports the status with an empty consensus.  Only this ZMW's words are written, after every lane has read them.
        if (verdict >= CCSX_COVERAGE_DRAFT_TOO_DIFFERENT && ((P.cov_gate >> verdict) & 1u)) {
            P.zstat[z] = CCSX_DRAFT_TOO_DIFFERENT + (verdict - CCSX_COVERAGE_DRAFT_TOO_DIFFERENT); P.nwin[z] = 0;
        }
    }
}

// k_coverage_post: one wave per ZMW on the polish stream after k_stitch.  For a ZMW that was polished (its status before the stitch is SUCCESS) it sums, over the
// windows, the passes the polish used (wmeta.y & 255: what k_stitch's ec sums) beside the passes that reached them (k_coverage's bytes), and upgrades a NONE
// verdict to READS_FAILED_POLISHING; with that verdict's gate bit the ZMW loses its consensus.
__global__ __launch_bounds__(64) void k_coverage_post(KParams P)
{
    if ((int)blockIdx.x >= P.n_zmw) return;
    const int lane = threadIdx.x;
    const int z = rfl(P.zmw_perm[blockIdx.x]);
    const size_t n = (size_t)P.n_zmw;
    int32_t *out = P.cov_zi + z;
    if (rfl(P.zstat[z]) != CCSX_SUCCESS) return;            // untested, or gated before the polish: used_sum = used_min = 0 as k_coverage left them
    const int nw = rfl(P.nwin[z]);
    const size_t w0 = (size_t)(P.wb_off[z] - z);
    int usum = 0, umin = 0x7fffffff, rsum = 0;
    for (int w = lane; w < nw; w += LANES) {
        const int used = P.wmeta[w0 + w].y & 255;
        usum += used; umin = used < umin ? used : umin; rsum += (int)P.cov_reach[w0 + w];
    }
    usum = wave_reduce_add_i32(usum); rsum = wave_reduce_add_i32(rsum);
    umin = -wave_reduce_max_i32(-umin);
    if (lane == 0) {
        out[7 * n] = rsum; out[8 * n] = usum; out[9 * n] = nw > 0 ? umin : 0;
        const int stat = P.out_status[z];
        if (out[0] == CCSX_COVERAGE_NONE && (stat == CCSX_SUCCESS || stat == CCSX_LOW_RQ) &&
            (long long)(rsum - usum) * 100 > (long long)P.cov.max_lost_percent * rsum) {
            out[0] = CCSX_COVERAGE_READS_FAILED_POLISHING;
            if ((P.cov_gate >> CCSX_COVERAGE_READS_FAILED_POLISHING) & 1u) { P.out_status[z] = CCSX_READS_FAILED_POLISHING; P.out_len[z] = 0; }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// The launch schedule of a batch: ccsx_launch_all at the end lists its stages, Schedule holds them.
namespace {

// the schedule's environment switches (ccsx_host.cpp lists them for ccsx_runtime_switches(); results never depend on them)
struct LaunchSwitches {
    bool trace;             // CCSX_TRACE: debugging aid: serialise and name every launch
    bool tb_aside;          // CCSX_TB_ASIDE=0: the trace-backs of k_align16 stay on the draft stream (A/B switch)
    long long max_blocks;   // CCSX_POLISH_MAX_BLOCKS: a test hook that forces the polish stage's per-slot grids into small pieces.  A multiple of 8 (the kernels
                            // take their windows in XCD-contiguous order), ignored unless > 8
    LaunchSwitches()
    {
        const char *aside = getenv("CCSX_TB_ASIDE"), *blocks = getenv("CCSX_POLISH_MAX_BLOCKS");
        const long long v = blocks ? atoll(blocks) : 0;
        trace = getenv("CCSX_TRACE") != nullptr;
        tb_aside = !(aside && aside[0] == '0');
        max_blocks = v > 8 ? (v & ~7ll) : (1ll << 24) - 256;
    }
};

// [0, total) in order, in pieces of at most `max`: fn(first, count)
template <typename T, typename F> inline void for_each_piece(T total, T max, F fn)
{
    for (T first = 0; first < total; first += max) fn(first, (total - first) < max ? (total - first) : max);
}

struct Schedule {
    const KParams &P;
    const ccsx_launch_queues &q;
    const LaunchSwitches &sw;
    const hipStream_t st;         // the draft stream: everything but the polish stage and what runs beside it on q.aux
    const bool second_stream;     // q.aux and its events are there
    // CCSX_RUN_POLISH (the polish seam), CCSX_RUN_HD (ccsx_hd_batch: the polish seam's first half), CCSX_RUN_TRAIN (ccsx_train_batch: the same first half): the
    // drafts are the caller's — k_draft_in instead of the generators, one alignment round whose outcome is final (P.opts.no_fallback_draft is set for such a run)
    const bool caller_drafts;
    const size_t lds_read;        // the packed read; k_poa_init: the lengths of up to 255 passes
    const char *failed = nullptr;

    Schedule(const KParams &P_, const ccsx_launch_queues &q_, int mode, const LaunchSwitches &sw_)
        : P(P_), q(q_), sw(sw_), st(q_.draft), second_stream(q_.aux && q_.ev_aux), caller_drafts(mode == CCSX_RUN_POLISH || mode == CCSX_RUN_HD || mode == CCSX_RUN_TRAIN),
          lds_read((((size_t)P_.maxL_max + 15) / 16) * 4 + 64 + 4 * (CCSX_MAX_PASSES + 1)) {}

    // ---- every status is captured: `failed` is the name of the first launch or call that failed (ccsx_api.cpp reports it)
    void check(hipError_t e, const char *name) { if (e != hipSuccess && !failed) failed = name; }
    template <typename... KA, typename... A>
    void launch(const char *name, void (*kernel)(KA...), dim3 grid, dim3 block, size_t lds, hipStream_t s, const A &... args)
    {
        hipLaunchKernelGGL(kernel, grid, block, lds, s, args...);
        check(hipGetLastError(), name);
    }
    void record(hipEvent_t e, hipStream_t s) { check(hipEventRecord(e, s), "hipEventRecord"); }
    void wait(hipStream_t s, hipEvent_t e) { check(hipStreamWaitEvent(s, e, 0), "hipStreamWaitEvent"); }
    void memset(void *p, size_t bytes, hipStream_t s) { check(hipMemsetAsync(p, 0, bytes, s), "hipMemsetAsync"); }
    void trace_sync(hipStream_t s, const char *what) const
    {
        if (!sw.trace) return;
        hipError_t e = hipStreamSynchronize(s);
        fprintf(stderr, "[ccsx] %s done: %s\n", what, hipGetErrorString(e));
    }

    // ---- the stage events (ccsx_kernels.h).  Every one of them is recorded exactly once on every path through ccsx_launch_all, in the order below, so that
    // ccsx_timings never reads an event that was not recorded or was left from an earlier batch.  A run that ends early, or has no polish stage, records the
    // events of the stages it leaves out back to back on the draft stream (close_timing): those stages then take no time.
    // Who records what: START and TABLES_DONE tables(); DRAFT_DONE draft_stage(), in its pass 0; DRAFT_STAGE_DONE, POLISH_START, POLISH_DONE and END
    // polish_stage() in a full run, close_timing alone in the draft seam; in ccsx_hd_batch close_timing the first two, hd_finder(true) POLISH_DONE,
    // ccsx_launch_all END; in ccsx_train_batch close_timing the first two, train_counts() POLISH_DONE and END.
    void stage_event(ccsx_stage_event k, hipStream_t s) { if (q.ev) record(q.ev[k], s); }
    void close_timing(ccsx_stage_event from, ccsx_stage_event to)
    {
        static const ccsx_stage_event in_time_order[] = {CCSX_EV_START, CCSX_EV_TABLES_DONE, CCSX_EV_DRAFT_DONE, CCSX_EV_DRAFT_STAGE_DONE,
                                                         CCSX_EV_POLISH_START, CCSX_EV_POLISH_DONE, CCSX_EV_END};
        bool in = false;
        for (ccsx_stage_event k : in_time_order) {
            in = in || k == from;
            if (in) stage_event(k, st);
            if (k == to) break;
        }
    }
    hipEvent_t align16_done(int c) const { return q.ev_aux[CCSX_ORD_ALIGN16_DONE_0 + (c & 1)]; }   // (launch c of k_align16 uses the events and the region c & 1)
    hipEvent_t tb_done(int c) const { return q.ev_aux[CCSX_ORD_TB_DONE_0 + (c & 1)]; }

    void tables()
    {
        stage_event(CCSX_EV_START, st);
        memset(P.ticket_poa, 256, st);   // debug / phase-profile words (CCSX_DEBUG_CHECKS, CCSX_PROFILE_PHASES builds)
        memset(P.avalid, (size_t)(P.n_reads > 0 ? P.n_reads : 1), st);   // passes beyond top_passes are never visited by a kernel
        if (P.tflag) { memset(P.tflag, (size_t)P.n_zmw * 4, st); memset(P.tlen, (size_t)P.n_zmw * 4, st); }   // all undecided
        launch("k_setup", k_setup, dim3((P.n_zmw * CCSX_NCTX + 255) / 256), dim3(256), 0, st, P);
        trace_sync(st, "k_setup");
        stage_event(CCSX_EV_TABLES_DONE, st);
    }

    // one round of draft generation over the batch, in chunks of the POA scratch's slots
    void poa_round(int pass)
    {
        int cov = pass ? 2 * P.opts.max_poa_cov : P.opts.max_poa_cov;
        if (cov > PW_MAXREADS_SPEC) cov = PW_MAXREADS_SPEC;
        if (cov > P.max_reads) cov = P.max_reads;          // no ZMW of the batch has more passes
        for_each_piece(P.n_zmw, P.poa_slots, [&](int z0, int nb) {
            // the graphs [g0, g0 + ng) on stream s: initial graph, one DP (four graphs per wave) + one threading kernel per pass of the POA, heaviest path
            auto poa_range = [&](hipStream_t s, int g0, int ng, hipEvent_t after_first_dp, hipEvent_t before_first_dp) {
                launch("k_poa_init", k_poa_init, dim3(ng), dim3(64), lds_read, s, P, z0, pass, g0);
                if (before_first_dp) wait(s, before_first_dp);
                for (int rr = 1; rr < cov && pass < 2; ++rr) {
                    launch("k_poa_dp", k_poa_dp, dim3((ng + 3) / 4), dim3(64), 0, s, P, z0, pass, rr, g0 / 4);
                    if (rr == 1 && after_first_dp) record(after_first_dp, s);
                    launch("k_poa_thread", k_poa_thread, dim3(ng), dim3(64), lds_read, s, P, z0, pass, rr, g0);
                }
                if (pass < 2) launch("k_poa_finish", k_poa_finish, dim3(ng), dim3(64), 0, s, P, z0, pass, g0);   // (pass 2 = last resort: k_poa_init writes the draft itself)
            };
            // Pass 0 of a large batch runs as TWO half-batches on two streams, the second one a DP behind the first: k_poa_dp saturates the VALU and k_poa_thread
            // waits for HBM, their registers and LDS fit one SIMD together (94 + 64 VGPRs), so the threading of one half runs under the DP of the other.
            if (second_stream && pass == 0 && cov > 1 && nb >= 4096) {
                const int ha = ((nb / 2) + 3) & ~3;
                record(q.ev_aux[CCSX_ORD_POA_FORK], st);
                wait(q.aux, q.ev_aux[CCSX_ORD_POA_FORK]);
                poa_range(st, 0, ha, q.ev_aux[CCSX_ORD_FIRST_DP_DONE], nullptr);
                poa_range(q.aux, ha, nb - ha, nullptr, q.ev_aux[CCSX_ORD_FIRST_DP_DONE]);
                record(q.ev_aux[CCSX_ORD_POA_JOIN], q.aux);
                wait(st, q.ev_aux[CCSX_ORD_POA_JOIN]);
            } else poa_range(st, 0, nb, nullptr, nullptr);
        });
    }

    // alignment cascade: four passes per wave in 16-row bands, then the 64-row retry of the few that failed there, then the split alignment
    void align_cascade(int pass)
    {
        memset(P.align_retry, 64, st);
        const size_t lds16 = 4 * (CH16 / 16 + 3) * sizeof(uint32_t);
        // The trace-back of a launch runs on the second stream: beside the NEXT launch of k_align16 (a batch whose quads take several launches has two
        // scratch regions, launch c uses region c & 1 and waits for the trace-back of launch c - 2) and, the last one, beside the 64-row retry and the split
        // alignment — those read the retry list the 16-row kernel wrote, not the entries the trace-back writes, and their scratch lies behind the stored
        // moves.  The cascade ends with the waits for all of them.  (A trace-back is a long dependent walk of few waves: 42 % of k_align16's time on the 3-50-pass mix.)
        const bool aside = sw.tb_aside && second_stream && pass == 0 && P.n_quads >= 4096;
        int launches = 0;
        for_each_piece(P.n_quads, P.align16_slots, [&](int qb, int nb) {
            const int c = launches++;
            const int region = P.align16_regions > 1 ? (c & 1) : 0;
            if (aside && c >= 2) wait(st, tb_done(c));                                  // the region's last reader
            if (aside && c >= 1 && P.align16_regions <= 1) wait(st, tb_done(c - 1));   // (one region: in sequence)
            launch("k_align16", k_align16, dim3(nb), dim3(64), lds16, st, P, qb, pass, region);
            if (aside) { record(align16_done(c), st); wait(q.aux, align16_done(c)); }
            launch("k_align16_tb", k_align16_tb, dim3((4 * nb + 63) / 64), dim3(64), 0, aside ? q.aux : st, P, qb, nb, region);   // one lane per pass: entry rows / dirty masks from the stored moves
            if (aside) record(tb_done(c), q.aux);
        });
        launch("k_align", k_align, dim3(P.align_slots < 1 ? 1 : (P.align_slots > 4096 ? 4096 : P.align_slots)), dim3(64), lds_read, st, P, pass);
        trace_sync(st, "k_align");
        if (P.align_slots >= 2)                            // the split alignment uses two scratch slots per workgroup
            launch("k_rescue", k_rescue, dim3(P.align_slots / 2 > 2048 ? 2048 : P.align_slots / 2), dim3(64), lds_read, st, P, pass);
        if (aside) for (int c = launches > 2 ? launches - 2 : 0; c < launches; ++c) wait(st, tb_done(c));   // (the trace-backs run in order on one stream: the last one per region)
    }

    // pass 0 = the draft; passes 1, 2 = the fallback drafts of the ZMWs k_post marked (their waves run, all others leave at once: a further round of launches
    // costs microseconds unless something failed)
    // The passes flagged CCSX_PASS_STRAND_UNKNOWN are oriented before anything reads a pass's strand bit (a batch without one: nothing is launched).
    void orient()
    {
        if (!P.orient_flags) return;
        launch("k_orient", k_orient, dim3(P.orient_wgs), dim3(CCSX_ORIENT_THREADS), 0, st, P);
        trace_sync(st, "k_orient");
    }

    void draft_stage()
    {
        orient();
        if (caller_drafts) launch("k_draft_in", k_draft_in, dim3(P.n_zmw), dim3(64), 0, st, P);
        const int passes = (P.opts.no_fallback_draft || caller_drafts) ? 1 : 3;
        for (int pass = 0; pass < passes; ++pass) {
            if (!caller_drafts) poa_round(pass);
            trace_sync(st, "k_poa");
            if (P.tflag)                                    // tandem repeats: the ZMWs whose deciding draft this pass makes
                launch("k_sdust", k_sdust, dim3(P.n_zmw), dim3(64), (size_t)CCSX_SDUST_TABLE_BYTES + (size_t)P.sdust_words * 4, st, P, pass);
            if (pass == 0) stage_event(CCSX_EV_DRAFT_DONE, st);
            align_cascade(pass);
            launch("k_post", k_post, dim3((P.n_zmw + 255) / 256), dim3(256), 0, st, P, pass);
        }
    }

    // the batch's windows in compact order: the polish stage's grid map
    void window_map()
    {
        launch("k_wmap", k_wmap, dim3(1), dim3(1024), 0, st, P);
        launch("k_wmap_fill", k_wmap_fill, dim3((P.n_zmw + 3) / 4), dim3(256), 0, st, P);
    }

    // The draft screens a fused run was asked for (the requests of ccsx_submit_control / ccsx_consensus_control and their narrower forms): adapter palindromes,
    // the adapter screen, the control screen.  On the draft stream, on the final drafts and statuses k_polish is given; each writes its report only.
    void draft_screens()
    {
        const struct { const void *report; void (*kernel)(KParams); int threads; size_t lds; const char *name; } screens[] = {
            {P.fold_zi, k_fold, CCSX_FOLD_THREADS, (size_t)P.fold_bins * 4, "k_fold"},
            {P.adapt_zi, k_adapter, CCSX_ADAPTER_THREADS, (size_t)P.adapt_words * 8, "k_adapter"},
            {P.ctl_zi, k_control, CCSX_CONTROL_THREADS, (size_t)P.ctl_bins * 8, "k_control"}};
        for (const auto &s : screens) if (s.report) {
            launch(s.name, s.kernel, dim3(P.n_zmw), dim3(s.threads), s.lds, st, P);
            trace_sync(st, s.name);
        }
    }

    // The coverage screen's first kernel (a fused run with a ccsx_coverage_request): on the draft stream after the draft screens, so that they see the statuses
    // they see without it.  It reads what k_polish is given — final draft, window bounds, status after the cascade, entry rows — and no shared scratch.
    void coverage()
    {
        launch("k_coverage", k_coverage, dim3(P.n_zmw), dim3(64), 0, st, P);
        trace_sync(st, "k_coverage");
    }

    // The heteroduplex finder's three kernels on the draft stream.  Its inputs are what k_polish gets: the final draft, its window bounds, the status after the
    // cascade and the entry rows (k_polish trims large insertions in LDS only).  It reads no shared POA / alignment scratch.
    // in_place_of_polish (ccsx_hd_batch): the verdict is what the run has for a stitch, CCSX_EV_POLISH_DONE is recorded before it.
    void hd_finder(bool in_place_of_polish)
    {
        const long long groups = (P.total_wslots + HD_WG_WIN - 1) / HD_WG_WIN;   // (the grid covers the slot capacity, the map only the windows there are)
        launch("k_hd_pile", k_hd_pile, dim3((unsigned)(groups > 0 ? groups : 1)), dim3(64), 0, st, P);
        launch("k_hd_indel", k_hd_indel, dim3(P.n_zmw), dim3(64), 0, st, P);
        if (in_place_of_polish) stage_event(CCSX_EV_POLISH_DONE, st);
        launch("k_hd_verdict", k_hd_verdict, dim3(P.n_zmw), dim3(64), 0, st, P);
    }

    // The training counts in place of the polish stage (ccsx_train_batch), on the draft stream: the slot's count buffers zeroed, then k_train (ccsx_train.hip) over
    // the window slots, in the polish stage's launch pieces.  Nothing follows it: POLISH_DONE and END are recorded back to back.
    void train_counts()
    {
        const char *what = ccsx_train_launch(P, st, sw.max_blocks);
        if (what && !failed) failed = what;
        trace_sync(st, "k_train");
        stage_event(CCSX_EV_POLISH_DONE, st);
        stage_event(CCSX_EV_END, st);
    }

    // Two-stage queue of docs/img/ccs-impl.png ("Draft Stage" -> queue -> "Polish Stage"): the draft stage (tables, POA, alignment cascade, accounting, screens)
    // is enqueued on the draft stream, the polish stage (polish, kinetics, stitch) on the polish stream, which waits for the draft stage's last kernel through
    // CCSX_EV_DRAFT_STAGE_DONE.  With two different streams the draft stage of batch k+1 runs UNDER the polish stage of batch k (the register-only one-wave POA
    // and the LDS-bound polish workgroups share the SIMDs); the shared POA / alignment scratch is touched by the draft stage only, so the draft stream alone
    // orders its users.  The same stream for both: serial stages.
    void polish_stage()
    {
        const hipStream_t sp = q.polish;
        if (q.ev) {
            record(q.ev[CCSX_EV_DRAFT_STAGE_DONE], st);
            if (sp != st) wait(sp, q.ev[CCSX_EV_DRAFT_STAGE_DONE]);
            record(q.ev[CCSX_EV_POLISH_START], sp);         // the polish stage starts here (after the queue between the stages)
        } else if (sp != st && !failed) failed = "two streams need events";
        // One workgroup per window slot.  A grid may not exceed 2^32 threads in all: 256 threads x 16.7 M slots — 8192 ZMWs of 30 passes x 20 kb have 10.8 M, and a
        // larger batch would silently lose its tail (round 4 met exactly this with a 512-thread experiment: 75 % of the ZMWs "failed").  The slots are therefore
        // launched in pieces of at most 2^24 - 256 workgroups (just under the limit, so that a 16384-ZMW batch of 10 kb inserts — 8.5 M slots of capacity — is ONE launch:
        // the profile's per-launch average and bench.py's per-batch duration then describe the same thing; LaunchSwitches::max_blocks forces small pieces).
        for_each_piece(P.total_wslots, sw.max_blocks, [&](long long s0, long long nb) {
            launch("k_polish", k_polish_t<PW_THREADS, PW_MINWAVES, PW_CHUNK_READS>, dim3(((unsigned)nb + 7u) & ~7u), dim3(PW_THREADS),
                   (size_t)P.pw_obs_bytes + (size_t)P.pw_gb_floats * 4, sp, P, (int)s0);
        });
        trace_sync(sp, "k_polish");
        if (P.opts.hifi_kinetics || P.wpile) {             // one alignment per (pass, window) segment feeds kinetics, the pileup summary or both
            const bool kin = P.opts.hifi_kinetics != 0, pile = P.wpile != nullptr;
            const auto kfn = kin ? (pile ? k_kinetics_t<1, 1> : k_kinetics_t<1, 0>) : k_kinetics_t<0, 1>;
            const char *const name = kin ? (pile ? "k_kinetics_pile" : "k_kinetics") : "k_pileup";
            for_each_piece(P.total_wslots, sw.max_blocks, [&](long long s0, long long nb) {
                launch(name, kfn, dim3(((unsigned)nb + 7u) & ~7u), dim3(256), 0, sp, P, (int)s0);
            });
            trace_sync(sp, "k_kinetics");
        }
        stage_event(CCSX_EV_POLISH_DONE, sp);
        launch("k_stitch", k_stitch, dim3(P.n_zmw), dim3(64), 0, sp, P);
        if (P.out_pile) launch("k_pile_stitch", k_pile_stitch, dim3(P.n_zmw), dim3(64), 0, sp, P);
        if (P.cov_zi) launch("k_coverage_post", k_coverage_post, dim3(P.n_zmw), dim3(64), 0, sp, P);   // the coverage screen's post-polish planes
        if (P.ho_cells) {                                  // the polisher hand-off, on the final lengths and quals (a batch with a ccsx_handoff_request only)
            launch("k_tile_select", k_tile_select, dim3(P.n_zmw), dim3(64), 0, sp, P);
            trace_sync(sp, "k_tile_select");
            launch("k_tile_scan", k_tile_scan, dim3((P.n_zmw + CCSX_TILE_SCAN_ZMWS - 1) / CCSX_TILE_SCAN_ZMWS), dim3(256), 0, sp, P);
            trace_sync(sp, "k_tile_scan");
            for_each_piece(P.total_wslots, sw.max_blocks, [&](long long s0, long long nb) {
                launch("k_tile_rows", k_tile_rows, dim3(((unsigned)nb + 7u) & ~7u), dim3(256), 0, sp, P, (int)s0);
            });
            trace_sync(sp, "k_tile_rows");
        }
        if (P.bc.rep && !failed) {                         // barcode calls on the final consensus (a batch with a ccsx_barcode_request only)
            failed = ccsx_barcode_launch(P.bc, sp);
            trace_sync(sp, "k_barcode");
        }
        if (P.sg.rep && !failed) {                         // segmentation of the final consensus (a batch with a ccsx_segment_request only)
            failed = ccsx_segment_launch(P.sg, sp);
            trace_sync(sp, "k_segment");
        }
        if (P.cd.rep && !failed) {                         // full-length cDNA reads of the final consensus (a batch with a ccsx_cdna_request only)
            failed = ccsx_cdna_launch(P.cd, sp);
            trace_sync(sp, "k_cdna");
        }
        if (P.rep.rep && !failed) {                        // representative reads into the result planes (a batch with a ccsx_represent_request only)
            failed = ccsx_represent_launch(P.rep, sp);
            trace_sync(sp, "k_represent");
        }
        stage_event(CCSX_EV_END, sp);
    }
};

}  // namespace

// The run modes share one schedule and leave it at four places (ccsx_orient_batch's runs its first kernel only).  No stage synchronises with the host.  No stage synchronises with the host.
const char *ccsx_launch_all(const KParams &P, const ccsx_launch_queues &q, int mode)
{
    static const LaunchSwitches switches;
    Schedule s(P, q, mode, switches);
    if (mode == CCSX_RUN_ORIENT) {                          // ccsx_orient_batch: k_orient alone, every stage event back to back behind it
        s.orient();
        s.close_timing(CCSX_EV_START, CCSX_EV_END);
        return s.failed;
    }
    s.tables();
    s.draft_stage();
    if (mode == CCSX_RUN_DRAFT) {                           // the draft seam ends here: drafts, window bounds, alignments and statuses are final
        s.close_timing(CCSX_EV_DRAFT_STAGE_DONE, CCSX_EV_END);
        return s.failed;
    }
    s.window_map();
    if (mode == CCSX_RUN_FUSED) {
        s.draft_screens();
        // The coverage screen before the finder (a call may carry both: ccsx_submit_hd_requests): k_coverage sees every status as the cascade left it, so its
        // report does not depend on the finder; a ZMW its gate takes is not SUCCESS any more and the finder leaves it UNTESTED (DESIGN.md §2 "In the fused path").
        if (P.cov_zi) {
            s.coverage();
            if (P.cov_gate & CCSX_COVERAGE_PRE_GATE) s.window_map();   // the gated ZMWs have no windows now: the finder's and the polish stage's map without them
        }
        if (P.hd_zi) {
            // the heteroduplex finder in the fused path (ccsx_submit_hd / ccsx_consensus_hd): on the draft stream, so that it belongs to this batch's draft
            // stage and runs under the previous batch's polish stage
            s.hd_finder(false);
            if (P.hd_split) s.window_map();                 // the split ZMWs have no windows now: the polish stage's map without them
            s.trace_sync(q.draft, "k_hd");
        }
    }
    if (mode == CCSX_RUN_HD) {                              // the heteroduplex finder instead of the polish stage, on the same stream
        s.close_timing(CCSX_EV_DRAFT_STAGE_DONE, CCSX_EV_POLISH_START);
        s.hd_finder(true);
        s.trace_sync(q.draft, "k_hd");
        s.stage_event(CCSX_EV_END, q.draft);
        return s.failed;
    }
    if (mode == CCSX_RUN_TRAIN) {                           // the training counts instead of the polish stage, on the same stream
        s.close_timing(CCSX_EV_DRAFT_STAGE_DONE, CCSX_EV_POLISH_START);
        s.train_counts();
        return s.failed;
    }
    s.polish_stage();
    return s.failed;
}

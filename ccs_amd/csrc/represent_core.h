// represent_core.h — the representative rule for the host and the device (DESIGN.md §2 "Representative rule"): the class of a ZMW, the set its representative
// pass is taken from, and the order that set is ranked in.  ccsx_represent_host (ccsx_represent_api.cpp) and k_represent (ccsx_represent.hip) are built from
// these and from nothing else of the rule.  Integers only.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "ccsx.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CCSX_RP_HD __host__ __device__ __forceinline__
#else
#define CCSX_RP_HD inline
#endif

#define CCSX_REPRESENT_QV 10   // qual / raw_qv of every base of an unpolished representative, draft or subread (a decision: DESIGN.md §2)

// passes of a ZMW the engine looks at: the first of them, up to opts.top_passes (as ccsx_top_passes: <= 0 and anything above CCSX_MAX_PASSES mean CCSX_MAX_PASSES)
CCSX_RP_HD int ccsx_rp_nall(int n_passes, int top_passes)
{
    const int top = (top_passes <= 0 || top_passes > CCSX_MAX_PASSES) ? CCSX_MAX_PASSES : top_passes;
    return n_passes < top ? n_passes : top;
}

// The class: the first of the four that holds.  st: the final status; nall: ccsx_rp_nall; Ld: the final draft's length; slot: the ZMW's capacity in the result
// planes (1.25 x its longest pass + 64: any pass fits).  A draft that does not fit its slot is never truncated: class NONE.
CCSX_RP_HD int ccsx_rp_class(int st, int nall, int Ld, int64_t slot, int subread_fallback)
{
    if (st == CCSX_SUCCESS || st == CCSX_LOW_RQ) return CCSX_REPRESENT_POLISHED;
    if (nall <= 0 || st == CCSX_TOO_SHORT || st == CCSX_TOO_LONG) return CCSX_REPRESENT_NONE;
    if (Ld > 0 && st != CCSX_TOO_FEW_PASSES && !subread_fallback) return Ld <= slot ? CCSX_REPRESENT_DRAFT : CCSX_REPRESENT_NONE;
    return CCSX_REPRESENT_SUBREAD;
}

// set C of a SUBREAD ZMW: its full-length passes (flag bit 1 clear) when it has one, else all nall passes
CCSX_RP_HD int ccsx_rp_member(int flag, int nfull) { return nfull < 1 || !(flag & 2); }

// (length, index-within-ZMW) order: pass q of length lq comes before pass i of length li.  The representative is the member of C that exactly |C| / 2 members
// come before — the rank k_poa_init's median uses
CCSX_RP_HD int ccsx_rp_before(int lq, int q, int li, int i) { return lq < li || (lq == li && q < i); }

// the report of n ZMWs on the device: [2][n] int32, class then pass
#define CCSX_RP_PLANES 2

// what k_represent is given (ccsx_represent.hip): the slot's inputs, final draft and result planes as they stand after k_stitch
struct RepresentParams {
    int32_t n;
    int32_t top_passes, subread_fallback;
    const int32_t *read_off;             // [n + 1]
    const int64_t *base_off;             // [R + 1]
    const uint8_t *bases, *pw, *ipd, *flags;   // pw / ipd: read only when out_kin is set
    const int64_t *seq_off;              // [n + 1] the capacity layout of draft and result planes: slot of z = seq_off[z + 1] - seq_off[z]
    const uint8_t *draft;                // final drafts at seq_off
    const int32_t *draft_len;            // [n]
    const int32_t *status;               // [n] final status (k_stitch's): read, never written
    int32_t *out_len;                    // [n]
    float *out_rq, *out_ec;              // [n]
    uint8_t *out_seq, *out_qual;         // planes at seq_off
    float *out_raw;                      // NULL: no such plane
    uint8_t *out_kin;                    // fi plane, fp = out_kin + kin_plane; NULL: no kinetics asked for
    long long kin_plane;
    int32_t *rep;                        // [CCSX_RP_PLANES][n]
};
#define CCSX_REPRESENT_THREADS 256

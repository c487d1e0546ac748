// ccsx_represent.hip — representative reads (DESIGN.md §2 "Representative rule", §4 "k_represent").  The rule itself is represent_core.h; this file is its layout
// on the device.  Integers only; no result depends on the launch geometry, on the order of the lanes or on scheduling: the only atomics are LDS counts.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ccsx.h"
#include "represent_core.h"

namespace {

constexpr int NT = CCSX_REPRESENT_THREADS;
static_assert(CCSX_MAX_PASSES <= NT, "k_represent ranks one pass per thread");

// L bytes from src to dst over the workgroup.  The destination decides the shape: single bytes up to its first 16-byte boundary, then 16 bytes per lane and step
// (consecutive lanes, consecutive 16-byte words: whole cache lines per wave), single bytes behind the last whole word.  The source of a draft sits at the same
// offset of its plane as the destination, a pass's wherever base_off put it: its 16 bytes are loaded as the hardware's unaligned access allows.
// MASK: only the low two bits of a base byte count.
template <bool MASK> __device__ __forceinline__ void copy_bytes(uint8_t *dst, const uint8_t *src, int L, int tid)
{
    const int lead = (int)((16u - (unsigned)((uintptr_t)dst & 15u)) & 15u), head = lead < L ? lead : L;
    if (tid < head) dst[tid] = MASK ? (uint8_t)(src[tid] & 3) : src[tid];
    const int words = (L - head) >> 4;
    for (int k = tid; k < words; k += NT) {
        uint4 v;
        __builtin_memcpy(&v, src + head + 16 * (size_t)k, 16);
        if (MASK) { v.x &= 0x03030303u; v.y &= 0x03030303u; v.z &= 0x03030303u; v.w &= 0x03030303u; }
        *reinterpret_cast<uint4 *>(dst + head + 16 * (size_t)k) = v;
    }
    const int done = head + (words << 4);
    if (tid < L - done) dst[done + tid] = MASK ? (uint8_t)(src[done + tid] & 3) : src[done + tid];
}

// L elements of dst set to v, in the same shape (T: uint8_t with V = its byte in every lane of a word, or float with V = its bits)
template <typename T> __device__ __forceinline__ void fill_wide(T *dst, T v, uint32_t word, int L, int tid)
{
    constexpr int PER = 16 / (int)sizeof(T);
    const int lead = (int)(((16u - (unsigned)((uintptr_t)dst & 15u)) & 15u) / sizeof(T)), head = lead < L ? lead : L;
    if (tid < head) dst[tid] = v;
    const int words = (L - head) / PER;
    for (int k = tid; k < words; k += NT) *reinterpret_cast<uint4 *>(dst + head + PER * (size_t)k) = make_uint4(word, word, word, word);
    const int done = head + words * PER;
    if (tid < L - done) dst[done + tid] = v;
}

// ---- k_represent: one 256-thread workgroup per ZMW.  A POLISHED ZMW leaves after reading its status, a NONE one after its pass count and draft length.  For a
// SUBREAD ZMW thread q holds pass q (at most CCSX_MAX_PASSES = 255 after the top_passes cut): the full-length passes are counted by ballot, the lengths of the
// members of C go to LDS (-1: not a member), every member counts the members before it in (length, index) order — nall broadcast reads of LDS per lane, all
// lanes at once — and the one with |C| / 2 before it is the representative.  Then the copy and the fills over the whole workgroup (copy_bytes / fill_wide).
// Reads: status, read_off, base_off, flags, draft_len, and the chosen source's bytes.  Writes: of a DRAFT / SUBREAD ZMW seq_len, rq, ec and the first seq_len
// elements of its slot in seq, qual, raw_qv (and fi, fp of a SUBREAD ZMW when asked); of every ZMW its two report words.  Nothing else.
__global__ __launch_bounds__(NT) void k_represent(RepresentParams R)
{
    __shared__ int sLen[NT];
    __shared__ int sFull, sMembers, sPick;
    const int tid = threadIdx.x, z = blockIdx.x;
    if (z >= R.n) return;
    int32_t *const rcls = R.rep, *const rpass = R.rep + R.n;
    const int st = R.status[z];
    if (st == CCSX_SUCCESS || st == CCSX_LOW_RQ) {
        if (tid == 0) { rcls[z] = CCSX_REPRESENT_POLISHED; rpass[z] = -1; }
        return;
    }
    const int r0 = R.read_off[z], nall = ccsx_rp_nall(R.read_off[z + 1] - r0, R.top_passes);
    const int64_t so = R.seq_off[z], slot = R.seq_off[z + 1] - so;
    const int Ld = R.draft_len[z];
    const int cls = ccsx_rp_class(st, nall, Ld, slot, R.subread_fallback);
    if (cls == CCSX_REPRESENT_POLISHED || cls == CCSX_REPRESENT_NONE) {
        if (tid == 0) { rcls[z] = cls; rpass[z] = -1; }
        return;
    }
    const uint8_t *src = R.draft + so;
    int L = Ld, pick = -1;
    int64_t bo = 0;
    if (cls == CCSX_REPRESENT_SUBREAD) {
        if (tid == 0) { sFull = 0; sMembers = 0; sPick = -1; }
        __syncthreads();
        const bool have = tid < nall;
        const int flag = have ? R.flags[r0 + tid] : 2;
        const int len = have ? (int)(R.base_off[r0 + tid + 1] - R.base_off[r0 + tid]) : 0;
        const int nf = __popcll(__ballot(have && !(flag & 2)));
        if ((tid & 63) == 0 && nf) atomicAdd(&sFull, nf);
        __syncthreads();
        const int nfull = sFull;
        const bool member = have && ccsx_rp_member(flag, nfull);
        sLen[tid] = member ? len : -1;
        const int nm = __popcll(__ballot(member));
        if ((tid & 63) == 0 && nm) atomicAdd(&sMembers, nm);
        __syncthreads();
        if (member) {
            int rank = 0;
            for (int q = 0; q < nall; ++q) { const int lq = sLen[q]; rank += (lq >= 0 && ccsx_rp_before(lq, q, len, tid)) ? 1 : 0; }
            if (rank == sMembers / 2) sPick = tid;                   // (ranks are distinct: exactly one member)
        }
        __syncthreads();
        pick = sPick;
        if (pick < 0) return;                                        // (cannot happen: nall >= 1, so C has a member of every rank below |C|)
        bo = R.base_off[r0 + pick];
        L = (int)(R.base_off[r0 + pick + 1] - bo);
        src = R.bases + bo;
        if (L > slot) return;                                        // (cannot happen: a slot is sized by the ZMW's longest pass)
    }
    copy_bytes<true>(R.out_seq + so, src, L, tid);
    fill_wide<uint8_t>(R.out_qual + so, (uint8_t)CCSX_REPRESENT_QV, 0x01010101u * CCSX_REPRESENT_QV, L, tid);
    if (R.out_raw) fill_wide<float>(R.out_raw + so, (float)CCSX_REPRESENT_QV, __float_as_uint((float)CCSX_REPRESENT_QV), L, tid);
    if (R.out_kin && pick >= 0) {
        copy_bytes<false>(R.out_kin + so, R.ipd + bo, L, tid);
        copy_bytes<false>(R.out_kin + R.kin_plane + so, R.pw + bo, L, tid);
    }
    if (tid == 0) { R.out_len[z] = L; R.out_rq[z] = -1.0f; R.out_ec[z] = 0.0f; rcls[z] = cls; rpass[z] = pick; }
}

}  // namespace

const char *ccsx_represent_launch(const RepresentParams &R, hipStream_t st)
{
    if (R.n <= 0) return nullptr;
    hipLaunchKernelGGL(k_represent, dim3((unsigned)R.n), dim3(NT), 0, st, R);
    return hipGetLastError() != hipSuccess ? "k_represent" : nullptr;
}

// ccsx_inflate.hip — k_inflate: raw DEFLATE streams (the payloads of BGZF blocks) decoded on the device, one wave64 per stream (DESIGN.md §2 "BGZF inflate").
//
// The decoder is inflate_core.h, the code the host runs with one lane; here its lane group is the wave.  The decode tables (primary table + sub-tables for the
// literal / length and the distance code) and the stream's whole output window (at most 64 KiB) live in LDS: a back-reference reads bytes that another lane of the
// same wave wrote, and within one wave LDS operations complete in program order — no global-memory visibility between lanes is relied on.  The symbol loop is
// uniform (readfirstlane keeps the bit buffer and the table entries in scalar registers); match and stored copies use all 64 lanes; the window is written to HBM
// once, at the end, in 16-byte pieces.  About 75 KiB of LDS per workgroup: two streams per CU.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ccsx.h"
#include "inflate_core.h"

#define INFL_WIN_BYTES 65536

struct infl_wave {
    static __device__ int lane() { return (int)threadIdx.x; }
    static __device__ int nlanes() { return 64; }
    static __device__ void sync() { __syncthreads(); }
    static __device__ uint64_t ballot(bool p) { return __ballot(p); }
    static __device__ uint64_t lanes_below() { return (1ull << threadIdx.x) - 1ull; }
    static __device__ uint32_t uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
};

// src / dst: the call's compressed and inflated bytes; blk[b] names stream b's ranges in them (validated on the host: inside src / dst, out_len <= 64 KiB, output
// ranges disjoint; the kernel checks the lengths again, it indexes LDS by them).  A stream that does not decode gets its status and no output bytes.
__global__ __launch_bounds__(64) void k_inflate(const uint8_t *__restrict__ src, int64_t src_len, const ccsx_deflate_block *__restrict__ blk, int32_t n_blocks,
                                                uint8_t *__restrict__ dst, int64_t dst_len, int32_t *__restrict__ status)
{
    __shared__ __attribute__((aligned(16))) uint8_t sWin[INFL_WIN_BYTES + 16];
    __shared__ ccsx_infl_tables sTab;
    const int b = (int)blockIdx.x;
    if (b >= n_blocks) return;
    const int lane = (int)threadIdx.x;
    const int64_t in_off = blk[b].in_off, out_off = blk[b].out_off;
    const int32_t in_len = blk[b].in_len, out_len = blk[b].out_len;
    if (in_len < 0 || out_len < 0 || out_len > INFL_WIN_BYTES || in_off < 0 || in_off > src_len - in_len || out_off < 0 || out_off > dst_len - out_len) {
        if (lane == 0) status[b] = CCSX_INFLATE_OUTPUT_OVERRUN;
        return;
    }
    // the window starts at the output's own misalignment, so LDS and HBM addresses of a byte agree modulo 16
    const int skew = (int)((uintptr_t)(dst + out_off) & 15);
    uint8_t *win = sWin + skew;
    const int rc = ccsx_infl_stream<infl_wave>(src + in_off, in_len, win, out_len, &sTab);
    __syncthreads();
    if (lane == 0) status[b] = rc;
    if (rc != CCSX_INFLATE_OK) return;
    uint8_t *out = dst + out_off;
    const int head = out_len < ((16 - skew) & 15) ? out_len : ((16 - skew) & 15);
    if (lane < head) out[lane] = win[lane];
    const int body = (out_len - head) & ~15;
    const uint4 *from = (const uint4 *)(win + head);              // sWin + skew + head: 16-byte aligned whenever body > 0
    uint4 *to = (uint4 *)(out + head);
    for (int i = lane; i < (body >> 4); i += 64) to[i] = from[i];
    for (int i = head + body + lane; i < out_len; i += 64) out[i] = win[i];
}

extern "C" int ccsx_launch_inflate(hipStream_t stream, const uint8_t *src, int64_t src_len, const ccsx_deflate_block *blk, int32_t n_blocks, uint8_t *dst,
                                   int64_t dst_len, int32_t *status)
{
    if (n_blocks <= 0) return 0;
    hipLaunchKernelGGL(k_inflate, dim3((unsigned)n_blocks), dim3(64), 0, stream, src, src_len, blk, n_blocks, dst, dst_len, status);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

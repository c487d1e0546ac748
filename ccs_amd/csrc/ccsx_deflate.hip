// ccsx_deflate.hip — k_deflate: spans of at most 64 KiB encoded as raw DEFLATE streams (the payloads of BGZF blocks) on the device, one workgroup of 256 lanes per
// span (DESIGN.md §2 "BGZF deflate").
//
// The encoder is deflate_core.h, the code the host runs with one lane; here its lane group is the workgroup.  The span's input (64 KiB) and the encoder's work
// area (hash table, the matches of one sub-block of 8192 positions, the sub-block's staged bits, counts and codes: about 83 KiB) live in LDS, about 147 KiB per
// workgroup: one span per CU.  Match search, counts, token bit lengths and bit placement run on all lanes (LDS integer atomics: max for the hash table, add for the
// counts, or for the bits, all order-free); the greedy parse, the minimum-redundancy tree and the block header are one lane's work between two barriers.  A
// sub-block's bytes go from the staging area to HBM as they are finished; the stored fallback is decided here, at the end of the span.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ccsx.h"
#include "deflate_core.h"

#define DEFL_THREADS 256

struct defl_group {
    static __device__ int lane() { return (int)threadIdx.x; }
    static __device__ int nlanes() { return DEFL_THREADS; }
    static __device__ void sync() { __syncthreads(); }
    static __device__ void atomic_add(uint32_t *p, uint32_t v) { atomicAdd(p, v); }
    static __device__ void atomic_or(uint32_t *p, uint32_t v) { atomicOr(p, v); }
    static __device__ void atomic_xor(uint32_t *p, uint32_t v) { atomicXor(p, v); }
    static __device__ void atomic_max(uint32_t *p, uint32_t v) { atomicMax(p, v); }
};

// src / dst: the call's plain and compressed bytes; span[s] names span s's ranges in them (validated on the host: inside src / dst, in_len <= 64 KiB, output
// ranges disjoint; the kernel checks them again, it indexes LDS by in_len).  A span whose stream does not fit its out_cap gets OUTPUT_FULL and out_len 0.
__global__ __launch_bounds__(DEFL_THREADS) void k_deflate(const uint8_t *__restrict__ src, int64_t src_len, const ccsx_deflate_span *__restrict__ span, int32_t n_spans,
                                                           uint8_t *__restrict__ dst, int64_t dst_len, int32_t *__restrict__ out_len, uint32_t *__restrict__ crc,
                                                           int32_t *__restrict__ status)
{
    __shared__ __attribute__((aligned(16))) uint8_t sIn[CCSX_DEFL_MAX_IN + 16];
    __shared__ ccsx_defl_work sWork;
    const int s = (int)blockIdx.x;
    if (s >= n_spans) return;
    const int lane = (int)threadIdx.x;
    const int64_t in_off = span[s].in_off, out_off = span[s].out_off;
    const int32_t in_len = span[s].in_len, out_cap = span[s].out_cap;
    if (in_len < 0 || in_len > CCSX_DEFL_MAX_IN || out_cap < 0 || in_off < 0 || in_off > src_len - in_len || out_off < 0 || out_off > dst_len - out_cap) {
        if (lane == 0) { status[s] = CCSX_DEFLATE_OUTPUT_FULL; out_len[s] = 0; crc[s] = 0; }
        return;
    }
    // the input starts at its own misalignment, so LDS and HBM addresses of a byte agree modulo 16
    const uint8_t *from = src + in_off;
    const int skew = (int)((uintptr_t)from & 15);
    uint8_t *in = sIn + skew;
    const int head = in_len < ((16 - skew) & 15) ? in_len : ((16 - skew) & 15);
    if (lane < head) in[lane] = from[lane];
    const int body = (in_len - head) & ~15;
    const uint4 *g = (const uint4 *)(from + head);
    uint4 *l = (uint4 *)(in + head);                              // sIn + skew + head: 16-byte aligned whenever body > 0
    for (int i = lane; i < (body >> 4); i += DEFL_THREADS) l[i] = g[i];
    for (int i = head + body + lane; i < in_len; i += DEFL_THREADS) in[i] = from[i];
    __syncthreads();
    int32_t n_out = 0;
    uint32_t c = 0;
    const int rc = ccsx_defl_span<defl_group>(in, in_len, dst + out_off, out_cap, &sWork, &n_out, &c);
    if (lane == 0) { status[s] = rc; out_len[s] = n_out; crc[s] = c; }
}

extern "C" int ccsx_launch_deflate(hipStream_t stream, const uint8_t *src, int64_t src_len, const ccsx_deflate_span *span, int32_t n_spans, uint8_t *dst,
                                   int64_t dst_len, int32_t *out_len, uint32_t *crc, int32_t *status)
{
    if (n_spans <= 0) return 0;
    hipLaunchKernelGGL(k_deflate, dim3((unsigned)n_spans), dim3(DEFL_THREADS), 0, stream, src, src_len, span, n_spans, dst, dst_len, out_len, crc, status);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

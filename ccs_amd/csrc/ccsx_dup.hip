// ccsx_dup.hip — duplicate reads (DESIGN.md §2 "Duplicate rule", §4 "k_dup_*").  The rule itself is dup_core.h; this file is its layout on the device: the
// signatures (k_dup_sign), the keys (k_dup_keys), a radix sort of (key, read) pairs (rocPRIM's: plumbing, not the rule), the buckets (k_dup_buckets) and the sets
// of every bucket of two or more (k_dup_verify).  Integers only.  No result depends on the launch geometry, on the order of the lanes, of the work list or of the
// unions: the atomics are a counter whose order is not read, LDS minima, maxima and sums, and compare-and-swap hooks whose fixed point is the same in any order.
#include <cstring>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#include <stdint.h>

#include "ccsx.h"
#include "dup_core.h"
#include "wave_ops.h"

namespace {

constexpr int NT = CCSX_DUP_VERIFY_THREADS;
constexpr int MAXB = CCSX_DUP_MAX_BUCKET;
static_assert(MAXB % NT == 0, "k_dup_verify keeps MAXB / NT roots a thread");
constexpr int NONE = 0x7fffffff;

// the minimum of unsigned v over the wave, in every lane (the identity is 0xffffffff)
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) { return (uint32_t)~wave_reduce_max_i32(~(int)(v ^ 0x80000000u)) ^ 0x80000000u; }

// ---- k_dup_sign: one wave per read, four reads a workgroup.  Lane j holds base j of both windows (end 1 already reverse-complemented); two ballots per end give
// the window's low and high bits, which every lane spreads into the packed words, so the k-mers are shared without LDS: lane j hashes the k-mer at j of both ends
// and a wave reduction takes the minima.  The 48 bytes leave as three 16-byte stores, lanes 0 .. 2.
// Reads: seq[seq_off[z] + (0 .. L - 1)], and only when L >= window; writes: the read's own signature.
__global__ __launch_bounds__(CCSX_DUP_SIGN_THREADS) void k_dup_sign(DupSignParams S)
{
    const int lane = threadIdx.x & 63, z = blockIdx.x * (CCSX_DUP_SIGN_THREADS / 64) + (threadIdx.x >> 6);
    if (z >= S.n) return;                                            // (wave-uniform; the kernel has no barrier)
    const int L = S.seq_len[z], W = S.opts.window, k = S.opts.kmer;
    DupWin e0{0ull, 0ull}, e1{0ull, 0ull};                           // untested: everything but len 0
    uint32_t m0 = 0u, m1 = 0u;
    if (L >= W) {
        const uint8_t *c = S.seq + S.seq_off[z];
        const bool in = lane < W;
        const int b0 = in ? ccsx_bc_base(c, L, 0, lane) : 0, b1 = in ? ccsx_bc_base(c, L, 1, lane) : 0;
        e0 = ccsx_dup_win_of_bits(__ballot(b0 & 1), __ballot(b0 & 2)); e1 = ccsx_dup_win_of_bits(__ballot(b1 & 1), __ballot(b1 & 2));
        const bool has = lane + k <= W;
        m0 = wave_min_u32(has ? ccsx_dup_hash32(ccsx_dup_kmer(e0, lane, k)) : 0xffffffffu);
        m1 = wave_min_u32(has ? ccsx_dup_hash32(ccsx_dup_kmer(e1, lane, k)) : 0xffffffffu);
    }
    if (lane < 3) {                                                  // ccsx_dup_sig: end[0], end[1], then mini[0], mini[1], len, window
        const unsigned long long len = (unsigned long long)(uint32_t)(L > 0 ? L : 0), win = L >= W ? (unsigned long long)(uint32_t)W : 0ull;
        const ulonglong2 v = lane == 0 ? make_ulonglong2(e0.w0, e0.w1) : lane == 1 ? make_ulonglong2(e1.w0, e1.w1)
                                                                       : make_ulonglong2((unsigned long long)m0 | ((unsigned long long)m1 << 32), len | (win << 32));
        reinterpret_cast<ulonglong2 *>(S.sig + z)[lane] = v;
    }
}

// the third 16 bytes of a signature: mini[0], mini[1], len, window
struct SigTail { uint32_t mini[2]; int32_t len, window; };
__device__ __forceinline__ SigTail sig_tail(const ccsx_dup_sig *s)
{
    const ulonglong2 v = reinterpret_cast<const ulonglong2 *>(s)[2];
    return {{(uint32_t)v.x, (uint32_t)(v.x >> 32)}, (int32_t)(uint32_t)v.y, (int32_t)(uint32_t)(v.y >> 32)};
}

// ---- k_dup_keys: one thread per read: its key and its index, the sort's input; thread 0 empties the work list
__global__ __launch_bounds__(256) void k_dup_keys(DupClusterParams P)
{
    const int z = blockIdx.x * 256 + threadIdx.x;
    if (z == 0) P.list[0] = 0;
    if (z >= P.n) return;
    const SigTail t = sig_tail(P.sig + z);
    ccsx_dup_sig s{};
    s.mini[0] = t.mini[0]; s.mini[1] = t.mini[1]; s.window = t.window;
    P.key[0][z] = ccsx_dup_key(s);
    P.idx[0][z] = (uint32_t)z;
}

// ---- k_dup_buckets: one thread per sorted position.  An untested read reports itself.  The first position of a bucket (its key differs from the one before)
// reports a bucket of one directly and appends any other to the work list; the list's order is the order of the atomic additions and nothing reads it as an order
__global__ __launch_bounds__(256) void k_dup_buckets(DupClusterParams P)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P.n) return;
    const DupOut out = ccsx_dup_out(P.rep, (size_t)P.n);
    const unsigned long long key = P.key[1][p];
    const int z = (int)P.idx[1][p];
    if (key == CCSX_DUP_KEY_UNTESTED) { ccsx_dup_put_alone(out, z, CCSX_DUP_UNTESTED); return; }
    if (p > 0 && P.key[1][p - 1] == key) return;
    if (p + 1 >= P.n || P.key[1][p + 1] != key) { ccsx_dup_put_alone(out, z, CCSX_DUP_TESTED); return; }
    P.list[1 + atomicAdd(&P.list[0], 1)] = p;
}

// the root of x, halving the path on the way: a member that is no root is given its grandparent.  Only a root is ever hooked (uf_unite's compare-and-swap
// expects par[hi] == hi) and a member that has a parent never becomes a root again, so these plain stores and the hooks never meet in one word; every value
// a word takes is an ancestor of its member, whoever writes last
__device__ __forceinline__ int uf_find(volatile int *par, int x)
{
    int p = par[x];
    while (p != x) {
        const int g = par[p];
        if (g == p) return p;
        par[x] = g; x = g; p = par[x];
    }
    return x;
}
// the root of x with no store at all: for the pass after the unions, where a word must END as the root, not merely hold an ancestor (a halving store of a
// lane that passes through could land after the owner's and leave an ancestor behind)
__device__ __forceinline__ int uf_root(const volatile int *par, int x)
{
    for (int p; (p = par[x]) != x; x = p) {}
    return x;
}
// hooks the larger root under the smaller: a parent is never above its child, a tree's root is its smallest member, and whatever the order of the unions the
// roots at the end are the smallest members of the components
__device__ __forceinline__ void uf_unite(int *par, int a, int b)
{
    for (;;) {
        a = uf_find(par, a); b = uf_find(par, b);
        if (a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        if (atomicCAS(&par[hi], hi, lo) == hi) return;               // (hi was still a root; otherwise another lane hooked it: look again)
    }
}

// ---- k_dup_verify: one 256-thread workgroup per listed bucket (the grid strides over the list).  The workgroup counts the bucket (the sorted positions from its
// first that carry its key); above CCSX_DUP_MAX_BUCKET every read of it is reported overflowed.  Otherwise the windows, lengths, groups, scores and read indices
// of its m reads go to LDS (32 KB for 512), the m (m - 1) / 2 pairs are dealt to the threads in turn, a pair that passes the group and the length clause and whose reads
// are not in one set yet is walked (dup_core.h: up to 8 walks of W steps) and a verified pair is united in LDS.  A member's local index is its rank in the bucket, which is in read order
// (the sort keeps equal keys in index order), so the root of a component is its smallest read.  Then per set: the largest score (LDS maximum), the smallest
// member that has it (LDS minimum), the size (LDS sum), and the four words of every member.
// Reads: key[1], idx[1] from the bucket's first position to one past its last; sig, group, score of its reads.  Writes: the report words of its reads only.
__global__ __launch_bounds__(NT) void k_dup_verify(DupClusterParams P)
{
    __shared__ unsigned long long sWin[MAXB][4];
    __shared__ int sIdx[MAXB], sLen[MAXB], sGroup[MAXB], sScore[MAXB], sPar[MAXB], sBest[MAXB], sRep[MAXB], sCnt[MAXB];
    __shared__ int sStop;
    const int tid = threadIdx.x, n = P.n, count = P.list[0];
    const DupOut out = ccsx_dup_out(P.rep, (size_t)n);
    const unsigned long long *key = P.key[1];
    const uint32_t *idx = P.idx[1];
    for (int b = blockIdx.x; b < count; b += gridDim.x) {            // (count and b are the same in every thread: the barriers below are uniform)
        const int p0 = P.list[1 + b];
        const unsigned long long key0 = key[p0];
        __syncthreads();                                             // (the bucket before is done with LDS)
        if (tid == 0) sStop = NONE;
        __syncthreads();
        for (int base = p0 + 1;; base += NT) {                       // the first position past the bucket
            const int pos = base + tid < n ? base + tid : n;         // (a position at or past n is a miss: the loop ends at the chunk that reaches n at the latest)
            const int miss = pos >= n || key[pos] != key0;
            if (miss) atomicMin(&sStop, pos);
            if (__syncthreads_or(miss)) break;
        }
        const int m = sStop - p0;
        if (m > MAXB) {
            for (int t = tid; t < m; t += NT) ccsx_dup_put_alone(out, (int)idx[p0 + t], CCSX_DUP_OVERFLOW);
            continue;
        }
        for (int t = tid; t < m; t += NT) {
            const int z = (int)idx[p0 + t];
            const ulonglong2 *s = reinterpret_cast<const ulonglong2 *>(P.sig + z);
            const ulonglong2 e0 = s[0], e1 = s[1];
            sWin[t][0] = e0.x; sWin[t][1] = e0.y; sWin[t][2] = e1.x; sWin[t][3] = e1.y;
            sIdx[t] = z; sLen[t] = sig_tail(P.sig + z).len;
            sGroup[t] = P.group ? P.group[z] : 0; sScore[t] = P.score ? P.score[z] : 0;
            sPar[t] = t; sBest[t] = (int)0x80000000; sRep[t] = NONE; sCnt[t] = 0;
        }
        __syncthreads();
        const int pairs = m * (m - 1) / 2;                           // (at most 130 816)
        for (int p = tid; p < pairs; p += NT) {
            // pair p = (i, j), i < j, p = j (j - 1) / 2 + i: j from a square root (8 p + 1 < 2^24 is exact in float), set right in integers
            int j = (int)((1.0f + sqrtf(1.0f + 8.0f * (float)p)) * 0.5f);
            while (j * (j - 1) / 2 > p) --j;
            while ((j + 1) * j / 2 <= p) ++j;
            const int i = p - j * (j - 1) / 2;
            if (!ccsx_dup_may_pair(sLen[i], sGroup[i], sLen[j], sGroup[j], P.opts)) continue;
            if (uf_find(sPar, i) == uf_find(sPar, j)) continue;      // (already one set: a pair more changes nothing; a stale "no" only costs its walks)
            const DupEnds a = ccsx_dup_ends(sWin[i]), c = ccsx_dup_ends(sWin[j]);
            if (ccsx_dup_ends_agree(a, c, P.opts)) uf_unite(sPar, i, j);
        }
        __syncthreads();
        // every member's root: read only (uf_root stores nothing, so nothing moves while the lanes walk), kept in registers — a thread has at most MAXB / NT
        // members —, and written behind a barrier, when no lane reads a parent any more
        int root[MAXB / NT];
#pragma unroll
        for (int q = 0; q < MAXB / NT; ++q) root[q] = tid + q * NT < m ? uf_root(sPar, tid + q * NT) : 0;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < MAXB / NT; ++q) if (tid + q * NT < m) sPar[tid + q * NT] = root[q];
        __syncthreads();
        for (int t = tid; t < m; t += NT) { atomicMax(&sBest[sPar[t]], sScore[t]); atomicAdd(&sCnt[sPar[t]], 1); }
        __syncthreads();
        for (int t = tid; t < m; t += NT) if (sScore[t] == sBest[sPar[t]]) atomicMin(&sRep[sPar[t]], t);
        __syncthreads();
        for (int t = tid; t < m; t += NT) {
            const int z = sIdx[t], r = sPar[t], rep = sIdx[sRep[r]];
            out.status[z] = CCSX_DUP_TESTED; out.rep[z] = rep; out.set_size[z] = sCnt[r]; out.dup[z] = rep != z;
        }
    }
}

}  // namespace

size_t ccsx_dup_sort_bytes(int n)
{
    size_t bytes = 0;
    if (n <= 0) return 0;
    if (rocprim::radix_sort_pairs((void *)nullptr, bytes, (unsigned long long *)nullptr, (unsigned long long *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr,
                                  (size_t)n, 0u, 64u, (hipStream_t)0) != hipSuccess) return 0;
    return bytes;
}

const char *ccsx_dup_sign_launch(const DupSignParams &S, hipStream_t st)
{
    if (S.n <= 0) return nullptr;
    const int per = CCSX_DUP_SIGN_THREADS / 64;
    hipLaunchKernelGGL(k_dup_sign, dim3((unsigned)((S.n + per - 1) / per)), dim3(CCSX_DUP_SIGN_THREADS), 0, st, S);
    return hipGetLastError() != hipSuccess ? "k_dup_sign" : nullptr;
}

const char *ccsx_dup_cluster_launch(const DupClusterParams &P, hipStream_t st)
{
    if (P.n <= 0) return nullptr;
    const unsigned blocks = (unsigned)((P.n + 255) / 256);
    hipLaunchKernelGGL(k_dup_keys, dim3(blocks), dim3(256), 0, st, P);
    if (hipGetLastError() != hipSuccess) return "k_dup_keys";
    size_t bytes = P.sort_tmp_bytes;
    if (rocprim::radix_sort_pairs(P.sort_tmp, bytes, P.key[0], P.key[1], P.idx[0], P.idx[1], (size_t)P.n, 0u, 64u, st) != hipSuccess) return "radix sort";
    hipLaunchKernelGGL(k_dup_buckets, dim3(blocks), dim3(256), 0, st, P);
    if (hipGetLastError() != hipSuccess) return "k_dup_buckets";
    // the work list's length is on the device: a grid of at most 2048 workgroups strides over it (never more workgroups than there can be buckets)
    const unsigned grid = (unsigned)std::min(2048, std::max(1, P.n / 2));
    hipLaunchKernelGGL(k_dup_verify, dim3(grid), dim3(NT), 0, st, P);
    return hipGetLastError() != hipSuccess ? "k_dup_verify" : nullptr;
}

// ccsx_refine.hip — the polisher hand-back (DESIGN.md §2 "Polisher hand-back"; docs/faq/revio.md:35-51, steps 2 and 3): the refined tiles of a second polisher
// are spliced into the consensus on the device, the read quality of the merged per-base values is summed, and the spliced sequence is left where k_draft_in
// finds a caller's draft — the polish seam then scores it once more, for QVs only.  Integers only except the one final division; no result depends on the
// launch geometry or on scheduling: the only atomics add integer counts.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ccsx.h"
#include "refine_core.h"
#include "wave_ops.h"

namespace {

constexpr int LANES = 64;

__device__ const uint64_t perr_fx[CCSX_REFINE_NQ] = {CCSX_REFINE_PERR_TABLE};

__device__ __forceinline__ int64_t wave_sum_i64(int64_t v)
{
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor((long long)v, m);
    return v;
}

// first index in [0, n) whose tile_zmw is >= key (n: none); the list is nondecreasing when this is called
__device__ __forceinline__ int64_t tile_lower_bound(const int32_t *tile_zmw, int64_t n, int32_t key)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (tile_zmw[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// ---- k_refine_check: one workgroup per 256 consecutive tiles.  Thread t takes tile g0 + t: the list-order violations are counted, and a tile whose ZMW
// exists gets its classes from its raw values, compared in 64 bits.  The rows of the workgroup's tiles are one contiguous block of new_seq / new_qual: the
// threads walk it byte by byte, consecutive lanes on consecutive bytes, and load a byte only when it is one of the first new_len entries of its row and
// 0 <= new_len <= U — nothing beyond min(new_len, U) is dereferenced.  base is not touched at all.
__global__ __launch_bounds__(CCSX_REFINE_THREADS) void k_refine_check(RefineParams R)
{
    __shared__ int32_t s_nl[CCSX_REFINE_THREADS];          // entries of the tile's rows that are read (0: none)
    __shared__ uint32_t s_bad[CCSX_REFINE_THREADS];        // a bad symbol among them
    const int t = threadIdx.x;
    const int64_t g0 = (int64_t)blockIdx.x * CCSX_REFINE_THREADS, g = g0 + t;
    bool viol = false;
    uint32_t cls = 0;
    int32_t read = 0;
    if (g < R.n_tiles) {
        const int32_t z = R.tile_zmw[g];
        const bool prev = g > 0;
        const int32_t zp = prev ? R.tile_zmw[g - 1] : 0;
        viol = z < 0 || z >= R.n_zmw || (prev && z < zp);
        if (z >= 0 && z < R.n_zmw) {
            const int64_t L = R.base_len[z], s = R.tile_start[g], l = R.tile_len[g], nl = R.tile_new_len[g];
            const bool len_ok = nl >= 0 && nl <= R.stride;
            if (s < 0 || l < 1 || s + l > L || !len_ok) cls |= CCSX_REFINE_CLS_TILE;
            if (prev && zp == z && s < (int64_t)R.tile_start[g - 1] + (int64_t)R.tile_len[g - 1]) cls |= CCSX_REFINE_CLS_ORDER;
            if (len_ok) read = (int32_t)nl;
        }
    }
    s_nl[t] = read; s_bad[t] = 0u;
    __syncthreads();
    {
        const int64_t left = R.n_tiles - g0;
        const uint32_t U = (uint32_t)R.stride, total = (uint32_t)(left < CCSX_REFINE_THREADS ? left : CCSX_REFINE_THREADS) * U;   // <= 256 x 256 bytes
        const uint8_t *ns = R.new_seq + g0 * R.stride, *nq = R.new_qual + g0 * R.stride;
        for (uint32_t b = (uint32_t)t; b < total; b += CCSX_REFINE_THREADS) {
            const uint32_t r = b / U, i = b - r * U;
            if ((int32_t)i < s_nl[r] && (ns[b] > 3 || nq[b] > CCSX_REFINE_NQ - 1)) atomicOr(&s_bad[r], 1u);
        }
    }
    __syncthreads();
    if (g < R.n_tiles) R.tile_cls[g] = cls | (s_bad[t] ? CCSX_REFINE_CLS_SYMBOL : 0u);
    const int nv = __popcll(__ballot(viol));
    if ((t & (LANES - 1)) == 0 && nv) atomicAdd(R.counts + 2, nv);
}

// ---- k_refine_plan: one wave per ZMW.  The ZMW's run of tiles by binary search, its classes reduced, L', the code and n_applied; the slot's din_len / din_bb
// for k_draft_in and the report planes.
__global__ __launch_bounds__(LANES) void k_refine_plan(RefineParams R)
{
    const int lane = threadIdx.x, z = blockIdx.x;
    if (z >= R.n_zmw) return;
    const int64_t C = R.seq_off[z + 1] - R.seq_off[z];
    int64_t L = R.base_len[z];
    if (L > C) L = 0;                                      // (a base row longer than its slot is no base row: the call refuses it, and no kernel would follow it)
    const int32_t bb = R.backbone[z], passes = R.read_off[z + 1] - R.read_off[z];
    int32_t code, napp = 0;
    int64_t len = 0, first = 0;
    if (L <= 0 || bb < 0) code = CCSX_REFINE_SKIPPED;
    else if (bb >= passes) code = CCSX_REFINE_BAD_BACKBONE;
    else if (R.counts[2] != 0) { code = CCSX_REFINE_BAD_LIST; len = L; }
    else {
        first = tile_lower_bound(R.tile_zmw, R.n_tiles, z);
        const int64_t end = tile_lower_bound(R.tile_zmw, R.n_tiles, z + 1);
        len = L;
        if (first == end) code = CCSX_REFINE_RESCORED;
        else {
            uint32_t cls = 0;
            int64_t delta = 0;
            for (int64_t g = first + lane; g < end; g += LANES) {
                cls |= R.tile_cls[g];
                delta += (int64_t)R.tile_new_len[g] - (int64_t)R.tile_len[g];
            }
            const bool c1 = __ballot(cls & CCSX_REFINE_CLS_TILE) != 0, c2 = __ballot(cls & CCSX_REFINE_CLS_ORDER) != 0, c3 = __ballot(cls & CCSX_REFINE_CLS_SYMBOL) != 0;
            const int64_t Lp = L + wave_sum_i64(delta);
            if (c1) code = CCSX_REFINE_BAD_TILE;
            else if (c2) code = CCSX_REFINE_BAD_ORDER;
            else if (c3) code = CCSX_REFINE_BAD_SYMBOL;
            else if (Lp > C) code = CCSX_REFINE_TOO_LONG;
            else if (Lp < 1) code = CCSX_REFINE_EMPTY;
            else { code = CCSX_REFINE_REFINED; len = Lp; napp = (int32_t)(end - first); }
        }
    }
    if (lane == 0) {
        R.code[z] = code; R.n_applied[z] = napp; R.new_len[z] = (int32_t)len; R.tile_first[z] = first;
        R.din_len[z] = (int32_t)len; R.din_bb[z] = bb;
        if (code == CCSX_REFINE_REFINED) { atomicAdd(R.counts, 1); atomicAdd(R.counts + 1, napp); }
    }
}

// ---- k_refine_splice: one wave per ZMW.  D_z into the slot's draft buffer, M_z into qual_merged when asked, the sum of perr_fx over M_z.  The offsets of the
// tiles in the output are the prefix of their length deltas, taken 64 tiles at a time with a carry: a ZMW may have any number of tiles.  Every copy below writes
// consecutive bytes from consecutive lanes.  Only a ZMW with code REFINED has its tiles read: all of them were found valid, in order and inside the base row,
// and L' fits the slot.
__global__ __launch_bounds__(LANES) void k_refine_splice(RefineParams R)
{
    __shared__ uint64_t sperr[CCSX_REFINE_NQ];
    const int lane = threadIdx.x, z = blockIdx.x;
    for (int i = lane; i < CCSX_REFINE_NQ; i += LANES) sperr[i] = perr_fx[i];
    __syncthreads();
    if (z >= R.n_zmw) return;
    const int32_t code = R.code[z], len = R.new_len[z];
    if (len <= 0) { if (lane == 0) R.rq_merged[z] = 0.0f; return; }
    const int64_t off = R.seq_off[z];
    const uint8_t *base = R.base_seq + off, *bq = R.base_qual + off;
    uint8_t *out = R.draft + off, *qm = R.qual_merged ? R.qual_merged + off : nullptr;
    uint64_t acc = 0;
    auto put = [&](int64_t o, uint8_t s, uint8_t q) {
        out[o] = s;
        if (qm) qm[o] = q;
        acc += q < CCSX_REFINE_NQ ? sperr[q] : 0ull;
    };
    auto copy_base = [&](int64_t b0, int64_t b1, int64_t o0) { for (int64_t i = b0 + lane; i < b1; i += LANES) put(o0 + (i - b0), base[i], bq[i]); };
    if (code != CCSX_REFINE_REFINED) copy_base(0, len, 0);
    else {
        const int64_t L = R.base_len[z], g0 = R.tile_first[z];
        const int32_t nt = R.n_applied[z];
        int64_t carry = 0, prev_end = 0;                   // the deltas of the tiles before this chunk; the base position behind the previous tile
        for (int32_t c = 0; c < nt; c += LANES) {
            const int cnt = nt - c < LANES ? nt - c : LANES;
            const bool have = lane < cnt;
            const int64_t g = g0 + c + (have ? lane : 0);
            const int32_t s = have ? R.tile_start[g] : 0, l = have ? R.tile_len[g] : 0, nl = have ? R.tile_new_len[g] : 0;
            const int32_t incl = wave_scan_add_i32(nl - l);
            const int32_t os = s + (incl - (nl - l));      // the tile's first output position, without the carry
            for (int j = 0; j < cnt; ++j) {
                const int64_t sj = __builtin_amdgcn_readlane(s, j), lj = __builtin_amdgcn_readlane(l, j), nlj = __builtin_amdgcn_readlane(nl, j);
                const int64_t oj = (int64_t)__builtin_amdgcn_readlane(os, j) + carry;
                copy_base(prev_end, sj, oj - (sj - prev_end));
                const uint8_t *ns = R.new_seq + (g0 + c + j) * R.stride, *nq = R.new_qual + (g0 + c + j) * R.stride;
                for (int64_t i = lane; i < nlj; i += LANES) put(oj + i, ns[i], nq[i]);
                prev_end = sj + lj;
            }
            carry += __builtin_amdgcn_readlane(incl, LANES - 1);
        }
        copy_base(prev_end, L, prev_end + carry);
    }
    const uint64_t sum = (uint64_t)wave_sum_i64((int64_t)acc);
    if (lane == 0) R.rq_merged[z] = (float)(1.0 - (double)sum / 4294967296.0 / (double)len);
}

}  // namespace

const char *ccsx_refine_launch(const RefineParams &R, hipStream_t st)
{
    if (hipMemsetAsync(R.counts, 0, 3 * sizeof(int32_t), st) != hipSuccess) return "hipMemsetAsync (refine counts)";
    if (R.n_tiles > 0) {
        hipLaunchKernelGGL(k_refine_check, dim3((unsigned)((R.n_tiles + CCSX_REFINE_THREADS - 1) / CCSX_REFINE_THREADS)), dim3(CCSX_REFINE_THREADS), 0, st, R);
        if (hipGetLastError() != hipSuccess) return "k_refine_check";
    }
    hipLaunchKernelGGL(k_refine_plan, dim3(R.n_zmw), dim3(LANES), 0, st, R);
    if (hipGetLastError() != hipSuccess) return "k_refine_plan";
    hipLaunchKernelGGL(k_refine_splice, dim3(R.n_zmw), dim3(LANES), 0, st, R);
    if (hipGetLastError() != hipSuccess) return "k_refine_splice";
    return nullptr;
}

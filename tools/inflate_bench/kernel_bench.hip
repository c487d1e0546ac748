// kernel_bench — k_inflate alone: the BGZF blocks of a BAM file resident in HBM, timed with HIP events (tools/inflate_bench.py builds and runs it).
// usage: kernel_bench IN.bam [target inflated bytes = 1e9] [rounds = 7]
// The file's blocks are taken in order until the target is reached (a smaller file is taken whole and the figure says so); every round is one launch over all
// of them.  The output of the first round is checked against zlib, block by block.
#include <hip/hip_runtime.h>
#include <zlib.h>

#include <cstring>

#include "../../ccs_amd/csrc/ccsx_inflate.hip"
#include "../bgzf_bench.h"

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: kernel_bench IN.bam [bytes] [rounds]\n"); return 2; }
    const double target = argc > 2 ? atof(argv[2]) : 1e9;
    const int rounds = argc > 3 ? atoi(argv[3]) : 7;
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<uint8_t> src;
    std::vector<ccsx_deflate_block> blk;
    int64_t out = 0;
    bgzf_walk(f, src, true, [&] { return out < target; }, [&](size_t at, size_t len, uint32_t isize) {
        if (isize) blk.push_back({(int64_t)at, (int32_t)(len - 8), (int32_t)isize, out});
        out += isize;
    });
    fclose(f);
    if (blk.empty()) { fprintf(stderr, "no blocks\n"); return 2; }
    uint8_t *d_src, *d_dst; ccsx_deflate_block *d_blk; int32_t *d_st;
    CK(hipMalloc((void **)&d_src, src.size() + 16)); CK(hipMalloc((void **)&d_dst, (size_t)out + 16));
    CK(hipMalloc((void **)&d_blk, blk.size() * sizeof(blk[0]))); CK(hipMalloc((void **)&d_st, blk.size() * 4));
    CK(hipMemcpy(d_src, src.data(), src.size(), hipMemcpyHostToDevice));
    CK(hipMemcpy(d_blk, blk.data(), blk.size() * sizeof(blk[0]), hipMemcpyHostToDevice));
    const auto launch = [&](hipStream_t s) { return ccsx_launch_inflate(s, d_src, (int64_t)src.size(), d_blk, (int32_t)blk.size(), d_dst, out, d_st); };
    const auto check0 = [&]() -> int {
        std::vector<uint8_t> got((size_t)out), ref(65536); std::vector<int32_t> st(blk.size());
        CK(hipMemcpy(got.data(), d_dst, (size_t)out, hipMemcpyDeviceToHost)); CK(hipMemcpy(st.data(), d_st, st.size() * 4, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < blk.size(); ++i) {
            z_stream zs; memset(&zs, 0, sizeof(zs)); inflateInit2(&zs, -15);
            zs.next_in = src.data() + blk[i].in_off; zs.avail_in = (uInt)blk[i].in_len; zs.next_out = ref.data(); zs.avail_out = 65536;
            const int rc = inflate(&zs, Z_FINISH); inflateEnd(&zs);
            if (rc != Z_STREAM_END || st[i] != 0 || (int32_t)zs.total_out != blk[i].out_len || memcmp(ref.data(), got.data() + blk[i].out_off, zs.total_out)) {
                fprintf(stderr, "block %zu differs from zlib (status %d)\n", i, st[i]); return 1;
            }
        }
        return 0;
    };
    std::vector<double> gbs;
    if (bgzf_time_rounds(rounds, (double)out, launch, check0, &gbs)) return 1;
    printf("k_inflate alone: %zu blocks, %.1f MB compressed -> %.1f MB inflated (ratio %.2f), every block equals zlib; %d rounds: median %.2f GB/s inflated (min %.2f, max %.2f)\n",
           blk.size(), src.size() / 1e6, out / 1e6, (double)out / src.size(), rounds, gbs[gbs.size() / 2], gbs.front(), gbs.back());
    return 0;
}

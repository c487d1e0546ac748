// kernel_bench — k_deflate alone: the inflated blocks of a BAM file resident in HBM, timed with HIP events (tools/deflate_bench.py builds and runs it).
// usage: kernel_bench IN.bam [target plain bytes = 5e8] [rounds = 7]
// The file's blocks are inflated on the host (zlib) and taken in order, as the spans a BGZF writer would cut, until the target is reached (a smaller file is
// taken whole and the figure says so); every round is one launch over all of them.  The output of the first round is checked span by span: equal to the host's
// run of the same encoder (deflate_core.h, one lane), and zlib inflates it back to the span.  It also prints what zlib level 1 and level 4 make of the same spans.
#include <hip/hip_runtime.h>
#include <zlib.h>

#include <cstring>

#include "../../ccs_amd/csrc/ccsx_deflate.hip"
#include "../bgzf_bench.h"

static size_t zlib_len(const uint8_t *p, size_t n, int level)
{
    static std::vector<uint8_t> out(compressBound(65536) + 64);
    z_stream zs; memset(&zs, 0, sizeof(zs));
    deflateInit2(&zs, level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY);
    zs.next_in = const_cast<Bytef *>(p); zs.avail_in = (uInt)n; zs.next_out = out.data(); zs.avail_out = (uInt)out.size();
    deflate(&zs, Z_FINISH);
    const size_t len = zs.total_out;
    deflateEnd(&zs);
    return len;
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: kernel_bench IN.bam [bytes] [rounds]\n"); return 2; }
    const double target = argc > 2 ? atof(argv[2]) : 5e8;
    const int rounds = argc > 3 ? atoi(argv[3]) : 7;
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<uint8_t> src, comp;
    std::vector<ccsx_deflate_span> span;
    int64_t cap_total = 0;
    bgzf_walk(f, comp, false, [&] { return (double)src.size() < target; }, [&](size_t, size_t len, uint32_t isize) {
        if (!isize) return;
        const size_t at = src.size();
        src.resize(at + isize);
        z_stream zs; memset(&zs, 0, sizeof(zs)); inflateInit2(&zs, -15);
        zs.next_in = comp.data(); zs.avail_in = (uInt)(len - 8); zs.next_out = src.data() + at; zs.avail_out = isize;
        const int rc = inflate(&zs, Z_FINISH); inflateEnd(&zs);
        if (rc != Z_STREAM_END || zs.total_out != isize) { fprintf(stderr, "a block does not inflate\n"); exit(2); }
        const int32_t cap = ccsx_defl_stored_len((int32_t)isize);
        span.push_back({(int64_t)at, (int32_t)isize, cap, cap_total});
        cap_total += cap;
    });
    fclose(f);
    if (span.empty()) { fprintf(stderr, "no blocks\n"); return 2; }
    const size_t n = span.size();
    uint8_t *d_src, *d_dst; ccsx_deflate_span *d_span; int32_t *d_len, *d_st; uint32_t *d_crc;
    CK(hipMalloc((void **)&d_src, src.size() + 16)); CK(hipMalloc((void **)&d_dst, (size_t)cap_total + 16));
    CK(hipMalloc((void **)&d_span, n * sizeof(span[0]))); CK(hipMalloc((void **)&d_len, n * 4)); CK(hipMalloc((void **)&d_st, n * 4)); CK(hipMalloc((void **)&d_crc, n * 4));
    CK(hipMemcpy(d_src, src.data(), src.size(), hipMemcpyHostToDevice));
    CK(hipMemcpy(d_span, span.data(), n * sizeof(span[0]), hipMemcpyHostToDevice));
    int64_t out_total = 0, z1 = 0, z4 = 0;
    size_t stored = 0;
    const auto launch = [&](hipStream_t s) { return ccsx_launch_deflate(s, d_src, (int64_t)src.size(), d_span, (int32_t)n, d_dst, cap_total, d_len, d_crc, d_st); };
    const auto check0 = [&]() -> int {
        std::vector<uint8_t> got((size_t)cap_total), ref(65536 + 64), back(65536);
        std::vector<int32_t> len(n), st(n); std::vector<uint32_t> crc(n);
        CK(hipMemcpy(got.data(), d_dst, (size_t)cap_total, hipMemcpyDeviceToHost)); CK(hipMemcpy(len.data(), d_len, n * 4, hipMemcpyDeviceToHost));
        CK(hipMemcpy(st.data(), d_st, n * 4, hipMemcpyDeviceToHost)); CK(hipMemcpy(crc.data(), d_crc, n * 4, hipMemcpyDeviceToHost));
        static ccsx_defl_work W;
        for (size_t i = 0; i < n; ++i) {
            int32_t hl = 0; uint32_t hc = 0;
            const uint8_t *p = src.data() + span[i].in_off;
            const int hs = ccsx_defl_span<ccsx_defl_serial>(p, span[i].in_len, ref.data(), span[i].out_cap, &W, &hl, &hc);
            if (st[i] != hs || len[i] != hl || crc[i] != hc || memcmp(ref.data(), got.data() + span[i].out_off, (size_t)hl)) { fprintf(stderr, "span %zu differs from the host's encoder\n", i); return 1; }
            if (crc[i] != (uint32_t)crc32(crc32(0L, Z_NULL, 0), p, (uInt)span[i].in_len)) { fprintf(stderr, "span %zu: CRC differs from zlib\n", i); return 1; }
            z_stream zs; memset(&zs, 0, sizeof(zs)); inflateInit2(&zs, -15);
            zs.next_in = got.data() + span[i].out_off; zs.avail_in = (uInt)len[i]; zs.next_out = back.data(); zs.avail_out = 65536;
            const int rc = inflate(&zs, Z_FINISH); inflateEnd(&zs);
            if (rc != Z_STREAM_END || (int32_t)zs.total_out != span[i].in_len || zs.avail_in != 0 || memcmp(back.data(), p, zs.total_out)) { fprintf(stderr, "span %zu: zlib does not inflate it back\n", i); return 1; }
            out_total += len[i];
            stored += len[i] == span[i].out_cap;
            z1 += (int64_t)zlib_len(p, (size_t)span[i].in_len, 1); z4 += (int64_t)zlib_len(p, (size_t)span[i].in_len, 4);
        }
        return 0;
    };
    std::vector<double> gbs;
    if (bgzf_time_rounds(rounds, (double)src.size(), launch, check0, &gbs)) return 1;
    printf("k_deflate alone: %zu spans, %.1f MB plain -> %.1f MB (ratio %.2f; %zu spans stored; zlib level 1 %.1f MB, level 4 %.1f MB: excess over level 1 %+.2f %%), every stream "
           "equals the host's encoder and inflates back with zlib; %d rounds: median %.2f GB/s of plain bytes (min %.2f, max %.2f)\n",
           n, src.size() / 1e6, out_total / 1e6, (double)src.size() / out_total, stored, z1 / 1e6, z4 / 1e6, 100.0 * (out_total - z1) / z1, rounds, gbs[gbs.size() / 2], gbs.front(),
           gbs.back());
    return 0;
}

// bgzf_bench.h — what the kernel-alone bench programs of the two BGZF codecs share (tools/inflate_bench/kernel_bench.hip, tools/deflate_bench/kernel_bench.hip):
// the HIP call check, the walk over a BAM file's BGZF blocks, and the event-timed rounds with a checked round 0.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

// The plain BGZF blocks of f in order, while more() holds and the file lasts.  What follows a block's 18-byte header (the DEFLATE stream, CRC32, ISIZE) is read
// to the end of `bytes` (keep) or replaces them; block(at, len, isize) gets where in `bytes` it begins, its length (the stream's: len - 8) and the block's
// ISIZE.  Anything but plain blocks of at most 64 KiB ends the program with status 2.
template <typename More, typename Block> static void bgzf_walk(FILE *f, std::vector<uint8_t> &bytes, bool keep, More more, Block block)
{
    uint8_t h[18];
    while (more() && fread(h, 1, 18, f) == 18) {
        if (h[0] != 0x1f || h[1] != 0x8b || h[12] != 'B' || h[13] != 'C' || (h[10] | h[11] << 8) != 6) { fprintf(stderr, "not a plain BGZF block\n"); exit(2); }
        const size_t bsize = (size_t)(h[16] | h[17] << 8) + 1, at = keep ? bytes.size() : 0;
        bytes.resize(at + bsize - 18);
        if (fread(bytes.data() + at, 1, bsize - 18, f) != bsize - 18) { fprintf(stderr, "truncated file\n"); exit(2); }
        const uint8_t *t = bytes.data() + bytes.size() - 4;
        const uint32_t isize = t[0] | t[1] << 8 | t[2] << 16 | (uint32_t)t[3] << 24;
        if (isize > 65536) { fprintf(stderr, "block larger than 64 KiB\n"); exit(2); }
        block(at, bsize - 18, isize);
    }
}

// rounds + 1 launches on a stream of their own, each between two events: round 0 warms up and is checked (check0() != 0 fails the run), the others give
// bytes / time in GB/s, sorted into *gbs.  launch(stream) != 0 is a failed launch.  Returns 0, or 1 after a message
template <typename Launch, typename Check> static int bgzf_time_rounds(int rounds, double bytes, Launch launch, Check check0, std::vector<double> *gbs)
{
    hipStream_t s; CK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    for (int r = 0; r <= rounds; ++r) {
        CK(hipEventRecord(e0, s));
        if (launch(s)) { fprintf(stderr, "launch failed\n"); return 1; }
        CK(hipEventRecord(e1, s));
        CK(hipEventSynchronize(e1));
        float ms = 0; CK(hipEventElapsedTime(&ms, e0, e1));
        if (r == 0) { if (check0()) return 1; }
        else gbs->push_back(bytes / (ms * 1e6));
    }
    std::sort(gbs->begin(), gbs->end());
    return 0;
}

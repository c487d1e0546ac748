// kernel_bench — k_segment alone: reads resident in HBM, timed with HIP events (tools/segment_bench.py builds and runs it).
// usage: kernel_bench [reads = 16384] [read length = 10000] [rounds = 7]
// Per configuration — 9 and 17 random adapters of 25 bases — every read is a whole array A0 S1 A1 .. SK AK of random segments that fills the read, every second
// one reverse complemented, so the kernel meets the hits, the start walks and the selection it meets in a run; one launch over all reads per round.  The
// report of the first round is compared with ccsx_segment_reads_host on the first 512 reads.  One line per configuration.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

static std::string g_err;
void ccsx_set_error(const std::string &s) { g_err = s; }
#include "../../ccs_amd/csrc/ccsx_segment.hip"
#include "../../ccs_amd/csrc/ccsx_barcode_api.cpp"
#include "../../ccs_amd/csrc/ccsx_segment_api.cpp"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

static uint64_t rng_state = 0x2545f4914f6cdd1dull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 32); }

int main(int argc, char **argv)
{
    const int n = argc > 1 ? atoi(argv[1]) : 16384, L = argc > 2 ? atoi(argv[2]) : 10000, rounds = argc > 3 ? atoi(argv[3]) : 7, M = 25;
    if (n < 1 || L < 17 * M + 16 * 50 || rounds < 1) { fprintf(stderr, "usage: kernel_bench [reads] [read length >= 1225] [rounds]\n"); return 2; }
    std::vector<uint8_t> seq((size_t)n * L);
    std::vector<int64_t> off((size_t)n);
    std::vector<int32_t> len((size_t)n, L);
    for (int z = 0; z < n; ++z) off[z] = (int64_t)z * L;
    const size_t rep_bytes = ccsx_sg_rep_bytes((size_t)n);
    uint8_t *d_seq; int64_t *d_off; int32_t *d_len; unsigned long long *d_set;                  // d_set: the packed set, the report behind it
    CK(hipMalloc((void **)&d_seq, seq.size())); CK(hipMalloc((void **)&d_off, (size_t)n * 8)); CK(hipMalloc((void **)&d_len, (size_t)n * 4));
    CK(hipMalloc((void **)&d_set, ccsx_sg_set_words(CCSX_SEGMENT_MAX_ADAPTERS) * 8 + rep_bytes));
    CK(hipMemcpy(d_off, off.data(), (size_t)n * 8, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_len, len.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    hipStream_t s; CK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    auto set = std::make_unique<ccsx_segment_set>();
    for (int na : {9, 17}) {
        memset(set.get(), 0, sizeof *set);
        set->n_adapters = na;
        for (int a = 0; a < na; ++a) { set->len[a] = M; for (int i = 0; i < M; ++i) set->seq[a][i] = (uint8_t)(rnd() & 3); }
        const int seg = (L - na * M) / (na - 1);                     // what is left of the read after the last adapter stays random
        for (int z = 0; z < n; ++z) {
            uint8_t *c = &seq[(size_t)z * L];
            for (int i = 0; i < L; ++i) c[i] = (uint8_t)(rnd() & 3);
            for (int a = 0; a < na; ++a) memcpy(c + (size_t)a * (M + seg), set->seq[a], M);
            if (z & 1) { std::reverse(c, c + L); for (int i = 0; i < L; ++i) c[i] = (uint8_t)(3 - c[i]); }
        }
        CK(hipMemcpy(d_seq, seq.data(), seq.size(), hipMemcpyHostToDevice));
        const int S = 2 * na;
        std::vector<unsigned long long> packed(ccsx_sg_set_words(na), 0ull);
        ccsx_sg_pack(set.get(), packed.data());
        CK(hipMemcpy(d_set, packed.data(), packed.size() * 8, hipMemcpyHostToDevice));
        SegmentParams G{};
        ccsx_segment_opts_default(&G.opts);
        G.n = n; G.n_adapters = na; G.seq = d_seq; G.seq_off = d_off; G.seq_len = d_len;
        ccsx_sg_bind(G, d_set);
        std::vector<double> us;
        long complete = 0;
        for (int r = 0; r <= rounds; ++r) {                          // round 0 warms up and is checked
            CK(hipEventRecord(e0, s));
            if (const char *failed = ccsx_segment_launch(G, s)) { fprintf(stderr, "launch failed: %s\n", failed); return 1; }
            CK(hipEventRecord(e1, s));
            CK(hipEventSynchronize(e1));
            float ms = 0; CK(hipEventElapsedTime(&ms, e0, e1));
            if (r == 0) {
                const int m = std::min(n, 512);
                std::vector<uint8_t> got(rep_bytes), want(ccsx_sg_rep_bytes((size_t)m));
                CK(hipMemcpy(got.data(), G.rep, rep_bytes, hipMemcpyDeviceToHost));
                const SegmentOut g = ccsx_sg_out((int32_t *)got.data(), (size_t)n), w = ccsx_sg_out((int32_t *)want.data(), (size_t)m);
                ccsx_segment_report rep{m, w.tested, w.overflow, w.n_hits, w.n_cuts, w.n_segments, w.complete, w.orient, w.leftover, w.pieces};
                if (ccsx_segment_reads_host(set.get(), &G.opts, seq.data(), off.data(), len.data(), m, &rep)) { fprintf(stderr, "host rule: %s\n", g_err.c_str()); return 1; }
                const int32_t *gp[CCSX_SG_PLANES] = {g.tested, g.overflow, g.n_hits, g.n_cuts, g.n_segments, g.complete, g.orient, g.leftover};
                const int32_t *wp[CCSX_SG_PLANES] = {w.tested, w.overflow, w.n_hits, w.n_cuts, w.n_segments, w.complete, w.orient, w.leftover};
                for (int k = 0; k < CCSX_SG_PLANES; ++k)
                    if (memcmp(gp[k], wp[k], (size_t)m * 4)) { fprintf(stderr, "plane %d differs from the host rule\n", k); return 1; }
                if (memcmp(g.pieces, w.pieces, (size_t)m * CCSX_SEGMENT_MAX_PIECES * sizeof(ccsx_segment_piece))) { fprintf(stderr, "the list differs from the host rule\n"); return 1; }
                for (int z = 0; z < n; ++z) complete += g.complete[z];
            } else us.push_back(ms * 1e3);
        }
        std::sort(us.begin(), us.end());
        const double steps = (double)n * S * L;
        printf("k_segment alone: %d reads of %d bases, %2d adapters of %d bases (%d segments of %d): median %9.1f us (min %.1f, max %.1f) over %d launches = %.1f G column "
               "steps/s; %ld reads complete; the first 512 reads equal the host rule\n", n, L, na, M, na - 1, seg, us[us.size() / 2], us.front(), us.back(), rounds,
               steps / (us[us.size() / 2] * 1e3), complete);
    }
    return 0;
}

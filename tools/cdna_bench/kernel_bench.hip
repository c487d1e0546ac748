// kernel_bench — k_cdna alone: reads resident in HBM, timed with HIP events (tools/cdna_bench.py builds and runs it).
// usage: kernel_bench [reads = 16384] [read length = 10000] [rounds = 7]
// Per configuration — 2 and 16 random primers of 25 bases, roles alternating — every read is 5p . random insert . A x 30 . rc(3p) with a 5' and a 3' primer of the
// set that fills the read, every second one reverse complemented and every eighth with a further primer inside the insert, so the kernel meets the calls at both
// ends, the poly(A) scan, the walk over the whole read, the start walks and every class from CONCATEMER on that it meets in a run; one launch over all reads per
// round.  The report of the first round is compared with ccsx_cdna_reads_host on the first 512 reads.  One line per configuration.
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
#include "../../ccs_amd/csrc/ccsx_cdna.hip"
#include "../../ccs_amd/csrc/ccsx_barcode_api.cpp"
#include "../../ccs_amd/csrc/ccsx_cdna_api.cpp"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

static uint64_t rng_state = 0x2545f4914f6cdd1dull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 32); }

int main(int argc, char **argv)
{
    const int n = argc > 1 ? atoi(argv[1]) : 16384, L = argc > 2 ? atoi(argv[2]) : 10000, rounds = argc > 3 ? atoi(argv[3]) : 7, M = 25, TAIL = 30;
    if (n < 1 || L < 1000 || rounds < 1) { fprintf(stderr, "usage: kernel_bench [reads] [read length >= 1000] [rounds]\n"); return 2; }
    std::vector<uint8_t> seq((size_t)n * L);
    std::vector<int64_t> off((size_t)n);
    std::vector<int32_t> len((size_t)n, L);
    for (int z = 0; z < n; ++z) off[z] = (int64_t)z * L;
    const size_t rep_bytes = ccsx_cd_rep_bytes((size_t)n);
    uint8_t *d_seq; int64_t *d_off; int32_t *d_len; unsigned long long *d_set;                  // d_set: the packed set, the report behind it
    CK(hipMalloc((void **)&d_seq, seq.size())); CK(hipMalloc((void **)&d_off, (size_t)n * 8)); CK(hipMalloc((void **)&d_len, (size_t)n * 4));
    CK(hipMalloc((void **)&d_set, ccsx_cd_set_words(CCSX_CDNA_MAX_PRIMERS) * 8 + rep_bytes));
    CK(hipMemcpy(d_off, off.data(), (size_t)n * 8, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_len, len.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    hipStream_t s; CK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    auto set = std::make_unique<ccsx_cdna_set>();
    for (int np : {2, 16}) {
        memset(set.get(), 0, sizeof *set);
        set->n_primers = np;
        for (int b = 0; b < np; ++b) { set->len[b] = M; set->role[b] = (uint8_t)(b & 1); for (int i = 0; i < M; ++i) set->seq[b][i] = (uint8_t)(rnd() & 3); }
        for (int z = 0; z < n; ++z) {
            uint8_t *c = &seq[(size_t)z * L];
            const int pair = 2 * (z % (np / 2));                     // the 5' primer `pair`, the 3' primer `pair + 1`
            for (int i = 0; i < L; ++i) c[i] = (uint8_t)(rnd() & 3);
            memcpy(c, set->seq[pair], M);
            if (z % 8 == 7) memcpy(c + L / 2, set->seq[rnd() % (uint32_t)np], M);                // a concatemer's junction
            c[L - M - TAIL - 1] = 1; c[L - M - TAIL - 2] = 2;        // the insert ends in two bases other than A
            memset(c + L - M - TAIL, 0, TAIL);
            for (int i = 0; i < M; ++i) c[L - M + i] = (uint8_t)(3 - set->seq[pair + 1][M - 1 - i]);
            if (z & 1) { std::reverse(c, c + L); for (int i = 0; i < L; ++i) c[i] = (uint8_t)(3 - c[i]); }
        }
        CK(hipMemcpy(d_seq, seq.data(), seq.size(), hipMemcpyHostToDevice));
        std::vector<unsigned long long> packed(ccsx_cd_set_words(np), 0ull);
        ccsx_cd_pack(set.get(), packed.data());
        CK(hipMemcpy(d_set, packed.data(), packed.size() * 8, hipMemcpyHostToDevice));
        CdnaParams D{};
        ccsx_cdna_opts_default(&D.opts);
        D.n = n; D.n_primers = np; D.seq = d_seq; D.seq_off = d_off; D.seq_len = d_len;
        ccsx_cd_bind(D, d_set);
        std::vector<double> us;
        long cls[7] = {0, 0, 0, 0, 0, 0, 0};
        for (int r = 0; r <= rounds; ++r) {                          // round 0 warms up and is checked
            CK(hipEventRecord(e0, s));
            if (const char *failed = ccsx_cdna_launch(D, s)) { fprintf(stderr, "launch failed: %s\n", failed); return 1; }
            CK(hipEventRecord(e1, s));
            CK(hipEventSynchronize(e1));
            float ms = 0; CK(hipEventElapsedTime(&ms, e0, e1));
            if (r == 0) {
                const int m = std::min(n, 512);
                std::vector<uint8_t> got(rep_bytes), want(ccsx_cd_rep_bytes((size_t)m));
                CK(hipMemcpy(got.data(), D.rep, rep_bytes, hipMemcpyDeviceToHost));
                const CdnaOut g = ccsx_cd_out((int32_t *)got.data(), (size_t)n), w = ccsx_cd_out((int32_t *)want.data(), (size_t)m);
                ccsx_cdna_report rep{m, w.tested, w.cls, w.strand, w.start, w.end, w.polya_len, w.n_internal, w.first_internal, w.idx, w.dist, w.second, w.clip};
                if (ccsx_cdna_reads_host(set.get(), &D.opts, seq.data(), off.data(), len.data(), m, &rep)) { fprintf(stderr, "host rule: %s\n", g_err.c_str()); return 1; }
                const int32_t *gp[12] = {g.tested, g.cls, g.strand, g.start, g.end, g.polya_len, g.n_internal, g.first_internal, g.idx, g.dist, g.second, g.clip};
                const int32_t *wp[12] = {w.tested, w.cls, w.strand, w.start, w.end, w.polya_len, w.n_internal, w.first_internal, w.idx, w.dist, w.second, w.clip};
                for (int k = 0; k < 12; ++k)
                    if (memcmp(gp[k], wp[k], (size_t)m * (k < 8 ? 4 : 8))) { fprintf(stderr, "array %d differs from the host rule\n", k); return 1; }
                for (int z = 0; z < n; ++z) ++cls[g.cls[z] >= 0 && g.cls[z] <= 6 ? g.cls[z] : 0];
            } else us.push_back(ms * 1e3);
        }
        std::sort(us.begin(), us.end());
        const double steps = (double)n * 2 * np * L;
        printf("k_cdna alone: %d reads of %d bases, %2d primers of %d bases, tails of %d: median %9.1f us (min %.1f, max %.1f) over %d launches = %.1f G column steps/s in "
               "phase C; %ld full-length reads, %ld concatemers, %ld others; the first 512 reads equal the host rule\n", n, L, np, M, TAIL, us[us.size() / 2], us.front(),
               us.back(), rounds, steps / (us[us.size() / 2] * 1e3), cls[6], cls[4], (long)n - cls[6] - cls[4]);
    }
    return 0;
}

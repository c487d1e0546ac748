// kernel_bench — k_barcode alone: reads resident in HBM, timed with HIP events (tools/barcode_bench.py builds and runs it).
// usage: kernel_bench [reads = 16384] [read length = 10000] [rounds = 7]
// Random reads and random barcode sets (16-mers); per configuration — 96 and 384 barcodes, windows 64 and 256 — one launch over all reads per round.  The
// report of the first round is compared with ccsx_barcode_reads_host on the first 512 reads.  One line per configuration.
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
#include "../../ccs_amd/csrc/ccsx_barcode.hip"
#include "../../ccs_amd/csrc/ccsx_barcode_api.cpp"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

static uint64_t rng_state = 0x2545f4914f6cdd1dull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 32); }

int main(int argc, char **argv)
{
    const int n = argc > 1 ? atoi(argv[1]) : 16384, L = argc > 2 ? atoi(argv[2]) : 10000, rounds = argc > 3 ? atoi(argv[3]) : 7;
    if (n < 1 || L < 1 || rounds < 1) { fprintf(stderr, "usage: kernel_bench [reads] [read length] [rounds]\n"); return 2; }
    std::vector<uint8_t> seq((size_t)n * L);
    for (auto &c : seq) c = (uint8_t)(rnd() & 3);
    std::vector<int64_t> off((size_t)n);
    std::vector<int32_t> len((size_t)n, L);
    for (int z = 0; z < n; ++z) off[z] = (int64_t)z * L;
    uint8_t *d_seq; int64_t *d_off; int32_t *d_len; unsigned long long *d_set;                  // d_set: the packed set, the report behind it
    CK(hipMalloc((void **)&d_seq, seq.size())); CK(hipMalloc((void **)&d_off, (size_t)n * 8)); CK(hipMalloc((void **)&d_len, (size_t)n * 4));
    CK(hipMalloc((void **)&d_set, ccsx_bc_set_words(CCSX_BARCODE_MAX) * 8 + ccsx_bc_rep_bytes((size_t)n)));
    CK(hipMemcpy(d_seq, seq.data(), seq.size(), hipMemcpyHostToDevice)); CK(hipMemcpy(d_off, off.data(), (size_t)n * 8, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_len, len.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    hipStream_t s; CK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    auto set = std::make_unique<ccsx_barcode_set>();
    for (int nb : {96, 384})
        for (int window : {64, 256}) {
            memset(set.get(), 0, sizeof *set);
            set->n_barcodes = nb;
            for (int b = 0; b < nb; ++b) { set->len[b] = 16; for (int i = 0; i < 16; ++i) set->seq[b][i] = (uint8_t)(rnd() & 3); }
            for (int z = 0; L >= 32 && z < 512 && z < n; z += 2) memcpy(&seq[(size_t)z * L + (z % 5)], set->seq[z % nb], 16);      // (some planted, so the check sees calls)
            CK(hipMemcpy(d_seq, seq.data(), std::min(seq.size(), (size_t)512 * L), hipMemcpyHostToDevice));
            std::vector<unsigned long long> packed(ccsx_bc_set_words(nb), 0ull);
            ccsx_bc_pack(set.get(), packed.data());
            CK(hipMemcpy(d_set, packed.data(), packed.size() * 8, hipMemcpyHostToDevice));
            BarcodeParams B{};
            ccsx_barcode_opts_default(&B.opts);
            B.opts.window = window;
            B.n = n; B.n_barcodes = nb; B.seq = d_seq; B.seq_off = d_off; B.seq_len = d_len;
            ccsx_bc_bind(B, d_set);
            std::vector<double> us;
            for (int r = 0; r <= rounds; ++r) {                      // round 0 warms up and is checked
                CK(hipEventRecord(e0, s));
                if (const char *failed = ccsx_barcode_launch(B, s)) { fprintf(stderr, "launch failed: %s\n", failed); return 1; }
                CK(hipEventRecord(e1, s));
                CK(hipEventSynchronize(e1));
                float ms = 0; CK(hipEventElapsedTime(&ms, e0, e1));
                if (r == 0) {
                    const int m = std::min(n, 512);
                    std::vector<int32_t> got((size_t)n * CCSX_BC_PLANES), want((size_t)m * CCSX_BC_PLANES);
                    CK(hipMemcpy(got.data(), B.rep, got.size() * 4, hipMemcpyDeviceToHost));
                    const BarcodeOut g = ccsx_bc_out(got.data(), (size_t)n), w = ccsx_bc_out(want.data(), (size_t)m);
                    ccsx_barcode_report rep{m, w.tested, w.call, w.bq, w.idx, w.dist, w.second, w.clip};
                    if (ccsx_barcode_reads_host(set.get(), &B.opts, seq.data(), off.data(), len.data(), m, &rep)) { fprintf(stderr, "host rule: %s\n", g_err.c_str()); return 1; }
                    const int32_t *gp[7] = {g.tested, g.call, g.bq, g.idx, g.dist, g.second, g.clip}, *wp[7] = {w.tested, w.call, w.bq, w.idx, w.dist, w.second, w.clip};
                    for (int k = 0; k < 7; ++k)
                        if (memcmp(gp[k], wp[k], (size_t)m * (k < 3 ? 1 : 2) * 4)) { fprintf(stderr, "field %d differs from the host rule\n", k); return 1; }
                } else us.push_back(ms * 1e3);
            }
            std::sort(us.begin(), us.end());
            const double steps = (double)n * 2 * nb * std::min(window, L);
            printf("k_barcode alone: %d reads of %d bases, %3d barcodes, window %3d: median %8.1f us (min %.1f, max %.1f) over %d rounds = %.1f G column steps/s; the first 512 reads "
                   "equal the host rule\n", n, L, nb, window, us[us.size() / 2], us.front(), us.back(), rounds, steps / (us[us.size() / 2] * 1e3));
        }
    return 0;
}

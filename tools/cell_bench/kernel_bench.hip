// kernel_bench — k_cell alone, beside k_cdna on the same reads in the same process: reads resident in HBM, timed with HIP events (tools/cell_bench.py builds and
// runs it; k_cdna comes from cdna_unit.hip, a translation unit of its own, since both kernels' files name their helpers alike).
// usage: kernel_bench [reads = 16384] [read length = 10000] [rounds = 7]
// Every read is 5p . random insert . A x 30 . rc(barcode . UMI) . rc(3p), the default design (12 U, 16 B at the 3' primer, the barcode next to it), with the two
// primers of the set, every second one reverse complemented; the barcode is a member of the whitelist, in every fourth read with a substitution, in every
// sixteenth with a lost base, in every 64th nobody's.  Whitelists of 4096 and 2^23 barcodes (ccsx_dup_hash of 0 .. n - 1: distinct, since the hash is a
// bijection).  One launch over all reads per round; the report of the first round is compared with ccsx_cell_reads_host on the first 512 reads.
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
#include "../../ccs_amd/csrc/ccsx_cell.hip"
#include "../../ccs_amd/csrc/ccsx_barcode_api.cpp"
#include "../../ccs_amd/csrc/ccsx_cdna_api.cpp"
#include "../../ccs_amd/csrc/ccsx_cell_api.cpp"
const char *ccsx_cdna_launch(const CdnaParams &D, hipStream_t st);   // cdna_unit.hip

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

static uint64_t rng_state = 0x2545f4914f6cdd1dull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 32); }

int main(int argc, char **argv)
{
    const int n = argc > 1 ? atoi(argv[1]) : 16384, L = argc > 2 ? atoi(argv[2]) : 10000, rounds = argc > 3 ? atoi(argv[3]) : 7, M = 25, TAIL = 30, B = 16, U = 12;
    if (n < 1 || L < 1000 || rounds < 1) { fprintf(stderr, "usage: kernel_bench [reads] [read length >= 1000] [rounds]\n"); return 2; }
    std::vector<uint8_t> seq((size_t)n * L);
    std::vector<int64_t> off((size_t)n);
    std::vector<int32_t> len((size_t)n, L);
    for (int z = 0; z < n; ++z) off[z] = (int64_t)z * L;
    const size_t rep_bytes = ccsx_cl_rep_bytes((size_t)n);
    uint8_t *d_seq; int64_t *d_off; int32_t *d_len; unsigned long long *d_set, *d_table;        // d_set: the packed set, the report behind it
    CK(hipMalloc((void **)&d_seq, seq.size())); CK(hipMalloc((void **)&d_off, (size_t)n * 8)); CK(hipMalloc((void **)&d_len, (size_t)n * 4));
    CK(hipMalloc((void **)&d_set, ccsx_cd_set_words(2) * 8 + rep_bytes));
    CK(hipMalloc((void **)&d_table, (size_t)ccsx_cl_n_slots(CCSX_CELL_MAX_WHITELIST) * 8));
    CK(hipMemcpy(d_off, off.data(), (size_t)n * 8, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_len, len.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    hipStream_t s; CK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    auto set = std::make_unique<ccsx_cdna_set>();
    memset(set.get(), 0, sizeof *set);
    set->n_primers = 2;
    for (int b = 0; b < 2; ++b) { set->len[b] = M; set->role[b] = (uint8_t)b; for (int i = 0; i < M; ++i) set->seq[b][i] = (uint8_t)(rnd() & 3); }
    std::vector<unsigned long long> packed(ccsx_cd_set_words(2), 0ull);
    ccsx_cd_pack(set.get(), packed.data());
    CK(hipMemcpy(d_set, packed.data(), packed.size() * 8, hipMemcpyHostToDevice));
    ccsx_cell_design design;
    ccsx_cell_design_default(&design);
    for (int nw : {4096, CCSX_CELL_MAX_WHITELIST}) {
        std::vector<uint8_t> codes((size_t)nw * B);
        for (int k = 0; k < nw; ++k) { const uint32_t x = ccsx_dup_hash32((uint32_t)k); for (int j = 0; j < B; ++j) codes[(size_t)k * B + j] = (uint8_t)((x >> (2 * (B - 1 - j))) & 3); }
        ccsx_cell_whitelist *wl = ccsx_cell_whitelist_create(codes.data(), nw, B);
        if (!wl) { fprintf(stderr, "whitelist: %s\n", g_err.c_str()); return 1; }
        CK(hipMemcpy(d_table, wl->table, (size_t)wl->slots * 8, hipMemcpyHostToDevice));
        for (int z = 0; z < n; ++z) {
            uint8_t *c = &seq[(size_t)z * L], f[B + U + 1];
            for (int i = 0; i < L; ++i) c[i] = (uint8_t)(rnd() & 3);
            memcpy(c, set->seq[0], M);
            int nf = 0;
            const uint8_t *w = &codes[(size_t)(rnd() % (uint32_t)nw) * B];
            const int lost = z % 16 == 15 ? (int)(rnd() % B) : -1;
            for (int j = 0; j < B; ++j) if (j != lost) f[nf++] = z % 64 == 63 ? (uint8_t)(rnd() & 3) : w[j];
            if (z % 4 == 3 && lost < 0) f[rnd() % B] ^= 2;
            for (int j = 0; j < U; ++j) f[nf++] = (uint8_t)(rnd() & 3);
            uint8_t *p = c + L - M - nf - TAIL;                      // . A x 30 . rc(fields) . rc(3p)
            p[-1] = 1; p[-2] = 2;                                    // the insert ends in two bases other than A
            memset(p, 0, TAIL);
            for (int i = 0; i < nf; ++i) p[TAIL + i] = (uint8_t)(3 - f[nf - 1 - i]);
            for (int i = 0; i < M; ++i) c[L - M + i] = (uint8_t)(3 - set->seq[1][M - 1 - i]);
            if (z & 1) { std::reverse(c, c + L); for (int i = 0; i < L; ++i) c[i] = (uint8_t)(3 - c[i]); }
        }
        CK(hipMemcpy(d_seq, seq.data(), seq.size(), hipMemcpyHostToDevice));
        CellParams C{};
        ccsx_cdna_opts_default(&C.D.opts);
        C.D.n = n; C.D.n_primers = 2; C.D.seq = d_seq; C.D.seq_off = d_off; C.D.seq_len = d_len;
        ccsx_cd_bind(C.D, d_set);
        C.design = design; C.table = d_table; C.slots = wl->slots;
        std::vector<double> us[2];                                   // k_cell, k_cdna
        long tags[6] = {0, 0, 0, 0, 0, 0}, full = 0;
        for (int r = 0; r <= rounds; ++r) {                          // round 0 warms up and is checked
            for (int which = 0; which < 2; ++which) {
                CK(hipEventRecord(e0, s));
                if (const char *failed = which ? ccsx_cdna_launch(C.D, s) : ccsx_cell_launch(C, s)) { fprintf(stderr, "launch failed: %s\n", failed); return 1; }
                CK(hipEventRecord(e1, s));
                CK(hipEventSynchronize(e1));
                float ms = 0; CK(hipEventElapsedTime(&ms, e0, e1));
                if (r) us[which].push_back(ms * 1e3);
                if (r == 0 && which == 0) {
                    const int m = std::min(n, 512);
                    std::vector<uint8_t> got(rep_bytes), want(ccsx_cl_rep_bytes((size_t)m));
                    CK(hipMemcpy(got.data(), C.D.rep, rep_bytes, hipMemcpyDeviceToHost));
                    const CellOut g = ccsx_cl_out((int32_t *)got.data(), (size_t)n), w = ccsx_cl_out((int32_t *)want.data(), (size_t)m);
                    ccsx_cell_report rep{ccsx_cdna_report{m, w.cd.tested, w.cd.cls, w.cd.strand, w.cd.start, w.cd.end, w.cd.polya_len, w.cd.n_internal, w.cd.first_internal, w.cd.idx,
                                                          w.cd.dist, w.cd.second, w.cd.clip}, w.tag, w.bc_raw, w.bc, w.bc_hi, w.kind, w.shift, w.umi, w.tag_clip};
                    if (ccsx_cell_reads_host(set.get(), &C.D.opts, &design, wl, seq.data(), off.data(), len.data(), m, &rep)) { fprintf(stderr, "host rule: %s\n", g_err.c_str()); return 1; }
                    const void *gp[20] = {g.cd.tested, g.cd.cls, g.cd.strand, g.cd.start, g.cd.end, g.cd.polya_len, g.cd.n_internal, g.cd.first_internal, g.cd.idx, g.cd.dist,
                                          g.cd.second, g.cd.clip, g.tag, g.bc_raw, g.bc, g.bc_hi, g.kind, g.shift, g.umi, g.tag_clip};
                    const void *wp[20] = {w.cd.tested, w.cd.cls, w.cd.strand, w.cd.start, w.cd.end, w.cd.polya_len, w.cd.n_internal, w.cd.first_internal, w.cd.idx, w.cd.dist,
                                          w.cd.second, w.cd.clip, w.tag, w.bc_raw, w.bc, w.bc_hi, w.kind, w.shift, w.umi, w.tag_clip};
                    for (int k = 0; k < 20; ++k)
                        if (memcmp(gp[k], wp[k], (size_t)m * (k >= 8 && k < 12 ? 8 : 4))) { fprintf(stderr, "array %d differs from the host rule\n", k); return 1; }
                    for (int z = 0; z < n; ++z) { ++tags[g.tag[z] >= 0 && g.tag[z] <= 5 ? g.tag[z] : 0]; full += g.cd.cls[z] == CCSX_CDNA_FULL_LENGTH; }
                }
            }
        }
        for (auto &v : us) std::sort(v.begin(), v.end());
        const double mc = us[0][us[0].size() / 2], md = us[1][us[1].size() / 2];
        printf("k_cell alone: %d reads of %d bases, 2 primers of %d bases, 12 U + 16 B, whitelist of %7d: median %9.1f us (min %.1f, max %.1f) over %d launches; k_cdna on "
               "the same reads in the same process: median %9.1f us (min %.1f, max %.1f); ratio of the medians %.3f; %ld full-length reads; tags exact %ld, corrected %ld, "
               "ambiguous %ld, absent %ld; the first 512 reads equal the host rule\n", n, L, M, nw, mc, us[0].front(), us[0].back(), rounds, md, us[1].front(), us[1].back(),
               mc / md, full, tags[2], tags[3], tags[4], tags[5]);
        ccsx_cell_whitelist_destroy(wl);
    }
    return 0;
}

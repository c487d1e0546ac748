// barcode_sanitize — ccsx_barcode_reads_host (ccs_amd/csrc/ccsx_barcode_api.cpp over barcode_core.h: the walk and the call k_barcode runs) under AddressSanitizer +
// UndefinedBehaviorSanitizer, on the CPU.  Reads the case file tools/barcode_sanitize.py writes (every set and read of the tests' limit set, with the report the
// restatement expects): each read lives in a heap block of exactly its length and every report array in one of exactly n (or 2 n) words, so one access out of
// range is a report; the result is compared with the expected one, field for field.  Then seeded random sets and reads of its own, lengths and windows at their
// limits, twice each (the same bytes), and the argument errors.  Exit 0 = all of that held; a sanitizer report aborts.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

static std::string g_err;
void ccsx_set_error(const std::string &s) { g_err = s; }
#include "ccsx_barcode_api.cpp"

struct Report {
    int32_t n;
    int32_t *p[7];
    explicit Report(int32_t n_) : n(n_) { for (int k = 0; k < 7; ++k) p[k] = (int32_t *)malloc(((size_t)n * (k < 3 ? 1 : 2) + 0) * 4 + (n ? 0 : 1)); }
    ~Report() { for (auto q : p) free(q); }
    ccsx_barcode_report c() { return ccsx_barcode_report{n, p[0], p[1], p[2], p[3], p[4], p[5], p[6]}; }
    size_t words(int k) const { return (size_t)n * (k < 3 ? 1 : 2); }
};

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 32); }

// the reads packed behind one another in a block of exactly their total length
static int run(const ccsx_barcode_set &set, const ccsx_barcode_opts &o, const std::vector<std::vector<uint8_t>> &reads, Report &rep)
{
    size_t total = 0;
    for (auto &r : reads) total += r.size();
    uint8_t *seq = (uint8_t *)malloc(total ? total : 1);
    std::vector<int64_t> off(reads.size());
    std::vector<int32_t> len(reads.size());
    size_t at = 0;
    for (size_t z = 0; z < reads.size(); ++z) {
        off[z] = (int64_t)at; len[z] = (int32_t)reads[z].size();
        if (len[z]) memcpy(seq + at, reads[z].data(), reads[z].size());
        at += reads[z].size();
    }
    ccsx_barcode_report c = rep.c();
    const int rc = ccsx_barcode_reads_host(&set, &o, total ? seq : nullptr, off.data(), len.data(), (int32_t)reads.size(), &c);
    free(seq);
    return rc;
}

template <typename T> static bool rd(FILE *f, T *v, size_t n = 1) { return fread(v, sizeof(T), n, f) == n; }

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: barcode_sanitize CASES.bin\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    long n_cases = 0, n_reads = 0;
    auto set = std::make_unique<ccsx_barcode_set>();
    int32_t hdr[5];                                                  // n_barcodes, window, max_dist_pct, min_margin, n_reads
    while (rd(f, hdr, 5)) {
        memset(set.get(), 0, sizeof *set);
        set->n_barcodes = hdr[0];
        for (int b = 0; b < hdr[0]; ++b) {
            if (!rd(f, &set->len[b]) || set->len[b] < 0 || set->len[b] > CCSX_BARCODE_MAX_LEN || !rd(f, set->seq[b], (size_t)set->len[b])) { fprintf(stderr, "bad case file\n"); return 2; }
        }
        const ccsx_barcode_opts o{hdr[1], hdr[2], hdr[3]};
        std::vector<std::vector<uint8_t>> reads((size_t)hdr[4]);
        for (auto &r : reads) {
            int32_t L;
            if (!rd(f, &L) || L < 0) { fprintf(stderr, "bad case file\n"); return 2; }
            r.resize((size_t)L);
            if (L && !rd(f, r.data(), (size_t)L)) { fprintf(stderr, "bad case file\n"); return 2; }
        }
        Report got(hdr[4]), want(hdr[4]);
        for (int k = 0; k < 7; ++k)
            if (want.words(k) && !rd(f, want.p[k], want.words(k))) { fprintf(stderr, "bad case file\n"); return 2; }
        if (run(*set, o, reads, got) != 0) { fprintf(stderr, "case %ld refused: %s\n", n_cases, g_err.c_str()); return 3; }
        for (int k = 0; k < 7; ++k)
            if (got.words(k) && memcmp(got.p[k], want.p[k], got.words(k) * 4)) { fprintf(stderr, "case %ld: field %d differs from the restatement\n", n_cases, k); return 3; }
        ++n_cases; n_reads += hdr[4];
    }
    fclose(f);
    // seeded random sets and reads: lengths 8 .. 64, windows 8 .. 1024, reads of 0 .. 1100 bases, bytes of any value (only the low two bits are read)
    long n_random = 0;
    for (int it = 0; it < 300; ++it) {
        memset(set.get(), 0, sizeof *set);
        set->n_barcodes = it % 7 == 0 ? CCSX_BARCODE_MAX : 1 + (int32_t)(rnd() % 40);
        for (int b = 0; b < set->n_barcodes; ++b) {
            set->len[b] = (it & 1) ? (b & 1 ? CCSX_BARCODE_MAX_LEN : CCSX_BARCODE_MIN_LEN) : CCSX_BARCODE_MIN_LEN + (int32_t)(rnd() % 57);
            for (int i = 0; i < set->len[b]; ++i) set->seq[b][i] = (uint8_t)(rnd() & 3);
        }
        const ccsx_barcode_opts o{it % 5 == 0 ? CCSX_BARCODE_MAX_WINDOW : (it % 5 == 1 ? 8 : 8 + (int32_t)(rnd() % 1017)), (int32_t)(rnd() % 31), (int32_t)(rnd() % 65)};
        std::vector<std::vector<uint8_t>> reads(1 + rnd() % 6);
        for (auto &r : reads) { r.resize(rnd() % 5 == 0 ? rnd() % 9 : rnd() % 1101); for (auto &c : r) c = (uint8_t)rnd(); }
        Report a((int32_t)reads.size()), b((int32_t)reads.size());
        if (run(*set, o, reads, a) != 0 || run(*set, o, reads, b) != 0) { fprintf(stderr, "random case %d refused: %s\n", it, g_err.c_str()); return 3; }
        for (int k = 0; k < 7; ++k)
            if (a.words(k) && memcmp(a.p[k], b.p[k], a.words(k) * 4)) { fprintf(stderr, "random case %d: two runs differ in field %d\n", it, k); return 3; }
        for (size_t z = 0; z < reads.size(); ++z) {
            const bool tested = !reads[z].empty();
            if (a.p[0][z] != (tested ? 1 : 0) || a.p[1][z] < 0 || a.p[1][z] > 3 || a.p[2][z] < -1 || a.p[2][z] > 100) { fprintf(stderr, "random case %d: read %zu out of range\n", it, z); return 3; }
            for (int e = 0; e < 2 && tested; ++e) {
                const int32_t idx = a.p[3][2 * z + e], dist = a.p[4][2 * z + e], clip = a.p[6][2 * z + e];
                if (idx < 0 || idx >= set->n_barcodes || dist < 0 || dist > set->len[idx] || clip < 0 || clip > o.window || clip > (int32_t)reads[z].size()) {
                    fprintf(stderr, "random case %d: read %zu end %d out of range\n", it, z, e); return 3;
                }
            }
        }
        ++n_random;
    }
    // argument errors leave the report alone and name their cause
    {
        memset(set.get(), 0, sizeof *set);
        set->n_barcodes = 1; set->len[0] = 8;
        const ccsx_barcode_opts o{64, 20, 1};
        std::vector<std::vector<uint8_t>> reads(2, std::vector<uint8_t>(30, 1));
        Report r(2);
        set->len[0] = 65;
        if (run(*set, o, reads, r) == 0 || g_err.find("length outside") == std::string::npos) { fprintf(stderr, "length 65 was not refused\n"); return 3; }
        set->len[0] = 8; set->n_barcodes = CCSX_BARCODE_MAX + 1;
        if (run(*set, o, reads, r) == 0 || g_err.find("n_barcodes") == std::string::npos) { fprintf(stderr, "385 barcodes were not refused\n"); return 3; }
        set->n_barcodes = 1; set->seq[0][7] = 4;
        if (run(*set, o, reads, r) == 0 || g_err.find("code above 3") == std::string::npos) { fprintf(stderr, "code 4 was not refused\n"); return 3; }
    }
    printf("barcode_sanitize: %ld cases of the limit set (%ld reads) equal the restatement, %ld random cases twice; clean\n", n_cases, n_reads, n_random);
    return 0;
}

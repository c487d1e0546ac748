// cdna_sanitize — ccsx_cdna_reads_host and ccsx_cdna_check (ccs_amd/csrc/ccsx_cdna_api.cpp over cdna_core.h, barcode_core.h and segment_core.h: the walks, the
// scan and the classes k_cdna runs) under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU.  Reads the case file tools/cdna_sanitize.py writes (every set
// and read of the tests' limit set, with the report the restatement expects): the reads live in a heap block of exactly their length and every plane in one of
// exactly n or 2 n words, so one access out of range is a report; the result is compared with the expected one, field for field.  Then seeded random sets and
// reads of its own, lengths and options at their limits, twice each (the same bytes), and the argument errors.  Exit 0 = all of that held; a sanitizer report
// aborts.
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
#include "ccsx_cdna_api.cpp"

constexpr int NP = 12;                                               // the report's arrays: eight of n words, four of 2 n
struct Report {
    int32_t n;
    int32_t *p[NP];
    static size_t words(int k, int32_t n) { return (size_t)n * (k < 8 ? 1 : 2); }
    explicit Report(int32_t n_) : n(n_)
    {
        for (int k = 0; k < NP; ++k) { p[k] = (int32_t *)malloc(words(k, n) * 4 + (n ? 0 : 1)); memset(p[k], 0xA5, words(k, n) * 4); }
    }
    ~Report() { for (auto q : p) free(q); }
    ccsx_cdna_report c() { return ccsx_cdna_report{n, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], p[10], p[11]}; }
};

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 32); }

// the reads packed behind one another in a block of exactly their total length
static int run(const ccsx_cdna_set &set, const ccsx_cdna_opts &o, const std::vector<std::vector<uint8_t>> &reads, Report &rep)
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
    ccsx_cdna_report c = rep.c();
    const int rc = ccsx_cdna_reads_host(&set, &o, total ? seq : nullptr, off.data(), len.data(), (int32_t)reads.size(), &c);
    free(seq);
    return rc;
}

template <typename T> static bool rd(FILE *f, T *v, size_t n = 1) { return fread(v, sizeof(T), n, f) == n; }

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: cdna_sanitize CASES.bin\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    long n_cases = 0, n_reads = 0;
    auto set = std::make_unique<ccsx_cdna_set>();
    int32_t hdr[10];                                                 // n_primers, n_reads, then the eight options in the struct's order
    while (rd(f, hdr, 10)) {
        memset(set.get(), 0, sizeof *set);
        set->n_primers = hdr[0];
        for (int b = 0; b < hdr[0]; ++b) {
            int32_t role;
            if (!rd(f, &set->len[b]) || !rd(f, &role) || set->len[b] < 0 || set->len[b] > CCSX_CDNA_MAX_LEN || !rd(f, set->seq[b], (size_t)set->len[b])) { fprintf(stderr, "bad case file\n"); return 2; }
            set->role[b] = (uint8_t)role;
        }
        const ccsx_cdna_opts o{hdr[2], hdr[3], hdr[4], hdr[5], hdr[6], hdr[7], hdr[8], hdr[9]};
        std::vector<std::vector<uint8_t>> reads((size_t)hdr[1]);
        for (auto &r : reads) {
            int32_t L;
            if (!rd(f, &L) || L < 0) { fprintf(stderr, "bad case file\n"); return 2; }
            r.resize((size_t)L);
            if (L && !rd(f, r.data(), (size_t)L)) { fprintf(stderr, "bad case file\n"); return 2; }
        }
        Report got(hdr[1]), want(hdr[1]);
        for (int k = 0; k < NP; ++k)
            if (hdr[1] && !rd(f, want.p[k], Report::words(k, hdr[1]))) { fprintf(stderr, "bad case file\n"); return 2; }
        if (run(*set, o, reads, got) != 0) { fprintf(stderr, "case %ld refused: %s\n", n_cases, g_err.c_str()); return 3; }
        for (int k = 0; k < NP; ++k)
            if (hdr[1] && memcmp(got.p[k], want.p[k], Report::words(k, hdr[1]) * 4)) { fprintf(stderr, "case %ld: array %d differs from the restatement\n", n_cases, k); return 3; }
        ++n_cases; n_reads += hdr[1];
    }
    fclose(f);
    // seeded random sets and reads: 2 .. 64 primers of 8 .. 64 bases; reads of 0 .. 3000 bases that are random bytes (only the low two bits are read), a
    // two-letter alphabet (many chance hits), or primers of the set at both ends, on either strand, around inserts that hold runs of A or T and further primers
    long n_random = 0, n_full = 0, n_concat = 0;
    for (int it = 0; it < 300; ++it) {
        memset(set.get(), 0, sizeof *set);
        set->n_primers = it % 7 == 0 ? CCSX_CDNA_MAX_PRIMERS : 2 + (int32_t)(rnd() % 8);
        for (int b = 0; b < set->n_primers; ++b) {
            set->len[b] = (it & 1) ? (b & 1 ? CCSX_CDNA_MAX_LEN : CCSX_CDNA_MIN_LEN) : CCSX_CDNA_MIN_LEN + (int32_t)(rnd() % 57);
            set->role[b] = (uint8_t)(b == 0 ? 0 : b == 1 ? 1 : rnd() & 1);
            for (int i = 0; i < set->len[b]; ++i) set->seq[b][i] = (uint8_t)(rnd() & 3);
        }
        const ccsx_cdna_opts o{it % 3 == 0 ? 8 : it % 3 == 1 ? 1024 : 8 + (int32_t)(rnd() % 200), (int32_t)(rnd() % 31), (int32_t)(rnd() % 3), 1 + (int32_t)(rnd() % 8),
                               it % 4 == 0 ? 0 : it % 4 == 1 ? 64 : (int32_t)(rnd() % 10), it % 5 == 0 ? 16 : it % 5 == 1 ? 4096 : 16 + (int32_t)(rnd() % 600),
                               (int32_t)(rnd() % 40), it % 6 == 0 ? 65535 : 1 + (int32_t)(rnd() % 100)};
        std::vector<std::vector<uint8_t>> reads(1 + rnd() % 5);
        for (auto &r : reads) {
            const uint32_t kind = rnd() % 4;
            if (kind == 0) { r.resize(rnd() % 9); for (auto &c : r) c = (uint8_t)rnd(); }
            else if (kind == 1) { r.resize(rnd() % 3001); for (auto &c : r) c = (uint8_t)(rnd() & 0xfc); if (rnd() & 1) for (auto &c : r) c |= 3; }   // all A, or all T
            else {
                const auto put = [&](int b, bool rc) { const int m = set->len[b]; for (int i = 0; i < m; ++i) r.push_back((uint8_t)((rc ? 3 - set->seq[b][m - 1 - i] : set->seq[b][i]) | (rnd() & 0xfc))); };
                const bool anti = rnd() & 1;
                const int pieces = 1 + (int)(rnd() % (kind == 2 ? 1 : 4));
                put(anti ? 1 : 0, false);
                for (int q = 0; q < pieces; ++q) {
                    if (q) put((int)(rnd() % (uint32_t)set->n_primers), rnd() & 1);
                    for (uint32_t g = rnd() % 400; g; --g) r.push_back((uint8_t)rnd());
                    for (uint32_t g = rnd() % 150; g; --g) r.push_back((uint8_t)(rnd() % 16 ? (anti ? 3 : 0) : rnd()));
                }
                put(anti ? 0 : 1, true);
            }
        }
        Report a((int32_t)reads.size()), b((int32_t)reads.size());
        if (run(*set, o, reads, a) != 0 || run(*set, o, reads, b) != 0) { fprintf(stderr, "random case %d refused: %s\n", it, g_err.c_str()); return 3; }
        for (int k = 0; k < NP; ++k)
            if (memcmp(a.p[k], b.p[k], Report::words(k, a.n) * 4)) { fprintf(stderr, "random case %d: two runs differ in array %d\n", it, k); return 3; }
        for (size_t z = 0; z < reads.size(); ++z) {
            const int32_t L = (int32_t)reads[z].size(), tested = a.p[0][z], cls = a.p[1][z], strand = a.p[2][z], start = a.p[3][z], end = a.p[4][z], tail = a.p[5][z],
                          ni = a.p[6][z], first = a.p[7][z];
            bool ok = tested == (L > 0) && cls >= 0 && cls <= CCSX_CDNA_FULL_LENGTH && strand >= -1 && strand <= 1 && (strand < 0) == (cls <= CCSX_CDNA_SAME_ROLE) &&
                      tail >= 0 && tail <= o.polya_max && tail <= L && ni >= 0 && (ni > 0) == (first >= 0) && first < L && start >= 0 && end >= start && end <= L &&
                      (cls >= CCSX_CDNA_CONCATEMER ? end - start >= o.min_len : end == 0) && (cls != CCSX_CDNA_CONCATEMER || ni > 0);
            for (int e = 0; e < 2 && ok; ++e) {
                const int32_t idx = a.p[8][2 * z + e], clip = a.p[11][2 * z + e];
                ok = L > 0 ? idx >= 0 && idx < set->n_primers && clip >= 0 && clip <= (L < o.window ? L : o.window) : idx == -1 && clip == 0;
            }
            if (!ok) { fprintf(stderr, "random case %d: read %zu out of range\n", it, z); return 3; }
            n_full += cls == CCSX_CDNA_FULL_LENGTH; n_concat += cls == CCSX_CDNA_CONCATEMER;
        }
        ++n_random;
    }
    // argument errors name their cause
    {
        memset(set.get(), 0, sizeof *set);
        set->n_primers = 2; set->len[0] = 8; set->len[1] = 8; set->role[1] = 1;
        ccsx_cdna_opts o;
        ccsx_cdna_opts_default(&o);
        std::vector<std::vector<uint8_t>> reads(2, std::vector<uint8_t>(30, 1));
        Report r(2);
        if (run(*set, o, reads, r) != 0) { fprintf(stderr, "a valid call was refused: %s\n", g_err.c_str()); return 3; }
        set->len[1] = 65;
        if (run(*set, o, reads, r) == 0 || g_err.find("primer 1: length outside") == std::string::npos) { fprintf(stderr, "length 65 was not refused\n"); return 3; }
        set->len[1] = 8; set->n_primers = CCSX_CDNA_MAX_PRIMERS + 1;
        if (run(*set, o, reads, r) == 0 || g_err.find("n_primers") == std::string::npos) { fprintf(stderr, "65 primers were not refused\n"); return 3; }
        set->n_primers = 2; set->seq[0][7] = 4;
        if (run(*set, o, reads, r) == 0 || g_err.find("primer 0: code above 3") == std::string::npos) { fprintf(stderr, "code 4 was not refused\n"); return 3; }
        set->seq[0][7] = 0; set->role[1] = 2;
        if (run(*set, o, reads, r) == 0 || g_err.find("primer 1: role above 1") == std::string::npos) { fprintf(stderr, "role 2 was not refused\n"); return 3; }
        set->role[1] = 0;
        if (run(*set, o, reads, r) == 0 || g_err.find("needs a primer of role") == std::string::npos) { fprintf(stderr, "a set of one role was not refused\n"); return 3; }
        set->role[1] = 1; o.polya_max = 4097;
        if (run(*set, o, reads, r) == 0 || g_err.find("options out of range") == std::string::npos) { fprintf(stderr, "polya_max 4097 was not refused\n"); return 3; }
    }
    printf("cdna_sanitize: %ld cases of the limit set (%ld reads) equal the restatement, %ld random cases twice (%ld full-length reads, %ld concatemers); clean\n",
           n_cases, n_reads, n_random, n_full, n_concat);
    return 0;
}

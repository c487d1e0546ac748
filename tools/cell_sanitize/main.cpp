// cell_sanitize — ccsx_cell_reads_host, ccsx_cell_whitelist_create and ccsx_cell_check (ccs_amd/csrc/ccsx_cell_api.cpp over cell_core.h and cdna_core.h: the
// fields, the candidates, the probes and the classes k_cell runs) under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU.  Reads the case file
// tools/cell_sanitize.py writes (every case of the tests' limit set, with the report the restatement expects): the reads live in a heap block of exactly their
// length, the whitelist's codes in one of exactly n x bc_len bytes and every plane in one of exactly n or 2 n words, so one access out of range is a report; the
// result is compared with the expected one, field for field.  Then seeded random cases of its own, designs at their limits, twice each (the same bytes), and the
// argument errors.  Exit 0 = all of that held; a sanitizer report aborts.
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
#include "ccsx_cell_api.cpp"

constexpr int NP = 20;                                               // the report's arrays: eight of n words, four of 2 n, then the eight of the tag
struct Report {
    int32_t n;
    int32_t *p[NP];
    static size_t words(int k, int32_t n) { return (size_t)n * (k >= 8 && k < 12 ? 2 : 1); }
    explicit Report(int32_t n_) : n(n_)
    {
        for (int k = 0; k < NP; ++k) { p[k] = (int32_t *)malloc(words(k, n) * 4 + (n ? 0 : 1)); memset(p[k], 0xA5, words(k, n) * 4); }
    }
    ~Report() { for (auto q : p) free(q); }
    ccsx_cell_report c()
    {
        return ccsx_cell_report{ccsx_cdna_report{n, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], p[10], p[11]}, p[12], (uint32_t *)p[13], p[14], p[15], p[16],
                                p[17], (uint32_t *)p[18], p[19]};
    }
};
struct Whitelist {                                                   // the codes in a block of exactly their size; the object, freed with it
    uint8_t *codes = nullptr;
    ccsx_cell_whitelist *wl = nullptr;
    Whitelist(const std::vector<uint8_t> &c, int32_t n, int32_t b)
    {
        codes = (uint8_t *)malloc(c.size() ? c.size() : 1);
        if (!c.empty()) memcpy(codes, c.data(), c.size());
        wl = ccsx_cell_whitelist_create(codes, n, b);
    }
    ~Whitelist() { ccsx_cell_whitelist_destroy(wl); free(codes); }
};

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 32); }

// the reads packed behind one another in a block of exactly their total length
static int run(const ccsx_cdna_set &set, const ccsx_cdna_opts &o, const ccsx_cell_design *d, const ccsx_cell_whitelist *wl, const std::vector<std::vector<uint8_t>> &reads,
               Report &rep)
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
    ccsx_cell_report c = rep.c();
    const int rc = ccsx_cell_reads_host(&set, &o, d, wl, total ? seq : nullptr, off.data(), len.data(), (int32_t)reads.size(), &c);
    free(seq);
    return rc;
}

template <typename T> static bool rd(FILE *f, T *v, size_t n = 1) { return fread(v, sizeof(T), n, f) == n; }

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: cell_sanitize CASES.bin\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    long n_cases = 0, n_reads = 0;
    auto set = std::make_unique<ccsx_cdna_set>();
    int32_t hdr[16];                                                 // n_primers, n_reads, the eight options, the five members of the design, the whitelist's n or -1
    while (rd(f, hdr, 16)) {
        memset(set.get(), 0, sizeof *set);
        set->n_primers = hdr[0];
        for (int b = 0; b < hdr[0]; ++b) {
            int32_t role;
            if (!rd(f, &set->len[b]) || !rd(f, &role) || set->len[b] < 0 || set->len[b] > CCSX_CDNA_MAX_LEN || !rd(f, set->seq[b], (size_t)set->len[b])) { fprintf(stderr, "bad case file\n"); return 2; }
            set->role[b] = (uint8_t)role;
        }
        const ccsx_cdna_opts o{hdr[2], hdr[3], hdr[4], hdr[5], hdr[6], hdr[7], hdr[8], hdr[9]};
        const ccsx_cell_design d{hdr[10], hdr[11], hdr[12], hdr[13], hdr[14], {0, 0, 0}};
        std::unique_ptr<Whitelist> wl;
        if (hdr[15] >= 0) {
            std::vector<uint8_t> codes((size_t)hdr[15] * (size_t)d.bc_len);
            if (!codes.empty() && !rd(f, codes.data(), codes.size())) { fprintf(stderr, "bad case file\n"); return 2; }
            wl = std::make_unique<Whitelist>(codes, hdr[15], d.bc_len);
            if (!wl->wl) { fprintf(stderr, "case %ld: whitelist refused: %s\n", n_cases, g_err.c_str()); return 3; }
        }
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
        if (run(*set, o, &d, wl ? wl->wl : nullptr, reads, got) != 0) { fprintf(stderr, "case %ld refused: %s\n", n_cases, g_err.c_str()); return 3; }
        for (int k = 0; k < NP; ++k)
            if (hdr[1] && memcmp(got.p[k], want.p[k], Report::words(k, hdr[1]) * 4)) { fprintf(stderr, "case %ld: array %d differs from the restatement\n", n_cases, k); return 3; }
        ++n_cases; n_reads += hdr[1];
    }
    fclose(f);
    // seeded random cases: two primers of 8 .. 64 bases, designs from every corner (fields of 0 .. 16 bases, either side and order, with and without indels),
    // whitelists of 1 .. 3000 barcodes that are dense for short fields, reads that are random bytes, one letter, or molecules with the fields of a member of the
    // whitelist, as it is or with one edit, cut short at every distance from the fields
    long n_random = 0, n_listed = 0, n_ambiguous = 0;
    for (int it = 0; it < 300; ++it) {
        memset(set.get(), 0, sizeof *set);
        set->n_primers = 2;
        for (int b = 0; b < 2; ++b) {
            set->len[b] = (it & 1) ? (b & 1 ? CCSX_CDNA_MAX_LEN : CCSX_CDNA_MIN_LEN) : CCSX_CDNA_MIN_LEN + (int32_t)(rnd() % 57);
            set->role[b] = (uint8_t)b;
            for (int i = 0; i < set->len[b]; ++i) set->seq[b][i] = (uint8_t)(rnd() & 3);
        }
        ccsx_cdna_opts o;
        ccsx_cdna_opts_default(&o);
        o.min_len = 1 + (int32_t)(rnd() % 40); o.min_polya = (int32_t)(rnd() % 25); o.window = it % 3 == 0 ? 1024 : 64;
        ccsx_cell_design d{(int32_t)(rnd() % 17), it % 5 == 0 ? 16 : (int32_t)(rnd() % 17), (int32_t)(rnd() & 1), (int32_t)(rnd() & 1), (int32_t)(rnd() % 4 != 0), {0, 0, 0}};
        if (d.umi_len + d.bc_len == 0) d.umi_len = 1;
        const int T = d.umi_len + d.bc_len;
        std::unique_ptr<Whitelist> wl;
        std::vector<uint8_t> codes;
        int32_t nw = 0;
        if (d.bc_len > 0 && it % 6 != 0) {
            const uint64_t space = 1ull << (2 * d.bc_len);
            nw = (int32_t)(1 + rnd() % 3000);
            if ((uint64_t)nw > space) nw = (int32_t)space;
            // distinct barcodes: consecutive multiples of an odd stride, modulo the space (a bijection)
            const uint64_t stride = (rnd() | 1u), start = rnd();
            for (int32_t k = 0; k < nw; ++k) {
                const uint64_t x = (start + stride * (uint64_t)k) & (space - 1);
                for (int j = 0; j < d.bc_len; ++j) codes.push_back((uint8_t)((x >> (2 * (d.bc_len - 1 - j))) & 3));
            }
            wl = std::make_unique<Whitelist>(codes, nw, d.bc_len);
            if (!wl->wl) { fprintf(stderr, "random case %d: whitelist refused: %s\n", it, g_err.c_str()); return 3; }
        }
        std::vector<std::vector<uint8_t>> reads(1 + rnd() % 6);
        for (auto &r : reads) {
            const uint32_t kind = rnd() % 5;
            if (kind == 0) { r.resize(rnd() % 9); for (auto &c : r) c = (uint8_t)rnd(); }
            else if (kind == 1) { r.resize(rnd() % 1500); for (auto &c : r) c = (uint8_t)(rnd() & 0xfc); }
            else {
                std::vector<uint8_t> fields;                         // as they are read behind the design's primer
                std::vector<uint8_t> bc((size_t)d.bc_len), umi((size_t)d.umi_len);
                for (int j = 0; j < d.bc_len; ++j) bc[(size_t)j] = nw ? codes[(size_t)(rnd() % (uint32_t)nw) * (size_t)d.bc_len + (size_t)j] : (uint8_t)(rnd() & 3);
                for (auto &c : umi) c = (uint8_t)(rnd() & 3);
                const uint32_t e = rnd() % 4;
                if (!bc.empty() && e == 1) bc[rnd() % bc.size()] ^= 1;
                if (!bc.empty() && e == 2) bc.erase(bc.begin() + (long)(rnd() % bc.size()));
                if (!bc.empty() && e == 3) bc.insert(bc.begin() + (long)(rnd() % bc.size()), (uint8_t)(rnd() & 3));
                if (d.bc_first) { fields = bc; fields.insert(fields.end(), umi.begin(), umi.end()); }
                else { fields = umi; fields.insert(fields.end(), bc.begin(), bc.end()); }
                std::vector<uint8_t> insert(kind == 2 ? rnd() % 4 : rnd() % 300), tail(rnd() % 40, 0);
                for (auto &c : insert) c = (uint8_t)(rnd() & 3);
                if (kind == 3 && !fields.empty()) fields.resize(rnd() % fields.size());   // cut short: fewer than T bases behind the primer
                std::vector<uint8_t> sense;
                const auto put = [&](const std::vector<uint8_t> &v, bool rc) { for (size_t i = 0; i < v.size(); ++i) sense.push_back(rc ? (uint8_t)(3 - v[v.size() - 1 - i]) : v[i]); };
                const std::vector<uint8_t> p5(set->seq[0], set->seq[0] + set->len[0]), p3(set->seq[1], set->seq[1] + set->len[1]);
                put(p5, false);
                if (!d.side) put(fields, false);
                put(insert, false); put(tail, false);
                if (d.side) put(fields, true);
                put(p3, true);
                const bool anti = rnd() & 1;
                for (size_t i = 0; i < sense.size(); ++i) r.push_back((uint8_t)((anti ? 3 - sense[sense.size() - 1 - i] : sense[i]) | (rnd() & 0xfc)));
            }
        }
        Report a((int32_t)reads.size()), b((int32_t)reads.size());
        if (run(*set, o, &d, wl ? wl->wl : nullptr, reads, a) != 0 || run(*set, o, &d, wl ? wl->wl : nullptr, reads, b) != 0) {
            fprintf(stderr, "random case %d refused: %s\n", it, g_err.c_str()); return 3;
        }
        for (int k = 0; k < NP; ++k)
            if (memcmp(a.p[k], b.p[k], Report::words(k, a.n) * 4)) { fprintf(stderr, "random case %d: two runs differ in array %d\n", it, k); return 3; }
        for (size_t z = 0; z < reads.size(); ++z) {
            const int32_t L = (int32_t)reads[z].size(), cls = a.p[1][z], start = a.p[3][z], end = a.p[4][z], tag = a.p[12][z], bc = a.p[14][z], hi = a.p[15][z], kind = a.p[16][z],
                          shift = a.p[17][z], clip = a.p[19][z];
            bool ok = cls >= 0 && cls <= CCSX_CDNA_FULL_LENGTH && start >= 0 && end >= start && end <= L && tag >= CCSX_CELL_NONE && tag <= CCSX_CELL_ABSENT &&
                      (tag == CCSX_CELL_NONE ? clip == 0 && cls <= CCSX_CDNA_SHORT : clip == T + shift && cls >= CCSX_CDNA_SHORT) &&
                      (tag == CCSX_CELL_EXACT || tag == CCSX_CELL_CORRECTED ? bc >= 0 && bc < nw && hi == bc : tag == CCSX_CELL_AMBIGUOUS ? bc >= 0 && hi > bc && hi < nw : bc == -1 && hi == -1) &&
                      (tag == CCSX_CELL_CORRECTED ? kind >= 1 && kind <= (d.indels ? 3 : 1) && shift == (kind == 2 ? -1 : kind == 3 ? 1 : 0) : kind == 0 && shift == 0) &&
                      ((tag == CCSX_CELL_RAW) == (tag != CCSX_CELL_NONE && !wl));
            if (!ok) { fprintf(stderr, "random case %d: read %zu out of range (cls %d tag %d bc %d hi %d kind %d shift %d clip %d)\n", it, z, cls, tag, bc, hi, kind, shift, clip); return 3; }
            n_listed += tag == CCSX_CELL_EXACT || tag == CCSX_CELL_CORRECTED; n_ambiguous += tag == CCSX_CELL_AMBIGUOUS;
        }
        ++n_random;
    }
    // argument errors name their cause
    {
        memset(set.get(), 0, sizeof *set);
        set->n_primers = 2; set->len[0] = 8; set->len[1] = 8; set->role[1] = 1;
        ccsx_cdna_opts o;
        ccsx_cdna_opts_default(&o);
        ccsx_cell_design d;
        ccsx_cell_design_default(&d);
        std::vector<std::vector<uint8_t>> reads(2, std::vector<uint8_t>(30, 1));
        Report r(2);
        const std::vector<uint8_t> two{0, 1, 2, 3, 0, 1, 2, 3, 3, 2, 1, 0, 3, 2, 1, 0};
        Whitelist w8(two, 2, 8), dup(std::vector<uint8_t>{0, 1, 0, 1}, 2, 2);
        if (!w8.wl || dup.wl || g_err.find("barcodes 0 and 1 are the same") == std::string::npos) { fprintf(stderr, "the whitelist's builder: %s\n", g_err.c_str()); return 3; }
        if (run(*set, o, &d, nullptr, reads, r) != 0) { fprintf(stderr, "a valid call was refused: %s\n", g_err.c_str()); return 3; }
        if (run(*set, o, nullptr, nullptr, reads, r) == 0 || g_err.find("null cell design") == std::string::npos) { fprintf(stderr, "a null design was not refused\n"); return 3; }
        if (run(*set, o, &d, w8.wl, reads, r) == 0 || g_err.find("the whitelist's barcodes have 8 bases") == std::string::npos) { fprintf(stderr, "a whitelist of another length was not refused\n"); return 3; }
        d.bc_len = 17;
        if (run(*set, o, &d, nullptr, reads, r) == 0 || g_err.find("a field length outside") == std::string::npos) { fprintf(stderr, "bc_len 17 was not refused\n"); return 3; }
        d.bc_len = 0; d.umi_len = 0;
        if (run(*set, o, &d, nullptr, reads, r) == 0 || g_err.find("at least 1") == std::string::npos) { fprintf(stderr, "T = 0 was not refused\n"); return 3; }
        d.umi_len = 4; d.reserved[2] = 1;
        if (run(*set, o, &d, nullptr, reads, r) == 0 || g_err.find("reserved must be 0") == std::string::npos) { fprintf(stderr, "a reserved word was not refused\n"); return 3; }
        d.reserved[2] = 0; set->len[1] = 65;
        if (run(*set, o, &d, nullptr, reads, r) == 0 || g_err.find("primer 1: length outside") == std::string::npos) { fprintf(stderr, "length 65 was not refused\n"); return 3; }
    }
    printf("cell_sanitize: %ld cases of the limit set (%ld reads) equal the restatement, %ld random cases twice (%ld reads with a barcode of the whitelist, %ld ambiguous); clean\n",
           n_cases, n_reads, n_random, n_listed, n_ambiguous);
    return 0;
}

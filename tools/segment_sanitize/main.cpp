// segment_sanitize — ccsx_segment_reads_host (ccs_amd/csrc/ccsx_segment_api.cpp over segment_core.h: the walks, the selection and the classification k_segment
// runs) under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU.  Reads the case file tools/segment_sanitize.py writes (every set and read of the tests'
// limit set, with the report the restatement expects): each read lives in a heap block of exactly its length, every plane in one of exactly n words and the
// list in one of exactly n x 64 entries, so one access out of range is a report; the result is compared with the expected one, field for field.  Then seeded
// random sets and reads of its own, lengths and options at their limits, twice each (the same bytes), and the argument errors.  Exit 0 = all of that held; a
// sanitizer report aborts.
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
#include "ccsx_segment_api.cpp"

struct Report {
    int32_t n;
    int32_t *p[CCSX_SG_PLANES];
    ccsx_segment_piece *pieces;
    explicit Report(int32_t n_) : n(n_)
    {
        for (auto &q : p) { q = (int32_t *)malloc((size_t)n * 4 + (n ? 0 : 1)); memset(q, 0xA5, (size_t)n * 4); }
        pieces = (ccsx_segment_piece *)malloc(list_bytes() + (n ? 0 : 1));
        memset(pieces, 0xA5, list_bytes());
    }
    ~Report() { for (auto q : p) free(q); free(pieces); }
    size_t list_bytes() const { return (size_t)n * CCSX_SEGMENT_MAX_PIECES * sizeof(ccsx_segment_piece); }
    ccsx_segment_report c() { return ccsx_segment_report{n, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], pieces}; }
};

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 32); }

// the reads packed behind one another in a block of exactly their total length
static int run(const ccsx_segment_set &set, const ccsx_segment_opts &o, const std::vector<std::vector<uint8_t>> &reads, Report &rep)
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
    ccsx_segment_report c = rep.c();
    const int rc = ccsx_segment_reads_host(&set, &o, total ? seq : nullptr, off.data(), len.data(), (int32_t)reads.size(), &c);
    free(seq);
    return rc;
}

template <typename T> static bool rd(FILE *f, T *v, size_t n = 1) { return fread(v, sizeof(T), n, f) == n; }

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: segment_sanitize CASES.bin\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    static_assert(sizeof(ccsx_segment_piece) == 12, "the case file holds the list as 12-byte entries");
    long n_cases = 0, n_reads = 0;
    auto set = std::make_unique<ccsx_segment_set>();
    int32_t hdr[4];                                                  // n_adapters, max_dist_pct, min_len, n_reads
    while (rd(f, hdr, 4)) {
        memset(set.get(), 0, sizeof *set);
        set->n_adapters = hdr[0];
        for (int a = 0; a < hdr[0]; ++a) {
            if (!rd(f, &set->len[a]) || set->len[a] < 0 || set->len[a] > CCSX_SEGMENT_MAX_LEN || !rd(f, set->seq[a], (size_t)set->len[a])) { fprintf(stderr, "bad case file\n"); return 2; }
        }
        const ccsx_segment_opts o{hdr[1], hdr[2]};
        std::vector<std::vector<uint8_t>> reads((size_t)hdr[3]);
        for (auto &r : reads) {
            int32_t L;
            if (!rd(f, &L) || L < 0) { fprintf(stderr, "bad case file\n"); return 2; }
            r.resize((size_t)L);
            if (L && !rd(f, r.data(), (size_t)L)) { fprintf(stderr, "bad case file\n"); return 2; }
        }
        Report got(hdr[3]), want(hdr[3]);
        for (int k = 0; k < CCSX_SG_PLANES; ++k)
            if (hdr[3] && !rd(f, want.p[k], (size_t)hdr[3])) { fprintf(stderr, "bad case file\n"); return 2; }
        if (hdr[3] && !rd(f, (uint8_t *)want.pieces, want.list_bytes())) { fprintf(stderr, "bad case file\n"); return 2; }
        if (run(*set, o, reads, got) != 0) { fprintf(stderr, "case %ld refused: %s\n", n_cases, g_err.c_str()); return 3; }
        for (int k = 0; k < CCSX_SG_PLANES; ++k)
            if (hdr[3] && memcmp(got.p[k], want.p[k], (size_t)hdr[3] * 4)) { fprintf(stderr, "case %ld: plane %d differs from the restatement\n", n_cases, k); return 3; }
        if (hdr[3] && memcmp(got.pieces, want.pieces, got.list_bytes())) { fprintf(stderr, "case %ld: the list differs from the restatement\n", n_cases); return 3; }
        ++n_cases; n_reads += hdr[3];
    }
    fclose(f);
    // seeded random sets and reads: 2 .. 33 adapters of 8 .. 64 bases, reads of 0 .. 3000 bases over a two-letter alphabet or made of the set's own adapters (so
    // that hits, overlaps and overflows are common), bytes of any value (only the low two bits are read)
    long n_random = 0, n_overflow = 0, n_segments = 0;
    for (int it = 0; it < 300; ++it) {
        memset(set.get(), 0, sizeof *set);
        set->n_adapters = it % 7 == 0 ? CCSX_SEGMENT_MAX_ADAPTERS : 2 + (int32_t)(rnd() % 8);
        for (int a = 0; a < set->n_adapters; ++a) {
            set->len[a] = (it & 1) ? (a & 1 ? CCSX_SEGMENT_MAX_LEN : CCSX_SEGMENT_MIN_LEN) : CCSX_SEGMENT_MIN_LEN + (int32_t)(rnd() % 57);
            for (int i = 0; i < set->len[a]; ++i) set->seq[a][i] = (uint8_t)(rnd() & 3);
        }
        const ccsx_segment_opts o{(int32_t)(rnd() % 31), it % 5 == 0 ? 1 : it % 5 == 1 ? 65535 : 1 + (int32_t)(rnd() % 200)};
        std::vector<std::vector<uint8_t>> reads(1 + rnd() % 5);
        for (auto &r : reads) {
            const uint32_t kind = rnd() % 4;
            if (kind == 0) { r.resize(rnd() % 9); for (auto &c : r) c = (uint8_t)rnd(); }
            else if (kind == 1) { r.resize(rnd() % 3001); for (auto &c : r) c = (uint8_t)(rnd() & 0xfd); }      // two letters: many chance hits
            else {                                                   // adapters of the set in array order or at random, either strand, with fillers
                const int copies = 1 + (int)(rnd() % (kind == 2 ? 12 : 90));
                for (int q = 0; q < copies; ++q) {
                    const int a = kind == 2 ? q % set->n_adapters : (int)(rnd() % (uint32_t)set->n_adapters), m = set->len[a];
                    const bool rc = rnd() & 1;
                    for (int i = 0; i < m; ++i) r.push_back((uint8_t)((rc ? 3 - set->seq[a][m - 1 - i] : set->seq[a][i]) | (rnd() & 0xfc)));
                    for (uint32_t g = rnd() % (kind == 2 ? 300 : 20); g; --g) r.push_back((uint8_t)rnd());
                }
            }
        }
        Report a((int32_t)reads.size()), b((int32_t)reads.size());
        if (run(*set, o, reads, a) != 0 || run(*set, o, reads, b) != 0) { fprintf(stderr, "random case %d refused: %s\n", it, g_err.c_str()); return 3; }
        for (int k = 0; k < CCSX_SG_PLANES; ++k)
            if (memcmp(a.p[k], b.p[k], (size_t)a.n * 4)) { fprintf(stderr, "random case %d: two runs differ in plane %d\n", it, k); return 3; }
        if (memcmp(a.pieces, b.pieces, a.list_bytes())) { fprintf(stderr, "random case %d: two runs differ in the list\n", it); return 3; }
        for (size_t z = 0; z < reads.size(); ++z) {
            const int32_t L = (int32_t)reads[z].size(), tested = a.p[0][z], overflow = a.p[1][z], hits = a.p[2][z], cuts = a.p[3][z], segs = a.p[4][z], orient = a.p[6][z], left = a.p[7][z];
            bool ok = tested == (L > 0) && (overflow == 0 || overflow == 1) && overflow == (hits > CCSX_SEGMENT_MAX_HITS) && cuts >= 0 && cuts <= (overflow ? 0 : hits) &&
                      segs >= 0 && segs <= (cuts ? cuts - 1 : 0) && orient >= -1 && orient <= 2 && (orient == -1) == (segs == 0) && left >= 0 && left <= L;
            int32_t at = 0, inside = 0;
            for (int i = 0; i < CCSX_SEGMENT_MAX_PIECES && ok; ++i) {
                const ccsx_segment_piece &p = a.pieces[z * CCSX_SEGMENT_MAX_PIECES + i];
                if (i >= segs) { static const ccsx_segment_piece zero{}; ok = !memcmp(&p, &zero, sizeof p); continue; }
                ok = p.start >= at && p.end - p.start >= o.min_len && p.end <= L && p.index <= set->n_adapters - 2 && p.reverse <= 1;
                at = p.end; inside += p.end - p.start;
            }
            if (!ok || inside + left > L) { fprintf(stderr, "random case %d: read %zu out of range\n", it, z); return 3; }
            n_overflow += overflow; n_segments += segs;
        }
        ++n_random;
    }
    // argument errors name their cause
    {
        memset(set.get(), 0, sizeof *set);
        set->n_adapters = 2; set->len[0] = 8; set->len[1] = 8;
        const ccsx_segment_opts o{15, 50};
        std::vector<std::vector<uint8_t>> reads(2, std::vector<uint8_t>(30, 1));
        Report r(2);
        set->len[1] = 65;
        if (run(*set, o, reads, r) == 0 || g_err.find("adapter 1: length outside") == std::string::npos) { fprintf(stderr, "length 65 was not refused\n"); return 3; }
        set->len[1] = 8; set->n_adapters = CCSX_SEGMENT_MAX_ADAPTERS + 1;
        if (run(*set, o, reads, r) == 0 || g_err.find("n_adapters") == std::string::npos) { fprintf(stderr, "34 adapters were not refused\n"); return 3; }
        set->n_adapters = 2; set->seq[0][7] = 4;
        if (run(*set, o, reads, r) == 0 || g_err.find("adapter 0: code above 3") == std::string::npos) { fprintf(stderr, "code 4 was not refused\n"); return 3; }
    }
    printf("segment_sanitize: %ld cases of the limit set (%ld reads) equal the restatement, %ld random cases twice (%ld segments, %ld overflows); clean\n",
           n_cases, n_reads, n_random, n_segments, n_overflow);
    return 0;
}

// dup_sanitize — ccsx_dup_sign_reads_host, ccsx_dup_cluster_host and their checks (ccs_amd/csrc/ccsx_dup_api.cpp over dup_core.h and barcode_core.h: the
// signature, the walks and the predicate the k_dup_* kernels run) under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU.  Reads the case file
// tools/dup_sanitize.py writes (every case of the tests' limit set, with the signatures and the report the restatement expects): the reads live in a heap block of
// exactly their length, the signatures, groups, scores and every plane in blocks of exactly n entries, so one access out of range is a report; signatures and
// report are compared with the expected ones, byte for byte.  Then seeded random cases of its own, options at their limits, twice each (the same bytes), and the
// argument errors.  Exit 0 = all of that held; a sanitizer report aborts.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static std::string g_err;
void ccsx_set_error(const std::string &s) { g_err = s; }
#include "ccsx_barcode_api.cpp"
#include "ccsx_dup_api.cpp"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 32); }

template <typename T> struct Block {                                 // exactly n entries on the heap, poisoned
    T *p; size_t n;
    explicit Block(size_t n_) : p((T *)malloc(n_ * sizeof(T) + (n_ ? 0 : 1))), n(n_) { memset(p, 0xA5, n * sizeof(T)); }
    ~Block() { free(p); }
    Block(const Block &) = delete;
};
struct Outcome { std::vector<uint8_t> sig; std::vector<int32_t> planes; };

// the two host calls on a case: the reads packed behind one another in a block of exactly their total length
static int run(const ccsx_dup_opts &o, const std::vector<std::vector<uint8_t>> &reads, const std::vector<int32_t> *group, const std::vector<int32_t> *score, Outcome &out)
{
    const size_t n = reads.size();
    size_t total = 0;
    for (auto &r : reads) total += r.size();
    Block<uint8_t> seq(total);
    Block<int64_t> off(n);
    Block<int32_t> len(n), g(group ? n : 0), s(score ? n : 0), planes(4 * n);
    Block<ccsx_dup_sig> sig(n);
    size_t at = 0;
    for (size_t z = 0; z < n; ++z) {
        off.p[z] = (int64_t)at; len.p[z] = (int32_t)reads[z].size();
        if (len.p[z]) memcpy(seq.p + at, reads[z].data(), reads[z].size());
        at += reads[z].size();
        if (group) g.p[z] = (*group)[z];
        if (score) s.p[z] = (*score)[z];
    }
    if (ccsx_dup_sign_reads_host(&o, total ? seq.p : nullptr, off.p, len.p, (int32_t)n, sig.p)) return -1;
    ccsx_dup_report rep{(int32_t)n, planes.p, planes.p + n, planes.p + 2 * n, planes.p + 3 * n};
    if (ccsx_dup_cluster_host(&o, sig.p, group ? g.p : nullptr, score ? s.p : nullptr, (int32_t)n, &rep)) return -1;
    out.sig.assign((const uint8_t *)sig.p, (const uint8_t *)sig.p + n * sizeof(ccsx_dup_sig));
    out.planes.assign(planes.p, planes.p + 4 * n);
    return 0;
}

template <typename T> static bool rd(FILE *f, T *v, size_t n = 1) { return n == 0 || fread(v, sizeof(T), n, f) == n; }
#define MUST(x) do { if (!(x)) { fprintf(stderr, "dup_sanitize: %s:%d: %s failed (%s)\n", __FILE__, __LINE__, #x, g_err.c_str()); return 1; } } while (0)

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: dup_sanitize CASES.bin\n"); return 2; }
    static_assert(sizeof(ccsx_dup_sig) == 48, "ccsx_dup_sig is 48 bytes");
    FILE *f = fopen(argv[1], "rb");
    MUST(f);
    int cases = 0;
    int32_t head[7];
    while (rd(f, head, 7)) {
        const int32_t n = head[0];
        const ccsx_dup_opts o{head[1], head[2], head[3], head[4]};
        std::vector<std::vector<uint8_t>> reads((size_t)n);
        for (auto &r : reads) { int32_t L; MUST(rd(f, &L)); r.resize((size_t)L); MUST(rd(f, r.data(), r.size())); }
        std::vector<int32_t> group(head[5] ? n : 0), score(head[6] ? n : 0), want((size_t)4 * n);
        std::vector<uint8_t> want_sig((size_t)n * 48);
        MUST(rd(f, group.data(), group.size())); MUST(rd(f, score.data(), score.size()));
        MUST(rd(f, want_sig.data(), want_sig.size())); MUST(rd(f, want.data(), want.size()));
        Outcome got;
        MUST(run(o, reads, head[5] ? &group : nullptr, head[6] ? &score : nullptr, got) == 0);
        if (got.sig != want_sig || got.planes != want) { fprintf(stderr, "dup_sanitize: case %d differs from the restatement\n", cases); return 1; }
        ++cases;
    }
    fclose(f);
    // seeded random cases: options at their limits, reads around the window, copies, reverse complements and edits; twice, the same bytes
    int randoms = 0;
    for (int it = 0; it < 200; ++it) {
        ccsx_dup_opts o;
        o.window = it % 5 == 0 ? 16 : it % 5 == 1 ? 64 : 16 + (int)(rnd() % 49);
        o.kmer = it % 3 == 0 ? 8 : 8 + (int)(rnd() % 9);
        if (o.kmer > o.window) o.kmer = o.window;
        o.max_dist_pct = it % 7 == 0 ? 30 : (int)(rnd() % 31);
        o.max_len_diff_pct = it % 11 == 0 ? 20 : (int)(rnd() % 21);
        const int n = it % 13 == 0 ? 600 : 1 + (int)(rnd() % 60);
        std::vector<std::vector<uint8_t>> reads;
        std::vector<int32_t> group, score;
        for (int z = 0; z < n; ++z) {
            std::vector<uint8_t> r;
            if (z && rnd() % 3 == 0) {
                r = reads[rnd() % reads.size()];
                if (rnd() & 1) { std::vector<uint8_t> c(r.rbegin(), r.rend()); for (auto &b : c) b = (uint8_t)(3 - (b & 3)); r = c; }
                if (!r.empty() && (rnd() & 1)) r[rnd() % r.size()] ^= 1;
                if (it % 13 == 0) r = reads[0];                      // (a bucket above CCSX_DUP_MAX_BUCKET)
            } else {
                r.resize(rnd() % 8 == 0 ? rnd() % (size_t)o.window : (size_t)o.window + rnd() % 70);
                for (auto &b : r) b = (uint8_t)(rnd() & (rnd() % 4 ? 3 : 255));
            }
            reads.push_back(r);
            group.push_back((int32_t)(rnd() % 2)); score.push_back((int32_t)(rnd() % 5) - 2);
        }
        Outcome a, b;
        MUST(run(o, reads, it & 1 ? &group : nullptr, it & 2 ? &score : nullptr, a) == 0 && run(o, reads, it & 1 ? &group : nullptr, it & 2 ? &score : nullptr, b) == 0);
        MUST(a.sig == b.sig && a.planes == b.planes);
        for (int z = 0; z < n; ++z) {                                // the report is well-formed: a representative represents itself, in the read's set size
            const int32_t st = a.planes[z], rp = a.planes[n + z], sz = a.planes[2 * n + z], dp = a.planes[3 * n + z];
            MUST(st >= 0 && st <= 2 && rp >= 0 && rp < n && sz >= 1 && a.planes[n + rp] == rp && a.planes[2 * n + rp] == sz && dp == (rp != z) && (st == 1 || sz == 1));
        }
        ++randoms;
    }
    // the argument errors: nothing is read or written
    {
        ccsx_dup_opts o; ccsx_dup_opts_default(&o);
        uint8_t seq[64] = {0}; int64_t off[2] = {0, 32}; int32_t len[2] = {32, 32}; ccsx_dup_sig sig[2]; int32_t pl[8]; int32_t neg[2] = {0, -1};
        ccsx_dup_report rep{2, pl, pl + 2, pl + 4, pl + 6};
        MUST(ccsx_dup_sign_reads_host(&o, seq, off, len, 2, sig) == 0 && ccsx_dup_cluster_host(nullptr, sig, nullptr, nullptr, 2, &rep) == 0);
        ccsx_dup_opts bad = o; bad.kmer = 40;
        MUST(ccsx_dup_sign_reads_host(&bad, seq, off, len, 2, sig) == -1 && ccsx_dup_cluster_host(&bad, sig, nullptr, nullptr, 2, &rep) == -1);
        MUST(ccsx_dup_sign_reads_host(&o, nullptr, off, len, 2, sig) == -1 && ccsx_dup_sign_reads_host(&o, seq, off, len, 2, nullptr) == -1);
        MUST(ccsx_dup_sign_reads_host(&o, seq, off, len, -1, sig) == -1 && ccsx_dup_sign_reads_host(&o, seq, off, len, CCSX_DUP_MAX_READS + 1, sig) == -1);
        int64_t noff[2] = {0, -4};
        MUST(ccsx_dup_sign_reads_host(&o, seq, noff, len, 2, sig) == -1);
        MUST(ccsx_dup_cluster_host(&o, nullptr, nullptr, nullptr, 2, &rep) == -1 && ccsx_dup_cluster_host(&o, sig, nullptr, nullptr, 2, nullptr) == -1);
        MUST(ccsx_dup_cluster_host(&o, sig, neg, nullptr, 2, &rep) == -1 && ccsx_dup_cluster_host(&o, sig, nullptr, nullptr, -1, &rep) == -1);
        ccsx_dup_report other{3, pl, pl + 2, pl + 4, pl + 6}, hole{2, pl, nullptr, pl + 4, pl + 6};
        MUST(ccsx_dup_cluster_host(&o, sig, nullptr, nullptr, 2, &other) == -1 && ccsx_dup_cluster_host(&o, sig, nullptr, nullptr, 2, &hole) == -1);
        sig[1].window = 48;
        MUST(ccsx_dup_cluster_host(&o, sig, nullptr, nullptr, 2, &rep) == -1);
    }
    printf("dup_sanitize: %d limit cases equal the restatement, %d random cases twice, the argument errors: clean\n", cases, randoms);
    return 0;
}

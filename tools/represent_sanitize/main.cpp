// represent_sanitize — ccsx_represent_host (ccs_amd/csrc/ccsx_represent_api.cpp over represent_core.h: the class and the order k_represent uses) under
// AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU.  Reads the case file tools/represent_sanitize.py writes (every batch of the tests' limit set under the
// four flag combinations, with the planes the restatement expects): every input and output array lives in a heap block of exactly its size, every output byte
// starts as 0xA5, so one access out of range is a report and one byte written where the rule writes none is a difference.  Then seeded random batches of its
// own, twice each (the same bytes), and the argument errors.  Exit 0 = all of that held; a sanitizer report aborts.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static std::string g_err;
void ccsx_set_error(const std::string &s) { g_err = s; }
#include "ccsx_represent_api.cpp"

template <typename T> struct Block {                                 // exactly n elements on the heap
    T *p; size_t n;
    explicit Block(size_t n_, int fill = 0xA5) : p((T *)malloc(n_ * sizeof(T) + (n_ ? 0 : 1))), n(n_) { memset(p, fill, n * sizeof(T)); }
    ~Block() { free(p); }
    Block(const Block &) = delete;
    bool same(const Block &o) const { return n == o.n && (n == 0 || memcmp(p, o.p, n * sizeof(T)) == 0); }
    bool read(FILE *f) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
};

struct Out {                                                         // a results struct and a report of n ZMWs over `cap` plane elements, poisoned
    Block<int32_t> status, seq_len, np, iters, nwin, fn, rn, cls, pass;
    Block<float> rq, ec, raw;
    Block<uint8_t> seq, qual, fi, fp, ri, rp;
    Out(size_t n, size_t cap) : status(n), seq_len(n), np(n), iters(n), nwin(n), fn(n), rn(n), cls(n), pass(n), rq(n), ec(n), raw(cap), seq(cap), qual(cap), fi(cap), fp(cap),
                                ri(cap), rp(cap) {}
    bool same(const Out &o) const
    {
        return status.same(o.status) && seq_len.same(o.seq_len) && np.same(o.np) && iters.same(o.iters) && nwin.same(o.nwin) && fn.same(o.fn) && rn.same(o.rn) &&
               cls.same(o.cls) && pass.same(o.pass) && rq.same(o.rq) && ec.same(o.ec) && raw.same(o.raw) && seq.same(o.seq) && qual.same(o.qual) && fi.same(o.fi) &&
               fp.same(o.fp) && ri.same(o.ri) && rp.same(o.rp);
    }
};

struct Case {
    int32_t n, R, top, fb, kin;
    Block<int32_t> read_off, status, dlen;
    Block<int64_t> base_off, seq_off, doff;
    Block<uint8_t> flags, bases, pw, ipd, dseq;
    Block<int32_t> zmw_id; Block<float> snr;
    Case(int32_t n_, int32_t R_, int64_t nb, int64_t nd, int32_t top_, int32_t fb_, int32_t kin_)
        : n(n_), R(R_), top(top_), fb(fb_), kin(kin_), read_off((size_t)n_ + 1), status((size_t)n_), dlen((size_t)n_), base_off((size_t)R_ + 1), seq_off((size_t)n_ + 1),
          doff((size_t)n_), flags((size_t)R_), bases((size_t)nb), pw((size_t)nb), ipd((size_t)nb), dseq((size_t)nd), zmw_id((size_t)n_, 0), snr(4 * (size_t)n_, 0) {}
    int run(Out &o, ccsx_represent_report *rep_override = nullptr, int32_t res0 = 0, int hifi = -1, bool with_ipd = true)
    {
        const ccsx_batch b{n, R, base_off.p[R], zmw_id.p, snr.p, read_off.p, base_off.p, bases.p, pw.p, with_ipd ? ipd.p : nullptr, flags.p};
        ccsx_opts opts{};
        opts.top_passes = top; opts.hifi_kinetics = hifi >= 0 ? hifi : kin;
        ccsx_represent_report rep{n, o.cls.p, o.pass.p};
        const ccsx_represent_request req{fb, kin, rep_override ? rep_override : &rep, {res0, 0}};
        ccsx_results res{n, (int64_t)o.seq.n, seq_off.p, o.status.p, o.seq_len.p, o.seq.p, o.qual.p, o.raw.p, o.rq.p, o.np.p, o.ec.p, o.iters.p, o.nwin.p,
                         o.fi.p, o.fp.p, o.ri.p, o.rp.p, o.fn.p, o.rn.p};
        return ccsx_represent_host(&b, &opts, status.p, dseq.p, doff.p, dlen.p, &req, &res);
    }
    void layout()                                                    // seq_off: the capacity layout; doff: the drafts behind one another
    {
        seq_off.p[0] = 0;
        for (int z = 0; z < n; ++z) {
            int64_t maxL = 0;
            for (int r = read_off.p[z]; r < read_off.p[z + 1]; ++r) maxL = std::max<int64_t>(maxL, base_off.p[r + 1] - base_off.p[r]);
            seq_off.p[z + 1] = seq_off.p[z] + ccsx_draft_cap(maxL);
        }
        int64_t at = 0;
        for (int z = 0; z < n; ++z) { doff.p[z] = at; at += dlen.p[z]; }
    }
};

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 32); }

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: represent_sanitize CASES.bin\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    long n_cases = 0, n_zmws = 0;
    int64_t hdr[8];                                                  // n, R, bases, draft bases, plane elements, top_passes, subread_fallback, kinetics
    while (fread(hdr, 8, 8, f) == 8) {
        Case c((int32_t)hdr[0], (int32_t)hdr[1], hdr[2], hdr[3], (int32_t)hdr[5], (int32_t)hdr[6], (int32_t)hdr[7]);
        Out got((size_t)hdr[0], (size_t)hdr[4]), want((size_t)hdr[0], (size_t)hdr[4]);
        bool ok = c.read_off.read(f) && c.base_off.read(f) && c.flags.read(f) && c.bases.read(f) && c.pw.read(f) && c.ipd.read(f) && c.status.read(f) && c.dlen.read(f) &&
                  c.dseq.read(f);
        ok = ok && want.cls.read(f) && want.pass.read(f) && want.seq_len.read(f) && want.rq.read(f) && want.ec.read(f) && want.seq.read(f) && want.qual.read(f) &&
             want.raw.read(f) && want.fi.read(f) && want.fp.read(f);
        if (!ok) { fprintf(stderr, "bad case file\n"); return 2; }
        c.layout();
        if ((size_t)c.seq_off.p[c.n] != got.seq.n) { fprintf(stderr, "case %ld: the capacity layout differs from the restatement's\n", n_cases); return 3; }
        if (c.run(got) != 0) { fprintf(stderr, "case %ld refused: %s\n", n_cases, g_err.c_str()); return 3; }
        if (!got.same(want)) { fprintf(stderr, "case %ld: the planes differ from the restatement's\n", n_cases); return 3; }
        ++n_cases; n_zmws += c.n;
    }
    fclose(f);
    long n_random = 0;
    for (int it = 0; it < 300; ++it) {                               // random batches: 1 .. 6 ZMWs of 0 .. 9 passes (every fifth: 250 .. 270) of 0 .. 300 bases, any status 0 .. 14
        const int n = 1 + (int)(rnd() % 6);
        std::vector<int> np(n), len;
        int R = 0; int64_t nb = 0, nd = 0;
        for (int z = 0; z < n; ++z) { np[z] = (it % 5 == 0 && z == 0) ? 250 + (int)(rnd() % 21) : (int)(rnd() % 10); R += np[z]; }
        for (int r = 0; r < R; ++r) { len.push_back(rnd() % 7 == 0 ? 0 : (int)(rnd() % 301)); nb += len.back(); }
        std::vector<int> dl(n);
        for (int z = 0; z < n; ++z) { dl[z] = rnd() % 3 == 0 ? 0 : (int)(rnd() % 500); nd += dl[z]; }
        Case c(n, R, nb, nd, it % 4 == 0 ? (int)(rnd() % 6) : 0, (int)(rnd() & 1), (int)(rnd() & 1));
        c.read_off.p[0] = 0; c.base_off.p[0] = 0;
        for (int z = 0, r = 0; z < n; ++z) { for (int q = 0; q < np[z]; ++q, ++r) { c.base_off.p[r + 1] = c.base_off.p[r] + len[r]; c.flags.p[r] = (uint8_t)(rnd() & 7); } c.read_off.p[z + 1] = r; }
        for (int64_t i = 0; i < nb; ++i) { c.bases.p[i] = (uint8_t)rnd(); c.pw.p[i] = (uint8_t)rnd(); c.ipd.p[i] = (uint8_t)rnd(); }
        for (int64_t i = 0; i < nd; ++i) c.dseq.p[i] = (uint8_t)rnd();
        for (int z = 0; z < n; ++z) { c.status.p[z] = (int32_t)(rnd() % 15); c.dlen.p[z] = dl[z]; }
        c.layout();
        Out a((size_t)n, (size_t)c.seq_off.p[n]), b((size_t)n, (size_t)c.seq_off.p[n]);
        if (c.run(a) != 0 || c.run(b) != 0) { fprintf(stderr, "random case %d refused: %s\n", it, g_err.c_str()); return 3; }
        if (!a.same(b)) { fprintf(stderr, "random case %d: two runs differ\n", it); return 3; }
        for (int z = 0; z < n; ++z) {
            const int cls = a.cls.p[z], pass = a.pass.p[z];
            const int64_t slot = c.seq_off.p[z + 1] - c.seq_off.p[z];
            if (cls < 0 || cls > 3 || (cls == CCSX_REPRESENT_SUBREAD) != (pass >= 0) || pass >= np[z] || pass >= CCSX_MAX_PASSES) { fprintf(stderr, "random case %d: ZMW %d out of range\n", it, z); return 3; }
            if (cls >= CCSX_REPRESENT_DRAFT && (a.seq_len.p[z] < 0 || a.seq_len.p[z] > slot || a.rq.p[z] != -1.0f)) { fprintf(stderr, "random case %d: ZMW %d: bad length or rq\n", it, z); return 3; }
        }
        ++n_random;
    }
    {   // argument errors name their cause and leave every output byte alone
        Case c(2, 2, 20, 0, 0, 0, 1);
        c.read_off.p[0] = 0; c.read_off.p[1] = 1; c.read_off.p[2] = 2; c.base_off.p[0] = 0; c.base_off.p[1] = 10; c.base_off.p[2] = 20;
        memset(c.flags.p, 0, 2); c.status.p[0] = c.status.p[1] = CCSX_TOO_FEW_PASSES; c.dlen.p[0] = c.dlen.p[1] = 0;
        c.layout();
        Out clean((size_t)2, (size_t)c.seq_off.p[2]), o((size_t)2, (size_t)c.seq_off.p[2]);
        ccsx_represent_report other{3, o.cls.p, o.pass.p}, nocls{2, nullptr, o.pass.p};
        auto expect = [&](int rc, const char *w) { if (rc == 0 || g_err.find(w) == std::string::npos || !o.same(clean)) { fprintf(stderr, "not refused as '%s': %s\n", w, g_err.c_str()); exit(3); } };
        expect(c.run(o, &other), "sized for another batch"); expect(c.run(o, &nocls), "sized for another batch"); expect(c.run(o, nullptr, 7), "reserved must be 0");
        expect(c.run(o, nullptr, 0, 0), "needs opts.hifi_kinetics"); expect(c.run(o, nullptr, 0, 1, false), "needs batch.ipd");
        c.fb = 2; expect(c.run(o), "must be 0 or 1"); c.fb = 0;
        if (c.run(o) != 0 || o.same(clean)) { fprintf(stderr, "the valid call did nothing\n"); return 3; }
    }
    printf("represent_sanitize: %ld cases of the limit set (%ld ZMWs) equal the restatement, %ld random batches twice; clean\n", n_cases, n_zmws, n_random);
    return 0;
}

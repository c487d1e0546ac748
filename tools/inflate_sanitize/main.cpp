// inflate_sanitize — the DEFLATE decoder of k_inflate (ccs_amd/csrc/inflate_core.h) under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU.
// Reads the case file tools/inflate_sanitize.py writes (every valid, corrupt and flipped stream of tests/inflate_ref.py), decodes each from an input buffer of
// exactly in_len bytes into an output buffer of exactly out_len bytes (so one byte out of range is a report), then flips every bit of every short stream and a
// seeded sample of bits of the long ones.  Exit 0 = every decode ended in a status in range and the expected statuses matched; a sanitizer report aborts.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "inflate_core.h"

struct Case { std::vector<uint8_t> in; int64_t out_len; int32_t want; std::vector<uint8_t> expect; };

static int decode(const std::vector<uint8_t> &in, int64_t out_len, std::vector<uint8_t> *out)
{
    static ccsx_infl_tables T;
    uint8_t *i = (uint8_t *)malloc(in.size() ? in.size() : 1), *o = (uint8_t *)malloc(out_len ? (size_t)out_len : 1);
    if (in.size()) memcpy(i, in.data(), in.size());
    // (a buffer of size 0 is allocated with one byte that the decoder has no business touching: poisoned by reading it back below)
    if (!in.size()) i[0] = 0x5c;
    if (!out_len) o[0] = 0x5c;
    const int rc = ccsx_infl_stream_host(i, (int64_t)in.size(), o, out_len, &T);
    if (!out_len && o[0] != 0x5c) { fprintf(stderr, "a byte was written to an empty output\n"); exit(3); }
    if (out) out->assign(o, o + out_len);
    free(i); free(o);
    if (rc < 0 || rc > CCSX_INFLATE_OUTPUT_SHORT) { fprintf(stderr, "status %d out of range\n", rc); exit(3); }
    return rc;
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: inflate_sanitize CASES.bin\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<Case> cases;
    for (;;) {
        int64_t hdr[4];                                   // in_len, out_len, expected status (-1 = any), bytes of expected output (0 = none)
        if (fread(hdr, sizeof(hdr), 1, f) != 1) break;
        Case c; c.in.resize((size_t)hdr[0]); c.out_len = hdr[1]; c.want = (int32_t)hdr[2]; c.expect.resize((size_t)hdr[3]);
        if ((hdr[0] && fread(c.in.data(), 1, c.in.size(), f) != c.in.size()) || (hdr[3] && fread(c.expect.data(), 1, c.expect.size(), f) != c.expect.size())) { fprintf(stderr, "short case file\n"); return 2; }
        cases.push_back(std::move(c));
    }
    fclose(f);
    long n_ok = 0, n_bad = 0, n_flip = 0, n_flip_ok = 0, mism = 0;
    for (size_t k = 0; k < cases.size(); ++k) {
        const Case &c = cases[k];
        std::vector<uint8_t> out;
        const int rc = decode(c.in, c.out_len, &out);
        (rc == 0 ? n_ok : n_bad)++;
        if (c.want >= 0 && rc != c.want) { fprintf(stderr, "case %zu: status %d, expected %d\n", k, rc, c.want); ++mism; }
        if (c.want == 0 && out != c.expect) { fprintf(stderr, "case %zu: output differs\n", k); ++mism; }
    }
    uint64_t rng = 0x9e3779b97f4a7c15ull;
    for (const Case &c : cases) {
        if (c.want != 0 || c.in.empty()) continue;
        const size_t bits = c.in.size() * 8;
        const size_t n = bits <= 4096 ? bits : 256;       // every bit of a short stream, a seeded sample of a long one (its first 64 bytes twice as often)
        for (size_t j = 0; j < n; ++j) {
            size_t bit = j;
            if (bits > 4096) { rng = rng * 6364136223846793005ull + 1442695040888963407ull; bit = (size_t)((rng >> 20) % ((j & 1) ? 512 : bits)); }
            std::vector<uint8_t> in = c.in;
            in[bit >> 3] ^= (uint8_t)(1u << (bit & 7));
            ++n_flip;
            if (decode(in, c.out_len, nullptr) == 0) ++n_flip_ok;
        }
    }
    printf("inflate_sanitize: %zu cases (%ld OK, %ld with an error status, %ld mismatches); %ld bit flips, %ld of them still decode to out_len bytes\n",
           cases.size(), n_ok, n_bad, mism, n_flip, n_flip_ok);
    return mism ? 1 : 0;
}

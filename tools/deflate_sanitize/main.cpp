// deflate_sanitize — the DEFLATE encoder of k_deflate (ccs_amd/csrc/deflate_core.h) under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU, judged by
// the project's own decoder (ccs_amd/csrc/inflate_core.h).  Reads the case file tools/deflate_sanitize.py writes (every test input), adds seeded random inputs of
// its own, and for each: encodes from an input buffer of exactly in_len bytes into an output buffer of exactly the bound (so one byte out of range is a report),
// decodes the stream back and compares, checks the CRC against a bitwise CRC32, then encodes again into a buffer of exactly out_len bytes (same stream) and of
// out_len - 1 bytes (OUTPUT_FULL, nothing past the buffer).  Then the range / overlap check both codecs' entry points share (ccs_amd/csrc/codec_check.h) takes
// hostile lists of both item types, each from an array of exactly its items: offsets at the ends of int64 are refused without a signed overflow.
// Exit 0 = all of that held; a sanitizer report aborts.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "codec_check.h"
#include "deflate_core.h"
#include "inflate_core.h"

static std::string last_error;
void ccsx_set_error(const std::string &s) { last_error = s; }

static ccsx_defl_work W;
static ccsx_infl_tables T;
static long n_stored = 0, n_coded = 0, bytes_in = 0, bytes_out = 0;

static uint32_t crc_plain(const uint8_t *p, size_t n)
{
    uint32_t c = 0xffffffffu;
    for (size_t i = 0; i < n; ++i) { c ^= p[i]; for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1u))); }
    return ~c;
}

static int encode(const std::vector<uint8_t> &in, int32_t cap, std::vector<uint8_t> *out, uint32_t *crc)
{
    uint8_t *i = (uint8_t *)malloc(in.size() ? in.size() : 1), *o = (uint8_t *)malloc(cap ? (size_t)cap : 1);
    if (in.size()) memcpy(i, in.data(), in.size());
    if (!cap) o[0] = 0x5c;
    int32_t out_len = -1;
    const int rc = ccsx_defl_span<ccsx_defl_serial>(i, (int32_t)in.size(), o, cap, &W, &out_len, crc);
    if (!cap && o[0] != 0x5c) { fprintf(stderr, "a byte was written to an empty output\n"); exit(3); }
    if (rc != CCSX_DEFLATE_OK && rc != CCSX_DEFLATE_OUTPUT_FULL) { fprintf(stderr, "status %d out of range\n", rc); exit(3); }
    if (out_len < 0 || out_len > cap || (rc != CCSX_DEFLATE_OK && out_len != 0)) { fprintf(stderr, "out_len %d with status %d, cap %d\n", out_len, rc, cap); exit(3); }
    out->assign(o, o + out_len);
    free(i); free(o);
    return rc;
}

static int check(const std::vector<uint8_t> &in, size_t k)
{
    const int32_t bound = ccsx_defl_stored_len((int32_t)in.size());
    std::vector<uint8_t> s, s2, back(in.size());
    uint32_t crc = 0, crc2 = 0;
    if (encode(in, bound, &s, &crc) != CCSX_DEFLATE_OK) { fprintf(stderr, "case %zu: OUTPUT_FULL at the bound\n", k); return 1; }
    if (crc != crc_plain(in.data(), in.size())) { fprintf(stderr, "case %zu: CRC differs\n", k); return 1; }
    uint8_t *sp = (uint8_t *)malloc(s.size() ? s.size() : 1), *bp = (uint8_t *)malloc(in.size() ? in.size() : 1);
    memcpy(sp, s.data(), s.size());
    const int rc = ccsx_infl_stream_host(sp, (int64_t)s.size(), bp, (int64_t)in.size(), &T);
    const bool same = rc == CCSX_INFLATE_OK && (in.empty() || !memcmp(bp, in.data(), in.size()));
    // the stream ends where the final block ends: one byte less is no longer a whole stream
    const int rc_short = s.empty() ? -1 : ccsx_infl_stream_host(sp, (int64_t)s.size() - 1, bp, (int64_t)in.size(), &T);
    free(sp); free(bp);
    if (!same) { fprintf(stderr, "case %zu (%zu bytes): the decoder answers %d or other bytes\n", k, in.size(), rc); return 1; }
    if (rc_short == CCSX_INFLATE_OK) { fprintf(stderr, "case %zu (%zu bytes): bytes behind the final block\n", k, in.size()); return 1; }
    if (encode(in, (int32_t)s.size(), &s2, &crc2) != CCSX_DEFLATE_OK || s2 != s || crc2 != crc) { fprintf(stderr, "case %zu: another stream at out_cap == out_len\n", k); return 1; }
    if (encode(in, (int32_t)s.size() - 1, &s2, &crc2) != CCSX_DEFLATE_OUTPUT_FULL) { fprintf(stderr, "case %zu: no OUTPUT_FULL at out_cap == out_len - 1\n", k); return 1; }
    ((s.size() == (size_t)bound) ? n_stored : n_coded)++;
    bytes_in += (long)in.size(); bytes_out += (long)s.size();
    return 0;
}

// one list through the check: the items (in_off, in_len, out_len | out_cap, out_off) against src of 4 and dst of dst_len bytes; `want`: a part of the refusal's
// text, or NULL for a list that is accepted
template <typename D> static int hostile(const char *what, std::vector<typename D::Item> items, int64_t dst_len, const char *want)
{
    using Item = typename D::Item;
    Item *a = (Item *)malloc(items.size() ? items.size() * sizeof(Item) : 1);
    if (!items.empty()) memcpy(a, items.data(), items.size() * sizeof(Item));
    uint8_t src[4] = {0}, dst[1] = {0};
    std::vector<int32_t> order;
    last_error.clear();
    const int rc = ccsx_codec_check<D>("check", src, 4, a, (int32_t)items.size(), dst, dst_len, true, order);
    free(a);
    const bool ok = want ? (rc == -1 && last_error.find(want) != std::string::npos && last_error.find(D::noun) != std::string::npos) : rc == 0;
    if (!ok) fprintf(stderr, "range check, %s %s: rc %d, \"%s\"\n", D::noun, what, rc, last_error.c_str());
    return ok ? 0 : 1;
}

template <typename D> static int hostile_lists()
{
    const int64_t hi = INT64_MAX, lo = INT64_MIN, far = (int64_t)1 << 40;
    int bad = 0;
    bad += hostile<D>("ends at the ends", {{0, 2, 10, 0}, {2, 2, 10, 10}}, 20, nullptr);
    bad += hostile<D>("descending", {{0, 2, 10, 10}, {2, 2, 10, 0}}, 20, nullptr);
    bad += hostile<D>("input one past", {{0, 2, 10, 0}, {3, 2, 10, 10}}, 20, "input range outside src");
    bad += hostile<D>("output one past", {{0, 2, 10, 0}, {2, 2, 10, 11}}, 20, "output range outside dst");
    bad += hostile<D>("in_len -1", {{0, -1, 10, 0}}, 20, D::limited(typename D::Item{0, -1, 10, 0}) < 0 ? D::limit_text : "input range outside src");
    bad += hostile<D>("range length -1", {{0, 2, -1, 0}}, 20, D::limited(typename D::Item{0, 2, -1, 0}) < 0 ? D::limit_text : "output range outside dst");
    bad += hostile<D>("limit + 1", {{0, 65537, 65537, 0}}, far, D::limit_text);
    for (const int64_t off : {hi, lo, far, hi - 1, lo + 1, (int64_t)-1}) {
        bad += hostile<D>("in_off extreme", {{0, 2, 10, 0}, {off, 2, 10, 10}}, 20, "input range outside src");
        bad += hostile<D>("out_off extreme", {{0, 2, 10, 0}, {2, 2, 10, off}}, 20, "output range outside dst");
        bad += hostile<D>("out_off extreme in a dst as long as int64", {{0, 2, 10, 0}, {2, 2, 10, off}}, hi, off < 0 || off > hi - 10 ? "output range outside dst" : nullptr);
    }
    bad += hostile<D>("ends at the end of an int64 dst", {{0, 2, 10, hi - 10}, {2, 2, 10, 0}}, hi, nullptr);
    bad += hostile<D>("overlap by one", {{0, 2, 10, 0}, {2, 2, 10, 9}}, 20, "0 and 1: output ranges overlap");
    bad += hostile<D>("overlap by one, descending", {{0, 2, 10, 9}, {2, 2, 10, 0}}, 20, "1 and 0: output ranges overlap");
    bad += hostile<D>("overlap at the end of an int64 dst", {{0, 2, 10, hi - 10}, {2, 2, 10, hi - 19}}, hi, "1 and 0: output ranges overlap");
    bad += hostile<D>("empty range between two overlapping ones", {{0, 2, 10, 0}, {2, 0, 0, 5}, {2, 2, 10, 5}}, 15, "0 and 2: output ranges overlap");
    bad += hostile<D>("empty range between two that touch", {{0, 2, 10, 0}, {2, 0, 0, 10}, {2, 2, 10, 10}}, 20, nullptr);
    bad += hostile<D>("no items", {}, 0, nullptr);
    return bad;
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: deflate_sanitize CASES.bin\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<std::vector<uint8_t>> cases;
    for (;;) {
        int64_t n;
        if (fread(&n, sizeof(n), 1, f) != 1) break;
        std::vector<uint8_t> c((size_t)n);
        if (n && fread(c.data(), 1, c.size(), f) != c.size()) { fprintf(stderr, "short case file\n"); return 2; }
        cases.push_back(std::move(c));
    }
    fclose(f);
    // seeded random inputs: random lengths, alphabets of 1 .. 256 bytes, copies from earlier in the buffer at random distances
    uint64_t rng = 0x9e3779b97f4a7c15ull;
    auto next = [&rng]() { rng = rng * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(rng >> 33); };
    for (int k = 0; k < 300; ++k) {
        const uint32_t n = (k % 3 == 0) ? next() % 600 : (k % 3 == 1) ? next() % 9000 : next() % 65537, alpha = 1 + next() % 256, copy_every = 2 + next() % 40;
        std::vector<uint8_t> c;
        c.reserve(n);
        while (c.size() < n) {
            if (!c.empty() && next() % copy_every == 0) {
                const size_t d = 1 + next() % c.size(), l = 1 + next() % 400;
                for (size_t i = 0; i < l && c.size() < n; ++i) c.push_back(c[c.size() - d]);
            } else c.push_back((uint8_t)(next() % alpha));
        }
        cases.push_back(std::move(c));
    }
    long bad = 0;
    for (size_t k = 0; k < cases.size(); ++k) bad += check(cases[k], k);
    bad += hostile_lists<ccsx_inflate_items>() + hostile_lists<ccsx_deflate_items>();
    printf("deflate_sanitize: %zu inputs (%ld coded, %ld stored), %ld bytes in, %ld bytes out, %ld failures\n", cases.size(), n_coded, n_stored, bytes_in, bytes_out, bad);
    return bad ? 1 : 0;
}

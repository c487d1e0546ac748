// ccsx_deflate_api.cpp — the C ABI of the BGZF deflater (include/ccsx.h "BGZF deflate on the device"): an object of its own beside the consensus handle and the
// inflater.
//
// The deflater is the codec host of codec_host.h under the description below: ccsx_deflate_submit() enqueues upload -> k_deflate -> download, ccsx_deflate_wait()
// copies every OK span's stream (nothing else), the lengths, the CRCs and the statuses to the caller.  Nothing of it runs unless a caller creates a deflater.
#include "codec_host.h"
#include "deflate_core.h"

extern "C" int ccsx_launch_deflate(hipStream_t stream, const uint8_t *src, int64_t src_len, const ccsx_deflate_span *span, int32_t n_spans, uint8_t *dst,
                                   int64_t dst_len, int32_t *out_len, uint32_t *crc, int32_t *status);

#define DEFL_WG_PER_CU 1             // k_deflate holds about 147 KiB of LDS: one workgroup per CU

static_assert(CCSX_DEFL_MAX_IN == CCSX_DEFLATE_MAX_IN, "deflate_core.h and ccsx.h disagree on the span limit");

namespace {

struct Deflate : ccsx_deflate_items {
    static constexpr const char *object = "deflater", *create_name = "ccsx_deflater_create", *submit_name = "ccsx_deflate_submit", *wait_name = "ccsx_deflate_wait",
                                *host_hint = "ccsx_deflate_spans_host is the host's encoder";
    struct Results { int32_t *out_len; uint32_t *crc; int32_t *status; };
    static bool results_ok(const Results &r) { return r.out_len && r.crc && r.status; }
    static constexpr size_t planes = 3;          // out_len, crc, status
    static size_t down_words(size_t, size_t cap) { return planes * cap; }
    static constexpr bool read_prio = false;
    static int launch(hipStream_t st, const uint8_t *src, int64_t src_len, const Item *span, int32_t n, uint8_t *dst, int64_t dst_len, int32_t *res, size_t cap)
    {
        return ccsx_launch_deflate(st, src, src_len, span, n, dst, dst_len, res, (uint32_t *)(res + cap), res + 2 * cap);
    }
    static int32_t take(const Item &b, int32_t i, const int32_t *res, size_t cap, const Results &out)
    {
        const int32_t st = res[2 * cap + i];
        int32_t n = res[i];
        if (st != CCSX_DEFLATE_OK || n < 0 || n > b.out_cap) n = 0;
        out.status[i] = st;
        out.out_len[i] = n;
        out.crc[i] = (uint32_t)res[cap + i];
        return n;
    }
};

}   // namespace

struct ccsx_deflater_s : CodecHost<Deflate> {};

extern "C" {

int ccsx_deflate_rule_version(void) { return CCSX_DEFL_RULE_VERSION; }

int32_t ccsx_deflate_bound(int32_t in_len) { return ccsx_defl_stored_len(in_len); }

uint32_t ccsx_deflate_crc(const uint8_t *p, int64_t n)
{
    if (!p || n <= 0) return 0;
    // spans of the rule's size, each through the rule's sliced CRC, chained with the same shift operator
    uint32_t crc = 0, acc = 0;
    for (int64_t at = 0; at < n; at += CCSX_DEFL_MAX_IN) {
        const uint32_t m = (uint32_t)std::min<int64_t>(n - at, CCSX_DEFL_MAX_IN);
        const uint32_t c = ccsx_defl_crc<ccsx_defl_serial>(p + at, m, &acc);
        crc = ccsx_defl_gf2_mul(ccsx_defl_gf2_xpow_bytes(m), crc) ^ c;
    }
    return crc;
}

int ccsx_deflate_code_lengths(const uint32_t *freq, int32_t n, int32_t max_bits, uint8_t *lens)
{
    if (!freq || !lens || n < 2 || n > CCSX_DEFL_NLIT || max_bits < 1 || max_bits > 15) { ccsx_set_error("ccsx_deflate_code_lengths: null argument, n outside 2 .. 286 or max_bits outside 1 .. 15"); return -1; }
    if ((1 << max_bits) < n) { ccsx_set_error("ccsx_deflate_code_lengths: max_bits too small for n symbols"); return -1; }
    static thread_local ccsx_defl_work W;
    for (int32_t i = 0; i < CCSX_DEFL_NLIT; ++i) W.freq[i] = i < n ? freq[i] : 0u;
    ccsx_defl_build<ccsx_defl_serial>(&W, 0, n, max_bits);
    for (int32_t i = 0; i < n; ++i) lens[i] = W.len[i];
    return 0;
}

int32_t ccsx_deflate_fill_spans(int device)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) { ccsx_set_error("ccsx_deflate_fill_spans: no such HIP device"); return -1; }
    int cus = 0;
    HIPTRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    return (int32_t)cus * DEFL_WG_PER_CU;
}

int ccsx_deflater_create(int device, int64_t max_in_bytes, int64_t max_out_bytes, int32_t max_spans, ccsx_deflater *out)
{
    return codec_create(device, max_in_bytes, max_out_bytes, max_spans, out);
}

int ccsx_deflater_destroy(ccsx_deflater f) { codec_free(f); return 0; }

int ccsx_deflate_submit(ccsx_deflater f, const uint8_t *src, int64_t src_len, const ccsx_deflate_span *spans, int32_t n_spans, uint8_t *dst, int64_t dst_len,
                        int32_t *out_len, uint32_t *crc, int32_t *status, ccsx_ticket *ticket)
{
    return codec_submit(f, src, src_len, spans, n_spans, dst, dst_len, {out_len, crc, status}, ticket);
}

int ccsx_deflate_wait(ccsx_deflater f, ccsx_ticket ticket) { return codec_wait(f, ticket); }

int ccsx_deflate_spans(ccsx_deflater f, const uint8_t *src, int64_t src_len, const ccsx_deflate_span *spans, int32_t n_spans, uint8_t *dst, int64_t dst_len,
                       int32_t *out_len, uint32_t *crc, int32_t *status)
{
    return codec_run(f, src, src_len, spans, n_spans, dst, dst_len, {out_len, crc, status});
}

int ccsx_deflate_spans_host(const uint8_t *src, int64_t src_len, const ccsx_deflate_span *spans, int32_t n_spans, uint8_t *dst, int64_t dst_len, int32_t *out_len,
                            uint32_t *crc, int32_t *status)
{
    std::vector<int32_t> order;
    if (int rc = ccsx_codec_check<Deflate>("ccsx_deflate_spans_host", src, src_len, spans, n_spans, dst, dst_len, out_len && crc && status, order)) return rc;
    static thread_local ccsx_defl_work W;
    std::vector<uint8_t> tmp;        // a span's stream is built beside dst: of a span that does not fit, or is not OK, no byte of dst is written
    for (int32_t i = 0; i < n_spans; ++i) {
        const ccsx_deflate_span &b = spans[i];
        tmp.resize((size_t)std::max<int32_t>(b.out_cap, 1));
        int32_t n = 0;
        status[i] = ccsx_defl_span<ccsx_defl_serial>(src + b.in_off, b.in_len, tmp.data(), b.out_cap, &W, &n, &crc[i]);
        out_len[i] = status[i] == CCSX_DEFLATE_OK ? n : 0;
        if (out_len[i] > 0) std::memcpy(dst + b.out_off, tmp.data(), (size_t)out_len[i]);
    }
    return 0;
}

}   // extern "C"

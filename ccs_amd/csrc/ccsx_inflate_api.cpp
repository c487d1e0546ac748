// ccsx_inflate_api.cpp — the C ABI of the BGZF inflater (include/ccsx.h "BGZF inflate on the device"): an object of its own beside the consensus handle.
//
// The inflater is the codec host of codec_host.h under the description below: ccsx_inflate_submit() enqueues upload -> k_inflate -> download, ccsx_inflate_wait()
// copies every OK block's output range (nothing else) and the statuses to the caller.  Nothing of it runs unless a caller creates an inflater.
#include "codec_host.h"
#include "inflate_core.h"

extern "C" int ccsx_launch_inflate(hipStream_t stream, const uint8_t *src, int64_t src_len, const ccsx_deflate_block *blk, int32_t n_blocks, uint8_t *dst,
                                   int64_t dst_len, int32_t *status);

#define INFL_RULE_VERSION 1

namespace {

struct Inflate : ccsx_inflate_items {
    static constexpr const char *object = "inflater", *create_name = "ccsx_inflater_create", *submit_name = "ccsx_inflate_submit", *wait_name = "ccsx_inflate_wait",
                                *host_hint = "ccsx_inflate_blocks_host is the host's decoder";
    struct Results { int32_t *status; };
    static bool results_ok(const Results &r) { return r.status; }
    static constexpr size_t planes = 1;          // status
    static size_t down_words(size_t n, size_t) { return n; }
    static constexpr bool read_prio = true;
    static int launch(hipStream_t st, const uint8_t *src, int64_t src_len, const Item *blk, int32_t n, uint8_t *dst, int64_t dst_len, int32_t *res, size_t)
    {
        return ccsx_launch_inflate(st, src, src_len, blk, n, dst, dst_len, res);
    }
    static int32_t take(const Item &b, int32_t i, const int32_t *res, size_t, const Results &out)
    {
        out.status[i] = res[i];
        return res[i] == CCSX_INFLATE_OK ? b.out_len : 0;
    }
};

}   // namespace

struct ccsx_inflater_s : CodecHost<Inflate> {};

extern "C" {

int ccsx_inflate_rule_version(void) { return INFL_RULE_VERSION; }

int ccsx_inflater_create(int device, int64_t max_in_bytes, int64_t max_out_bytes, int32_t max_blocks, ccsx_inflater *out)
{
    return codec_create(device, max_in_bytes, max_out_bytes, max_blocks, out);
}

int ccsx_inflater_destroy(ccsx_inflater f) { codec_free(f); return 0; }

int ccsx_inflate_submit(ccsx_inflater f, const uint8_t *src, int64_t src_len, const ccsx_deflate_block *blocks, int32_t n_blocks, uint8_t *dst, int64_t dst_len,
                        int32_t *status, ccsx_ticket *ticket)
{
    return codec_submit(f, src, src_len, blocks, n_blocks, dst, dst_len, {status}, ticket);
}

int ccsx_inflate_wait(ccsx_inflater f, ccsx_ticket ticket) { return codec_wait(f, ticket); }

int ccsx_inflate_blocks(ccsx_inflater f, const uint8_t *src, int64_t src_len, const ccsx_deflate_block *blocks, int32_t n_blocks, uint8_t *dst, int64_t dst_len,
                        int32_t *status)
{
    return codec_run(f, src, src_len, blocks, n_blocks, dst, dst_len, {status});
}

int ccsx_inflate_blocks_host(const uint8_t *src, int64_t src_len, const ccsx_deflate_block *blocks, int32_t n_blocks, uint8_t *dst, int64_t dst_len, int32_t *status)
{
    std::vector<int32_t> order;
    if (int rc = ccsx_codec_check<Inflate>("ccsx_inflate_blocks_host", src, src_len, blocks, n_blocks, dst, dst_len, status, order)) return rc;
    static thread_local ccsx_infl_tables T;
    for (int32_t i = 0; i < n_blocks; ++i) {
        const ccsx_deflate_block &b = blocks[i];
        status[i] = ccsx_infl_stream_host(src + b.in_off, b.in_len, dst + b.out_off, b.out_len, &T);
    }
    return 0;
}

}   // extern "C"

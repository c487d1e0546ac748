// ccsx_inflate_api.cpp — the C ABI of the BGZF inflater (include/ccsx.h "BGZF inflate on the device"): an object of its own beside the consensus handle.
//
// One inflater = one GPU, one non-blocking stream and INFL_SLOTS call slots.  A slot owns the device copies of one call (compressed bytes, block list, inflated
// bytes, statuses) and their page-locked staging.  ccsx_inflate_submit() validates the call, copies src and the block list into the slot's staging and enqueues
// upload -> k_inflate -> download; ccsx_inflate_wait() waits for the slot's event and copies every block's output range (nothing else) and the statuses to the
// caller.  Nothing here touches a ccsx_handle, and nothing of it runs unless a caller creates an inflater.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ccsx.h"
#include "ccsx_internal.h"
#include "inflate_core.h"

extern "C" int ccsx_launch_inflate(hipStream_t stream, const uint8_t *src, int64_t src_len, const ccsx_deflate_block *blk, int32_t n_blocks, uint8_t *dst,
                                   int64_t dst_len, int32_t *status);

#define HIPTRY(expr)                                                                                           \
    do {                                                                                                       \
        hipError_t e_ = (expr);                                                                                \
        if (e_ != hipSuccess) {                                                                                \
            ccsx_set_error(std::string(#expr) + ": " + hipGetErrorString(e_));                                 \
            return -2;                                                                                         \
        }                                                                                                      \
    } while (0)

#define INFL_SLOTS 2
#define INFL_RULE_VERSION 1

namespace {

struct InflSlot {
    uint8_t *d_src = nullptr, *d_dst = nullptr, *h_src = nullptr, *h_dst = nullptr;
    ccsx_deflate_block *d_blk = nullptr, *h_blk = nullptr;
    int32_t *d_status = nullptr, *h_status = nullptr;
    hipEvent_t done = nullptr;
    ccsx_ticket ticket = 0;         // 0 = free
    uint8_t *dst = nullptr;         // the caller's buffers of the call in flight
    int32_t *status = nullptr;
    int32_t n_blocks = 0;
    int64_t dst_len = 0;
};

}   // namespace

struct ccsx_inflater_s {
    int device = 0;
    int64_t max_in = 0, max_out = 0;
    int32_t max_blocks = 0;
    hipStream_t stream = nullptr;
    InflSlot slot[INFL_SLOTS];
    ccsx_ticket next_ticket = 1;
    std::vector<int32_t> order;     // scratch of the overlap check
};

// the argument errors of a call: nothing was enqueued when this fails
static int infl_check(const char *fn, const uint8_t *src, int64_t src_len, const ccsx_deflate_block *blocks, int32_t n_blocks, const uint8_t *dst, int64_t dst_len,
                      const int32_t *status, std::vector<int32_t> &order)
{
    const std::string f(fn);
    if (src_len < 0 || dst_len < 0 || n_blocks < 0) { ccsx_set_error(f + ": negative size"); return -1; }
    if ((n_blocks > 0 && (!blocks || !status)) || (src_len > 0 && !src) || (dst_len > 0 && !dst)) { ccsx_set_error(f + ": null argument"); return -1; }
    bool monotone = true;
    for (int32_t i = 0; i < n_blocks; ++i) {
        const ccsx_deflate_block &b = blocks[i];
        if (b.out_len < 0 || b.out_len > CCSX_INFLATE_MAX_OUT) { ccsx_set_error(f + ": block " + std::to_string(i) + ": out_len outside 0 .. 65536"); return -1; }
        if (b.in_len < 0 || b.in_off < 0 || b.in_off > src_len - b.in_len) { ccsx_set_error(f + ": block " + std::to_string(i) + ": input range outside src"); return -1; }
        if (b.out_off < 0 || b.out_off > dst_len - b.out_len) { ccsx_set_error(f + ": block " + std::to_string(i) + ": output range outside dst"); return -1; }
        if (i && b.out_off < blocks[i - 1].out_off + blocks[i - 1].out_len) monotone = false;
    }
    if (!monotone) {                 // (a BGZF reader's blocks are in order: the sort is for everyone else).  Empty blocks overlap nothing and are left out
        order.clear();
        for (int32_t i = 0; i < n_blocks; ++i) if (blocks[i].out_len > 0) order.push_back(i);
        std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return blocks[a].out_off < blocks[b].out_off; });
        for (size_t k = 1; k < order.size(); ++k) {
            const ccsx_deflate_block &p = blocks[order[k - 1]], &q = blocks[order[k]];
            if (q.out_off < p.out_off + p.out_len) {
                ccsx_set_error(f + ": blocks " + std::to_string(order[k - 1]) + " and " + std::to_string(order[k]) + ": output ranges overlap"); return -1;
            }
        }
    }
    return 0;
}

static void infl_free(ccsx_inflater f)
{
    if (!f) return;
    (void)hipSetDevice(f->device);
    if (f->stream) (void)hipStreamSynchronize(f->stream);
    for (InflSlot &s : f->slot) {
        if (s.d_src) (void)hipFree(s.d_src);
        if (s.d_dst) (void)hipFree(s.d_dst);
        if (s.d_blk) (void)hipFree(s.d_blk);
        if (s.d_status) (void)hipFree(s.d_status);
        if (s.h_src) (void)hipHostFree(s.h_src);
        if (s.h_dst) (void)hipHostFree(s.h_dst);
        if (s.h_blk) (void)hipHostFree(s.h_blk);
        if (s.h_status) (void)hipHostFree(s.h_status);
        if (s.done) (void)hipEventDestroy(s.done);
    }
    if (f->stream) (void)hipStreamDestroy(f->stream);
    delete f;
}

static int infl_create(ccsx_inflater f)
{
    // the priority machinery of ccsx_create: the engine's polish stream holds the device's highest priority, its draft streams the lowest.  The inflater takes the
    // lowest: its kernels are short and fill the CUs k_polish leaves (DESIGN.md §7 "GPU inflate" has the A/B); CCSX_INFLATE_PRIO=high|low|none overrides
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    const char *pe = getenv("CCSX_INFLATE_PRIO");
    if (pe && !strcmp(pe, "none")) HIPTRY(hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking));
    else HIPTRY(hipStreamCreateWithPriority(&f->stream, hipStreamNonBlocking, (pe && !strcmp(pe, "high")) ? prio_hi : prio_lo));
    for (InflSlot &s : f->slot) {
        const size_t in = (size_t)std::max<int64_t>(f->max_in, 1), out = (size_t)std::max<int64_t>(f->max_out, 1), nb = (size_t)std::max<int32_t>(f->max_blocks, 1);
        HIPTRY(hipMalloc((void **)&s.d_src, in + 16));
        HIPTRY(hipMalloc((void **)&s.d_dst, out + 16));
        HIPTRY(hipMalloc((void **)&s.d_blk, nb * sizeof(ccsx_deflate_block)));
        HIPTRY(hipMalloc((void **)&s.d_status, nb * sizeof(int32_t)));
        HIPTRY(hipHostMalloc((void **)&s.h_src, in, hipHostMallocDefault));
        HIPTRY(hipHostMalloc((void **)&s.h_dst, out, hipHostMallocDefault));
        HIPTRY(hipHostMalloc((void **)&s.h_blk, nb * sizeof(ccsx_deflate_block), hipHostMallocDefault));
        HIPTRY(hipHostMalloc((void **)&s.h_status, nb * sizeof(int32_t), hipHostMallocDefault));
        HIPTRY(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
    }
    return 0;
}

// upload -> k_inflate -> download of the call staged in slot s, and its event
static int infl_enqueue(ccsx_inflater f, InflSlot *s, int64_t src_len)
{
    const int32_t n_blocks = s->n_blocks;
    if (n_blocks > 0) {
        if (src_len > 0) HIPTRY(hipMemcpyAsync(s->d_src, s->h_src, (size_t)src_len, hipMemcpyHostToDevice, f->stream));
        HIPTRY(hipMemcpyAsync(s->d_blk, s->h_blk, (size_t)n_blocks * sizeof(ccsx_deflate_block), hipMemcpyHostToDevice, f->stream));
        if (ccsx_launch_inflate(f->stream, s->d_src, src_len, s->d_blk, n_blocks, s->d_dst, s->dst_len, s->d_status)) { ccsx_set_error("ccsx_inflate_submit: kernel launch failed"); return -2; }
        if (s->dst_len > 0) HIPTRY(hipMemcpyAsync(s->h_dst, s->d_dst, (size_t)s->dst_len, hipMemcpyDeviceToHost, f->stream));
        HIPTRY(hipMemcpyAsync(s->h_status, s->d_status, (size_t)n_blocks * sizeof(int32_t), hipMemcpyDeviceToHost, f->stream));
    }
    HIPTRY(hipEventRecord(s->done, f->stream));
    return 0;
}

extern "C" {

int ccsx_inflate_rule_version(void) { return INFL_RULE_VERSION; }

int ccsx_inflater_create(int device, int64_t max_in_bytes, int64_t max_out_bytes, int32_t max_blocks, ccsx_inflater *out)
{
    if (!out) { ccsx_set_error("ccsx_inflater_create: null argument"); return -1; }
    if (max_in_bytes < 1 || max_out_bytes < 1 || max_blocks < 1 || max_in_bytes > ((int64_t)1 << 32) || max_out_bytes > ((int64_t)1 << 32)) {
        ccsx_set_error("ccsx_inflater_create: capacities must be at least 1 (bytes: at most 4 GiB)"); return -1;
    }
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) { ccsx_set_error("ccsx_inflater_create: no HIP device available (ccsx_inflate_blocks_host is the host's decoder)"); return -2; }
    if (device < 0 || device >= n) { ccsx_set_error("ccsx_inflater_create: bad device ordinal"); return -1; }
    HIPTRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPTRY(hipGetDeviceProperties(&prop, device));
    if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos) {
        ccsx_set_error(std::string("ccsx_inflater_create: kernels are built for gfx950 only, device is ") + prop.gcnArchName);
        return -2;
    }
    ccsx_inflater f = new ccsx_inflater_s();
    f->device = device; f->max_in = max_in_bytes; f->max_out = max_out_bytes; f->max_blocks = max_blocks;
    const int rc = infl_create(f);
    if (rc) { infl_free(f); return rc; }
    *out = f;
    return 0;
}

int ccsx_inflater_destroy(ccsx_inflater f)
{
    infl_free(f);
    return 0;
}

int ccsx_inflate_submit(ccsx_inflater f, const uint8_t *src, int64_t src_len, const ccsx_deflate_block *blocks, int32_t n_blocks, uint8_t *dst, int64_t dst_len,
                        int32_t *status, ccsx_ticket *ticket)
{
    if (!f || !ticket) { ccsx_set_error("ccsx_inflate_submit: null argument"); return -1; }
    if (src_len > f->max_in || dst_len > f->max_out || n_blocks > f->max_blocks) {
        ccsx_set_error("ccsx_inflate_submit: the call exceeds the inflater's capacities (" + std::to_string(f->max_in) + " bytes in, " + std::to_string(f->max_out) +
                       " bytes out, " + std::to_string(f->max_blocks) + " blocks)");
        return -1;
    }
    if (int rc = infl_check("ccsx_inflate_submit", src, src_len, blocks, n_blocks, dst, dst_len, status, f->order)) return rc;
    InflSlot *s = nullptr;
    for (InflSlot &c : f->slot) if (!c.ticket) { s = &c; break; }
    if (!s) { ccsx_set_error("ccsx_inflate_submit: two tickets are in flight already: wait for one"); return -1; }
    HIPTRY(hipSetDevice(f->device));
    s->dst = dst; s->status = status; s->n_blocks = n_blocks; s->dst_len = dst_len;
    if (n_blocks > 0) {
        if (src_len > 0) std::memcpy(s->h_src, src, (size_t)src_len);
        std::memcpy(s->h_blk, blocks, (size_t)n_blocks * sizeof(ccsx_deflate_block));
    }
    if (const int rc = infl_enqueue(f, s, src_len)) { (void)hipStreamSynchronize(f->stream); return rc; }   // (what was enqueued reads the slot's staging: drain it)
    s->ticket = f->next_ticket++;
    *ticket = s->ticket;
    return 0;
}

int ccsx_inflate_wait(ccsx_inflater f, ccsx_ticket ticket)
{
    if (!f) { ccsx_set_error("ccsx_inflate_wait: null argument"); return -1; }
    InflSlot *s = nullptr;
    for (InflSlot &c : f->slot) if (c.ticket == ticket && ticket != 0) { s = &c; break; }
    if (!s) { ccsx_set_error("ccsx_inflate_wait: unknown or already waited-for ticket"); return -1; }
    HIPTRY(hipSetDevice(f->device));
    const hipError_t e = hipEventSynchronize(s->done);
    s->ticket = 0;
    if (e != hipSuccess) { ccsx_set_error(std::string("ccsx_inflate_wait: ") + hipGetErrorString(e)); return -2; }
    for (int32_t i = 0; i < s->n_blocks; ++i) {
        const ccsx_deflate_block &b = s->h_blk[i];
        s->status[i] = s->h_status[i];
        if (s->h_status[i] == CCSX_INFLATE_OK && b.out_len > 0) std::memcpy(s->dst + b.out_off, s->h_dst + b.out_off, (size_t)b.out_len);
    }
    return 0;
}

int ccsx_inflate_blocks(ccsx_inflater f, const uint8_t *src, int64_t src_len, const ccsx_deflate_block *blocks, int32_t n_blocks, uint8_t *dst, int64_t dst_len,
                        int32_t *status)
{
    ccsx_ticket t = 0;
    if (int rc = ccsx_inflate_submit(f, src, src_len, blocks, n_blocks, dst, dst_len, status, &t)) return rc;
    return ccsx_inflate_wait(f, t);
}

int ccsx_inflate_blocks_host(const uint8_t *src, int64_t src_len, const ccsx_deflate_block *blocks, int32_t n_blocks, uint8_t *dst, int64_t dst_len, int32_t *status)
{
    std::vector<int32_t> order;
    if (int rc = infl_check("ccsx_inflate_blocks_host", src, src_len, blocks, n_blocks, dst, dst_len, status, order)) return rc;
    static thread_local ccsx_infl_tables T;
    for (int32_t i = 0; i < n_blocks; ++i) {
        const ccsx_deflate_block &b = blocks[i];
        status[i] = ccsx_infl_stream_host(src + b.in_off, b.in_len, dst + b.out_off, b.out_len, &T);
    }
    return 0;
}

}   // extern "C"

// ccsx_deflate_api.cpp — the C ABI of the BGZF deflater (include/ccsx.h "BGZF deflate on the device"): an object of its own beside the consensus handle and the
// inflater.
//
// One deflater = one GPU, one non-blocking stream and DEFL_SLOTS call slots.  A slot owns the device copies of one call (plain bytes, span list, compressed bytes,
// lengths, CRCs, statuses) and their page-locked staging.  ccsx_deflate_submit() validates the call, copies src and the span list into the slot's staging and
// enqueues upload -> k_deflate -> download; ccsx_deflate_wait() waits for the slot's event and copies every OK span's stream (nothing else), the lengths, the CRCs
// and the statuses to the caller.  Nothing here touches a ccsx_handle, and nothing of it runs unless a caller creates a deflater.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ccsx.h"
#include "ccsx_internal.h"
#include "deflate_core.h"

extern "C" int ccsx_launch_deflate(hipStream_t stream, const uint8_t *src, int64_t src_len, const ccsx_deflate_span *span, int32_t n_spans, uint8_t *dst,
                                   int64_t dst_len, int32_t *out_len, uint32_t *crc, int32_t *status);

#define HIPTRY(expr)                                                                                           \
    do {                                                                                                       \
        hipError_t e_ = (expr);                                                                                \
        if (e_ != hipSuccess) {                                                                                \
            ccsx_set_error(std::string(#expr) + ": " + hipGetErrorString(e_));                                 \
            return -2;                                                                                         \
        }                                                                                                      \
    } while (0)

#define DEFL_SLOTS 2
#define DEFL_WG_PER_CU 1             // k_deflate holds about 147 KiB of LDS: one workgroup per CU

static_assert(CCSX_DEFL_MAX_IN == CCSX_DEFLATE_MAX_IN, "deflate_core.h and ccsx.h disagree on the span limit");

namespace {

struct DeflSlot {
    uint8_t *d_src = nullptr, *d_dst = nullptr, *h_src = nullptr, *h_dst = nullptr;
    ccsx_deflate_span *d_span = nullptr, *h_span = nullptr;
    int32_t *d_res = nullptr, *h_res = nullptr;   // out_len[n], crc[n], status[n] behind one another (max_spans each)
    hipEvent_t done = nullptr;
    ccsx_ticket ticket = 0;         // 0 = free
    uint8_t *dst = nullptr;         // the caller's buffers of the call in flight
    int32_t *out_len = nullptr, *status = nullptr;
    uint32_t *crc = nullptr;
    int32_t n_spans = 0;
    int64_t dst_len = 0;
};

}   // namespace

struct ccsx_deflater_s {
    int device = 0;
    int64_t max_in = 0, max_out = 0;
    int32_t max_spans = 0;
    hipStream_t stream = nullptr;
    DeflSlot slot[DEFL_SLOTS];
    ccsx_ticket next_ticket = 1;
    std::vector<int32_t> order;     // scratch of the overlap check
};

// the argument errors of a call: nothing was enqueued when this fails
static int defl_check(const char *fn, const uint8_t *src, int64_t src_len, const ccsx_deflate_span *spans, int32_t n_spans, const uint8_t *dst, int64_t dst_len,
                      const int32_t *out_len, const uint32_t *crc, const int32_t *status, std::vector<int32_t> &order)
{
    const std::string f(fn);
    if (src_len < 0 || dst_len < 0 || n_spans < 0) { ccsx_set_error(f + ": negative size"); return -1; }
    if ((n_spans > 0 && (!spans || !status || !out_len || !crc)) || (src_len > 0 && !src) || (dst_len > 0 && !dst)) { ccsx_set_error(f + ": null argument"); return -1; }
    bool monotone = true;
    for (int32_t i = 0; i < n_spans; ++i) {
        const ccsx_deflate_span &b = spans[i];
        if (b.in_len < 0 || b.in_len > CCSX_DEFLATE_MAX_IN) { ccsx_set_error(f + ": span " + std::to_string(i) + ": in_len outside 0 .. 65536"); return -1; }
        if (b.in_off < 0 || b.in_off > src_len - b.in_len) { ccsx_set_error(f + ": span " + std::to_string(i) + ": input range outside src"); return -1; }
        if (b.out_cap < 0 || b.out_off < 0 || b.out_off > dst_len - b.out_cap) { ccsx_set_error(f + ": span " + std::to_string(i) + ": output range outside dst"); return -1; }
        if (i && b.out_off < spans[i - 1].out_off + spans[i - 1].out_cap) monotone = false;
    }
    if (!monotone) {                 // (a BGZF writer's spans are in order: the sort is for everyone else).  Empty ranges overlap nothing and are left out
        order.clear();
        for (int32_t i = 0; i < n_spans; ++i) if (spans[i].out_cap > 0) order.push_back(i);
        std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return spans[a].out_off < spans[b].out_off; });
        for (size_t k = 1; k < order.size(); ++k) {
            const ccsx_deflate_span &p = spans[order[k - 1]], &q = spans[order[k]];
            if (q.out_off < p.out_off + p.out_cap) {
                ccsx_set_error(f + ": spans " + std::to_string(order[k - 1]) + " and " + std::to_string(order[k]) + ": output ranges overlap"); return -1;
            }
        }
    }
    return 0;
}

static void defl_free(ccsx_deflater f)
{
    if (!f) return;
    (void)hipSetDevice(f->device);
    if (f->stream) (void)hipStreamSynchronize(f->stream);
    for (DeflSlot &s : f->slot) {
        if (s.d_src) (void)hipFree(s.d_src);
        if (s.d_dst) (void)hipFree(s.d_dst);
        if (s.d_span) (void)hipFree(s.d_span);
        if (s.d_res) (void)hipFree(s.d_res);
        if (s.h_src) (void)hipHostFree(s.h_src);
        if (s.h_dst) (void)hipHostFree(s.h_dst);
        if (s.h_span) (void)hipHostFree(s.h_span);
        if (s.h_res) (void)hipHostFree(s.h_res);
        if (s.done) (void)hipEventDestroy(s.done);
    }
    if (f->stream) (void)hipStreamDestroy(f->stream);
    delete f;
}

static int defl_create(ccsx_deflater f)
{
    // as the inflater: the lowest stream priority of the device, so that the engine's polish stream keeps its CUs
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    HIPTRY(hipStreamCreateWithPriority(&f->stream, hipStreamNonBlocking, prio_lo));
    for (DeflSlot &s : f->slot) {
        const size_t in = (size_t)std::max<int64_t>(f->max_in, 1), out = (size_t)std::max<int64_t>(f->max_out, 1), nb = (size_t)std::max<int32_t>(f->max_spans, 1);
        HIPTRY(hipMalloc((void **)&s.d_src, in + 16));
        HIPTRY(hipMalloc((void **)&s.d_dst, out + 16));
        HIPTRY(hipMalloc((void **)&s.d_span, nb * sizeof(ccsx_deflate_span)));
        HIPTRY(hipMalloc((void **)&s.d_res, 3 * nb * sizeof(int32_t)));
        HIPTRY(hipHostMalloc((void **)&s.h_src, in, hipHostMallocDefault));
        HIPTRY(hipHostMalloc((void **)&s.h_dst, out, hipHostMallocDefault));
        HIPTRY(hipHostMalloc((void **)&s.h_span, nb * sizeof(ccsx_deflate_span), hipHostMallocDefault));
        HIPTRY(hipHostMalloc((void **)&s.h_res, 3 * nb * sizeof(int32_t), hipHostMallocDefault));
        HIPTRY(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
    }
    return 0;
}

// upload -> k_deflate -> download of the call staged in slot s, and its event
static int defl_enqueue(ccsx_deflater f, DeflSlot *s, int64_t src_len)
{
    const int32_t n = s->n_spans;
    const size_t nb = (size_t)std::max<int32_t>(f->max_spans, 1);
    if (n > 0) {
        if (src_len > 0) HIPTRY(hipMemcpyAsync(s->d_src, s->h_src, (size_t)src_len, hipMemcpyHostToDevice, f->stream));
        HIPTRY(hipMemcpyAsync(s->d_span, s->h_span, (size_t)n * sizeof(ccsx_deflate_span), hipMemcpyHostToDevice, f->stream));
        if (ccsx_launch_deflate(f->stream, s->d_src, src_len, s->d_span, n, s->d_dst, s->dst_len, s->d_res, (uint32_t *)(s->d_res + nb), s->d_res + 2 * nb)) {
            ccsx_set_error("ccsx_deflate_submit: kernel launch failed"); return -2;
        }
        if (s->dst_len > 0) HIPTRY(hipMemcpyAsync(s->h_dst, s->d_dst, (size_t)s->dst_len, hipMemcpyDeviceToHost, f->stream));
        HIPTRY(hipMemcpyAsync(s->h_res, s->d_res, 3 * nb * sizeof(int32_t), hipMemcpyDeviceToHost, f->stream));
    }
    HIPTRY(hipEventRecord(s->done, f->stream));
    return 0;
}

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
    if (!out) { ccsx_set_error("ccsx_deflater_create: null argument"); return -1; }
    if (max_in_bytes < 1 || max_out_bytes < 1 || max_spans < 1 || max_in_bytes > ((int64_t)1 << 32) || max_out_bytes > ((int64_t)1 << 32)) {
        ccsx_set_error("ccsx_deflater_create: capacities must be at least 1 (bytes: at most 4 GiB)"); return -1;
    }
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) { ccsx_set_error("ccsx_deflater_create: no HIP device available (ccsx_deflate_spans_host is the host's encoder)"); return -2; }
    if (device < 0 || device >= n) { ccsx_set_error("ccsx_deflater_create: bad device ordinal"); return -1; }
    HIPTRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPTRY(hipGetDeviceProperties(&prop, device));
    if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos) {
        ccsx_set_error(std::string("ccsx_deflater_create: kernels are built for gfx950 only, device is ") + prop.gcnArchName);
        return -2;
    }
    ccsx_deflater f = new ccsx_deflater_s();
    f->device = device; f->max_in = max_in_bytes; f->max_out = max_out_bytes; f->max_spans = max_spans;
    const int rc = defl_create(f);
    if (rc) { defl_free(f); return rc; }
    *out = f;
    return 0;
}

int ccsx_deflater_destroy(ccsx_deflater f)
{
    defl_free(f);
    return 0;
}

int ccsx_deflate_submit(ccsx_deflater f, const uint8_t *src, int64_t src_len, const ccsx_deflate_span *spans, int32_t n_spans, uint8_t *dst, int64_t dst_len,
                        int32_t *out_len, uint32_t *crc, int32_t *status, ccsx_ticket *ticket)
{
    if (!f || !ticket) { ccsx_set_error("ccsx_deflate_submit: null argument"); return -1; }
    if (src_len > f->max_in || dst_len > f->max_out || n_spans > f->max_spans) {
        ccsx_set_error("ccsx_deflate_submit: the call exceeds the deflater's capacities (" + std::to_string(f->max_in) + " bytes in, " + std::to_string(f->max_out) +
                       " bytes out, " + std::to_string(f->max_spans) + " spans)");
        return -1;
    }
    if (int rc = defl_check("ccsx_deflate_submit", src, src_len, spans, n_spans, dst, dst_len, out_len, crc, status, f->order)) return rc;
    DeflSlot *s = nullptr;
    for (DeflSlot &c : f->slot) if (!c.ticket) { s = &c; break; }
    if (!s) { ccsx_set_error("ccsx_deflate_submit: two tickets are in flight already: wait for one"); return -1; }
    HIPTRY(hipSetDevice(f->device));
    s->dst = dst; s->out_len = out_len; s->crc = crc; s->status = status; s->n_spans = n_spans; s->dst_len = dst_len;
    if (n_spans > 0) {
        if (src_len > 0) std::memcpy(s->h_src, src, (size_t)src_len);
        std::memcpy(s->h_span, spans, (size_t)n_spans * sizeof(ccsx_deflate_span));
    }
    if (const int rc = defl_enqueue(f, s, src_len)) { (void)hipStreamSynchronize(f->stream); return rc; }   // (what was enqueued reads the slot's staging: drain it)
    s->ticket = f->next_ticket++;
    *ticket = s->ticket;
    return 0;
}

int ccsx_deflate_wait(ccsx_deflater f, ccsx_ticket ticket)
{
    if (!f) { ccsx_set_error("ccsx_deflate_wait: null argument"); return -1; }
    DeflSlot *s = nullptr;
    for (DeflSlot &c : f->slot) if (c.ticket == ticket && ticket != 0) { s = &c; break; }
    if (!s) { ccsx_set_error("ccsx_deflate_wait: unknown or already waited-for ticket"); return -1; }
    HIPTRY(hipSetDevice(f->device));
    const hipError_t e = hipEventSynchronize(s->done);
    s->ticket = 0;
    if (e != hipSuccess) { ccsx_set_error(std::string("ccsx_deflate_wait: ") + hipGetErrorString(e)); return -2; }
    const size_t nb = (size_t)std::max<int32_t>(f->max_spans, 1);
    for (int32_t i = 0; i < s->n_spans; ++i) {
        const ccsx_deflate_span &b = s->h_span[i];
        const int32_t st = s->h_res[2 * nb + i];
        int32_t n = s->h_res[i];
        if (st != CCSX_DEFLATE_OK || n < 0 || n > b.out_cap) n = 0;
        s->status[i] = st;
        s->out_len[i] = n;
        s->crc[i] = (uint32_t)s->h_res[nb + i];
        if (n > 0) std::memcpy(s->dst + b.out_off, s->h_dst + b.out_off, (size_t)n);
    }
    return 0;
}

int ccsx_deflate_spans(ccsx_deflater f, const uint8_t *src, int64_t src_len, const ccsx_deflate_span *spans, int32_t n_spans, uint8_t *dst, int64_t dst_len,
                       int32_t *out_len, uint32_t *crc, int32_t *status)
{
    ccsx_ticket t = 0;
    if (int rc = ccsx_deflate_submit(f, src, src_len, spans, n_spans, dst, dst_len, out_len, crc, status, &t)) return rc;
    return ccsx_deflate_wait(f, t);
}

int ccsx_deflate_spans_host(const uint8_t *src, int64_t src_len, const ccsx_deflate_span *spans, int32_t n_spans, uint8_t *dst, int64_t dst_len, int32_t *out_len,
                            uint32_t *crc, int32_t *status)
{
    std::vector<int32_t> order;
    if (int rc = defl_check("ccsx_deflate_spans_host", src, src_len, spans, n_spans, dst, dst_len, out_len, crc, status, order)) return rc;
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

// codec_host.h — the host side of a ticketed codec service on one GPU, written once for the BGZF inflater and deflater (ccsx_inflate_api.cpp,
// ccsx_deflate_api.cpp; DESIGN.md §2 "Codec host").
//
// One codec object = one GPU, one non-blocking stream and CODEC_SLOTS call slots.  A slot owns the device copies of one call (input bytes, item list, output bytes,
// result words) and their page-locked staging.  codec_submit() validates the call (codec_check.h), copies src and the item list into the slot's staging and
// enqueues upload -> kernel -> download -> event; codec_wait() waits for the slot's event and copies the results and, of every item, the bytes its codec says are
// its own (nothing else) to the caller.  Nothing here touches a ccsx_handle.
//
// A codec is described by a struct D over the item description of codec_check.h:
//   object, create_name, submit_name, wait_name, host_hint   the nouns and exported names of the messages
//   Results, results_ok()          the caller's result arrays of a call
//   planes, down_words(n, cap)     the result area is `planes` planes of max_items int32 each; the words of it a call of n items downloads
//   read_prio                      whether CCSX_INFLATE_PRIO=high|low|none overrides the stream's priority
//   launch()                       the kernel over a staged call, its result planes at res, res + cap, ...
//   take()                         after the download: item i's results to the caller; returns the bytes of its output range that go to the caller's dst
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ccsx.h"
#include "ccsx_internal.h"
#include "codec_check.h"

#define CODEC_SLOTS 2

template <typename D> struct CodecSlot {
    using Item = typename D::Item;
    uint8_t *d_src = nullptr, *d_dst = nullptr, *h_src = nullptr, *h_dst = nullptr;
    Item *d_item = nullptr, *h_item = nullptr;
    int32_t *d_res = nullptr, *h_res = nullptr;   // D::planes planes behind one another (max_items words each)
    hipEvent_t done = nullptr;
    ccsx_ticket ticket = 0;         // 0 = free
    uint8_t *dst = nullptr;         // the caller's buffers of the call in flight
    typename D::Results out{};
    int32_t n = 0;
    int64_t dst_len = 0;
};

template <typename D> struct CodecHost {
    using Codec = D;
    int device = 0;
    int64_t max_in = 0, max_out = 0;
    int32_t max_items = 0;
    hipStream_t stream = nullptr;
    CodecSlot<D> slot[CODEC_SLOTS];
    ccsx_ticket next_ticket = 1;
    std::vector<int32_t> order;     // scratch of the overlap check
    size_t plane() const { return (size_t)std::max<int32_t>(max_items, 1); }
};

// What a codec's create does first: makes `device` current if it is there and a gfx950.  `fn` is the exported function's name, `hint` what its "no HIP
// device available (...)" says in the brackets.  -1: bad ordinal, -2: no device, a HIP failure or another architecture.  ccsx_create (ccsx_api.cpp) keeps its
// own copy of these lines on purpose: it is the one piece of this check that a run without a codec executes, and it stays the code it was
static inline int codec_use_gfx950_device(int device, const char *fn, const char *hint)
{
    const std::string f(fn);
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) { ccsx_set_error(f + ": no HIP device available (" + hint + ")"); return -2; }
    if (device < 0 || device >= n) { ccsx_set_error(f + ": bad device ordinal"); return -1; }
    HIPTRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPTRY(hipGetDeviceProperties(&prop, device));
    if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos) {
        ccsx_set_error(f + ": kernels are built for gfx950 only, device is " + prop.gcnArchName);
        return -2;
    }
    return 0;
}

template <typename H> static void codec_free(H *f)
{
    if (!f) return;
    (void)hipSetDevice(f->device);
    if (f->stream) (void)hipStreamSynchronize(f->stream);
    for (auto &s : f->slot) {
        for (void *p : {(void *)s.d_src, (void *)s.d_dst, (void *)s.d_item, (void *)s.d_res}) if (p) (void)hipFree(p);
        for (void *p : {(void *)s.h_src, (void *)s.h_dst, (void *)s.h_item, (void *)s.h_res}) if (p) (void)hipHostFree(p);
        if (s.done) (void)hipEventDestroy(s.done);
    }
    if (f->stream) (void)hipStreamDestroy(f->stream);
    delete f;
}

template <typename H> static int codec_alloc(H *f)
{
    using D = typename H::Codec;
    // the priority machinery of ccsx_create: the engine's polish stream holds the device's highest priority, its draft streams the lowest.  A codec takes the
    // lowest: its kernels are short and fill the CUs k_polish leaves (DESIGN.md §7 "GPU inflate" has the A/B); for the inflater CCSX_INFLATE_PRIO=high|low|none
    // overrides
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    const char *pe = D::read_prio ? getenv("CCSX_INFLATE_PRIO") : nullptr;
    if (pe && !strcmp(pe, "none")) HIPTRY(hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking));
    else HIPTRY(hipStreamCreateWithPriority(&f->stream, hipStreamNonBlocking, (pe && !strcmp(pe, "high")) ? prio_hi : prio_lo));
    for (auto &s : f->slot) {
        const size_t in = (size_t)std::max<int64_t>(f->max_in, 1), out = (size_t)std::max<int64_t>(f->max_out, 1), nb = f->plane();
        HIPTRY(hipMalloc((void **)&s.d_src, in + 16));
        HIPTRY(hipMalloc((void **)&s.d_dst, out + 16));
        HIPTRY(hipMalloc((void **)&s.d_item, nb * sizeof(typename D::Item)));
        HIPTRY(hipMalloc((void **)&s.d_res, D::planes * nb * sizeof(int32_t)));
        HIPTRY(hipHostMalloc((void **)&s.h_src, in, hipHostMallocDefault));
        HIPTRY(hipHostMalloc((void **)&s.h_dst, out, hipHostMallocDefault));
        HIPTRY(hipHostMalloc((void **)&s.h_item, nb * sizeof(typename D::Item), hipHostMallocDefault));
        HIPTRY(hipHostMalloc((void **)&s.h_res, D::planes * nb * sizeof(int32_t), hipHostMallocDefault));
        HIPTRY(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
    }
    return 0;
}

// upload -> kernel -> download of the call staged in slot s, and its event
template <typename H> static int codec_enqueue(H *f, CodecSlot<typename H::Codec> *s, int64_t src_len)
{
    using D = typename H::Codec;
    const int32_t n = s->n;
    if (n > 0) {
        if (src_len > 0) HIPTRY(hipMemcpyAsync(s->d_src, s->h_src, (size_t)src_len, hipMemcpyHostToDevice, f->stream));
        HIPTRY(hipMemcpyAsync(s->d_item, s->h_item, (size_t)n * sizeof(typename D::Item), hipMemcpyHostToDevice, f->stream));
        if (D::launch(f->stream, s->d_src, src_len, s->d_item, n, s->d_dst, s->dst_len, s->d_res, f->plane())) {
            ccsx_set_error(std::string(D::submit_name) + ": kernel launch failed"); return -2;
        }
        if (s->dst_len > 0) HIPTRY(hipMemcpyAsync(s->h_dst, s->d_dst, (size_t)s->dst_len, hipMemcpyDeviceToHost, f->stream));
        HIPTRY(hipMemcpyAsync(s->h_res, s->d_res, D::down_words((size_t)n, f->plane()) * sizeof(int32_t), hipMemcpyDeviceToHost, f->stream));
    }
    HIPTRY(hipEventRecord(s->done, f->stream));
    return 0;
}

template <typename H> static int codec_create(int device, int64_t max_in_bytes, int64_t max_out_bytes, int32_t max_items, H **out)
{
    using D = typename H::Codec;
    const std::string fn(D::create_name);
    if (!out) { ccsx_set_error(fn + ": null argument"); return -1; }
    if (max_in_bytes < 1 || max_out_bytes < 1 || max_items < 1 || max_in_bytes > ((int64_t)1 << 32) || max_out_bytes > ((int64_t)1 << 32)) {
        ccsx_set_error(fn + ": capacities must be at least 1 (bytes: at most 4 GiB)"); return -1;
    }
    if (const int rc = codec_use_gfx950_device(device, D::create_name, D::host_hint)) return rc;
    H *f = new H();
    f->device = device; f->max_in = max_in_bytes; f->max_out = max_out_bytes; f->max_items = max_items;
    const int rc = codec_alloc(f);
    if (rc) { codec_free(f); return rc; }
    *out = f;
    return 0;
}

template <typename H> static int codec_submit(H *f, const uint8_t *src, int64_t src_len, const typename H::Codec::Item *items, int32_t n, uint8_t *dst, int64_t dst_len,
                                              const typename H::Codec::Results &res, ccsx_ticket *ticket)
{
    using D = typename H::Codec;
    const std::string fn(D::submit_name);
    if (!f || !ticket) { ccsx_set_error(fn + ": null argument"); return -1; }
    if (src_len > f->max_in || dst_len > f->max_out || n > f->max_items) {
        ccsx_set_error(fn + ": the call exceeds the " + D::object + "'s capacities (" + std::to_string(f->max_in) + " bytes in, " + std::to_string(f->max_out) +
                       " bytes out, " + std::to_string(f->max_items) + " " + D::noun + "s)");
        return -1;
    }
    if (int rc = ccsx_codec_check<D>(D::submit_name, src, src_len, items, n, dst, dst_len, D::results_ok(res), f->order)) return rc;
    CodecSlot<D> *s = nullptr;
    for (auto &c : f->slot) if (!c.ticket) { s = &c; break; }
    if (!s) { ccsx_set_error(fn + ": two tickets are in flight already: wait for one"); return -1; }
    HIPTRY(hipSetDevice(f->device));
    s->dst = dst; s->out = res; s->n = n; s->dst_len = dst_len;
    if (n > 0) {
        if (src_len > 0) std::memcpy(s->h_src, src, (size_t)src_len);
        std::memcpy(s->h_item, items, (size_t)n * sizeof(typename D::Item));
    }
    if (const int rc = codec_enqueue(f, s, src_len)) { (void)hipStreamSynchronize(f->stream); return rc; }   // (what was enqueued reads the slot's staging: drain it)
    s->ticket = f->next_ticket++;
    *ticket = s->ticket;
    return 0;
}

template <typename H> static int codec_wait(H *f, ccsx_ticket ticket)
{
    using D = typename H::Codec;
    const std::string fn(D::wait_name);
    if (!f) { ccsx_set_error(fn + ": null argument"); return -1; }
    CodecSlot<D> *s = nullptr;
    for (auto &c : f->slot) if (c.ticket == ticket && ticket != 0) { s = &c; break; }
    if (!s) { ccsx_set_error(fn + ": unknown or already waited-for ticket"); return -1; }
    HIPTRY(hipSetDevice(f->device));
    const hipError_t e = hipEventSynchronize(s->done);
    s->ticket = 0;                   // (the slot is free again whatever the event says)
    if (e != hipSuccess) { ccsx_set_error(fn + ": " + hipGetErrorString(e)); return -2; }
    for (int32_t i = 0; i < s->n; ++i) {
        const typename D::Item &b = s->h_item[i];
        const int32_t bytes = D::take(b, i, s->h_res, f->plane(), s->out);
        if (bytes > 0) std::memcpy(s->dst + b.out_off, s->h_dst + b.out_off, (size_t)bytes);
    }
    return 0;
}

// the synchronous call: submit and wait
template <typename H> static int codec_run(H *f, const uint8_t *src, int64_t src_len, const typename H::Codec::Item *items, int32_t n, uint8_t *dst, int64_t dst_len,
                                           const typename H::Codec::Results &res)
{
    ccsx_ticket t = 0;
    if (int rc = codec_submit(f, src, src_len, items, n, dst, dst_len, res, &t)) return rc;
    return codec_wait(f, t);
}

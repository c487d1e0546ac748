// ccsx_api.cpp — C ABI over the HIP kernels: handle lifecycle, HBM layout, the asynchronous batch pipeline.
//
// One handle = one GPU, four HIP streams (H2D, draft stage, polish stage, D2H) and CCSX_SLOTS batch slots.  A slot owns
// the device copies of one batch (inputs, host-derived layout, per-ZMW state, outputs) and the page-locked host arrays its
// asynchronous uploads read from; the large POA / alignment scratch is shared: only the draft stage touches it, and the
// draft stages of all batches run back to back on the draft stream.  ccsx_submit() enqueues upload -> draft stage ->
// polish stage -> download of a batch and returns; while batch k is polished, batch k+1 uploads and is drafted / aligned
// and batch k-1 downloads (submit/wait tickets, double-buffered staging; the two-stage queue of
// docs/img/ccs-impl.png).  The synchronous entry points (upload / run / sync / download, consensus_batch) are the
// same machinery on slot 0.  There is no CPU fallback: without a usable device every entry point fails with a
// message (ccsx_last_error).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <mutex>
#include <string>
#include <vector>

#include "ccsx.h"
#include "ccsx_internal.h"
#include "ccsx_kernels.h"
#include "refine_core.h"

#define CCSX_SLOTS 3

namespace {

// a device buffer and a page-locked host array (below) free themselves: a slot's buffers are named where they are declared and nowhere else.  Their owners die in
// destroy_handle(), with the handle's device current and its streams drained
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    int reserve(size_t bytes)
    {
        if (bytes <= cap) return 0;
        // the new block first: a failed growth leaves the old buffer (and every KParams that points into it) intact
        // (a buffer that has to grow AGAIN belongs to a stream of unequal batches — the driver's cost-binned tickets of a mixed run: every regrowth is a
        // synchronous hipMalloc + hipFree, for the shared POA scratch tens of GB behind a stream synchronisation — so regrowth takes half as much again)
        // (the headroom is capped at 1 GB, and a request that fails WITH headroom is repeated at the exact size before anything is given up — the
        // POA scratch is sized to 3/4 of the handle's budget, half as much again may simply not exist)
        const size_t head = std::min<size_t>(p ? bytes / 2 : bytes / 8, (size_t)1 << 30);
        size_t want = bytes + head + 256;
        void *np_ = nullptr;
        hipError_t e = hipMalloc(&np_, want);
        if (e != hipSuccess) { (void)hipGetLastError(); want = bytes + 256; e = hipMalloc(&np_, want); }
        if (e != hipSuccess && p) {                      // not enough room for both: give the old block back and try once more, with and without headroom
            (void)hipGetLastError();
            (void)hipFree(p); p = nullptr; cap = 0;
            want = bytes + head + 256;
            e = hipMalloc(&np_, want);
            if (e != hipSuccess) { (void)hipGetLastError(); want = bytes + 256; e = hipMalloc(&np_, want); }
        }
        if (e != hipSuccess) { (void)hipGetLastError(); ccsx_set_error(std::string("hipMalloc(") + std::to_string(want) + "): " + hipGetErrorString(e)); return -2; }
        if (p) (void)hipFree(p);
        p = np_; cap = want;
        return 0;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

// grow-only page-locked host array: the source of asynchronous H2D copies must outlive the call that enqueues them
template <typename T> struct PinVec {
    T *p = nullptr;
    size_t cap = 0, n = 0;
    PinVec() = default;
    PinVec(const PinVec &) = delete;
    PinVec &operator=(const PinVec &) = delete;
    ~PinVec() { release(); }
    int assign(size_t count, T fill)
    {
        if (resize(count)) return -2;
        std::fill(p, p + count, fill);
        return 0;
    }
    int resize(size_t count)
    {
        if (count > cap) {
            if (p) (void)hipHostFree(p);
            p = nullptr; cap = 0;
            const size_t want = count + count / 8 + 64;
            hipError_t e = hipHostMalloc((void **)&p, want * sizeof(T), hipHostMallocDefault);
            if (e != hipSuccess) { ccsx_set_error(std::string("hipHostMalloc(") + std::to_string(want * sizeof(T)) + "): " + hipGetErrorString(e)); return -2; }
            cap = want;
        }
        n = count;
        return 0;
    }
    T &operator[](size_t i) { return p[i]; }
    const T &operator[](size_t i) const { return p[i]; }
    size_t size() const { return n; }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = n = 0; }
};

// the batch-level figures of a staged batch, each computed once: the largest per-ZMW capacities (ccsx_zmw_caps), the most passes of a ZMW after the top_passes
// cap, k_align16's work items, and the totals of the capacity layout
struct BatchTotals {
    int64_t maxL_max = 1, vcap_max = 1, dcap_max = 0;
    int need_max = 2, nr_max = 1, n_quads = 0;
    int64_t total_wslots = 0, cap_total = 0;
};

struct Slot {
    // inputs
    DevBuf d_snr, d_read_off, d_base_off, d_bases, d_pw, d_ipd, d_flags;
    // layout
    DevBuf d_read_zmw, d_vcap, d_dcap, d_seq_off, d_wb_off, d_ent_off, d_wslot, d_zperm, d_rperm, d_quads, d_retry;
    // state
    DevBuf d_tabME, d_tabINS, d_tabDL, d_tabZ, d_dmask, d_draft, d_zmw_i32 /* 7 x n int32 */, d_wbounds, d_ticket;
    DevBuf d_avalid, d_ascore, d_ent;
    DevBuf d_wseq, d_wqv, d_wsum, d_wmeta;
    DevBuf d_out_seq, d_out_qual, d_out_raw, d_out_i32 /* 6 x n */, d_out_f32 /* 2 x n */;
    DevBuf d_wtpl, d_wtmeta, d_wkin, d_out_kin;   // HiFi kinetics only (d_wtpl, d_wtmeta: also the pileup summary)
    DevBuf d_wpile, d_out_pile;                   // pileup summary only (ccsx_consensus_pileup / ccsx_submit_pileup)
    DevBuf d_tflag, d_tlen;                       // tandem repeats only (ccsx_extras with tandem_len or a threshold)
    DevBuf d_din_len, d_din_bb;                   // caller-supplied drafts (ccsx_polish_batch): lengths, orientation references
    DevBuf d_hd_wcnt, d_hd_wrec, d_hd_wminp, d_hd_isite, d_hd_zi, d_hd_minp, d_hd_sites;   // heteroduplex finder only (ccsx_hd_batch)
    DevBuf d_train;                               // model training only (ccsx_train_batch): [n][400] + [n] int64, then [3][n] int32
    DevBuf d_fold;                                // adapter palindromes only (ccsx_fold_request): [4][n] report
    DevBuf d_adapt;                               // adapter screen only (ccsx_adapter_request): [9][n] report + [n][16] hits
    DevBuf d_ctl;                                 // control screen only (ccsx_control_request): the slot's own index, then the [8][n] report
    DevBuf d_cov;                                 // coverage screen only (ccsx_coverage_request): the [10][n] report, then one byte per window slot
    DevBuf d_poa_log;                             // POA log only (ccsx_poa_log): [n][2][max_reads] records of CCSX_POA_LOG_WORDS int32
    DevBuf d_ho, d_ho_out;                        // polisher hand-off only (ccsx_handoff_request): counts, tile ranks / slots, qual sums, core offsets; the output arrays
    DevBuf d_orient;                              // pass orientation only (a batch with a CCSX_PASS_STRAND_UNKNOWN pass): [n] anchors, [2][R] votes, [2][R] strand / call
    DevBuf d_pattern;                             // barcode calls, segmentation or cDNA reads only (a ticket carries one of them): the packed set, then the report
    DevBuf d_rp;                                  // representative reads only (ccsx_represent_request): the [2][n] report
    DevBuf d_rf_tiles, d_rf_base, d_rf_rep;       // polisher hand-back only (ccsx_submit_refine): the tile list and its classes; base lengths, backbones, seq, qual; the report
    RefineParams RP{};                            // ... its kernels' parameters as enqueued (the report's download reads them)
    // host copies of the layout (page-locked: sources of the asynchronous uploads)
    PinVec<int32_t> read_zmw, vcap, dcap, zperm, rperm, wb_off, read_off, quads, qperm;
    PinVec<int64_t> seq_off, ent_off, base_off;
    PinVec<uint32_t> ctl_index;                   // control screen only: the index as uploaded (a ticket's control is its own: three may be in flight)
    PinVec<unsigned long long> pattern_set;       // barcode calls, segmentation or cDNA reads only: the packed set as uploaded (a ticket's set is its own, as its control is)
    PinVec<int32_t> anchor;                       // pass orientation only: the anchor pass of every ZMW as uploaded
    bool orient_pending = false, orient_ran = false;   // the staged batch carries the bit and k_orient has yet to run on it / has run (its report is on the device)
    KParams P;
    hipEvent_t ev[CCSX_EV_COUNT] = {}, ev_up = nullptr, ev_done = nullptr;   // ev: the stage events (ccsx_stage_event)
    hipEvent_t ev_aux[CCSX_ORD_COUNT] = {};                                  // the ordering events of the second stream (ccsx_order_event)
    bool staged = false, ran = false, inflight = false;
    bool tm_ok = false; ccsx_timings tm{};   // the slot's timings as taken by retire() (valid until the slot is staged again)
    ccsx_results *res = nullptr;      // destination of an in-flight submit (cleared by retire(): the caller's struct is not touched again)
    ccsx_drafts *drafts_out = nullptr; // ... of an in-flight ccsx_submit_draft
    int mode = CCSX_RUN_FUSED;
    int64_t ticket = -1;
    BatchTotals T;                    // batch-level figures of the staged batch (layout)

    void release()                    // (the buffers free themselves)
    {
        for (auto &e : ev) if (e) { (void)hipEventDestroy(e); e = nullptr; }
        for (auto &e : ev_aux) if (e) { (void)hipEventDestroy(e); e = nullptr; }
        if (ev_up) { (void)hipEventDestroy(ev_up); ev_up = nullptr; }
        if (ev_done) { (void)hipEventDestroy(ev_done); ev_done = nullptr; }
    }
};

// POA / alignment scratch is sized from the free memory of the device; handles created on the same device by
// different host threads must not all claim the same free bytes: sizing is serialised per process.
std::mutex g_scratch_mutex;

// a buffer of [k][n] planes, reserved for the k pointers of `dst`, which are set to its planes in order
template <typename T> int carve_planes(std::initializer_list<T **> dst, DevBuf &buf, size_t n)
{
    if (buf.reserve(dst.size() * n * sizeof(T))) return -2;
    T *p = (T *)buf.p;
    for (T **d : dst) { *d = p; p += n; }
    return 0;
}

}  // namespace

struct ccsx_handle_s {
    int device = 0;
    hipStream_t s_in = nullptr, s_draft = nullptr, s_comp = nullptr, s_out = nullptr;   // s_comp: polish stage (and the synchronous calls' copies)
    hipStream_t s_aux = nullptr;                              // second stream of the POA stage (forked from and joined into s_draft inside one launch)
    hipEvent_t ev_epoch = nullptr, ev_epoch_nx = nullptr;   // origin of ccsx_timings.start_ms / end_ms: recorded at creation and moved forward every few
    float age_ms = 0.0f;              // end of the latest batch whose timings were read, relative to the current origin
    double epoch_ms = 0.0;            // minutes (epoch_ms = its distance from the creation), so that the float milliseconds HIP reports stay well below
                                      // 2^23 ms and keep their sub-microsecond resolution in long runs
    bool poisoned = false;            // a submit failed after work was enqueued: the handle refuses further batches
    bool poa_log = false;             // ccsx_poa_log: batches staged from now on keep the POA log
    ccsx_model model;
    ccsx_opts opts;
    DevBuf d_model, d_poa, d_align;   // shared by all slots
    DevBuf d_hd_lf;                   // log-factorial table of the heteroduplex finder (built at its first use)
    DevBuf d_reads;                   // ccsx_barcode_reads / ccsx_segment_reads / ccsx_cdna_reads / ccsx_cell_reads only: the call's set, report and reads (no slot is touched; the call ends synchronised)
    DevBuf d_dup;                     // ccsx_dup_sign_reads / ccsx_dup_cluster only: the call's reads and signatures, or its signatures, keys, sort scratch and report
    DevBuf d_cell_wl;                 // ccsx_cell_reads only: the resident copy of a whitelist's table (DESIGN.md §2 "Cell-tag rule") ...
    uint64_t cell_wl_serial = 0;      // ... and whose it is (0: nobody's); a call that brings another whitelist uploads it
    DevBuf d_orient;                  // k_orient's tables, shared by all slots like the POA scratch (reserved by the first batch that carries CCSX_PASS_STRAND_UNKNOWN)
    ccsx_orient_opts orient_opts;     // ccsx_set_orient_opts: the options of the batches staged from now on
    Slot slot[CCSX_SLOTS];
    int last = 0;                     // slot of the most recent stage / run (stage accessors, timings)
    int64_t next_ticket = 0;
    int handles_on_device = 1;        // share of the device's free memory this handle may take for scratch
};

// the host-side part of a finished slot's outputs: the capacity-layout offsets the caller's structs carry, and the drafts' backbone words without the cascade's marks
static void finish_outputs(const Slot &S, ccsx_results *res, ccsx_drafts *d)
{
    const int n = S.P.n_zmw;
    if (res && res->seq_off) std::memcpy(res->seq_off, S.seq_off.p, (size_t)(n + 1) * 8);
    if (d) {
        std::memcpy(d->seq_off, S.seq_off.p, (size_t)(n + 1) * 8);
        if (d->win_off) for (int z = 0; z <= n; ++z) d->win_off[z] = S.wb_off[z];
        for (int z = 0; z < n; ++z) d->backbone[z] &= 255;   // (the device word also carries the cascade's marks)
    }
}

// stage durations of a slot's last run.  draft_ms = the first POA pass, align_ms = alignment cascade + accounting + the whole
// fallback round (POA included), polish_ms from the polish stage's own start event (it may have queued behind the previous batch)
static int slot_timings(ccsx_handle h, Slot &S, ccsx_timings *t)
{
    HIPTRY(hipEventSynchronize(S.ev[CCSX_EV_END]));
    std::memset(t, 0, sizeof(*t));
    HIPTRY(hipEventElapsedTime(&t->setup_ms, S.ev[CCSX_EV_START], S.ev[CCSX_EV_TABLES_DONE]));
    HIPTRY(hipEventElapsedTime(&t->draft_ms, S.ev[CCSX_EV_TABLES_DONE], S.ev[CCSX_EV_DRAFT_DONE]));
    HIPTRY(hipEventElapsedTime(&t->align_ms, S.ev[CCSX_EV_DRAFT_DONE], S.ev[CCSX_EV_DRAFT_STAGE_DONE]));
    HIPTRY(hipEventElapsedTime(&t->queue_ms, S.ev[CCSX_EV_DRAFT_STAGE_DONE], S.ev[CCSX_EV_POLISH_START]));
    HIPTRY(hipEventElapsedTime(&t->polish_ms, S.ev[CCSX_EV_POLISH_START], S.ev[CCSX_EV_POLISH_DONE]));
    HIPTRY(hipEventElapsedTime(&t->stitch_ms, S.ev[CCSX_EV_POLISH_DONE], S.ev[CCSX_EV_END]));
    HIPTRY(hipEventElapsedTime(&t->total_ms, S.ev[CCSX_EV_START], S.ev[CCSX_EV_END]));
    float a = 0.0f, b = 0.0f;
    HIPTRY(hipEventElapsedTime(&a, h->ev_epoch, S.ev[CCSX_EV_START]));
    HIPTRY(hipEventElapsedTime(&b, h->ev_epoch, S.ev[CCSX_EV_END]));
    t->start_ms = h->epoch_ms + (double)a; t->end_ms = h->epoch_ms + (double)b;
    h->age_ms = b;                    // (the origin moves forward at the next submit that finds the handle idle: rebase_epoch)
    return 0;
}

// The one way a slot stops being in flight (ccsx_wait, ccsx_poll when it first sees the batch done, a submit that reuses the slot, the synchronous calls,
// destroy).  Its timings are taken NOW, as doubles against the current origin (a later rebase_epoch cannot invalidate them), together with the
// polish workgroups its results report; then the host-side part of its outputs.  Afterwards nothing touches the ticket's caller structs again.
static int retire(ccsx_handle h, Slot &S)
{
    if (!S.inflight) return 0;
    HIPTRY(hipEventSynchronize(S.ev_done));
    S.inflight = false;
    S.tm_ok = S.ran && slot_timings(h, S, &S.tm) == 0;
    if (S.tm_ok && S.res && S.res->n_windows) for (int z = 0; z < S.P.n_zmw; ++z) S.tm.polish_workgroups += S.res->n_windows[z];
    finish_outputs(S, S.res, S.drafts_out);
    S.res = nullptr; S.drafts_out = nullptr;
    return 0;
}

static void drain_streams(ccsx_handle h) { for (hipStream_t s : {h->s_in, h->s_draft, h->s_aux, h->s_comp, h->s_out}) if (s) (void)hipStreamSynchronize(s); }

static void destroy_handle(ccsx_handle h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    drain_streams(h);
    for (auto &s : h->slot) { (void)retire(h, s); s.release(); }
    if (h->ev_epoch) (void)hipEventDestroy(h->ev_epoch);
    if (h->ev_epoch_nx) (void)hipEventDestroy(h->ev_epoch_nx);
    if (h->s_in) (void)hipStreamDestroy(h->s_in);
    if (h->s_draft && h->s_draft != h->s_comp) (void)hipStreamDestroy(h->s_draft);
    if (h->s_aux) (void)hipStreamDestroy(h->s_aux);
    if (h->s_comp) (void)hipStreamDestroy(h->s_comp);
    if (h->s_out) (void)hipStreamDestroy(h->s_out);
    delete h;                         // frees every buffer of the handle and its slots (they were drained above; hipFree needs no stream)
}

static int refuse(const char *fn, const char *what) { ccsx_set_error(std::string(fn) + ": " + what); return -1; }

// ---- The analyses on final reads: barcode calls, segmentation and full-length cDNA reads (DESIGN.md §2 "Barcode calls", "Segment rule", "cDNA rule").  Each is
// described once, by a struct of its types, its nouns, its check / pack / launch and the arrays of its report; everything between an entry point and the kernel is
// one template over that struct.  The third, struct Cdna, supplied a core header (rule, packed set, report layout), a kernel with its launch, a check, such a
// struct and its member of KParams; no template changed for it.
struct ReadsCopy { void *host; const void *dev; size_t bytes_per_read; };

struct Barcodes {
    using Request = ccsx_barcode_request; using Set = ccsx_barcode_set; using Opts = ccsx_barcode_opts; using Report = ccsx_barcode_report; using Params = BarcodeParams;
    static constexpr const char *noun = "barcode", *title = "barcode calls";
    static int count(const Set &s) { return s.n_barcodes; }
    static size_t set_words(int nb) { return ccsx_bc_set_words(nb); }
    static size_t rep_bytes(size_t n) { return ccsx_bc_rep_bytes(n); }
    static int check(const Set *s, const Opts *o, const Report *r, int64_t n, const char *fn, Opts *out) { return ccsx_barcode_check(s, o, r, n, fn, out); }
    static void pack(const Set *s, unsigned long long *packed) { ccsx_bc_pack(s, packed); }
    static Params params(int nb, int n, const Opts &o, const void *base) { Params B{}; B.n = n; B.n_barcodes = nb; B.opts = o; ccsx_bc_bind(B, base); return B; }
    static const char *launch(const Params &B, hipStream_t st) { return ccsx_barcode_launch(B, st); }
    static Params &of(KParams &P) { return P.bc; }
    static std::vector<ReadsCopy> copies(const Report &r, const Params &B)
    {
        const BarcodeOut d = ccsx_bc_out(B.rep, (size_t)B.n);
        return {{r.tested, d.tested, 4}, {r.call, d.call, 4}, {r.bq, d.bq, 4}, {r.idx, d.idx, 8}, {r.dist, d.dist, 8}, {r.second, d.second, 8}, {r.clip, d.clip, 8}};
    }
};

struct Segments {
    using Request = ccsx_segment_request; using Set = ccsx_segment_set; using Opts = ccsx_segment_opts; using Report = ccsx_segment_report; using Params = SegmentParams;
    static constexpr const char *noun = "segment", *title = "segmentation";
    static int count(const Set &s) { return s.n_adapters; }
    static size_t set_words(int na) { return ccsx_sg_set_words(na); }
    static size_t rep_bytes(size_t n) { return ccsx_sg_rep_bytes(n); }
    static int check(const Set *s, const Opts *o, const Report *r, int64_t n, const char *fn, Opts *out) { return ccsx_segment_check(s, o, r, n, fn, out); }
    static void pack(const Set *s, unsigned long long *packed) { ccsx_sg_pack(s, packed); }
    static Params params(int na, int n, const Opts &o, const void *base) { Params G{}; G.n = n; G.n_adapters = na; G.opts = o; ccsx_sg_bind(G, base); return G; }
    static const char *launch(const Params &G, hipStream_t st) { return ccsx_segment_launch(G, st); }
    static Params &of(KParams &P) { return P.sg; }
    static std::vector<ReadsCopy> copies(const Report &r, const Params &G)
    {
        const SegmentOut d = ccsx_sg_out(G.rep, (size_t)G.n);
        return {{r.tested, d.tested, 4}, {r.overflow, d.overflow, 4}, {r.n_hits, d.n_hits, 4}, {r.n_cuts, d.n_cuts, 4}, {r.n_segments, d.n_segments, 4},
                {r.complete, d.complete, 4}, {r.orient, d.orient, 4}, {r.leftover_bases, d.leftover, 4},
                {r.pieces, d.pieces, CCSX_SEGMENT_MAX_PIECES * sizeof(ccsx_segment_piece)}};
    }
};

struct Cdna {
    using Request = ccsx_cdna_request; using Set = ccsx_cdna_set; using Opts = ccsx_cdna_opts; using Report = ccsx_cdna_report; using Params = CdnaParams;
    static constexpr const char *noun = "cdna", *title = "cDNA reads";
    static int count(const Set &s) { return s.n_primers; }
    static size_t set_words(int np) { return ccsx_cd_set_words(np); }
    static size_t rep_bytes(size_t n) { return ccsx_cd_rep_bytes(n); }
    static int check(const Set *s, const Opts *o, const Report *r, int64_t n, const char *fn, Opts *out) { return ccsx_cdna_check(s, o, r, n, fn, out); }
    static void pack(const Set *s, unsigned long long *packed) { ccsx_cd_pack(s, packed); }
    static Params params(int np, int n, const Opts &o, const void *base) { Params D{}; D.n = n; D.n_primers = np; D.opts = o; ccsx_cd_bind(D, base); return D; }
    static const char *launch(const Params &D, hipStream_t st) { return ccsx_cdna_launch(D, st); }
    static Params &of(KParams &P) { return P.cd; }
    static std::vector<ReadsCopy> copies(const Report &r, const Params &D)
    {
        const CdnaOut d = ccsx_cd_out(D.rep, (size_t)D.n);
        return {{r.tested, d.tested, 4}, {r.cls, d.cls, 4}, {r.strand, d.strand, 4}, {r.start, d.start, 4}, {r.end, d.end, 4}, {r.polya_len, d.polya_len, 4},
                {r.n_internal, d.n_internal, 4}, {r.first_internal, d.first_internal, 4}, {r.idx, d.idx, 8}, {r.dist, d.dist, 8}, {r.second, d.second, 8},
                {r.clip, d.clip, 8}};
    }
};

// a request of analysis A as build_wants checked and copied it: the options, the set packed (A::set_words) and its count
template <typename A> struct ReadsWant {
    const typename A::Request *req = nullptr;
    typename A::Opts opts{};
    std::vector<unsigned long long> set;
    int count = 0;
};

// the set of a checked request or call, packed
template <typename A> static std::vector<unsigned long long> reads_pack(const typename A::Set *set)
{
    std::vector<unsigned long long> packed(A::set_words(A::count(*set)), 0ull);
    A::pack(set, packed.data());
    return packed;
}

template <typename A> static int reads_request_check(const typename A::Request *q, const ccsx_batch *b, ReadsWant<A> *w, const char *fn)
{
    if (q->reserved[0] != 0 || q->reserved[1] != 0) { ccsx_set_error(std::string(fn) + ": " + A::noun + " request: reserved must be 0"); return -1; }
    if (A::check(q->set, q->opts, q->report, b->n_zmw, fn, &w->opts)) return -1;
    w->set = reads_pack<A>(q->set);
    w->count = A::count(*q->set);
    return 0;
}

// The set is the slot's own, in page-locked memory that lives as long as the slot (as the control's index): its copy is enqueued on `st` with the slot's other
// uploads.  The kernel reads the results where k_stitch leaves them.  A ticket carries one analysis at most (build_wants), so the slot has one buffer for it.
template <typename A> static int reads_attach(Slot &S, const ReadsWant<A> &w, hipStream_t st)
{
    KParams &P = S.P;
    const size_t n = (size_t)P.n_zmw, words = w.set.size();
    if (S.d_pattern.reserve(words * 8 + A::rep_bytes(n)) || S.pattern_set.resize(words)) return -2;
    std::copy(w.set.begin(), w.set.end(), S.pattern_set.p);
    typename A::Params &K = A::of(P);
    K = A::params(w.count, (int)n, w.opts, S.d_pattern.p);
    K.seq = P.out_seq; K.seq_off = P.seq_off; K.seq_len = P.out_len;
    if (hipError_t e = hipMemcpyAsync(S.d_pattern.p, S.pattern_set.p, words * 8, hipMemcpyHostToDevice, st)) {
        ccsx_set_error(std::string(A::title) + ": set upload: " + hipGetErrorString(e)); return -2;
    }
    return 0;
}

// the report's arrays into the caller's, on `s`
template <typename A> static int reads_download(const typename A::Params &K, const typename A::Report *r, hipStream_t s)
{
    if (!K.n) return 0;
    for (const ReadsCopy &c : A::copies(*r, K)) HIPTRY(hipMemcpyAsync(c.host, c.dev, (size_t)K.n * c.bytes_per_read, hipMemcpyDeviceToHost, s));
    return 0;
}

// The kernel of analysis A on the caller's reads: a buffer of the handle's own on the polish stream, behind whatever tickets have enqueued there; no slot is
// staged, retired or recycled.  Layout of the buffer: [set + report][seq_off: n x 8][seq_len: n x 4, padded][seq]
template <typename A> static int reads_enqueue(ccsx_handle h, const std::vector<unsigned long long> &packed, int count, const typename A::Opts &o, const uint8_t *seq,
                                               const int64_t *seq_off, const int32_t *seq_len, int32_t n, int64_t bytes, const typename A::Report *report, hipStream_t st)
{
    const size_t words = packed.size(), head = words * 8 + A::rep_bytes((size_t)n), head8 = (head + 7) & ~(size_t)7, len4 = ((size_t)n * 4 + 7) & ~(size_t)7;
    if (h->d_reads.reserve(head8 + (size_t)n * 8 + len4 + (size_t)bytes)) return -2;
    uint8_t *base = (uint8_t *)h->d_reads.p;
    int64_t *d_off = (int64_t *)(base + head8);
    int32_t *d_len = (int32_t *)(base + head8 + (size_t)n * 8);
    uint8_t *d_seq = base + head8 + (size_t)n * 8 + len4;
    HIPTRY(hipMemcpyAsync(base, packed.data(), words * 8, hipMemcpyHostToDevice, st));
    HIPTRY(hipMemcpyAsync(d_off, seq_off, (size_t)n * 8, hipMemcpyHostToDevice, st));
    HIPTRY(hipMemcpyAsync(d_len, seq_len, (size_t)n * 4, hipMemcpyHostToDevice, st));
    if (bytes) HIPTRY(hipMemcpyAsync(d_seq, seq, (size_t)bytes, hipMemcpyHostToDevice, st));
    typename A::Params K = A::params(count, n, o, base);
    K.seq = d_seq; K.seq_off = d_off; K.seq_len = d_len;
    (void)hipGetLastError();
    if (const char *failed = A::launch(K, st)) { ccsx_set_error(std::string("kernel launch failed: ") + failed); return -2; }
    return reads_download<A>(K, report, st);
}

// the body of ccsx_barcode_reads / ccsx_segment_reads (`fn`)
template <typename A> static int reads_sync(ccsx_handle h, const typename A::Set *set, const typename A::Opts *opts, const uint8_t *seq, const int64_t *seq_off,
                                            const int32_t *seq_len, int32_t n, typename A::Report *report, const char *fn)
{
    typename A::Opts o;
    int64_t bytes;
    if (A::check(set, opts, report, n, fn, &o) || ccsx_check_reads(seq, seq_off, seq_len, n, fn, &bytes)) return -1;
    if (!h) return refuse(fn, "null argument");
    if (n == 0) return 0;
    const std::vector<unsigned long long> packed = reads_pack<A>(set);
    HIPTRY(hipSetDevice(h->device));
    const int rc = reads_enqueue<A>(h, packed, A::count(*set), o, seq, seq_off, seq_len, n, bytes, report, h->s_comp);
    if (rc) { (void)hipStreamSynchronize(h->s_comp); return rc; }   // (whatever was enqueued reads and writes the caller's arrays: it ends before the call does)
    HIPTRY(hipStreamSynchronize(h->s_comp));
    return 0;
}

extern "C" {

int ccsx_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int ccsx_device_numa_node(int device)
{
    char id[64] = {0};
    if (hipDeviceGetPCIBusId(id, (int)sizeof(id), device) != hipSuccess) return -1;
    return ccsx_pci_numa_node(id);
}

int ccsx_bind_thread_to_device(int device) { return ccsx_bind_thread_to_node(ccsx_device_numa_node(device)); }

void *ccsx_alloc_pinned(size_t bytes)
{
    void *p = nullptr;
    hipError_t e = hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault);
    if (e != hipSuccess) { ccsx_set_error(std::string("hipHostMalloc(") + std::to_string(bytes) + "): " + hipGetErrorString(e)); return nullptr; }
    return p;
}

void ccsx_free_pinned(void *p)
{
    if (p) (void)hipHostFree(p);
}

static int create_impl(ccsx_handle h)
{
    HIPTRY(hipStreamCreateWithFlags(&h->s_in, hipStreamNonBlocking));
    // The polish stream gets the device's highest priority, the draft stage's streams the lowest: without the second POA stream the priorities change nothing
    // (tools/r03_prio.sh), with it they decide — three plain streams: 473 ms per 16384-ZMW step, polish high: 436, draft high: 438, no second stream: 441
    // (profiles/r05_poa_half_batches.txt).  CCSX_STAGE_PRIO=draft|polish|none overrides (none: plain streams).
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    const char *pe_env = getenv("CCSX_STAGE_PRIO");
    const char *pe = pe_env ? (strcmp(pe_env, "none") ? pe_env : nullptr) : "polish";
    const int p_draft = (pe && !strcmp(pe, "draft")) ? prio_hi : prio_lo, p_polish = (pe && !strcmp(pe, "polish")) ? prio_hi : prio_lo;
    if (pe) HIPTRY(hipStreamCreateWithPriority(&h->s_comp, hipStreamNonBlocking, p_polish));
    else HIPTRY(hipStreamCreateWithFlags(&h->s_comp, hipStreamNonBlocking));
    if (h->opts.serial_stages) h->s_draft = h->s_comp;
    else if (pe) HIPTRY(hipStreamCreateWithPriority(&h->s_draft, hipStreamNonBlocking, p_draft));
    else HIPTRY(hipStreamCreateWithFlags(&h->s_draft, hipStreamNonBlocking));
    HIPTRY(hipStreamCreateWithFlags(&h->s_out, hipStreamNonBlocking));
    // the POA stage's second stream (two half-batches, the threading of one under the DP of the other; not with serial stages, whose point is that a kernel's
    // counters are its own — CCSX_POA_SPLIT=2 forces it there for a measurement of the draft stage alone —; CCSX_POA_SPLIT=0 turns it off for an A/B; plain streams
    // (CCSX_STAGE_PRIO=none) get none: the three-way competition costs more than the overlap buys)
    { const char *e = getenv("CCSX_POA_SPLIT"); if (((!h->opts.serial_stages && pe) || (e && !strcmp(e, "2"))) && !(e && !strcmp(e, "0"))) { if (pe) HIPTRY(hipStreamCreateWithPriority(&h->s_aux, hipStreamNonBlocking, p_draft)); else HIPTRY(hipStreamCreateWithFlags(&h->s_aux, hipStreamNonBlocking)); } }
    HIPTRY(hipEventCreate(&h->ev_epoch));
    HIPTRY(hipEventCreate(&h->ev_epoch_nx));
    HIPTRY(hipEventRecord(h->ev_epoch, h->s_draft));         // the stream the tickets' first events are recorded on
    for (auto &s : h->slot) {
        for (auto &ev : s.ev) HIPTRY(hipEventCreate(&ev));
        for (auto &ev : s.ev_aux) HIPTRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        HIPTRY(hipEventCreateWithFlags(&s.ev_up, hipEventDisableTiming));
        HIPTRY(hipEventCreateWithFlags(&s.ev_done, hipEventDisableTiming));
    }
    if (h->d_model.reserve(sizeof(ccsx_model))) return -2;
    HIPTRY(hipMemcpy(h->d_model.p, &h->model, sizeof(ccsx_model), hipMemcpyHostToDevice));
    return 0;
}

int ccsx_create(int device_ordinal, const ccsx_model *model, const ccsx_opts *opts, ccsx_handle *out)
{
    if (!model || !opts || !out) { ccsx_set_error("ccsx_create: null argument"); return -1; }
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) { ccsx_set_error("ccsx_create: no HIP device available (this library has no CPU fallback)"); return -2; }
    if (device_ordinal < 0 || device_ordinal >= n) { ccsx_set_error("ccsx_create: bad device ordinal"); return -1; }
    HIPTRY(hipSetDevice(device_ordinal));
    hipDeviceProp_t prop;
    HIPTRY(hipGetDeviceProperties(&prop, device_ordinal));
    if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos) {
        ccsx_set_error(std::string("ccsx_create: kernels are built for gfx950 only, device is ") + prop.gcnArchName);
        return -2;
    }
    ccsx_handle h = new ccsx_handle_s();
    h->device = device_ordinal;
    h->model = *model;
    h->opts = *opts;
    if (h->opts.max_poa_cov < 1) h->opts.max_poa_cov = 1;
    if (h->opts.max_qv <= 0) h->opts.max_qv = 50;                    // (0 = default; a caller that zero-initialises the struct gets SPEC v7's cap)
    if (h->opts.max_qv > 93) h->opts.max_qv = 93;
    if (const char *e = std::getenv("CCSX_SERIAL_STAGES")) h->opts.serial_stages = std::atoi(e) != 0;   // A/B switch without a rebuild
    h->handles_on_device = opts->handles_per_device > 1 ? opts->handles_per_device : 1;
    ccsx_orient_opts_default(&h->orient_opts);
    const int rc = create_impl(h);
    if (rc) { destroy_handle(h); return rc; }        // no leak on a failed create (streams, events, device memory)
    *out = h;
    return 0;
}

int ccsx_destroy(ccsx_handle h)
{
    if (!h) return -1;
    destroy_handle(h);
    return 0;
}

// What a fused run carries beside the consensus: the optional outputs of a ccsx_extras and the three requests, already checked and copied (build_wants).
// An empty one asks for nothing.
struct Wants {
    ccsx_pileup *pile = nullptr;
    int32_t *tandem_len = nullptr; bool tandem = false; int min_tandem = 0;   // tandem: k_sdust runs (a length array to fill, or a threshold > 0)
    const ccsx_hd_request *hd = nullptr; ccsx_hd_opts hd_opts{};
    const ccsx_fold_request *fold = nullptr; ccsx_fold_opts fold_opts{};
    const ccsx_adapter_request *adapters = nullptr; ccsx_adapter_set adapter_set{}; ccsx_adapter_opts adapter_opts{};
    const ccsx_control_request *control = nullptr; ccsx_control_opts control_opts{}; std::vector<uint8_t> control_seq;
    const ccsx_coverage_request *coverage = nullptr; ccsx_coverage_opts coverage_opts{};
    const ccsx_orient_opts *orient = nullptr;   // ccsx_orient_batch's own options (NULL: the handle's, ccsx_set_orient_opts); already checked
    const ccsx_handoff_request *handoff = nullptr; ccsx_handoff_opts handoff_opts{}; ccsx_handoff_out handoff_out{};   // (the out struct is copied: it is read during the call only)
    ReadsWant<Barcodes> barcodes;
    ReadsWant<Segments> segments;
    ReadsWant<Cdna> cdna;
    bool represent = false; ccsx_represent_request represent_req{};   // (the request is copied: it is read during the call only)
    bool handoff_written_only = false;          // the synchronous form: counts is known when the copies are enqueued, only the written slots are copied
};

// the longest draft of a slot's batch that can reach status SUCCESS (that needs length <= opts.max_length, and no draft exceeds its slot), at least `floor`:
// what the LDS of k_sdust, k_fold, k_adapter and k_control is sized for
static int64_t longest_draft(ccsx_handle h, const Slot &S, int32_t floor)
{
    return std::min<int64_t>(std::max<int64_t>(floor, S.T.dcap_max), std::max<int32_t>(h->opts.max_length, floor));
}

// `units`: the LDS units (histogram bins, bitmap words) a draft screen's kernel needs for the slot's longest draft; -1, refused under the screen's name, when they
// exceed what its LDS holds (nothing has been enqueued by the request then)
static int64_t screen_units(int64_t longest, int64_t units, int64_t max_units, const char *screen)
{
    if (units <= max_units) return units;
    ccsx_set_error(std::string(screen) + ": drafts of up to " + std::to_string(longest) + " bases need more LDS than it has (lower opts.max_length)");
    return -1;
}

// a report of [k][n] int32 planes into the caller's k arrays, copied on `s`
static int download_planes(std::initializer_list<int32_t *> dst, const int32_t *src, size_t n, hipStream_t s)
{
    for (int32_t *d : dst) { HIPTRY(hipMemcpyAsync(d, src, n * 4, hipMemcpyDeviceToHost, s)); src += n; }
    return 0;
}

static int validate(const ccsx_batch *b)
{
    if (!b || b->n_zmw <= 0 || !b->read_off || !b->base_off || !b->bases || !b->pw || !b->flags || !b->snr) {
        ccsx_set_error("ccsx_upload: null or empty batch");
        return -1;
    }
    if (b->read_off[0] != 0 || b->base_off[0] != 0) { ccsx_set_error("ccsx_upload: offsets must start at 0"); return -1; }
    for (int z = 0; z < b->n_zmw; ++z)
        if (b->read_off[z + 1] < b->read_off[z]) { ccsx_set_error("ccsx_upload: read_off not monotone"); return -1; }
    const int R = b->read_off[b->n_zmw];
    if (R != b->n_reads) { ccsx_set_error("ccsx_upload: n_reads != read_off[n_zmw]"); return -1; }
    for (int r = 0; r < R; ++r)
        if (b->base_off[r + 1] < b->base_off[r]) { ccsx_set_error("ccsx_upload: base_off not monotone"); return -1; }
    if (b->base_off[R] != b->n_bases) { ccsx_set_error("ccsx_upload: n_bases != base_off[n_reads]"); return -1; }
    for (int z = 0; z < b->n_zmw; ++z) {                  // partial passes (flag bit 1) must follow the ZMW's full-length passes
        bool partial = false;
        for (int r = b->read_off[z]; r < b->read_off[z + 1]; ++r) {
            if (b->flags[r] & 2) partial = true;
            else if (partial) { ccsx_set_error("ccsx_upload: a full-length pass follows a partial pass (flags bit 1) in a ZMW"); return -1; }
        }
    }
    return 0;
}

// ---- staging a batch: the steps of stage(), in its order.  Each returns 0, -1 (the batch is refused; no step has enqueued anything yet) or -2 ----

// The host-derived layout of the batch in the slot's page-locked arrays, and its batch-level figures.  `top`: the passes of a ZMW the engine uses (ccsx_top_passes).
// First the capacity layout: per ZMW its capacities (ccsx_zmw_caps) and the offsets they add up to, per pass its ZMW and its entry-row slots.  Then the launch
// order, longest first (stable within 256-base classes, so a uniform batch keeps its input order and its locality): mixed batches (BASELINE configs[4]: 1-25 kb,
// 3-50 passes) otherwise end on a few long stragglers.
static int layout(Slot &S, const ccsx_batch *b, int top, BatchTotals *out)
{
    const int n = b->n_zmw, R = b->n_reads;
    if (S.read_zmw.resize(R > 0 ? R : 1) || S.vcap.resize(n) || S.dcap.resize(n) || S.seq_off.assign(n + 1, 0) || S.wb_off.assign(n + 1, 0) ||
        S.ent_off.assign(R + 1, 0) || S.read_off.resize(n + 1) || S.base_off.resize(R + 1) || S.zperm.resize(n) || S.rperm.resize(R > 0 ? R : 1))
        return -2;
    BatchTotals &T = *out;
    T = BatchTotals{};
    ccsx_for_each_zmw_caps(b, [&](int z, const ccsx_zmw_caps &c) {
        S.dcap[z] = (int32_t)c.dcap;
        S.vcap[z] = (int32_t)c.vcap;
        S.seq_off[z + 1] = S.seq_off[z] + S.dcap[z];
        S.wb_off[z + 1] = S.wb_off[z] + (int32_t)c.wcap;
        const int need = 2 * ((int)c.wcap - 1);                    // window-edge columns of a pass
        for (int r = b->read_off[z]; r < b->read_off[z + 1]; ++r) {
            S.read_zmw[r] = z;
            S.ent_off[r + 1] = S.ent_off[r] + ((need + 3) & ~3);   // (a multiple of 4: k_align16_tb stores four entries at a time)
        }
        T.nr_max = std::max(T.nr_max, std::min(b->read_off[z + 1] - b->read_off[z], top)); T.need_max = std::max(T.need_max, need);
        T.maxL_max = std::max(T.maxL_max, c.maxL); T.vcap_max = std::max<int64_t>(T.vcap_max, S.vcap[z]); T.dcap_max = std::max<int64_t>(T.dcap_max, S.dcap[z]);
    });
    if (T.maxL_max > 65535) { ccsx_set_error("ccsx_upload: subreads longer than 65535 bases are not supported"); return -1; }
    std::memcpy(S.read_off.p, b->read_off, (size_t)(n + 1) * 4);
    std::memcpy(S.base_off.p, b->base_off, (size_t)(R + 1) * 8);
    T.total_wslots = (int64_t)S.wb_off[n] - n; T.cap_total = S.seq_off[n];
    auto order_by = [](PinVec<int32_t> &perm, size_t cnt_items, auto len_of) {
        const int NBK = 258;
        std::vector<int32_t> cnt(NBK + 1, 0);
        auto cls = [&](int64_t l) { int c = (int)(l >> 8); return NBK - 1 - (c > NBK - 1 ? NBK - 1 : c); };   // descending length
        for (size_t i = 0; i < cnt_items; ++i) ++cnt[cls(len_of(i)) + 1];
        for (int i = 0; i < NBK; ++i) cnt[i + 1] += cnt[i];
        for (size_t i = 0; i < cnt_items; ++i) perm[cnt[cls(len_of(i))]++] = (int32_t)i;
    };
    order_by(S.zperm, (size_t)n, [&](size_t z) { return (int64_t)S.dcap[z]; });
    if (R > 0) order_by(S.rperm, (size_t)R, [&](size_t r) { return b->base_off[r + 1] - b->base_off[r]; });
    // k_align16's work items: up to four consecutive passes of one ZMW (of the passes the engine uses), longest first
    std::vector<int32_t> qpack; std::vector<int64_t> qlen;
    for (int z = 0; z < n; ++z) {
        const int r0 = b->read_off[z];
        int nr = std::min(b->read_off[z + 1] - r0, top);
        while (nr > 0 && (b->flags[r0 + nr - 1] & 2)) --nr;   // partial passes are aligned by k_rescue (anchored at one end), not here
        for (int g = 0; g < nr; g += 4) {
            const int c = std::min(4, nr - g);
            int64_t ml = 0;
            for (int q = 0; q < c; ++q) ml = std::max<int64_t>(ml, b->base_off[r0 + g + q + 1] - b->base_off[r0 + g + q]);
            qpack.push_back(((r0 + g) << 2) | (c - 1)); qlen.push_back(ml);
        }
    }
    T.n_quads = (int)qpack.size();
    if (S.quads.resize(T.n_quads > 0 ? T.n_quads : 1)) return -2;
    if (T.n_quads > 0) {
        if (S.qperm.resize(T.n_quads)) return -2;
        order_by(S.qperm, (size_t)T.n_quads, [&](size_t q) { return qlen[q]; });
        for (int q = 0; q < T.n_quads; ++q) S.quads[q] = qpack[S.qperm[q]];
    }
    if (T.total_wslots > 0x7fff0000ll) { ccsx_set_error("ccsx_upload: batch too large (more than 2^31 window slots): split it"); return -1; }
    return 0;
}

// the words of k_sdust's LDS mask, which covers the longest draft the cascade aligns; -1, refused, when mask and tables exceed a CU's LDS
static int32_t sdust_mask_words(ccsx_handle h, const Slot &S)
{
    const int64_t longest = longest_draft(h, S, 16), words = (longest + 31) / 32;
    if ((int64_t)CCSX_SDUST_TABLE_BYTES + 4 * words <= 160 * 1024) return (int32_t)words;
    ccsx_set_error("tandem-repeat detection: drafts of up to " + std::to_string(longest) + " bases need more LDS than a CU has (lower opts.max_length)");
    return -1;
}

// a slot buffer of `bytes`, and the KParams pointer `dst` to it: a buffer's size and its binding are written once, here
#define RES(dst, buf, bytes) do { if ((buf).reserve(bytes)) return -2; (dst) = (decltype(dst))(buf).p; } while (0)

// the batch's arrays and the slot's layout into their device buffers, bound to P: H2D copies enqueued on `st`, in this order
static int upload_inputs(Slot &S, const ccsx_batch *b, bool ipd, hipStream_t st, KParams &P)
{
    const size_t n = (size_t)b->n_zmw, R = (size_t)b->n_reads, R1 = R > 0 ? R : 1, NB = (size_t)b->n_bases;
#define UP(dst, buf, src, bytes) do { RES(dst, buf, bytes); HIPTRY(hipMemcpyAsync((buf).p, (src), (bytes), hipMemcpyHostToDevice, st)); } while (0)
    UP(P.snr, S.d_snr, b->snr, n * 16);
    UP(P.read_off, S.d_read_off, b->read_off, (n + 1) * 4);
    UP(P.base_off, S.d_base_off, b->base_off, (R + 1) * 8);
    UP(P.bases, S.d_bases, b->bases, NB);
    UP(P.pw, S.d_pw, b->pw, NB);
    if (ipd) UP(P.ipd, S.d_ipd, b->ipd, NB);
    UP(P.flags, S.d_flags, b->flags, R1);
    UP(P.read_zmw, S.d_read_zmw, S.read_zmw.p, R1 * 4);
    UP(P.vcap, S.d_vcap, S.vcap.p, n * 4);
    UP(P.dcap, S.d_dcap, S.dcap.p, n * 4);
    UP(P.seq_off, S.d_seq_off, S.seq_off.p, (n + 1) * 8);
    UP(P.wb_off, S.d_wb_off, S.wb_off.p, (n + 1) * 4);
    UP(P.ent_off, S.d_ent_off, S.ent_off.p, (R + 1) * 8);
    UP(P.zmw_perm, S.d_zperm, S.zperm.p, S.zperm.size() * 4);
    UP(P.read_perm, S.d_rperm, S.rperm.p, S.rperm.size() * 4);
    UP(P.quads, S.d_quads, S.quads.p, S.quads.size() * 4);
#undef UP
    return 0;
}

// the slot's per-ZMW state, per-window and per-pass working arrays and outputs, sized by the layout and bound to P; the optional analyses' only when they run
static int reserve_state(Slot &S, size_t n, size_t R, bool kin, bool pile, bool tandem, bool handoff, KParams &P)
{
    const size_t R1 = R > 0 ? R : 1, wins = (size_t)S.T.total_wslots + 1, cap = (size_t)S.T.cap_total, ents = (size_t)(S.ent_off[R] + 1);
    RES(P.tabME, S.d_tabME, n * 192 * 4); RES(P.tabINS, S.d_tabINS, n * 192 * 4); RES(P.tabDL, S.d_tabDL, n * 16 * 4); RES(P.tabZ, S.d_tabZ, n * 32 * 4);
    RES(P.draft, S.d_draft, cap);
    if (carve_planes<int32_t>({&P.draft_len, &P.nwin, &P.zstat, &P.nreads_used, &P.np, &P.zref, &P.nfull}, S.d_zmw_i32, n)) return -2;
    RES(P.wbounds, S.d_wbounds, (size_t)S.wb_off[n] * 4);
    RES(P.wslot_zmw, S.d_wslot, wins * 4 + (n + 2) * 4);      // compact window map + first index per ZMW, built by k_wmap
    P.wstart = P.wslot_zmw + wins;
    RES(P.ticket_poa, S.d_ticket, 256);
    P.ticket_align = P.ticket_poa + 1; P.debug = P.ticket_poa + 4; P.phase = (unsigned long long *)(P.ticket_poa + 16);
    RES(P.avalid, S.d_avalid, R1); RES(P.ascore, S.d_ascore, R1 * 4);
    RES(P.align_retry, S.d_retry, (R1 + 16) * 4);
    RES(P.ent, S.d_ent, ents * 4); RES(P.dmask, S.d_dmask, ents * 4);
    RES(P.wseq, S.d_wseq, wins * 32); RES(P.wqv, S.d_wqv, wins * 32 * 4);
    RES(P.wsum, S.d_wsum, wins * 4); RES(P.wmeta, S.d_wmeta, wins * 16);
    RES(P.out_seq, S.d_out_seq, cap); RES(P.out_qual, S.d_out_qual, cap); RES(P.out_raw, S.d_out_raw, cap * 4);
    if (carve_planes<int32_t>({&P.out_status, &P.out_len, &P.out_iters, &P.out_nwin, &P.out_fn, &P.out_rn}, S.d_out_i32, n)) return -2;
    if (carve_planes<float>({&P.out_rq, &P.out_ec}, S.d_out_f32, n)) return -2;
    if (kin || pile || handoff) { RES(P.wtpl, S.d_wtpl, wins * 32); RES(P.wtmeta, S.d_wtmeta, wins * 4); }   // k_polish keeps the converged templates
    if (kin) { RES(P.wkin, S.d_wkin, wins * 32 * 4); RES(P.out_kin, S.d_out_kin, cap * 4); P.kin_plane = S.T.cap_total; }
    if (pile) { RES(P.wpile, S.d_wpile, wins * 32 * 4); RES(P.out_pile, S.d_out_pile, cap * 3); P.pile_plane = S.T.cap_total; }
    if (tandem) { RES(P.tflag, S.d_tflag, n * 4); RES(P.tlen, S.d_tlen, n * 4); }
    return 0;
}
#undef RES

// ---- the shared POA / alignment scratch: what a batch needs per resident POA graph / retry alignment / k_align16 quad, how many of each it gets
struct SlotSizes { size_t poa_bytes, align_i32, align16_i32; };
struct ScratchPlan { int poa_slots, align_slots, align16_slots, align16_regions; };

static SlotSizes scratch_slot_sizes(const BatchTotals &T)
{
    // per vertex CCSX_POA_BYTES_PER_VERTEX (ccsx_kernels.h; the kernels' layout static_asserts the same figure) + the pass's path + the state block;
    // (origin, dirty bits) per cell and edge + band starts + best cell (score, row, entry row) per edge;
    // k_align16 stores a quad's moves instead (2 bits per band row and column + 2 bits of band step and an edge flag per column: 18 words per block of 16 draft
    // columns and pass): four passes' moves + the four final band starts, padded, for the draft CAPACITY of the batch's longest insert
    return {(((size_t)T.vcap_max + 64) * CCSX_POA_BYTES_PER_VERTEX + (size_t)T.maxL_max * 4 + 1024 + 255) & ~(size_t)255,
            (size_t)T.need_max * 128 + 4 * (size_t)T.need_max + 64,
            (size_t)4 * (size_t)ccsx_tb_stride((int)T.dcap_max) + 16};
}

// the sizing expressions of the plan (plan_scratch) and of the clamps after a failed growth (launch)
static size_t slots_that_fit(size_t room, size_t per_slot, size_t at_least) { return std::max(at_least, room / per_slot); }
static size_t align16_words(int regions, int slots, size_t slot_i32) { return (size_t)regions * slots * slot_i32; }   // k_align16's part of the alignment scratch: the retry's slots lie behind it

// Resident POA graphs / alignment slots for a batch of n ZMWs, R passes and n_quads quads within `budget` bytes: as many as fit, never more than the work.
// opt_poa_slots: opts.poa_slots; one_region, max16: the process's CCSX_A16_ONE_REGION and CCSX_ALIGN16_MAX_SLOTS.
static ScratchPlan plan_scratch(size_t budget, int n, int R, int n_quads, const SlotSizes &sz, int opt_poa_slots, bool one_region, int max16)
{
    ScratchPlan p;
    p.poa_slots = std::min(opt_poa_slots > 0 ? opt_poa_slots : 16384, n);   // four graphs per wave: 16384 = 4 waves per SIMD
    p.poa_slots = (int)std::min<size_t>((size_t)p.poa_slots, slots_that_fit(budget * 3 / 4, sz.poa_bytes, 1));
    p.align_slots = std::min(4096, std::max(R, 2));             // the 64-row retry and the split alignment (two slots per pass) run grid-stride loops of <= 4096 workgroups
    p.align_slots = (int)std::min<size_t>((size_t)p.align_slots, slots_that_fit(budget / 16, sz.align_i32 * 4, 2));
    // every quad of the batch in ONE launch if that fits 12 GB (16384 ZMWs x 10 passes x 10 kb: 9.3 GB); a batch of long inserts and many passes takes a few
    // equal launches instead of tens of GB of scratch (a launch's trace-back still has thousands of waves)
    const size_t fit = slots_that_fit(std::min<size_t>(budget / 8, (size_t)12 << 30), sz.align16_i32 * 4, 1), nq = (size_t)std::max(n_quads, 1);
    auto equal_launches = [nq](size_t at_most) { const size_t launches = (nq + at_most - 1) / at_most; return (int)((nq + launches - 1) / launches); };
    p.align16_regions = 1;
    if (nq <= fit) p.align16_slots = (int)nq;
    else if (one_region) p.align16_slots = equal_launches(fit);   // (A/B switch: equal launches in ONE region, in sequence)
    else { p.align16_slots = equal_launches(std::max<size_t>(1, fit / 2)); p.align16_regions = 2; }   // two regions of half the space: launch c's trace-back runs under launch c + 1
    if (max16 > 0 && p.align16_slots > max16) { p.align16_slots = max16; p.align16_regions = 2; }     // test hook: forces several launches
    return p;
}

// the shared scratch as the handle holds it now, for the slots P has
static void bind_scratch(ccsx_handle h, KParams &P)
{
    P.poa_scratch = (uint8_t *)h->d_poa.p; P.align_scratch = (int32_t *)h->d_align.p;
    P.retry_scratch = P.align_scratch + align16_words(P.align16_regions, P.align16_slots, P.align16_slot_i32);
}

// The plan for this handle's share of the device's free memory, bound to P, and the scratch grown to it.  The scratch is shared by the handle's batch slots; it only grows,
// and growing waits for the draft and polish streams.
static int grow_scratch(ccsx_handle h, int n, int R, const BatchTotals &T, KParams &P)
{
    const SlotSizes sz = scratch_slot_sizes(T);
    static const bool one_region = [] { const char *e = getenv("CCSX_A16_ONE_REGION"); return e && e[0] == '1'; }();
    static const int max16 = [] { const char *e = getenv("CCSX_ALIGN16_MAX_SLOTS"); const int v = e ? atoi(e) : 0; return v > 0 ? v : 0; }();
    std::lock_guard<std::mutex> lk(g_scratch_mutex);
    size_t freeb = 0, totalb = 0;
    HIPTRY(hipMemGetInfo(&freeb, &totalb));
    freeb /= (size_t)h->handles_on_device;
    freeb += h->d_poa.cap + h->d_align.cap;                      // what we already hold is reusable
    ScratchPlan p = plan_scratch(freeb > (size_t)6 << 30 ? freeb - ((size_t)4 << 30) : freeb / 2, n, R, T.n_quads, sz, h->opts.poa_slots, one_region, max16);
    const size_t need_align = ((size_t)p.align_slots * sz.align_i32 + align16_words(p.align16_regions, p.align16_slots, sz.align16_i32)) * 4;
    if ((size_t)p.poa_slots * sz.poa_bytes > h->d_poa.cap || need_align > h->d_align.cap) {
        HIPTRY(hipStreamSynchronize(h->s_draft));                // kernels of an earlier batch may still use the old scratch
        HIPTRY(hipStreamSynchronize(h->s_comp));
        for (int attempt = 0;; ++attempt) {                      // another process / handle may have taken the memory meanwhile
            if (h->d_poa.reserve((size_t)p.poa_slots * sz.poa_bytes) == 0) break;
            if (attempt >= 4 || p.poa_slots <= 1) return -2;
            p.poa_slots = std::max(1, p.poa_slots / 2);
        }
        if (h->d_align.reserve(need_align)) return -2;
    }
    P.poa_slot_bytes = sz.poa_bytes; P.poa_slots = p.poa_slots;
    P.align_slot_i32 = sz.align_i32; P.align_slots = p.align_slots;
    P.align16_slot_i32 = sz.align16_i32; P.align16_slots = p.align16_slots; P.align16_regions = p.align16_regions;
    bind_scratch(h, P);
    return 0;
}

// ---- pass orientation's host side (DESIGN.md §2 "Pass orientation")
static int orient_opts_check(const ccsx_orient_opts *o, const char *fn)
{
    if (o->min_votes < 1 || o->ratio < 2 || o->ratio > 16) { ccsx_set_error(std::string(fn) + ": orient options out of range (min_votes >= 1; 2 <= ratio <= 16)"); return -1; }
    return 0;
}

// The anchor pass of every ZMW into S.anchor (index within the ZMW; -1: no full-length pass) when some pass of the batch carries CCSX_PASS_STRAND_UNKNOWN: among the
// full-length passes the one whose length is closest to the median (element n / 2 of the sorted lengths), ties to the first — the fallback draft's backbone
// rule.  *longest: the longest anchor, 0 when no pass carries the bit (S.anchor is not touched then).
static int orient_anchors(Slot &S, const ccsx_batch *b, int64_t *longest)
{
    *longest = 0;
    bool any = false;
    for (int r = 0; r < b->n_reads && !any; ++r) any = (b->flags[r] & CCSX_PASS_STRAND_UNKNOWN) != 0;
    if (!any) return 0;
    if (S.anchor.resize((size_t)b->n_zmw)) return -2;
    std::vector<int64_t> len;
    *longest = 1;
    for (int z = 0; z < b->n_zmw; ++z) {
        const int r0 = b->read_off[z];
        len.clear();
        for (int r = r0; r < b->read_off[z + 1] && !(b->flags[r] & 2); ++r) len.push_back(b->base_off[r + 1] - b->base_off[r]);   // (the partial passes follow)
        int a = -1;
        if (!len.empty()) {
            std::vector<int64_t> sorted(len);
            std::nth_element(sorted.begin(), sorted.begin() + sorted.size() / 2, sorted.end());
            const int64_t med = sorted[sorted.size() / 2];
            for (int i = 0; i < (int)len.size(); ++i)
                if (a < 0 || std::llabs(len[i] - med) < std::llabs(len[a] - med)) a = i;
            *longest = std::max(*longest, len[a]);
        }
        S.anchor[z] = a;
    }
    return 0;
}

// the report planes and the anchors of a staged batch that carries the bit (the anchors' upload enqueued on `st`), and the handle's tables grown to the batch's
// longest anchor: growing waits for the draft stream, whose earlier batches may still use them
static int orient_attach(ccsx_handle h, Slot &S, int64_t longest_anchor, const ccsx_orient_opts &o, hipStream_t st, KParams &P)
{
    const size_t n = (size_t)P.n_zmw, R1 = (size_t)(P.n_reads > 0 ? P.n_reads : 1), R = (size_t)P.n_reads;
    if (S.d_orient.reserve(n * 4 + R1 * 8 + R1 * 2)) return -2;
    P.orient = o;
    P.orient_anchor = (const int32_t *)S.d_orient.p;
    P.orient_votes = (int32_t *)S.d_orient.p + n;
    P.orient_rep8 = (uint8_t *)(P.orient_votes + 2 * R);
    P.orient_flags = (uint8_t *)S.d_flags.p;
    P.orient_tab_words = ccsx_orient_slots((int)longest_anchor);
    P.orient_wgs = (int32_t)std::min<size_t>(n, CCSX_ORIENT_MAX_WGS);
    const size_t need = (size_t)P.orient_wgs * (size_t)P.orient_tab_words * 4;
    if (need > h->d_orient.cap) {
        HIPTRY(hipStreamSynchronize(h->s_draft));
        if (h->d_orient.reserve(need)) return -2;
    }
    P.orient_tab = (uint32_t *)h->d_orient.p;
    HIPTRY(hipMemcpyAsync(S.d_orient.p, S.anchor.p, n * 4, hipMemcpyHostToDevice, st));
    return 0;
}

// Stage a batch into a slot: host-derived layout, device buffers, H2D copies enqueued on `st` (nothing waits here except
// hipMalloc growth).  The batch's own arrays must stay valid until the copies have run (pinned arrays copy by DMA).
// W.pile: this run also computes the pileup summary (its buffers are reserved and its pointers set only then).
// W.tandem: it also runs tandem-repeat detection (k_sdust), flagging ZMWs at W.min_tandem > 0 (the same rule for its buffers and pointers).
// The slot's KParams are built from nothing (the requests' part is attach()'s) and replace the old ones only when every step has succeeded.
static int stage(ccsx_handle h, Slot &S, const ccsx_batch *b, hipStream_t st, const Wants &W)
{
    if (validate(b)) return -1;
    const bool kin = h->opts.hifi_kinetics != 0, pile = W.pile != nullptr;
    if (kin && !b->ipd) { ccsx_set_error("ccsx_upload: opts.hifi_kinetics needs batch.ipd"); return -1; }
    const int n = b->n_zmw, R = b->n_reads;
    int rc;
    if ((rc = layout(S, b, ccsx_top_passes(h->opts.top_passes), &S.T))) return rc;
    int64_t longest_anchor = 0;                                  // > 0: some pass carries CCSX_PASS_STRAND_UNKNOWN
    if ((rc = orient_anchors(S, b, &longest_anchor))) return rc;
    const BatchTotals &T = S.T;
    KParams P;
    std::memset(&P, 0, sizeof(P));
    if (W.tandem) {
        P.min_tandem = W.min_tandem;
        if ((P.sdust_words = sdust_mask_words(h, S)) < 0) return -1;
    }
    const bool handoff = W.handoff != nullptr;                   // (its cells carry the passes' ipd bytes when the batch has them)
    if ((rc = upload_inputs(S, b, kin || (handoff && b->ipd), st, P)) || (rc = reserve_state(S, (size_t)n, (size_t)R, kin, pile, W.tandem, handoff, P))) return rc;
    if ((rc = grow_scratch(h, n, R, T, P))) return rc;
    if (h->poa_log) {                                            // every record starts as -1: "this generator did not reach this pass"
        const size_t bytes = (size_t)(n > 0 ? n : 1) * 2 * (size_t)T.nr_max * CCSX_POA_LOG_WORDS * 4;
        if (S.d_poa_log.reserve(bytes)) return -2;
        P.poa_log = (int32_t *)S.d_poa_log.p; P.poa_log_stride = T.nr_max;
        HIPTRY(hipMemsetAsync(P.poa_log, 0xff, bytes, st));
    }
    P.n_zmw = n; P.n_reads = R; P.maxL_max = (int32_t)T.maxL_max; P.vcap_max = (int32_t)T.vcap_max; P.need_max = T.need_max; P.max_reads = T.nr_max;
    P.n_quads = T.n_quads; P.total_wslots = T.total_wslots;
    P.opts = h->opts;
    P.perr_floor = ccsx_perr_floor(h->opts.max_qv);
    P.model = (const ccsx_model *)h->d_model.p;
    if (ccsx_polish_lds(T.nr_max, &P.pw_obs_bytes, &P.pw_gb_floats)) { ccsx_set_error("ccsx_upload: cannot size the polish kernel's LDS"); return -2; }
    if (longest_anchor > 0 && (rc = orient_attach(h, S, longest_anchor, W.orient ? *W.orient : h->orient_opts, st, P))) return rc;
    S.P = P;
    S.staged = true; S.ran = false; S.tm_ok = false;
    S.orient_pending = longest_anchor > 0; S.orient_ran = false;
    return 0;
}

// all kernels of one staged batch; every launch status is captured (a bad launch configuration fails here, not at the next sync)
static int launch(ccsx_handle h, Slot &S)
{
    (void)hipGetLastError();
    // The shared scratch may have been re-allocated (a later, larger batch) since this slot was staged.  It only grows, so what was planned at staging still fits;
    // the clamps are for a failed growth, and only ever shrink the plan to what the buffers hold.
    KParams &P = S.P;
    if ((size_t)P.poa_slots * P.poa_slot_bytes > h->d_poa.cap) P.poa_slots = (int)slots_that_fit(h->d_poa.cap, P.poa_slot_bytes, 1);
    const size_t words = h->d_align.cap / 4;
    if ((size_t)P.align_slots * P.align_slot_i32 + align16_words(P.align16_regions, P.align16_slots, P.align16_slot_i32) > words) {
        if ((size_t)P.align_slots * P.align_slot_i32 > words / 2) P.align_slots = (int)slots_that_fit(words / 2, P.align_slot_i32, 1);
        const size_t used = (size_t)P.align_slots * P.align_slot_i32, left = words > used ? words - used : 0;
        P.align16_slots = (int)slots_that_fit(left, (size_t)P.align16_regions * P.align16_slot_i32, 1);
    }
    bind_scratch(h, P);
    if (!h->d_poa.p || !h->d_align.p) { ccsx_set_error("kernel launch refused: the POA / alignment scratch is not allocated (an earlier allocation failed)"); return -2; }
    // k_orient runs once per staged batch: it resolves the flags in place, so a batch that is run again (ccsx_run twice) is oriented already and keeps its report
    uint8_t *const orient_flags = P.orient_flags;
    if (S.orient_pending) {
        P.orient_tab = (uint32_t *)h->d_orient.p;                // (the tables only grow, like the scratch above)
        if ((size_t)P.orient_wgs * (size_t)P.orient_tab_words * 4 > h->d_orient.cap) { ccsx_set_error("kernel launch refused: k_orient's tables are not allocated (an earlier allocation failed)"); return -2; }
    } else P.orient_flags = nullptr;
    const char *failed = ccsx_launch_all(S.P, {h->s_draft, h->s_comp, h->s_aux, S.ev, h->s_aux ? S.ev_aux : nullptr}, S.mode);
    P.orient_flags = orient_flags;
    if (failed) { ccsx_set_error(std::string("kernel launch failed: ") + failed); return -2; }
    if (S.orient_pending) { S.orient_pending = false; S.orient_ran = true; }
    S.ran = true;
    return 0;
}

static int check_results(const Slot &S, const ccsx_results *res, bool have_kin)
{
    const int n = S.P.n_zmw;
    if (!res || res->n_zmw != n || res->seq_capacity < S.seq_off[n]) { ccsx_set_error("ccsx_download: result buffers too small"); return -1; }
    if (!have_kin && (res->fi || res->fp || res->ri || res->rp)) {
        ccsx_set_error("ccsx_download: kinetics buffers given but the handle was created without opts.hifi_kinetics");
        return -1;
    }
    return 0;
}

static int check_pile(const Slot &S, const ccsx_pileup *pile)
{
    if (!pile || !pile->coverage || !pile->matches || !pile->mismatches || pile->seq_capacity < S.seq_off[S.P.n_zmw]) {
        ccsx_set_error("ccsx_pileup: missing planes, or smaller than the capacity layout (ccsx_result_layout)"); return -1;
    }
    return 0;
}

// the three planes of the pileup summary (the slot was staged with pile = true)
static int enqueue_pile_download(const Slot &S, ccsx_pileup *pile, hipStream_t s)
{
    const size_t pl = (size_t)S.seq_off[S.P.n_zmw];
    HIPTRY(hipMemcpyAsync(pile->coverage, S.P.out_pile, pl, hipMemcpyDeviceToHost, s));
    HIPTRY(hipMemcpyAsync(pile->matches, S.P.out_pile + pl, pl, hipMemcpyDeviceToHost, s));
    HIPTRY(hipMemcpyAsync(pile->mismatches, S.P.out_pile + 2 * pl, pl, hipMemcpyDeviceToHost, s));
    return 0;
}

static int enqueue_download(Slot &S, ccsx_results *res, hipStream_t s)
{
    const int n = S.P.n_zmw;
    const KParams &P = S.P;
#define DOWN(dst, src, bytes) do { if (dst) HIPTRY(hipMemcpyAsync((dst), (src), (bytes), hipMemcpyDeviceToHost, s)); } while (0)
    DOWN(res->status, P.out_status, (size_t)n * 4);
    DOWN(res->seq_len, P.out_len, (size_t)n * 4);
    DOWN(res->iters, P.out_iters, (size_t)n * 4);
    DOWN(res->n_windows, P.out_nwin, (size_t)n * 4);
    DOWN(res->rq, P.out_rq, (size_t)n * 4);
    DOWN(res->ec, P.out_ec, (size_t)n * 4);
    DOWN(res->np, P.np, (size_t)n * 4);
    DOWN(res->seq, P.out_seq, (size_t)S.seq_off[n]);
    DOWN(res->qual, P.out_qual, (size_t)S.seq_off[n]);
    DOWN(res->raw_qv, P.out_raw, (size_t)S.seq_off[n] * 4);
    DOWN(res->fn, P.out_fn, (size_t)n * 4);
    DOWN(res->rn, P.out_rn, (size_t)n * 4);
    if (P.out_kin) {
        const size_t pl = (size_t)S.seq_off[n];
        DOWN(res->fi, P.out_kin, pl); DOWN(res->fp, P.out_kin + pl, pl);
        DOWN(res->ri, P.out_kin + 2 * pl, pl); DOWN(res->rp, P.out_kin + 3 * pl, pl);
    }
#undef DOWN
    return 0;
}

// ---- asynchronous pipeline -------------------------------------------------------------------------------
// The origin of ccsx_timings.start_ms / end_ms moves forward every 5 minutes of handle lifetime so that HIP's float milliseconds keep their resolution.
// not inside the getter (it stalled behind every queued download and relied on negative elapsed times for slots recorded before the new origin) — only when
// NO slot is in flight, i.e. every event of a completed slot lies before the new origin and none is pending: called from submit.  CCSX_EPOCH_REBASE_MS: test hook.
static int rebase_epoch(ccsx_handle h)
{
    static const float limit = [] { const char *e = std::getenv("CCSX_EPOCH_REBASE_MS"); return e ? (float)std::atof(e) : 300000.0f; }();
    if (h->age_ms <= limit) return 0;
    for (auto &S : h->slot) if (S.inflight) return 0;
    float d = 0.0f;
    HIPTRY(hipEventRecord(h->ev_epoch_nx, h->s_draft));
    HIPTRY(hipEventSynchronize(h->ev_epoch_nx));
    HIPTRY(hipEventElapsedTime(&d, h->ev_epoch, h->ev_epoch_nx));
    h->epoch_ms += (double)d;
    std::swap(h->ev_epoch, h->ev_epoch_nx);
    h->age_ms = 0.0f;
    for (auto &S : h->slot) S.ran = false;               // events recorded before the new origin can no longer be measured against it; what retire() took (Slot::tm) stays readable
    return 0;
}

static int check_drafts(const Slot &S, const ccsx_drafts *d, bool input)
{
    const int n = S.P.n_zmw;
    if (!d || d->n_zmw != n || !d->seq || !d->len || !d->backbone || !d->seq_off || d->seq_capacity < S.seq_off[n] || (!input && !d->status)) {
        ccsx_set_error("ccsx_drafts: missing arrays, or sized for another batch (ccsx_draft_layout)"); return -1;
    }
    if (!input && d->win_bounds && (!d->win_off || d->win_capacity < S.wb_off[n])) { ccsx_set_error("ccsx_drafts: win_bounds needs win_off and ccsx_draft_layout's capacity"); return -1; }
    if (input) for (int z = 0; z <= n; ++z) if (d->seq_off[z] != S.seq_off[z]) { ccsx_set_error("ccsx_polish_batch: drafts.seq_off is not the capacity layout of ccsx_draft_layout"); return -1; }
    return 0;
}

// the caller's drafts (the polish seam, the heteroduplex finder), copied on `st`: bases into the slot's draft buffer, lengths + orientation references beside them
static int upload_drafts(Slot &S, const ccsx_drafts *d, hipStream_t st)
{
    const int n = S.P.n_zmw;
    if (S.d_din_len.reserve((size_t)n * 4) || S.d_din_bb.reserve((size_t)n * 4)) return -2;
    HIPTRY(hipMemcpyAsync(S.d_draft.p, d->seq, (size_t)S.seq_off[n], hipMemcpyHostToDevice, st));
    HIPTRY(hipMemcpyAsync(S.d_din_len.p, d->len, (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIPTRY(hipMemcpyAsync(S.d_din_bb.p, d->backbone, (size_t)n * 4, hipMemcpyHostToDevice, st));
    S.P.din_len = (const int32_t *)S.d_din_len.p; S.P.din_bb = (const int32_t *)S.d_din_bb.p;
    S.P.opts.no_fallback_draft = 1;                       // (this slot's copy of the options: the alignment's outcome on a given draft is final)
    return 0;
}

// ---- the heteroduplex finder's host side, shared by ccsx_hd_batch (slot 0, caller drafts) and the fused path (ccsx_hd_request)
static int hd_opts_check(const ccsx_hd_opts *o, ccsx_hd_opts *hd, const char *fn)
{
    if (o) *hd = *o; else ccsx_hd_opts_default(hd);
    if (hd->min_strand_passes < 1 || hd->min_sites < 1 || hd->min_indel < 1 || hd->min_indel > 21 || !(hd->min_alt_frac >= 0.0f && hd->min_alt_frac <= 1.0f) ||
        !(hd->max_pvalue >= 0.0 && hd->max_pvalue <= 1.0)) {
        ccsx_set_error(std::string(fn) + ": options out of range (min_strand_passes, min_sites >= 1; 1 <= min_indel <= 21; min_alt_frac, max_pvalue in [0, 1])"); return -1;
    }
    return 0;
}

static int hd_report_check(const ccsx_hd_report *out, int n_zmw, const char *fn)
{
    if (out->n_zmw != n_zmw || !out->verdict || !out->n_sub_sites || !out->n_indel_sites || !out->n_listed || !out->min_p || !out->sites) {
        ccsx_set_error(std::string(fn) + ": report arrays missing, or sized for another batch"); return -1;
    }
    return 0;
}

static int hd_request_check(const ccsx_hd_request *q, const ccsx_batch *b, ccsx_hd_opts *hd, const char *fn)
{
    if (!q || !q->report) { ccsx_set_error(std::string(fn) + ": null request or report"); return -1; }
    if (q->reserved != 0 || (q->split != 0 && q->split != 1)) { ccsx_set_error(std::string(fn) + ": split must be 0 or 1 and reserved 0"); return -1; }
    if (hd_opts_check(q->opts, hd, fn)) return -1;
    return hd_report_check(q->report, b->n_zmw, fn);
}

// log k!, a sequential sum of log(k) in double (the rule's table), built once per handle by a synchronous copy BEFORE the first kernel that reads it is
// enqueued: no in-flight work reads it while it is written, and it is never written again
static int hd_table(ccsx_handle h)
{
    if (h->d_hd_lf.p) return 0;
    std::vector<double> lf(CCSX_HD_LF_N, 0.0);
    for (int q = 1; q < CCSX_HD_LF_N; ++q) lf[q] = lf[q - 1] + std::log((double)q);
    if (h->d_hd_lf.reserve(lf.size() * 8)) return -2;
    HIPTRY(hipMemcpy(h->d_hd_lf.p, lf.data(), lf.size() * 8, hipMemcpyHostToDevice));
    return 0;
}

// the finder's buffers of a staged slot (about 200 bytes per window slot: the per-window site records dominate), its options and pointers; the sites
// list is cleared on `st` (entries beyond n_listed stay zero).  stage() clears KParams, so a later run of the slot without a request has none of it.
static int hd_attach(ccsx_handle h, Slot &S, const ccsx_hd_opts &hd, int split, hipStream_t st)
{
    const int n = S.P.n_zmw;
    const size_t wins = (size_t)S.P.total_wslots + 1;
    if (S.d_hd_wcnt.reserve(wins * 4) ||
        S.d_hd_wrec.reserve(wins * CCSX_HD_WIN_SITES * sizeof(ccsx_hd_site)) || S.d_hd_wminp.reserve(wins * 8) ||
        S.d_hd_isite.reserve((size_t)n * CCSX_HD_MAX_SITES * sizeof(ccsx_hd_site)) || S.d_hd_zi.reserve((size_t)n * 6 * 4) ||
        S.d_hd_minp.reserve((size_t)n * 8) || S.d_hd_sites.reserve((size_t)n * CCSX_HD_MAX_SITES * sizeof(ccsx_hd_site))) return -2;
    HIPTRY(hipMemsetAsync(S.d_hd_sites.p, 0, (size_t)n * CCSX_HD_MAX_SITES * sizeof(ccsx_hd_site), st));
    KParams &P = S.P;
    P.hd = hd; P.hd_split = split; P.hd_lf = (const double *)h->d_hd_lf.p;
    P.hd_wcnt = (int32_t *)S.d_hd_wcnt.p; P.hd_wrec = (ccsx_hd_site *)S.d_hd_wrec.p; P.hd_wminp = (double *)S.d_hd_wminp.p;
    P.hd_isite = (ccsx_hd_site *)S.d_hd_isite.p; P.hd_zi = (int32_t *)S.d_hd_zi.p; P.hd_minp = (double *)S.d_hd_minp.p;
    P.hd_sites = (ccsx_hd_site *)S.d_hd_sites.p;
    return 0;
}

// the report of a fused run (status: the one after the cascade, which k_hd_verdict keeps before a split)
static int enqueue_hd_download(const Slot &S, ccsx_hd_report *out, hipStream_t s)
{
    const int n = S.P.n_zmw;
    const KParams &P = S.P;
    HIPTRY(hipMemcpyAsync(out->verdict, P.hd_zi, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIPTRY(hipMemcpyAsync(out->n_sub_sites, P.hd_zi + n, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIPTRY(hipMemcpyAsync(out->n_indel_sites, P.hd_zi + 2 * (size_t)n, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIPTRY(hipMemcpyAsync(out->n_listed, P.hd_zi + 3 * (size_t)n, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIPTRY(hipMemcpyAsync(out->min_p, P.hd_minp, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    HIPTRY(hipMemcpyAsync(out->sites, P.hd_sites, (size_t)n * CCSX_HD_MAX_SITES * sizeof(ccsx_hd_site), hipMemcpyDeviceToHost, s));
    if (out->status) HIPTRY(hipMemcpyAsync(out->status, P.hd_zi + 5 * (size_t)n, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    return 0;
}

// ---- adapter palindromes' host side (ccsx_fold_request): argument checks before anything is enqueued, buffers and pointers of a staged slot, the report's download
static int fold_request_check(const ccsx_fold_request *q, const ccsx_batch *b, ccsx_fold_opts *o, const char *fn)
{
    if (!q || !q->report) { ccsx_set_error(std::string(fn) + ": null request or report"); return -1; }
    if (q->reserved[0] != 0 || q->reserved[1] != 0) { ccsx_set_error(std::string(fn) + ": reserved must be 0"); return -1; }
    if (q->opts) *o = *q->opts; else ccsx_fold_opts_default(o);
    if (o->max_occ < 1 || o->max_occ > 64 || o->min_hits < 1 || o->min_arm < 1 || o->min_span_tenths < 0 || o->min_span_tenths > 10 || o->end_slack < 0) {
        ccsx_set_error(std::string(fn) + ": options out of range (1 <= max_occ <= 64; min_hits, min_arm >= 1; 0 <= min_span_tenths <= 10; end_slack >= 0)"); return -1;
    }
    const ccsx_fold_report *r = q->report;
    if (r->n_zmw != b->n_zmw || !r->verdict || !r->fold || !r->hits || !r->span) { ccsx_set_error(std::string(fn) + ": report arrays missing, or sized for another batch"); return -1; }
    return 0;
}

// k_fold's LDS histogram covers the longest draft the cascade aligns (screen_units); -1 when that is beyond its LDS bound
static int fold_attach(ccsx_handle h, Slot &S, const ccsx_fold_opts &o)
{
    const int64_t l = longest_draft(h, S, 16), bins = screen_units(l, ((2 * l - CCSX_FOLD_K - 1) >> 6) + 2, CCSX_FOLD_MAX_BINS, "adapter-palindrome detection");
    if (bins < 0) return -1;
    if (S.d_fold.reserve((size_t)S.P.n_zmw * 16)) return -2;
    S.P.fold = o; S.P.fold_zi = (int32_t *)S.d_fold.p; S.P.fold_bins = (int32_t)bins;
    return 0;
}

// ---- the adapter screen's host side (ccsx_adapter_request): the same three steps.  The checked set and options are copied into `set` / `o`
static int adapter_request_check(const ccsx_adapter_request *q, const ccsx_batch *b, ccsx_adapter_set *set, ccsx_adapter_opts *o, const char *fn)
{
    if (!q || !q->report) { ccsx_set_error(std::string(fn) + ": null adapter request or report"); return -1; }
    if (q->reserved[0] != 0 || q->reserved[1] != 0) { ccsx_set_error(std::string(fn) + ": adapter request: reserved must be 0"); return -1; }
    if (!q->adapters) { ccsx_set_error(std::string(fn) + ": null adapter set"); return -1; }
    if (q->opts) *o = *q->opts; else ccsx_adapter_opts_default(o);
    if (o->max_dist_pct < 0 || o->max_dist_pct > 30 || o->min_copies < 1 || o->max_insert < 0 || o->end_slack < 0) {
        ccsx_set_error(std::string(fn) + ": adapter options out of range (0 <= max_dist_pct <= 30; min_copies >= 1; max_insert, end_slack >= 0)"); return -1;
    }
    *set = *q->adapters;
    if (set->n_adapters < 1 || set->n_adapters > CCSX_ADAPTER_MAX_PATTERNS) { ccsx_set_error(std::string(fn) + ": n_adapters outside 1 .. 8"); return -1; }
    for (int a = 0; a < set->n_adapters; ++a) {
        if (set->len[a] < CCSX_ADAPTER_MIN_LEN || set->len[a] > CCSX_ADAPTER_MAX_LEN) {
            ccsx_set_error(std::string(fn) + ": adapter " + std::to_string(a) + ": length outside 16 .. 64"); return -1;
        }
        for (int i = 0; i < set->len[a]; ++i)
            if (set->seq[a][i] > 3) { ccsx_set_error(std::string(fn) + ": adapter " + std::to_string(a) + ": code above 3"); return -1; }
    }
    const ccsx_adapter_report *r = q->report;
    if (r->n_zmw != b->n_zmw || !r->tested || !r->verdict || !r->n_hits || !r->n_listed || !r->covered || !r->max_gap || !r->first_start || !r->last_end ||
        !r->min_dist || !r->hits) { ccsx_set_error(std::string(fn) + ": adapter report arrays missing, or sized for another batch"); return -1; }
    return 0;
}

// k_adapter's two LDS bitmaps are sized from the longest draft the cascade aligns (screen_units), so a handle opened with a larger max_length gets larger
// bitmaps; -1 when that is beyond their LDS bound
static int adapter_attach(ccsx_handle h, Slot &S, const ccsx_adapter_set &set, const ccsx_adapter_opts &o)
{
    static_assert(sizeof(ccsx_adapter_hit) == 12, "k_adapter writes a hit as three words");
    const int n = S.P.n_zmw;
    const int64_t l = longest_draft(h, S, 32), words = screen_units(l, (l + 31) >> 5, CCSX_ADAPTER_MAX_WORDS, "adapter screen");
    if (words < 0) return -1;
    if (S.d_adapt.reserve((size_t)n * (9 * 4 + CCSX_ADAPTER_MAX_HITS * sizeof(ccsx_adapter_hit)))) return -2;
    KParams &P = S.P;
    P.adapt = o; P.adapt_zi = (int32_t *)S.d_adapt.p; P.adapt_hits = P.adapt_zi + (size_t)9 * n; P.adapt_words = (int32_t)words; P.adapt_n = set.n_adapters;
    for (int a = 0; a < CCSX_ADAPTER_MAX_PATTERNS; ++a) {
        P.adapt_len[a] = a < set.n_adapters ? (uint8_t)set.len[a] : 0;
        for (int w = 0; w < 4; ++w) P.adapt_seq[a][w] = 0u;
        for (int i = 0; a < set.n_adapters && i < set.len[a]; ++i) P.adapt_seq[a][i >> 4] |= (uint32_t)set.seq[a][i] << (2 * (i & 15));
    }
    return 0;
}

// ---- the control screen's host side (ccsx_control_request): the same three steps.  The checked sequence and options are copied into `seq` / `o`
static int control_request_check(const ccsx_control_request *q, const ccsx_batch *b, std::vector<uint8_t> *seq, ccsx_control_opts *o, const char *fn)
{
    if (!q || !q->report) { ccsx_set_error(std::string(fn) + ": null control request or report"); return -1; }
    if (q->reserved[0] != 0 || q->reserved[1] != 0) { ccsx_set_error(std::string(fn) + ": control request: reserved must be 0"); return -1; }
    if (!q->control || !q->control->seq) { ccsx_set_error(std::string(fn) + ": null control sequence"); return -1; }
    if (q->control->reserved != 0) { ccsx_set_error(std::string(fn) + ": control sequence: reserved must be 0"); return -1; }
    if (q->opts) *o = *q->opts; else ccsx_control_opts_default(o);
    if (o->max_occ < 1 || o->max_occ > 64 || o->min_matched < 1 || o->min_ctl_tenths < 0 || o->min_ctl_tenths > 10 || o->min_draft_tenths < 0 || o->min_draft_tenths > 10) {
        ccsx_set_error(std::string(fn) + ": control options out of range (1 <= max_occ <= 64; min_matched >= 1; 0 <= min_ctl_tenths, min_draft_tenths <= 10)"); return -1;
    }
    const int32_t M = q->control->len;
    if (M < CCSX_CONTROL_MIN_LEN || M > CCSX_CONTROL_MAX_LEN) { ccsx_set_error(std::string(fn) + ": control length outside 64 .. 4096"); return -1; }
    for (int32_t i = 0; i < M; ++i)
        if (q->control->seq[i] > 3) { ccsx_set_error(std::string(fn) + ": control: code above 3"); return -1; }
    seq->assign(q->control->seq, q->control->seq + M);
    const ccsx_control_report *r = q->report;
    if (r->n_zmw != b->n_zmw || !r->verdict || !r->strand || !r->hits || !r->matched || !r->ctl_start || !r->ctl_end || !r->draft_start || !r->draft_end) {
        ccsx_set_error(std::string(fn) + ": control report arrays missing, or sized for another batch"); return -1;
    }
    return 0;
}

// The index k_control reads (ccsx_kernels.h), into idx[CCSX_CONTROL_INDEX_WORDS]: every 15-mer position of the control in increasing (code, position), without the
// codes that occur more than max_occ times.  The order is total, so the same control and max_occ give the same bytes.
static void control_index_build(const std::vector<uint8_t> &c, int max_occ, uint32_t *idx)
{
    const int M = (int)c.size(), K = CCSX_FOLD_K, np_ = M - K + 1;
    std::vector<uint64_t> key((size_t)np_);                     // code << 16 | position
    uint32_t F = 0u;
    for (int i = 0; i < M; ++i) {
        F = ((F << 2) | c[i]) & ((1u << (2 * K)) - 1u);
        if (i >= K - 1) key[i - K + 1] = ((uint64_t)F << 16) | (uint64_t)(i - K + 1);
    }
    std::sort(key.begin(), key.end());
    std::fill(idx, idx + CCSX_CONTROL_POS_WORD, 0xffffffffu);
    std::fill(idx + CCSX_CONTROL_POS_WORD, idx + CCSX_CONTROL_INDEX_WORDS, 0u);
    uint16_t *pos = reinterpret_cast<uint16_t *>(idx + CCSX_CONTROL_POS_WORD);
    uint32_t *filt = idx + CCSX_CONTROL_FILTER_WORD;
    int m = 0;
    for (int a = 0, e; a < np_; a = e) {
        for (e = a + 1; e < np_ && (key[e] >> 16) == (key[a] >> 16); ++e) {}
        if (e - a > max_occ) continue;
        const uint32_t code = (uint32_t)(key[a] >> 16), hsh = ccsx_fmix32(code) & (uint32_t)(CCSX_CONTROL_FILTER_BITS - 1);
        filt[hsh >> 5] |= 1u << (hsh & 31u);
        for (int k = a; k < e; ++k, ++m) { idx[m] = code; pos[m] = (uint16_t)(key[k] & 0xffffu); }
    }
}

// k_control's two LDS histograms cover the longest draft the cascade aligns (screen_units); -1 when that is beyond their LDS bound.  The index is the slot's
// own, in page-locked memory that lives as long as the slot: its copy is enqueued on `st` with the slot's other uploads, and a slot is only staged again after
// its ticket has been retired, so no ticket in flight reads an index another one replaces.
static int control_attach(ccsx_handle h, Slot &S, const std::vector<uint8_t> &seq, const ccsx_control_opts &o, hipStream_t st)
{
    const int n = S.P.n_zmw, M = (int)seq.size();
    const int64_t l = longest_draft(h, S, 16), bins = screen_units(l, ((l - CCSX_FOLD_K + M - CCSX_FOLD_K) >> 6) + 2, CCSX_CONTROL_MAX_BINS, "control screen");
    if (bins < 0) return -1;
    if (S.d_ctl.reserve((size_t)CCSX_CONTROL_INDEX_WORDS * 4 + (size_t)n * 32) || S.ctl_index.resize(CCSX_CONTROL_INDEX_WORDS)) return -2;
    control_index_build(seq, o.max_occ, S.ctl_index.p);
    KParams &P = S.P;
    P.ctl = o; P.ctl_index = (const uint32_t *)S.d_ctl.p; P.ctl_zi = (int32_t *)S.d_ctl.p + CCSX_CONTROL_INDEX_WORDS; P.ctl_len = M; P.ctl_bins = (int32_t)bins;
    if (hipError_t e = hipMemcpyAsync(S.d_ctl.p, S.ctl_index.p, (size_t)CCSX_CONTROL_INDEX_WORDS * 4, hipMemcpyHostToDevice, st)) {
        ccsx_set_error(std::string("control screen: index upload: ") + hipGetErrorString(e)); return -2;
    }
    return 0;
}

// ---- the coverage screen's host side (ccsx_coverage_request): the same three steps.  The checked options are copied into `o`
static int coverage_request_check(const ccsx_coverage_request *q, const ccsx_batch *b, ccsx_coverage_opts *o, const char *fn)
{
    if (!q || !q->report) { ccsx_set_error(std::string(fn) + ": null coverage request or report"); return -1; }
    if (q->reserved[0] != 0 || q->reserved[1] != 0) { ccsx_set_error(std::string(fn) + ": coverage request: reserved must be 0"); return -1; }
    if (q->gate & ~0x3cu) { ccsx_set_error(std::string(fn) + ": coverage request: gate has bits outside 2 .. 5"); return -1; }
    if (q->opts) *o = *q->opts; else ccsx_coverage_opts_default(o);
    if (o->drop_percent < 0 || o->drop_percent > 100 || o->max_lost_percent < 0 || o->max_lost_percent > 100 || o->block < 1 || o->block > 4096 ||
        o->min_spans < 0 || o->min_spans > CCSX_MAX_PASSES) {
        ccsx_set_error(std::string(fn) + ": coverage options out of range (0 <= drop_percent, max_lost_percent <= 100; 1 <= block <= 4096; 0 <= min_spans <= 255)"); return -1;
    }
    const ccsx_coverage_report *r = q->report;
    if (r->n_zmw != b->n_zmw || !r->verdict || !r->np_aligned || !r->spans || !r->cov_max || !r->clean_min || !r->drop_window || !r->drop_windows || !r->reach_sum ||
        !r->used_sum || !r->used_min) { ccsx_set_error(std::string(fn) + ": coverage report arrays missing, or sized for another batch"); return -1; }
    return 0;
}

// the report's planes and the reach bytes of every window slot; min_spans 0 becomes the handle's min_passes here.  Nothing is enqueued: k_coverage writes every
// plane of every ZMW and the byte of every window k_coverage_post reads
static int coverage_attach(ccsx_handle h, Slot &S, const ccsx_coverage_opts &o, uint32_t gate)
{
    const size_t n = (size_t)S.P.n_zmw, wins = (size_t)S.P.total_wslots + 1;
    if (S.d_cov.reserve(n * CCSX_COVERAGE_PLANES * 4 + wins)) return -2;
    KParams &P = S.P;
    P.cov = o; P.cov_gate = gate; P.cov_zi = (int32_t *)S.d_cov.p; P.cov_reach = (uint8_t *)(P.cov_zi + n * CCSX_COVERAGE_PLANES);
    if (P.cov.min_spans == 0) P.cov.min_spans = h->opts.min_passes;
    return 0;
}

// ---- the polisher hand-off's host side (DESIGN.md §2 "Polisher hand-off")
void ccsx_handoff_opts_default(ccsx_handoff_opts *o)
{
    if (!o) return;
    o->tile_len = 100; o->max_rows = 20; o->skip_above = 45; o->reserved = 0;   // DESIGN.md §2 "Polisher hand-off": the reasons for them
}

int ccsx_handoff_rule_version(void) { return 1; }

#define CCSX_HANDOFF_MAX_TILES (1ll << 26)   // the kernels index tiles, and M x R slots, with int32

// a request as the caller gave it: every refusal by its own message; the options (NULL: the defaults) and the out struct copied
static int handoff_request_check(const ccsx_handoff_request *q, ccsx_handoff_opts *o, ccsx_handoff_out *out, const char *fn)
{
    const std::string f(fn);
    if (q->reserved[0] || q->reserved[1]) { ccsx_set_error(f + ": handoff request: reserved must be 0"); return -1; }
    if (q->opts) *o = *q->opts; else ccsx_handoff_opts_default(o);
    if (o->reserved) { ccsx_set_error(f + ": handoff options: reserved must be 0"); return -1; }
    if (o->tile_len < 16 || o->tile_len > 128 || o->max_rows < 1 || o->max_rows > 32 || o->skip_above < 0 || o->skip_above > 94) {
        ccsx_set_error(f + ": handoff options out of range (16 <= tile_len <= 128; 1 <= max_rows <= 32; 0 <= skip_above <= 94)");
        return -1;
    }
    if (!q->out) { ccsx_set_error(f + ": null handoff out"); return -1; }
    *out = *q->out;
    if (!out->counts || !out->tile_zmw || !out->tile_start || !out->tile_len || !out->tile_qsum || !out->tile_rows || !out->row_pass || !out->row_strand || !out->cells) {
        ccsx_set_error(f + ": handoff out arrays missing");
        return -1;
    }
    if (out->max_tiles < 1 || out->max_tiles > CCSX_HANDOFF_MAX_TILES) { ccsx_set_error(f + ": handoff out: max_tiles must be 1 .. 2^26"); return -1; }
    return 0;
}

// the slot's scratch and output arrays, reserved by the first request and grown by a larger one; nothing is enqueued: the kernels write every word they read
static int handoff_attach(Slot &S, const ccsx_handoff_opts &o, int64_t max_tiles)
{
    KParams &P = S.P;
    const size_t n = (size_t)P.n_zmw, wins = (size_t)P.total_wslots + 1, M = (size_t)max_tiles, R = (size_t)o.max_rows, T = (size_t)o.tile_len;
    const size_t tiles = (size_t)ccsx_handoff_tile_off(S.T.cap_total, (int)n, o.tile_len) + 1;
    if (tiles > 0x7fff0000ull) { ccsx_set_error("handoff: batch too large (more than 2^31 tiles): split it"); return -1; }
    if (S.d_ho.reserve((2 * n + 2 * tiles + wins) * 4) || S.d_ho_out.reserve(M * R * T * 4 + (5 * M + 2) * 4 + 2 * M * R)) return -2;
    P.ho = o; P.ho_max_tiles = (int32_t)M;
    P.ho_zcnt = (int32_t *)S.d_ho.p; P.ho_tslot = P.ho_zcnt + 2 * n; P.ho_tqsum = P.ho_tslot + tiles; P.ho_woff = P.ho_tqsum + tiles;
    P.ho_cells = (uchar4 *)S.d_ho_out.p; P.ho_hdr = (int32_t *)(P.ho_cells + M * R * T); P.ho_counts = P.ho_hdr + 5 * M; P.ho_rows = (uint8_t *)(P.ho_counts + 2);
    return 0;
}

// the output arrays into the caller's, host or device memory (hipMemcpyDefault), on `s`: the whole capacity, or — written_only, when the run has ended — the
// slots that were written
static int enqueue_handoff_download(const Slot &S, const ccsx_handoff_out &out, bool written_only, hipStream_t s)
{
    const KParams &P = S.P;
    const size_t M = (size_t)P.ho_max_tiles, R = (size_t)P.ho.max_rows, T = (size_t)P.ho.tile_len;
    size_t m = M;
    if (written_only) {
        int32_t c[2] = {0, 0};
        HIPTRY(hipMemcpyAsync(c, P.ho_counts, 8, hipMemcpyDeviceToHost, s));
        HIPTRY(hipStreamSynchronize(s));
        m = std::min<size_t>(M, (size_t)std::max(c[1], 0));
    }
    HIPTRY(hipMemcpyAsync(out.counts, P.ho_counts, 8, hipMemcpyDefault, s));
    if (!m) return 0;
    int32_t *const hdr[5] = {out.tile_zmw, out.tile_start, out.tile_len, out.tile_qsum, out.tile_rows};
    for (int k = 0; k < 5; ++k) HIPTRY(hipMemcpyAsync(hdr[k], P.ho_hdr + (size_t)k * M, m * 4, hipMemcpyDefault, s));
    HIPTRY(hipMemcpyAsync(out.row_pass, P.ho_rows, m * R, hipMemcpyDefault, s));
    HIPTRY(hipMemcpyAsync(out.row_strand, P.ho_rows + M * R, m * R, hipMemcpyDefault, s));
    HIPTRY(hipMemcpyAsync(out.cells, P.ho_cells, m * R * T * 4, hipMemcpyDefault, s));
    return 0;
}

// ---- the representative reads' host side (DESIGN.md §2 "Representative rule"; the request's checks: ccsx_represent_api.cpp).  k_represent's parameters are the
// slot's own inputs, final drafts and result planes: nothing is uploaded, the [2][n] report is all it reserves.
static int represent_attach(Slot &S, const ccsx_represent_request &q)
{
    KParams &P = S.P;
    const size_t n = (size_t)P.n_zmw;
    if (S.d_rp.reserve((n ? n : 1) * CCSX_RP_PLANES * 4)) return -2;
    RepresentParams R{};
    R.n = (int32_t)n; R.top_passes = P.opts.top_passes; R.subread_fallback = q.subread_fallback;
    R.read_off = P.read_off; R.base_off = P.base_off; R.bases = P.bases; R.pw = P.pw; R.ipd = P.ipd; R.flags = P.flags;
    R.seq_off = P.seq_off; R.draft = P.draft; R.draft_len = P.draft_len; R.status = P.out_status;
    R.out_len = P.out_len; R.out_rq = P.out_rq; R.out_ec = P.out_ec; R.out_seq = P.out_seq; R.out_qual = P.out_qual; R.out_raw = P.out_raw;
    R.out_kin = q.kinetics ? P.out_kin : nullptr; R.kin_plane = P.kin_plane;
    R.rep = (int32_t *)S.d_rp.p;
    if (q.kinetics && (!P.out_kin || !P.ipd)) { ccsx_set_error("represent request: kinetics needs opts.hifi_kinetics and batch.ipd"); return -1; }
    P.rep = R;
    return 0;
}

// what a ccsx_extras asks for (NULL: nothing); -1 for a malformed one
static int extras_want(const ccsx_extras *ex, bool *tandem)
{
    *tandem = false;
    if (!ex) return 0;
    if (ex->min_tandem_repeat_length < 0 || ex->reserved != 0) { ccsx_set_error("ccsx_extras: min_tandem_repeat_length must be >= 0 and reserved 0"); return -1; }
    *tandem = ex->tandem_len != nullptr || ex->min_tandem_repeat_length > 0;
    return 0;
}

// The requests of which a call carries one at most (NULL: none): each changes what the polish stage leaves or reads
struct Exclusive {
    const ccsx_handoff_request *handoff = nullptr;
    const ccsx_barcode_request *barcodes = nullptr;
    const ccsx_segment_request *segments = nullptr;
    const ccsx_hd_request *hd = nullptr;
    const ccsx_cdna_request *cdna = nullptr;
};

// The Wants of one call of the exported function `fn` (NULL extras or request: none of it).  Enqueues nothing and needs no handle: the requests are checked
// first, each refused by its own message, then the extras; the caller's null-argument check follows (without a batch there is nothing to measure a report
// against, and that check refuses the call).
static int build_wants(const ccsx_extras *ex, const Exclusive &x, const ccsx_fold_request *fold, const ccsx_adapter_request *adapters,
                       const ccsx_control_request *control, const ccsx_batch *b, const char *fn, Wants *W, const ccsx_coverage_request *coverage = nullptr)
{
    *W = Wants{};
    if (x.cdna && x.handoff) return refuse(fn, "the cdna request and the hand-off are not combined");
    if (x.cdna && x.hd) return refuse(fn, "the cdna and the heteroduplex requests are not combined");
    if (x.cdna && x.barcodes) return refuse(fn, "the cdna and the barcode requests are not combined");
    if (x.cdna && x.segments) return refuse(fn, "the cdna and the segment requests are not combined");
    if (x.cdna && b && reads_request_check(x.cdna, b, &W->cdna, fn)) return -1;
    if (x.segments && x.handoff) return refuse(fn, "the segment request and the hand-off are not combined");
    if (x.segments && x.hd) return refuse(fn, "the segment and the heteroduplex requests are not combined");
    if (x.segments && x.barcodes) return refuse(fn, "the segment and the barcode requests are not combined");
    if (x.segments && b && reads_request_check(x.segments, b, &W->segments, fn)) return -1;
    if (x.barcodes && x.handoff) return refuse(fn, "the barcode request and the hand-off are not combined");
    if (x.barcodes && x.hd) return refuse(fn, "the barcode and the heteroduplex requests are not combined");
    if (x.barcodes && b && reads_request_check(x.barcodes, b, &W->barcodes, fn)) return -1;
    if (x.handoff && handoff_request_check(x.handoff, &W->handoff_opts, &W->handoff_out, fn)) return -1;
    if (coverage && b && coverage_request_check(coverage, b, &W->coverage_opts, fn)) return -1;
    if (x.hd && b && hd_request_check(x.hd, b, &W->hd_opts, fn)) return -1;
    if (fold && b && fold_request_check(fold, b, &W->fold_opts, fn)) return -1;
    if (adapters && b && adapter_request_check(adapters, b, &W->adapter_set, &W->adapter_opts, fn)) return -1;
    if (control && b && control_request_check(control, b, &W->control_seq, &W->control_opts, fn)) return -1;
    if (extras_want(ex, &W->tandem)) return -1;
    W->hd = x.hd; W->fold = fold; W->adapters = adapters; W->control = control; W->coverage = coverage; W->handoff = x.handoff; W->barcodes.req = x.barcodes; W->segments.req = x.segments; W->cdna.req = x.cdna;
    if (ex) { W->pile = ex->pile; W->tandem_len = ex->tandem_len; W->min_tandem = W->tandem ? ex->min_tandem_repeat_length : 0; }
    return 0;
}

// What W asks for on a staged slot: checks, buffers and pointers, in the order of what can still be refused.  -1 only while this call has enqueued nothing
// (the pileup planes, the LDS bounds of k_fold, k_adapter and k_control), -2 otherwise; the steps that enqueue on `st` (the control index's upload, after its own
// LDS check, and the finder's memset) come last.
static int attach(ccsx_handle h, Slot &S, const Wants &W, hipStream_t st)
{
    int rc;
    if (W.pile && (rc = check_pile(S, W.pile))) return rc;
    if (W.fold && (rc = fold_attach(h, S, W.fold_opts))) return rc;
    if (W.adapters && (rc = adapter_attach(h, S, W.adapter_set, W.adapter_opts))) return rc;
    if (W.coverage && (rc = coverage_attach(h, S, W.coverage_opts, W.coverage->gate))) return rc;
    if (W.handoff && (rc = handoff_attach(S, W.handoff_opts, W.handoff_out.max_tiles))) return rc;
    if (W.barcodes.req && (rc = reads_attach(S, W.barcodes, st))) return rc;
    if (W.segments.req && (rc = reads_attach(S, W.segments, st))) return rc;
    if (W.cdna.req && (rc = reads_attach(S, W.cdna, st))) return rc;
    if (W.represent && (rc = represent_attach(S, W.represent_req))) return rc;
    if (W.control && (rc = control_attach(h, S, W.control_seq, W.control_opts, st))) return rc;
    if (W.hd && ((rc = hd_table(h)) || (rc = hd_attach(h, S, W.hd_opts, W.hd->split, st)))) return rc;
    return 0;
}

// everything W receives beside the ccsx_results, copied on `s`
static int enqueue_wants_download(const Slot &S, const Wants &W, hipStream_t s)
{
    int rc;
    const size_t n = (size_t)S.P.n_zmw;
    if (W.pile && (rc = enqueue_pile_download(S, W.pile, s))) return rc;
    if (W.tandem_len) HIPTRY(hipMemcpyAsync(W.tandem_len, S.P.tlen, n * 4, hipMemcpyDeviceToHost, s));
    if (W.hd && (rc = enqueue_hd_download(S, W.hd->report, s))) return rc;
    if (W.fold) {
        const ccsx_fold_report *r = W.fold->report;
        if ((rc = download_planes({r->verdict, r->fold, r->hits, r->span}, S.P.fold_zi, n, s))) return rc;
    }
    if (W.adapters) {
        const ccsx_adapter_report *r = W.adapters->report;
        if ((rc = download_planes({r->tested, r->verdict, r->n_hits, r->n_listed, r->covered, r->max_gap, r->first_start, r->last_end, r->min_dist},
                                  S.P.adapt_zi, n, s))) return rc;
        HIPTRY(hipMemcpyAsync(r->hits, S.P.adapt_hits, n * CCSX_ADAPTER_MAX_HITS * sizeof(ccsx_adapter_hit), hipMemcpyDeviceToHost, s));
    }
    if (W.control) {
        const ccsx_control_report *r = W.control->report;
        if ((rc = download_planes({r->verdict, r->strand, r->hits, r->matched, r->ctl_start, r->ctl_end, r->draft_start, r->draft_end}, S.P.ctl_zi, n, s))) return rc;
    }
    if (W.coverage) {
        const ccsx_coverage_report *r = W.coverage->report;
        if ((rc = download_planes({r->verdict, r->np_aligned, r->spans, r->cov_max, r->clean_min, r->drop_window, r->drop_windows, r->reach_sum, r->used_sum, r->used_min},
                                  S.P.cov_zi, n, s))) return rc;
    }
    if (W.handoff && (rc = enqueue_handoff_download(S, W.handoff_out, W.handoff_written_only, s))) return rc;
    if (W.barcodes.req && (rc = reads_download<Barcodes>(S.P.bc, W.barcodes.req->report, s))) return rc;
    if (W.segments.req && (rc = reads_download<Segments>(S.P.sg, W.segments.req->report, s))) return rc;
    if (W.cdna.req && (rc = reads_download<Cdna>(S.P.cd, W.cdna.req->report, s))) return rc;
    if (W.represent && n) {
        const ccsx_represent_report *r = W.represent_req.report;
        if ((rc = download_planes({r->cls, r->pass}, S.P.rep.rep, n, s))) return rc;
    }
    return 0;
}

// ---- the polisher hand-back's host side (DESIGN.md §2 "Polisher hand-back"): a request as its entry points checked and copied it
struct RefineReq {
    const ccsx_results *base;
    const int32_t *backbone;
    ccsx_refine_tiles tiles;
    ccsx_refine_report rep;
};

#define CCSX_REFINE_MAX_TILES (1ll << 26)

void ccsx_refine_tiles_init(ccsx_refine_tiles *t)
{
    if (!t) return;
    std::memset(t, 0, sizeof *t);
    t->stride = 128;
}

int ccsx_refine_rule_version(void) { return 1; }

uint64_t ccsx_refine_perr(int32_t q)
{
    static const uint64_t perr_fx[CCSX_REFINE_NQ] = {CCSX_REFINE_PERR_TABLE};
    return q >= 0 && q < CCSX_REFINE_NQ ? perr_fx[q] : 0;
}

// every refusal that needs no staged batch, each by its own message; the tiles and report structs are copied (they are read during the call only)
static int refine_request_check(const ccsx_batch *b, const ccsx_results *base, const int32_t *backbone, const ccsx_refine_tiles *t, const ccsx_refine_report *rep,
                                RefineReq *rf, const char *fn)
{
    if (!b || !base || !backbone || !t || !rep) return refuse(fn, "null argument");
    if (t->n_tiles < 0 || t->n_tiles > CCSX_REFINE_MAX_TILES) return refuse(fn, "refine tiles: n_tiles must be 0 .. 2^26");
    if (t->stride < 1 || t->stride > 256) return refuse(fn, "refine tiles: stride must be 1 .. 256");
    if (t->reserved0 || t->reserved[0] || t->reserved[1]) return refuse(fn, "refine tiles: reserved must be 0");
    if (t->n_tiles > 0 && (!t->tile_zmw || !t->tile_start || !t->tile_len || !t->new_len || !t->new_seq || !t->new_qual)) return refuse(fn, "refine tiles: arrays missing");
    if (!rep->counts || !rep->code || !rep->n_applied || !rep->new_len || !rep->rq_merged) return refuse(fn, "refine report: arrays missing");
    if (base->n_zmw != b->n_zmw || !base->seq_off || !base->seq_len || !base->seq || !base->qual) return refuse(fn, "base: missing arrays, or sized for another batch");
    *rf = RefineReq{base, backbone, *t, *rep};
    return 0;
}

// `base` against the staged batch: the capacity layout, and no row longer than its slot
static int refine_base_check(const Slot &S, const ccsx_results *base, const char *fn)
{
    const int n = S.P.n_zmw;
    if (base->seq_capacity < S.seq_off[n]) return refuse(fn, "base: smaller than the capacity layout of this batch (ccsx_result_layout)");
    for (int z = 0; z <= n; ++z) if (base->seq_off[z] != S.seq_off[z]) return refuse(fn, "base: seq_off is not the capacity layout of this batch (ccsx_result_layout)");
    for (int z = 0; z < n; ++z) if (base->seq_len[z] > S.seq_off[z + 1] - S.seq_off[z]) return refuse(fn, "base: a sequence is longer than its slot");
    return 0;
}

// The hand-back of a staged slot on `st`: the slot's buffers (reserved by the first request), the copies of the tile list (host or device memory), of base and
// of the backbones, then k_refine_check, k_refine_plan and k_refine_splice, which leave the slot as upload_drafts would: the drafts in the draft buffer, din_len,
// din_bb.
static int refine_enqueue(Slot &S, const RefineReq &rf, hipStream_t st)
{
    const size_t n = (size_t)S.P.n_zmw, cap = (size_t)S.seq_off[n], M = (size_t)rf.tiles.n_tiles, U = (size_t)rf.tiles.stride;
    if (S.d_din_len.reserve(n * 4) || S.d_din_bb.reserve(n * 4)) return -2;
    if (S.d_rf_tiles.reserve(M * 5 * 4 + 2 * M * U + 16) || S.d_rf_base.reserve(n * 8 + 2 * cap + 16) || S.d_rf_rep.reserve(n * 8 + 16 + n * 16 + cap + 16)) return -2;
    RefineParams R{};
    R.n_zmw = (int32_t)n; R.stride = (int32_t)U; R.n_tiles = (int64_t)M;
    R.read_off = S.P.read_off; R.seq_off = S.P.seq_off;
    int32_t *ti = (int32_t *)S.d_rf_tiles.p;
    R.tile_zmw = ti; R.tile_start = ti + M; R.tile_len = ti + 2 * M; R.tile_new_len = ti + 3 * M; R.tile_cls = (uint32_t *)(ti + 4 * M);
    uint8_t *tb = (uint8_t *)(ti + 5 * M);
    R.new_seq = tb; R.new_qual = tb + M * U;
    int32_t *bi = (int32_t *)S.d_rf_base.p;
    R.base_len = bi; R.backbone = bi + n;
    uint8_t *bs = (uint8_t *)(bi + 2 * n);
    R.base_seq = bs; R.base_qual = bs + cap;
    R.tile_first = (int64_t *)S.d_rf_rep.p;
    R.counts = (int32_t *)(R.tile_first + n);
    R.code = R.counts + 4; R.n_applied = R.code + n; R.new_len = R.n_applied + n; R.rq_merged = (float *)(R.new_len + n);
    R.qual_merged = rf.rep.qual_merged ? (uint8_t *)(R.rq_merged + n) : nullptr;
    R.draft = (uint8_t *)S.d_draft.p; R.din_len = (int32_t *)S.d_din_len.p; R.din_bb = (int32_t *)S.d_din_bb.p;
    if (M) {
        const ccsx_refine_tiles &t = rf.tiles;
        HIPTRY(hipMemcpyAsync(ti, t.tile_zmw, M * 4, hipMemcpyDefault, st));
        HIPTRY(hipMemcpyAsync(ti + M, t.tile_start, M * 4, hipMemcpyDefault, st));
        HIPTRY(hipMemcpyAsync(ti + 2 * M, t.tile_len, M * 4, hipMemcpyDefault, st));
        HIPTRY(hipMemcpyAsync(ti + 3 * M, t.new_len, M * 4, hipMemcpyDefault, st));
        HIPTRY(hipMemcpyAsync(tb, t.new_seq, M * U, hipMemcpyDefault, st));
        HIPTRY(hipMemcpyAsync(tb + M * U, t.new_qual, M * U, hipMemcpyDefault, st));
    }
    HIPTRY(hipMemcpyAsync(bi, rf.base->seq_len, n * 4, hipMemcpyHostToDevice, st));
    HIPTRY(hipMemcpyAsync(bi + n, rf.backbone, n * 4, hipMemcpyHostToDevice, st));
    if (cap) {
        HIPTRY(hipMemcpyAsync(bs, rf.base->seq, cap, hipMemcpyHostToDevice, st));
        HIPTRY(hipMemcpyAsync(bs + cap, rf.base->qual, cap, hipMemcpyHostToDevice, st));
    }
    if (const char *failed = ccsx_refine_launch(R, st)) { ccsx_set_error(std::string("kernel launch failed: ") + failed); return -2; }
    S.RP = R;
    S.P.din_len = R.din_len; S.P.din_bb = R.din_bb;
    S.P.opts.no_fallback_draft = 1;                       // (as upload_drafts: the alignment's outcome on a given draft is final)
    return 0;
}

// the report of the slot's hand-back into the caller's host arrays, on `s` (after CCSX_EV_END)
static int refine_download(const Slot &S, const ccsx_refine_report &rep, hipStream_t s)
{
    const RefineParams &R = S.RP;
    const size_t n = (size_t)R.n_zmw;
    HIPTRY(hipMemcpyAsync(rep.counts, R.counts, 12, hipMemcpyDeviceToHost, s));
    if (int rc = download_planes({rep.code, rep.n_applied, rep.new_len}, R.code, n, s)) return rc;
    HIPTRY(hipMemcpyAsync(rep.rq_merged, R.rq_merged, n * 4, hipMemcpyDeviceToHost, s));
    if (rep.qual_merged && S.seq_off[n] > 0) HIPTRY(hipMemcpyAsync(rep.qual_merged, R.qual_merged, (size_t)S.seq_off[n], hipMemcpyDeviceToHost, s));
    return 0;
}

// one batch through the handle's pipeline: the fused path (ccsx_submit and its variants, with their Wants), the draft seam or the polish seam
static int submit_impl(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, ccsx_ticket *ticket, int mode, ccsx_drafts *dr_out, const ccsx_drafts *dr_in, uint32_t flags,
                       const Wants &W, const char *fn, const RefineReq *rf = nullptr)
{
    if (!h || !b || !ticket || (mode != CCSX_RUN_DRAFT && !res) || (mode == CCSX_RUN_DRAFT && !dr_out) || (mode == CCSX_RUN_POLISH && !dr_in && !rf)) return refuse(fn, "null argument");
#ifdef CCSX_FAULT_INJECTION                                          // test builds only (tests/test_cli_bam.py builds its own copy of the library)
    if (const char *e = std::getenv("CCSX_TEST_FAIL_SUBMIT"))        // fault injection for the driver's error-path test
        if (std::atoll(e) == (long long)h->next_ticket) { ++h->next_ticket; ccsx_set_error("injected failure (CCSX_TEST_FAIL_SUBMIT)"); return -2; }
#endif
    if (h->poisoned) { ccsx_set_error("ccsx_submit: an earlier submit failed after work had been enqueued; destroy the handle"); return -2; }
    HIPTRY(hipSetDevice(h->device));
    if (int rc0 = rebase_epoch(h)) return rc0;
    Slot &S = h->slot[h->next_ticket % CCSX_SLOTS];
    if (int rc0 = retire(h, S)) return rc0;              // (a batch never waited for: the caller's buffers are complete whether or not it ever waits)
    if (W.hd) if (int rc0 = hd_table(h)) return rc0;     // (its synchronous copy before anything of this ticket is enqueued; attach() then finds it built)
    // A failure after the first enqueue must not leave copies or kernels running on a slot the next submit would rewrite
    // (ADVICE r02): drain every stream, mark the slot unusable and refuse further batches on this handle.
    auto fail = [&](int rc_) {
        drain_streams(h);
        (void)hipGetLastError();
        S.staged = false; S.ran = false; S.ticket = -1;
        h->poisoned = true;
        return rc_;
    };
    auto unstage = [&](int rc_) { (void)hipStreamSynchronize(h->s_in); S.staged = false; return rc_; };   // refused after staging, before anything else was enqueued
    int rc = stage(h, S, b, h->s_in, W);
    if (rc) return rc == -1 ? (S.staged = false, rc) : fail(rc);     // -1: rejected by validation before anything was enqueued
    if (mode != CCSX_RUN_DRAFT && (rc = check_results(S, res, S.P.out_kin != nullptr))) return unstage(rc);
    if (mode != CCSX_RUN_FUSED && !rf && (rc = check_drafts(S, mode == CCSX_RUN_DRAFT ? dr_out : dr_in, mode == CCSX_RUN_POLISH))) return unstage(rc);
    if (rf && (rc = refine_base_check(S, rf->base, fn))) return unstage(rc);
    if ((rc = attach(h, S, W, h->s_in))) return rc == -1 ? unstage(rc) : fail(rc);
    S.mode = mode;
    S.P.qv_only = (mode == CCSX_RUN_POLISH && (flags & CCSX_QV_ONLY)) ? 1 : 0;
#define HIPTRY_F(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { ccsx_set_error(std::string(#expr) + ": " + hipGetErrorString(e_)); return fail(-2); } } while (0)
    // the drafts of the polish seam: the caller's, or — the hand-back — spliced on the upload stream by the three kernels, ahead of ev_up
    if (mode == CCSX_RUN_POLISH && (rc = rf ? refine_enqueue(S, *rf, h->s_in) : upload_drafts(S, dr_in, h->s_in))) return fail(rc);
    HIPTRY_F(hipEventRecord(S.ev_up, h->s_in));
    HIPTRY_F(hipStreamWaitEvent(h->s_draft, S.ev_up, 0));
    if ((rc = launch(h, S))) return fail(rc);
    // CCSX_EV_END (end of the last kernel) doubles as the "results ready" event of the download stream
    HIPTRY_F(hipStreamWaitEvent(h->s_out, S.ev[CCSX_EV_END], 0));
    if (mode == CCSX_RUN_DRAFT) {
        const int n = S.P.n_zmw;
        const KParams &P = S.P;
        HIPTRY_F(hipMemcpyAsync(dr_out->status, P.zstat, (size_t)n * 4, hipMemcpyDeviceToHost, h->s_out));
        HIPTRY_F(hipMemcpyAsync(dr_out->len, P.draft_len, (size_t)n * 4, hipMemcpyDeviceToHost, h->s_out));
        HIPTRY_F(hipMemcpyAsync(dr_out->backbone, P.zref, (size_t)n * 4, hipMemcpyDeviceToHost, h->s_out));   // (low byte: masked by retire)
        HIPTRY_F(hipMemcpyAsync(dr_out->seq, P.draft, (size_t)S.seq_off[n], hipMemcpyDeviceToHost, h->s_out));
        if (dr_out->n_windows) HIPTRY_F(hipMemcpyAsync(dr_out->n_windows, P.nwin, (size_t)n * 4, hipMemcpyDeviceToHost, h->s_out));
        if (dr_out->win_bounds) HIPTRY_F(hipMemcpyAsync(dr_out->win_bounds, P.wbounds, (size_t)S.wb_off[n] * 4, hipMemcpyDeviceToHost, h->s_out));
    } else if ((rc = enqueue_download(S, res, h->s_out))) return fail(rc);
    if ((rc = enqueue_wants_download(S, W, h->s_out))) return fail(rc);
    if (rf && (rc = refine_download(S, rf->rep, h->s_out))) return fail(rc);
    HIPTRY_F(hipEventRecord(S.ev_done, h->s_out));
#undef HIPTRY_F
    S.res = mode == CCSX_RUN_DRAFT ? nullptr : res; S.drafts_out = mode == CCSX_RUN_DRAFT ? dr_out : nullptr; S.inflight = true; S.ticket = h->next_ticket;
    h->last = (int)(h->next_ticket % CCSX_SLOTS);
    *ticket = h->next_ticket++;
    return 0;
}

// the fused entry points: the Wants of the call (requests, then extras), the argument this entry point may not be given as NULL, the submit
int ccsx_submit(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, ccsx_ticket *ticket)
{
    return submit_impl(h, b, res, ticket, CCSX_RUN_FUSED, nullptr, nullptr, 0, Wants{}, __func__);
}
int ccsx_submit_pileup(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, ccsx_pileup *pile, ccsx_ticket *ticket)
{
    const ccsx_extras ex = {pile, nullptr, 0, 0};
    Wants W;
    if (build_wants(&ex, {}, nullptr, nullptr, nullptr, b, __func__, &W) || (!pile && refuse(__func__, "null argument"))) return -1;
    return submit_impl(h, b, res, ticket, CCSX_RUN_FUSED, nullptr, nullptr, 0, W, __func__);
}
int ccsx_submit_extras(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const ccsx_extras *ex, ccsx_ticket *ticket)
{
    Wants W;
    if (build_wants(ex, {}, nullptr, nullptr, nullptr, b, __func__, &W)) return -1;
    return submit_impl(h, b, res, ticket, CCSX_RUN_FUSED, nullptr, nullptr, 0, W, __func__);
}
int ccsx_submit_fold(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const ccsx_extras *ex, const ccsx_fold_request *fold, ccsx_ticket *ticket)
{
    Wants W;
    if (build_wants(ex, {}, fold, nullptr, nullptr, b, __func__, &W) || (!fold && refuse(__func__, "null request or report"))) return -1;
    return submit_impl(h, b, res, ticket, CCSX_RUN_FUSED, nullptr, nullptr, 0, W, __func__);
}
int ccsx_submit_screen(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const ccsx_extras *ex, const ccsx_fold_request *fold, const ccsx_adapter_request *adapters,
                       ccsx_ticket *ticket)
{
    Wants W;
    if (build_wants(ex, {}, fold, adapters, nullptr, b, __func__, &W)) return -1;
    return submit_impl(h, b, res, ticket, CCSX_RUN_FUSED, nullptr, nullptr, 0, W, __func__);
}
int ccsx_submit_control(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const ccsx_extras *ex, const ccsx_fold_request *fold, const ccsx_adapter_request *adapters,
                        const ccsx_control_request *control, ccsx_ticket *ticket)
{
    Wants W;
    if (build_wants(ex, {}, fold, adapters, control, b, __func__, &W)) return -1;
    return submit_impl(h, b, res, ticket, CCSX_RUN_FUSED, nullptr, nullptr, 0, W, __func__);
}
// the members of a ccsx_requests as build_wants takes them (NULL: none); -1 for nonzero reserved words
static int requests_wants(const ccsx_requests *rq, const ccsx_batch *b, const char *fn, Wants *W, const Exclusive &x = {})
{
    static const ccsx_requests none = {};
    if (!rq) rq = &none;
    if (rq->reserved[0] || rq->reserved[1] || rq->reserved[2]) return refuse(fn, "ccsx_requests: reserved must be NULL");
    return build_wants(rq->ex, x, rq->fold, rq->adapters, rq->control, b, fn, W, rq->coverage);
}
// the Wants of a call with a heteroduplex request beside the members of rq (the four ccsx_*_hd* entry points): the checks of ccsx_submit_hd, in its order
static int hd_requests_wants(const ccsx_requests *rq, const ccsx_hd_request *hd, const ccsx_batch *b, const char *fn, Wants *W)
{
    if (requests_wants(rq, b, fn, W, {nullptr, nullptr, nullptr, hd}) || (!hd && refuse(fn, "null request or report"))) return -1;
    return 0;
}
// the Wants of a call with a barcode, a segment or a cdna request (x: it alone) beside the members of rq: neither it nor the batch may be NULL
static int reads_wants(const ccsx_requests *rq, const ccsx_batch *b, const Exclusive &x, const char *noun, const char *fn, Wants *W)
{
    if (!x.barcodes && !x.segments && !x.cdna) return refuse(fn, (std::string("null ") + noun + " request").c_str());
    if (!b) return refuse(fn, "null argument");
    return requests_wants(rq, b, fn, W, x);
}
int ccsx_submit_requests(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const ccsx_requests *rq, ccsx_ticket *ticket)
{
    Wants W;
    if (requests_wants(rq, b, __func__, &W)) return -1;
    return submit_impl(h, b, res, ticket, CCSX_RUN_FUSED, nullptr, nullptr, 0, W, __func__);
}
int ccsx_submit_hd_requests(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const ccsx_requests *rq, const ccsx_hd_request *hd, ccsx_ticket *ticket)
{
    Wants W;
    if (hd_requests_wants(rq, hd, b, __func__, &W)) return -1;
    return submit_impl(h, b, res, ticket, CCSX_RUN_FUSED, nullptr, nullptr, 0, W, __func__);
}
int ccsx_submit_hd(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const ccsx_extras *ex, const ccsx_hd_request *hd, ccsx_ticket *ticket)
{
    const ccsx_requests rq = {ex, nullptr, nullptr, nullptr, nullptr, {nullptr, nullptr, nullptr}};
    Wants W;
    if (hd_requests_wants(&rq, hd, b, __func__, &W)) return -1;
    return submit_impl(h, b, res, ticket, CCSX_RUN_FUSED, nullptr, nullptr, 0, W, __func__);
}
int ccsx_submit_handoff(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const ccsx_requests *rq, const ccsx_handoff_request *ho, ccsx_ticket *ticket)
{
    Wants W;
    if (requests_wants(rq, b, __func__, &W, {ho}) || (!ho && refuse(__func__, "null handoff request"))) return -1;
    return submit_impl(h, b, res, ticket, CCSX_RUN_FUSED, nullptr, nullptr, 0, W, __func__);
}
int ccsx_submit_barcodes(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const ccsx_requests *rq, const ccsx_barcode_request *bc, ccsx_ticket *ticket)
{
    Wants W;
    if (reads_wants(rq, b, {nullptr, bc}, Barcodes::noun, __func__, &W)) return -1;
    return submit_impl(h, b, res, ticket, CCSX_RUN_FUSED, nullptr, nullptr, 0, W, __func__);
}
int ccsx_submit_segments(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const ccsx_requests *rq, const ccsx_segment_request *sg, ccsx_ticket *ticket)
{
    Wants W;
    if (reads_wants(rq, b, {nullptr, nullptr, sg}, Segments::noun, __func__, &W)) return -1;
    return submit_impl(h, b, res, ticket, CCSX_RUN_FUSED, nullptr, nullptr, 0, W, __func__);
}
int ccsx_submit_cdna(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const ccsx_requests *rq, const ccsx_cdna_request *cd, ccsx_ticket *ticket)
{
    Wants W;
    if (reads_wants(rq, b, {nullptr, nullptr, nullptr, nullptr, cd}, Cdna::noun, __func__, &W)) return -1;
    return submit_impl(h, b, res, ticket, CCSX_RUN_FUSED, nullptr, nullptr, 0, W, __func__);
}
// the Wants of a call with a representative request: the request checked against the batch and the handle's options and copied, then the members of rq
static int represent_wants(ccsx_handle h, const ccsx_batch *b, const ccsx_requests *rq, const ccsx_represent_request *rp, const char *fn, Wants *W)
{
    if (!rp) return refuse(fn, "null represent request");
    if (!h || !b) return refuse(fn, "null argument");
    if (ccsx_represent_check(rp, b, &h->opts, fn)) return -1;
    if (rq && rq->coverage && rq->coverage->gate != 0) return refuse(fn, "the represent request is not combined with the coverage gate");
    if (requests_wants(rq, b, fn, W)) return -1;
    W->represent_req = *rp; W->represent = true;
    return 0;
}
int ccsx_submit_represent(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const ccsx_requests *rq, const ccsx_represent_request *rp, ccsx_ticket *ticket)
{
    Wants W;
    if (represent_wants(h, b, rq, rp, __func__, &W)) return -1;
    return submit_impl(h, b, res, ticket, CCSX_RUN_FUSED, nullptr, nullptr, 0, W, __func__);
}
int ccsx_submit_draft(ccsx_handle h, const ccsx_batch *b, ccsx_drafts *drafts, ccsx_ticket *ticket)
{
    return submit_impl(h, b, nullptr, ticket, CCSX_RUN_DRAFT, drafts, nullptr, 0, Wants{}, __func__);
}
int ccsx_submit_polish(ccsx_handle h, const ccsx_batch *b, const ccsx_drafts *drafts, ccsx_results *res, uint32_t flags, ccsx_ticket *ticket)
{
    return submit_impl(h, b, res, ticket, CCSX_RUN_POLISH, nullptr, drafts, flags, Wants{}, __func__);
}
int ccsx_draft_batch(ccsx_handle h, const ccsx_batch *b, ccsx_drafts *drafts)
{
    ccsx_ticket t;
    if (int rc = ccsx_submit_draft(h, b, drafts, &t)) return rc;
    return ccsx_wait(h, t);
}
int ccsx_polish_batch(ccsx_handle h, const ccsx_batch *b, const ccsx_drafts *drafts, ccsx_results *res, uint32_t flags)
{
    ccsx_ticket t;
    if (int rc = ccsx_submit_polish(h, b, drafts, res, flags, &t)) return rc;
    return ccsx_wait(h, t);
}

int ccsx_submit_refine(ccsx_handle h, const ccsx_batch *b, const ccsx_results *base, const int32_t *backbone, const ccsx_refine_tiles *tiles, ccsx_results *res,
                       ccsx_refine_report *report, ccsx_ticket *ticket)
{
    RefineReq rf;
    if (refine_request_check(b, base, backbone, tiles, report, &rf, __func__)) return -1;
    return submit_impl(h, b, res, ticket, CCSX_RUN_POLISH, nullptr, nullptr, CCSX_QV_ONLY, Wants{}, __func__, &rf);
}
int ccsx_refine_batch(ccsx_handle h, const ccsx_batch *b, const ccsx_results *base, const int32_t *backbone, const ccsx_refine_tiles *tiles, ccsx_results *res,
                      ccsx_refine_report *report)
{
    ccsx_ticket t;
    if (int rc = ccsx_submit_refine(h, b, base, backbone, tiles, res, report, &t)) return rc;
    return ccsx_wait(h, t);
}

static Slot *slot_of(ccsx_handle h, ccsx_ticket t)
{
    if (!h || t < 0) return nullptr;
    Slot &S = h->slot[t % CCSX_SLOTS];
    return S.ticket == t ? &S : nullptr;
}

int ccsx_wait(ccsx_handle h, ccsx_ticket ticket)
{
    Slot *S = slot_of(h, ticket);
    if (!S) { ccsx_set_error("ccsx_wait: unknown or recycled ticket"); return -1; }
    HIPTRY(hipSetDevice(h->device));
    return retire(h, *S);
}

int ccsx_poll(ccsx_handle h, ccsx_ticket ticket)
{
    Slot *S = slot_of(h, ticket);
    if (!S) { ccsx_set_error("ccsx_poll: unknown or recycled ticket"); return -1; }
    const hipError_t e = hipEventQuery(S->ev_done);
    if (e == hipErrorNotReady) return 0;
    if (e != hipSuccess) { ccsx_set_error(std::string("ccsx_poll: ") + hipGetErrorString(e)); return -2; }
    HIPTRY(hipSetDevice(h->device));
    return retire(h, *S) ? -2 : 1;
}

int ccsx_ticket_timings(ccsx_handle h, ccsx_ticket ticket, ccsx_timings *t)
{
    Slot *S = slot_of(h, ticket);
    if (!S || !t || !(S->ran || S->tm_ok)) { ccsx_set_error("ccsx_ticket_timings: unknown ticket"); return -1; }
    if (S->tm_ok) { *t = S->tm; return 0; }           // taken when the ticket was retired
    HIPTRY(hipSetDevice(h->device));
    return slot_timings(h, *S, t);                    // (still in flight: the live events, no polish workgroups yet)
}

// ---- synchronous form (slot 0): parity tests, stage read-backs, the resident-input leg of the benchmark ----
static int upload_impl(ccsx_handle h, const ccsx_batch *b, const Wants &W)
{
    if (!h) { ccsx_set_error("ccsx_upload: null handle"); return -1; }
    HIPTRY(hipSetDevice(h->device));
    for (auto &S : h->slot) if (int rc = retire(h, S)) return rc;
    Slot &S = h->slot[0];
    S.ticket = -1;                                       // (slot 0 is re-staged: its ticket is recycled, as by a submit; the other slots' tickets stay valid)
    const int rc = stage(h, S, b, h->s_comp, W);
    if (rc) { S.staged = false; return rc; }
    S.mode = CCSX_RUN_FUSED;
    HIPTRY(hipStreamSynchronize(h->s_comp));
    h->last = 0;
    return 0;
}

int ccsx_upload(ccsx_handle h, const ccsx_batch *b) { return upload_impl(h, b, Wants{}); }

int ccsx_run(ccsx_handle h)
{
    if (!h || !h->slot[0].staged || h->slot[0].mode != CCSX_RUN_FUSED) { ccsx_set_error("ccsx_run: no batch uploaded for the fused path: call ccsx_upload first"); return -1; }
    HIPTRY(hipSetDevice(h->device));
    h->last = 0;
    return launch(h, h->slot[0]);
}

int ccsx_sync(ccsx_handle h)
{
    if (!h) return -1;
    HIPTRY(hipSetDevice(h->device));
    HIPTRY(hipStreamSynchronize(h->s_draft));
    HIPTRY(hipStreamSynchronize(h->s_comp));
    Slot &S = h->slot[h->last];
#ifdef CCSX_PROFILE_PHASES
    if (S.staged && S.ran) {
        unsigned long long ph[16];
        HIPTRY(hipMemcpy(ph, S.P.phase, sizeof(ph), hipMemcpyDeviceToHost));
        static const char *nm[8] = {"prologue", "tables+lanes", "chunk plan", "fill", "score", "select/apply", "qv+store", "validity+list"};
        unsigned long long tot = 0;
        for (int i = 0; i < 8; ++i) tot += ph[i];
        for (int i = 0; i < 8; ++i) std::fprintf(stderr, "[ccsx phase] %-14s %6.2f %%  (%llu cycles)\n", nm[i], tot ? 100.0 * ph[i] / tot : 0.0, ph[i]);
        static const char *pn[6] = {"thr setup+read", "thr traceback", "thr ids+zero", "thr records", "thr order", "thr col records"};
        unsigned long long pt = 0;
        for (int i = 8; i < 14; ++i) pt += ph[i];
        for (int i = 8; i < 14; ++i) std::fprintf(stderr, "[ccsx phase] %-14s %6.2f %%  (%llu cycles)\n", pn[i - 8], pt ? 100.0 * ph[i] / pt : 0.0, ph[i]);
    }
#endif
#ifdef CCSX_DEBUG_CHECKS
    if (S.staged) {
        int32_t dbg[2] = {0, 0};
        HIPTRY(hipMemcpy(dbg, S.P.debug, 8, hipMemcpyDeviceToHost));
        if (dbg[0]) { ccsx_set_error("device bounds check failed: code " + std::to_string(dbg[0]) + " at kernel line " + std::to_string(dbg[1])); return -3; }
    }
#endif
    (void)S;
    return 0;
}

int ccsx_download(ccsx_handle h, ccsx_results *res)
{
    if (!h || !h->slot[0].ran || h->slot[0].mode != CCSX_RUN_FUSED || !res) { ccsx_set_error("ccsx_download: nothing to download: ccsx_upload + ccsx_run first"); return -1; }
    Slot &S = h->slot[0];
    if (int rc = check_results(S, res, S.P.out_kin != nullptr)) return rc;
    HIPTRY(hipSetDevice(h->device));
    if (int rc = enqueue_download(S, res, h->s_comp)) return rc;
    HIPTRY(hipStreamSynchronize(h->s_comp));
    finish_outputs(S, res, nullptr);
    return 0;
}

int ccsx_consensus_batch(ccsx_handle h, const ccsx_batch *b, ccsx_results *res)
{
    int rc;
    if ((rc = ccsx_upload(h, b))) return rc;
    if ((rc = ccsx_run(h))) return rc;
    if ((rc = ccsx_sync(h))) return rc;
    return ccsx_download(h, res);
}

int ccsx_pileup_rule_version(void) { return 1; }

// The synchronous form of a fused run with its Wants, for the exported function `fn`: upload, every check and attachment that can still refuse the call, the
// run, the downloads.
static int consensus_sync(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const Wants &W, const char *fn)
{
    if (!h || !b || !res) return refuse(fn, "null argument");
    int rc;
    if ((rc = upload_impl(h, b, W))) return rc;
    Slot &S = h->slot[0];
    if ((rc = check_results(S, res, S.P.out_kin != nullptr)) || (rc = attach(h, S, W, h->s_comp))) return rc;
    HIPTRY(hipStreamSynchronize(h->s_comp));             // (attach may have enqueued on s_comp; ccsx_run enqueues on the draft stream, which does not wait for it)
    if ((rc = ccsx_run(h)) || (rc = ccsx_sync(h)) || (rc = ccsx_download(h, res))) return rc;
    if ((rc = enqueue_wants_download(S, W, h->s_comp))) return rc;
    HIPTRY(hipStreamSynchronize(h->s_comp));
    return 0;
}

// the synchronous entry points: as the ticketed ones, the Wants of the call, the argument this entry point may not be given as NULL, the driver
int ccsx_consensus_pileup(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, ccsx_pileup *pile)
{
    const ccsx_extras ex = {pile, nullptr, 0, 0};
    Wants W;
    if (build_wants(&ex, {}, nullptr, nullptr, nullptr, b, __func__, &W) || (!pile && refuse(__func__, "null argument"))) return -1;
    return consensus_sync(h, b, res, W, __func__);
}

int ccsx_tandem_rule_version(void) { return 1; }

int ccsx_consensus_extras(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const ccsx_extras *ex)
{
    Wants W;
    if (build_wants(ex, {}, nullptr, nullptr, nullptr, b, __func__, &W)) return -1;
    return consensus_sync(h, b, res, W, __func__);
}

int ccsx_consensus_hd_requests(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const ccsx_requests *rq, const ccsx_hd_request *hd)
{
    Wants W;
    if (hd_requests_wants(rq, hd, b, __func__, &W)) return -1;
    return consensus_sync(h, b, res, W, __func__);
}

int ccsx_consensus_hd(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const ccsx_extras *ex, const ccsx_hd_request *hd)
{
    const ccsx_requests rq = {ex, nullptr, nullptr, nullptr, nullptr, {nullptr, nullptr, nullptr}};
    Wants W;
    if (hd_requests_wants(&rq, hd, b, __func__, &W)) return -1;
    return consensus_sync(h, b, res, W, __func__);
}

void ccsx_fold_opts_default(ccsx_fold_opts *o)
{
    if (!o) return;
    o->max_occ = 8; o->min_hits = 12; o->min_arm = 200; o->min_span_tenths = 8; o->end_slack = 100;   // DESIGN.md §2 "Adapter palindromes": the study behind them
}

int ccsx_fold_rule_version(void) { return 1; }

int ccsx_consensus_fold(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const ccsx_extras *ex, const ccsx_fold_request *fold)
{
    Wants W;
    if (build_wants(ex, {}, fold, nullptr, nullptr, b, __func__, &W) || (!fold && refuse(__func__, "null request or report"))) return -1;
    return consensus_sync(h, b, res, W, __func__);
}

void ccsx_adapter_opts_default(ccsx_adapter_opts *o)
{
    if (!o) return;
    o->max_dist_pct = 20; o->min_copies = 2; o->max_insert = 100; o->end_slack = 200;   // DESIGN.md §2 "Adapter screen": the reasons for them
}

int ccsx_adapter_rule_version(void) { return 1; }

int ccsx_adapter_set_default(ccsx_adapter_set *s)
{
    if (!s) { ccsx_set_error("ccsx_adapter_set_default: null argument"); return -1; }
    static const char hairpin[] = "ATCTCTCTCTTTTCCTCCTCCTCCGTTGTTGTTGTTGAGAGAGAT";   // the 45-base SMRTbell adapter
    std::memset(s, 0, sizeof *s);
    s->n_adapters = 1; s->len[0] = (int32_t)(sizeof hairpin - 1);
    for (int i = 0; i < s->len[0]; ++i) s->seq[0][i] = (uint8_t)(hairpin[i] == 'A' ? 0 : hairpin[i] == 'C' ? 1 : hairpin[i] == 'G' ? 2 : 3);
    return 0;
}

int ccsx_consensus_screen(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const ccsx_extras *ex, const ccsx_fold_request *fold, const ccsx_adapter_request *adapters)
{
    Wants W;
    if (build_wants(ex, {}, fold, adapters, nullptr, b, __func__, &W)) return -1;
    return consensus_sync(h, b, res, W, __func__);
}

void ccsx_control_opts_default(ccsx_control_opts *o)
{
    if (!o) return;
    o->max_occ = 4; o->min_matched = 30; o->min_ctl_tenths = 5; o->min_draft_tenths = 8;   // DESIGN.md §2 "Control screen": the study behind them
}

int ccsx_control_rule_version(void) { return 1; }

int ccsx_consensus_control(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const ccsx_extras *ex, const ccsx_fold_request *fold, const ccsx_adapter_request *adapters,
                           const ccsx_control_request *control)
{
    Wants W;
    if (build_wants(ex, {}, fold, adapters, control, b, __func__, &W)) return -1;
    return consensus_sync(h, b, res, W, __func__);
}

void ccsx_coverage_opts_default(ccsx_coverage_opts *o)
{
    if (!o) return;
    o->drop_percent = 50; o->block = 30; o->min_spans = 0; o->max_lost_percent = 50;   // DESIGN.md §2 "Coverage rule": the build's own, the reasons for them
}

int ccsx_coverage_rule_version(void) { return 1; }

int ccsx_consensus_requests(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const ccsx_requests *rq)
{
    Wants W;
    if (requests_wants(rq, b, __func__, &W)) return -1;
    return consensus_sync(h, b, res, W, __func__);
}

int ccsx_consensus_handoff(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const ccsx_requests *rq, const ccsx_handoff_request *ho)
{
    Wants W;
    if (requests_wants(rq, b, __func__, &W, {ho}) || (!ho && refuse(__func__, "null handoff request"))) return -1;
    W.handoff_written_only = true;
    return consensus_sync(h, b, res, W, __func__);
}

int ccsx_consensus_barcodes(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const ccsx_requests *rq, const ccsx_barcode_request *bc)
{
    Wants W;
    if (reads_wants(rq, b, {nullptr, bc}, Barcodes::noun, __func__, &W)) return -1;
    return consensus_sync(h, b, res, W, __func__);
}

int ccsx_consensus_segments(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const ccsx_requests *rq, const ccsx_segment_request *sg)
{
    Wants W;
    if (reads_wants(rq, b, {nullptr, nullptr, sg}, Segments::noun, __func__, &W)) return -1;
    return consensus_sync(h, b, res, W, __func__);
}

int ccsx_consensus_cdna(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const ccsx_requests *rq, const ccsx_cdna_request *cd)
{
    Wants W;
    if (reads_wants(rq, b, {nullptr, nullptr, nullptr, nullptr, cd}, Cdna::noun, __func__, &W)) return -1;
    return consensus_sync(h, b, res, W, __func__);
}

int ccsx_consensus_represent(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const ccsx_requests *rq, const ccsx_represent_request *rp)
{
    Wants W;
    if (represent_wants(h, b, rq, rp, __func__, &W)) return -1;
    return consensus_sync(h, b, res, W, __func__);
}

int ccsx_barcode_reads(ccsx_handle h, const ccsx_barcode_set *set, const ccsx_barcode_opts *opts, const uint8_t *seq, const int64_t *seq_off, const int32_t *seq_len,
                       int32_t n, ccsx_barcode_report *report)
{
    return reads_sync<Barcodes>(h, set, opts, seq, seq_off, seq_len, n, report, __func__);
}

int ccsx_segment_reads(ccsx_handle h, const ccsx_segment_set *set, const ccsx_segment_opts *opts, const uint8_t *seq, const int64_t *seq_off, const int32_t *seq_len,
                       int32_t n, ccsx_segment_report *report)
{
    return reads_sync<Segments>(h, set, opts, seq, seq_off, seq_len, n, report, __func__);
}

int ccsx_cdna_reads(ccsx_handle h, const ccsx_cdna_set *set, const ccsx_cdna_opts *opts, const uint8_t *seq, const int64_t *seq_off, const int32_t *seq_len,
                    int32_t n, ccsx_cdna_report *report)
{
    return reads_sync<Cdna>(h, set, opts, seq, seq_off, seq_len, n, report, __func__);
}

// ---- duplicate reads (DESIGN.md §2 "Duplicate rule").  Both calls are synchronous on the polish stream, behind whatever tickets have enqueued there, in a buffer
// of the handle's own: no slot is staged, retired or recycled.  Every part of the buffer starts on a multiple of 256 bytes
static size_t dup_carve(size_t &at, size_t bytes) { const size_t p = at; at = (at + bytes + 255) & ~(size_t)255; return p; }

static int dup_sign_enqueue(ccsx_handle h, const ccsx_dup_opts &o, const uint8_t *seq, const int64_t *seq_off, const int32_t *seq_len, int32_t n, int64_t bytes,
                            ccsx_dup_sig *sig, hipStream_t st)
{
    size_t at = 0;
    const size_t o_sig = dup_carve(at, (size_t)n * sizeof(ccsx_dup_sig)), o_off = dup_carve(at, (size_t)n * 8), o_len = dup_carve(at, (size_t)n * 4),
                 o_seq = dup_carve(at, (size_t)bytes);
    if (h->d_dup.reserve(at)) return -2;
    uint8_t *base = (uint8_t *)h->d_dup.p;
    DupSignParams S{};
    S.n = n; S.opts = o; S.seq = base + o_seq; S.seq_off = (const int64_t *)(base + o_off); S.seq_len = (const int32_t *)(base + o_len);
    S.sig = (ccsx_dup_sig *)(base + o_sig);
    HIPTRY(hipMemcpyAsync(base + o_off, seq_off, (size_t)n * 8, hipMemcpyHostToDevice, st));
    HIPTRY(hipMemcpyAsync(base + o_len, seq_len, (size_t)n * 4, hipMemcpyHostToDevice, st));
    if (bytes) HIPTRY(hipMemcpyAsync(base + o_seq, seq, (size_t)bytes, hipMemcpyHostToDevice, st));
    (void)hipGetLastError();
    if (const char *failed = ccsx_dup_sign_launch(S, st)) { ccsx_set_error(std::string("kernel launch failed: ") + failed); return -2; }
    HIPTRY(hipMemcpyAsync(sig, S.sig, (size_t)n * sizeof(ccsx_dup_sig), hipMemcpyDeviceToHost, st));
    return 0;
}

// k_cell on the caller's reads: ccsx_cdna_reads' path (the handle's d_reads on the polish stream, no slot touched) with the design and the whitelist's table, whose
// device copy stays resident between calls.  Layout of d_reads as reads_enqueue's, the report being ccsx_cl_rep_bytes
static int cell_enqueue(ccsx_handle h, const ccsx_cdna_set *set, const ccsx_cdna_opts &o, const ccsx_cell_design &d, const ccsx_cell_whitelist *wl, const uint8_t *seq,
                        const int64_t *seq_off, const int32_t *seq_len, int32_t n, int64_t bytes, const ccsx_cell_report *report, hipStream_t st)
{
    const std::vector<unsigned long long> packed = reads_pack<Cdna>(set);
    const size_t N = (size_t)n, words = packed.size(), head = words * 8 + ccsx_cl_rep_bytes(N), head8 = (head + 7) & ~(size_t)7, len4 = (N * 4 + 7) & ~(size_t)7;
    if (h->d_reads.reserve(head8 + N * 8 + len4 + (size_t)bytes)) return -2;
    if (wl && wl->serial != h->cell_wl_serial) {
        h->cell_wl_serial = 0;                                      // (a failed upload leaves nobody's table resident)
        if (h->d_cell_wl.reserve((size_t)wl->slots * 8)) return -2;
        HIPTRY(hipMemcpyAsync(h->d_cell_wl.p, wl->table, (size_t)wl->slots * 8, hipMemcpyHostToDevice, st));
        h->cell_wl_serial = wl->serial;
    }
    uint8_t *base = (uint8_t *)h->d_reads.p;
    int64_t *d_off = (int64_t *)(base + head8);
    int32_t *d_len = (int32_t *)(base + head8 + N * 8);
    uint8_t *d_seq = base + head8 + N * 8 + len4;
    HIPTRY(hipMemcpyAsync(base, packed.data(), words * 8, hipMemcpyHostToDevice, st));
    HIPTRY(hipMemcpyAsync(d_off, seq_off, N * 8, hipMemcpyHostToDevice, st));
    HIPTRY(hipMemcpyAsync(d_len, seq_len, N * 4, hipMemcpyHostToDevice, st));
    if (bytes) HIPTRY(hipMemcpyAsync(d_seq, seq, (size_t)bytes, hipMemcpyHostToDevice, st));
    CellParams K{};
    K.D = Cdna::params(set->n_primers, n, o, base);
    K.D.seq = d_seq; K.D.seq_off = d_off; K.D.seq_len = d_len;
    K.design = d;
    K.table = wl ? (const unsigned long long *)h->d_cell_wl.p : nullptr; K.slots = wl ? wl->slots : 0u;
    (void)hipGetLastError();
    if (const char *failed = ccsx_cell_launch(K, st)) { ccsx_set_error(std::string("kernel launch failed: ") + failed); return -2; }
    if (int rc = reads_download<Cdna>(K.D, &report->cdna, st)) return rc;
    const CellOut c = ccsx_cl_out(K.D.rep, N);
    const ReadsCopy planes[] = {{report->tag, c.tag, 4}, {report->bc_raw, c.bc_raw, 4}, {report->bc, c.bc, 4}, {report->bc_hi, c.bc_hi, 4}, {report->kind, c.kind, 4},
                                {report->shift, c.shift, 4}, {report->umi, c.umi, 4}, {report->tag_clip, c.tag_clip, 4}};
    for (const ReadsCopy &p : planes) HIPTRY(hipMemcpyAsync(p.host, p.dev, N * p.bytes_per_read, hipMemcpyDeviceToHost, st));
    return 0;
}

int ccsx_cell_reads(ccsx_handle h, const ccsx_cdna_set *set, const ccsx_cdna_opts *opts, const ccsx_cell_design *design, const ccsx_cell_whitelist *wl,
                    const uint8_t *seq, const int64_t *seq_off, const int32_t *seq_len, int32_t n, ccsx_cell_report *report)
{
    ccsx_cdna_opts o;
    int64_t bytes;
    if (ccsx_cell_check(set, opts, design, wl, report, n, __func__, &o) || ccsx_check_reads(seq, seq_off, seq_len, n, __func__, &bytes)) return -1;
    if (!h) return refuse(__func__, "null argument");
    if (n == 0) return 0;
    HIPTRY(hipSetDevice(h->device));
    const int rc = cell_enqueue(h, set, o, *design, wl, seq, seq_off, seq_len, n, bytes, report, h->s_comp);
    if (rc) { (void)hipStreamSynchronize(h->s_comp); return rc; }   // (whatever was enqueued reads and writes the caller's arrays: it ends before the call does)
    HIPTRY(hipStreamSynchronize(h->s_comp));
    return 0;
}

int ccsx_dup_sign_reads(ccsx_handle h, const ccsx_dup_opts *opts, const uint8_t *seq, const int64_t *seq_off, const int32_t *seq_len, int32_t n, ccsx_dup_sig *sig)
{
    ccsx_dup_opts o;
    int64_t bytes;
    if (ccsx_dup_check_sign(opts, seq, seq_off, seq_len, n, sig, __func__, &o, &bytes)) return -1;
    if (!h) return refuse(__func__, "null argument");
    if (n == 0) return 0;
    HIPTRY(hipSetDevice(h->device));
    const int rc = dup_sign_enqueue(h, o, seq, seq_off, seq_len, n, bytes, sig, h->s_comp);
    if (rc) { (void)hipStreamSynchronize(h->s_comp); return rc; }   // (whatever was enqueued reads and writes the caller's arrays: it ends before the call does)
    HIPTRY(hipStreamSynchronize(h->s_comp));
    return 0;
}

static int dup_cluster_enqueue(ccsx_handle h, const ccsx_dup_opts &o, const ccsx_dup_sig *sig, const int32_t *group, const int32_t *score, int32_t n,
                               const ccsx_dup_report *report, hipStream_t st)
{
    const size_t N = (size_t)n, tmp = ccsx_dup_sort_bytes(n);
    size_t at = 0;
    const size_t o_sig = dup_carve(at, N * sizeof(ccsx_dup_sig)), o_k0 = dup_carve(at, N * 8), o_k1 = dup_carve(at, N * 8), o_i0 = dup_carve(at, N * 4),
                 o_i1 = dup_carve(at, N * 4), o_grp = dup_carve(at, N * 4), o_sc = dup_carve(at, N * 4), o_list = dup_carve(at, (1 + N / 2) * 4),
                 o_rep = dup_carve(at, N * CCSX_DUP_PLANES * 4), o_tmp = dup_carve(at, tmp);
    if (h->d_dup.reserve(at)) return -2;
    uint8_t *base = (uint8_t *)h->d_dup.p;
    DupClusterParams P{};
    P.n = n; P.opts = o; P.sig = (const ccsx_dup_sig *)(base + o_sig);
    P.group = group ? (const int32_t *)(base + o_grp) : nullptr; P.score = score ? (const int32_t *)(base + o_sc) : nullptr;
    P.key[0] = (unsigned long long *)(base + o_k0); P.key[1] = (unsigned long long *)(base + o_k1);
    P.idx[0] = (uint32_t *)(base + o_i0); P.idx[1] = (uint32_t *)(base + o_i1);
    P.sort_tmp = base + o_tmp; P.sort_tmp_bytes = tmp;
    P.list = (int32_t *)(base + o_list); P.rep = (int32_t *)(base + o_rep);
    HIPTRY(hipMemcpyAsync(base + o_sig, sig, N * sizeof(ccsx_dup_sig), hipMemcpyHostToDevice, st));
    if (group) HIPTRY(hipMemcpyAsync(base + o_grp, group, N * 4, hipMemcpyHostToDevice, st));
    if (score) HIPTRY(hipMemcpyAsync(base + o_sc, score, N * 4, hipMemcpyHostToDevice, st));
    (void)hipGetLastError();
    if (const char *failed = ccsx_dup_cluster_launch(P, st)) { ccsx_set_error(std::string("kernel launch failed: ") + failed); return -2; }
    const DupOut d = ccsx_dup_out(P.rep, N), r = ccsx_dup_out(*report);
    HIPTRY(hipMemcpyAsync(r.status, d.status, N * 4, hipMemcpyDeviceToHost, st));
    HIPTRY(hipMemcpyAsync(r.rep, d.rep, N * 4, hipMemcpyDeviceToHost, st));
    HIPTRY(hipMemcpyAsync(r.set_size, d.set_size, N * 4, hipMemcpyDeviceToHost, st));
    HIPTRY(hipMemcpyAsync(r.dup, d.dup, N * 4, hipMemcpyDeviceToHost, st));
    return 0;
}

int ccsx_dup_cluster(ccsx_handle h, const ccsx_dup_opts *opts, const ccsx_dup_sig *sig, const int32_t *group, const int32_t *score, int32_t n,
                     ccsx_dup_report *report)
{
    ccsx_dup_opts o;
    if (ccsx_dup_check_cluster(opts, sig, group, n, report, __func__, &o)) return -1;
    if (!h) return refuse(__func__, "null argument");
    if (n == 0) return 0;
    HIPTRY(hipSetDevice(h->device));
    const int rc = dup_cluster_enqueue(h, o, sig, group, score, n, report, h->s_comp);
    if (rc) { (void)hipStreamSynchronize(h->s_comp); return rc; }
    HIPTRY(hipStreamSynchronize(h->s_comp));
    return 0;
}

int ccsx_get_timings(ccsx_handle h, ccsx_timings *t)
{
    if (!h || !t) { ccsx_set_error("ccsx_get_timings: no completed run"); return -1; }
    Slot &S = h->slot[h->last];
    if (!S.ran) { ccsx_set_error("ccsx_get_timings: no completed run"); return -1; }
    HIPTRY(hipSetDevice(h->device));
    if (int rc = slot_timings(h, S, t)) return rc;
    std::vector<int32_t> nwin(S.P.n_zmw);
    HIPTRY(hipMemcpy(nwin.data(), S.P.out_nwin, nwin.size() * 4, hipMemcpyDeviceToHost));
    int64_t tw = 0;
    for (int v : nwin) tw += v;
    t->polish_workgroups = tw;
    return 0;
}

// ---- stage access (parity tests): slot 0 as the last synchronous run left it (ccsx_run, ccsx_hd_batch) ----
static int stage_guard(ccsx_handle h, int32_t i, bool read_index, const char *fn)
{
    if (!h || !h->slot[0].ran || i < 0 || i >= (read_index ? h->slot[0].P.n_reads : h->slot[0].P.n_zmw)) { ccsx_set_error(std::string(fn) + ": bad state/index"); return -1; }
    HIPTRY(hipSetDevice(h->device));
    HIPTRY(hipStreamSynchronize(h->s_comp));
    return 0;
}

// ZMW z's window bounds into wb; returns their count for a draft of L bases (from the bounds: nwin may have been zeroed by a later status), or < 0
static int stage_bounds(const Slot &S, int z, int32_t L, std::vector<int32_t> &wb)
{
    wb.resize(S.wb_off[z + 1] - S.wb_off[z]);
    HIPTRY(hipMemcpy(wb.data(), S.P.wbounds + S.wb_off[z], wb.size() * 4, hipMemcpyDeviceToHost));
    int nw = 0;
    if (L > 0) while (nw + 1 < (int)wb.size() && wb[nw] < L) ++nw;
    return nw;
}

int ccsx_stage_draft(ccsx_handle h, int32_t z, uint8_t *draft, int32_t cap, int32_t *len)
{
    if (int rc = stage_guard(h, z, false, "ccsx_stage_draft")) return rc;
    const Slot &S = h->slot[0];
    int32_t L = 0;
    HIPTRY(hipMemcpy(&L, S.P.draft_len + z, 4, hipMemcpyDeviceToHost));
    if (L > cap) { ccsx_set_error("ccsx_stage_draft: buffer too small"); return -1; }
    if (L > 0) HIPTRY(hipMemcpy(draft, S.P.draft + S.seq_off[z], (size_t)L, hipMemcpyDeviceToHost));
    *len = L;
    return 0;
}

int ccsx_stage_windows(ccsx_handle h, int32_t z, int32_t *bounds, int32_t cap, int32_t *n_windows)
{
    if (int rc = stage_guard(h, z, false, "ccsx_stage_windows")) return rc;
    const Slot &S = h->slot[0];
    int32_t L = 0; std::vector<int32_t> wb;
    HIPTRY(hipMemcpy(&L, S.P.draft_len + z, 4, hipMemcpyDeviceToHost));
    const int nw = stage_bounds(S, z, L, wb);
    if (nw < 0) return nw;
    if (nw + 1 > cap) { ccsx_set_error("ccsx_stage_windows: buffer too small"); return -1; }
    for (int k = 0; k <= nw; ++k) bounds[k] = wb[k];
    *n_windows = nw;
    return 0;
}

// rstart[] holds the entry row for every window-edge column and -1 elsewhere (the kernel never
// materialises the other columns).
int ccsx_stage_align(ccsx_handle h, int32_t r, int32_t *rstart, int32_t cap, int32_t *valid, int32_t *score)
{
    if (int rc = stage_guard(h, r, true, "ccsx_stage_align")) return rc;
    const Slot &S = h->slot[0];
    const int z = (int)(std::upper_bound(S.read_off.p, S.read_off.p + S.P.n_zmw + 1, r) - S.read_off.p) - 1;
    uint8_t v = 0; int32_t sc = 0, L = 0;
    HIPTRY(hipMemcpy(&v, S.P.avalid + r, 1, hipMemcpyDeviceToHost));
    HIPTRY(hipMemcpy(&sc, S.P.ascore + r, 4, hipMemcpyDeviceToHost));
    HIPTRY(hipMemcpy(&L, S.P.draft_len + z, 4, hipMemcpyDeviceToHost));
    *valid = v; *score = sc;
    if (L + 1 > cap) { ccsx_set_error("ccsx_stage_align: buffer too small"); return -1; }
    for (int j = 0; j <= L; ++j) rstart[j] = -1;
    if (v) {
        std::vector<int32_t> wb;
        const int nw = stage_bounds(S, z, L, wb);
        if (nw < 0) return nw;
        std::vector<int32_t> ent(2 * nw);
        HIPTRY(hipMemcpy(ent.data(), S.P.ent + S.ent_off[r], ent.size() * 4, hipMemcpyDeviceToHost));
        for (int k = 0; k < 2 * nw; ++k) {
            int col = (k == 0) ? 0 : (k == 2 * nw - 1) ? L : wb[(k + 1) >> 1] + ((k & 1) ? -CCSX_WIN_OVERHANG : CCSX_WIN_OVERHANG);
            rstart[col] = ent[k];
        }
    }
    return 0;
}

// ccsx_stage_align and the dirty masks of the same pass, unpacked per draft position: interval k covers the positions col(k - 1) .. col(k) - 1, bit p - col(k - 1)
// (what k_polish's load_meta shifts together for a window)
int ccsx_stage_align_ev(ccsx_handle h, int32_t r, int32_t *rstart, int32_t cap, int32_t *valid, int32_t *score, uint8_t *dirty, int32_t dirty_cap)
{
    if (!rstart || !valid || !score || !dirty) { ccsx_set_error("ccsx_stage_align_ev: null argument"); return -1; }
    if (int rc = ccsx_stage_align(h, r, rstart, cap, valid, score)) return rc;
    const Slot &S = h->slot[0];
    const int z = (int)(std::upper_bound(S.read_off.p, S.read_off.p + S.P.n_zmw + 1, r) - S.read_off.p) - 1;
    int32_t L = 0;
    HIPTRY(hipMemcpy(&L, S.P.draft_len + z, 4, hipMemcpyDeviceToHost));
    if (L > dirty_cap) { ccsx_set_error("ccsx_stage_align_ev: buffer too small"); return -1; }
    for (int p = 0; p < L; ++p) dirty[p] = 0;
    if (*valid) {
        std::vector<int32_t> wb;
        const int nw = stage_bounds(S, z, L, wb);
        if (nw < 0) return nw;
        std::vector<uint32_t> dm(2 * nw);
        HIPTRY(hipMemcpy(dm.data(), S.P.dmask + S.ent_off[r], dm.size() * 4, hipMemcpyDeviceToHost));
        auto col = [&](int k) { return (k == 0) ? 0 : (k == 2 * nw - 1) ? L : wb[(k + 1) >> 1] + ((k & 1) ? -CCSX_WIN_OVERHANG : CCSX_WIN_OVERHANG); };
        for (int k = 1; k < 2 * nw; ++k)
            for (int p = col(k - 1); p < col(k); ++p) dirty[p] = (p - col(k - 1) < 32) ? (uint8_t)((dm[k] >> (p - col(k - 1))) & 1u) : 0;
    }
    return 0;
}

// the POA log of the batch the handle ran last (include/ccsx.h "The POA log")
int ccsx_poa_log(ccsx_handle h, int32_t on)
{
    if (!h) { ccsx_set_error("ccsx_poa_log: null handle"); return -1; }
    h->poa_log = on != 0;
    return 0;
}

int ccsx_stage_poa(ccsx_handle h, int32_t z, int32_t generator, int32_t *rec, int32_t cap_records, int32_t *n_records)
{
    if (!h || !rec || !n_records) { ccsx_set_error("ccsx_stage_poa: null argument"); return -1; }
    const Slot &S = h->slot[h->last];
    if (!S.ran || S.inflight || !S.P.poa_log) { ccsx_set_error("ccsx_stage_poa: the last batch was not run with the POA log (ccsx_poa_log first), or is still in flight"); return -1; }
    if (z < 0 || z >= S.P.n_zmw || generator < 0 || generator > 1) { ccsx_set_error("ccsx_stage_poa: bad index"); return -1; }
    const int32_t n = S.P.poa_log_stride;
    if (n > cap_records) { *n_records = n; ccsx_set_error("ccsx_stage_poa: buffer too small (n_records holds the records needed)"); return -1; }
    HIPTRY(hipSetDevice(h->device));
    HIPTRY(hipStreamSynchronize(h->s_draft));
    HIPTRY(hipStreamSynchronize(h->s_comp));
    HIPTRY(hipMemcpy(rec, S.P.poa_log + ((size_t)(2 * z + generator) * n) * CCSX_POA_LOG_WORDS, (size_t)n * CCSX_POA_LOG_WORDS * 4, hipMemcpyDeviceToHost));
    *n_records = n;
    return 0;
}

// the converged window templates k_polish kept (a run staged with kinetics or the pileup summary): per window the template, J and [cs, ce)
int ccsx_stage_polished(ccsx_handle h, int32_t z, uint8_t *tpl, int32_t *meta, int32_t cap, int32_t *n_windows, int32_t *passes_used, int32_t *backbone)
{
    if (int rc = stage_guard(h, z, false, "ccsx_stage_polished")) return rc;
    const Slot &S = h->slot[0];
    if (!S.P.wtpl || S.mode != CCSX_RUN_FUSED) { ccsx_set_error("ccsx_stage_polished: the last synchronous run kept no window templates (ccsx_consensus_pileup first)"); return -1; }
    if (!tpl || !meta || !n_windows || !passes_used || !backbone) { ccsx_set_error("ccsx_stage_polished: null argument"); return -1; }
    int32_t st = 0, nw = 0, nr = 0, zr = 0;
    HIPTRY(hipMemcpy(&st, S.P.zstat + z, 4, hipMemcpyDeviceToHost));
    HIPTRY(hipMemcpy(&nw, S.P.nwin + z, 4, hipMemcpyDeviceToHost));
    HIPTRY(hipMemcpy(&nr, S.P.nreads_used + z, 4, hipMemcpyDeviceToHost));
    HIPTRY(hipMemcpy(&zr, S.P.zref + z, 4, hipMemcpyDeviceToHost));
    if (st != CCSX_SUCCESS) nw = 0;                      // (k_stitch stitches no window of such a ZMW)
    if (nw > cap) { ccsx_set_error("ccsx_stage_polished: buffer too small"); return -1; }
    if (nw > 0) {
        const size_t w0 = (size_t)(S.wb_off[z] - z);
        std::vector<short2> tm(nw); std::vector<int4> wm(nw);
        HIPTRY(hipMemcpy(tpl, S.P.wtpl + w0 * 32, (size_t)nw * 32, hipMemcpyDeviceToHost));
        HIPTRY(hipMemcpy(tm.data(), S.P.wtmeta + w0, (size_t)nw * sizeof(short2), hipMemcpyDeviceToHost));
        HIPTRY(hipMemcpy(wm.data(), S.P.wmeta + w0, (size_t)nw * sizeof(int4), hipMemcpyDeviceToHost));
        for (int w = 0; w < nw; ++w) { meta[3 * w] = tm[w].x; meta[3 * w + 1] = tm[w].y; meta[3 * w + 2] = tm[w].y + wm[w].x; }
    }
    *n_windows = nw; *passes_used = nr; *backbone = zr & 255;
    return 0;
}

// what k_polish left per window of ZMW z (P.wmeta, a plain copy): core length, usable reads of the last round (all passes / full-length passes only), non-convergence, rounds
int ccsx_stage_wmeta(ccsx_handle h, int32_t z, int32_t *meta, int32_t cap, int32_t *n_windows)
{
    if (int rc = stage_guard(h, z, false, "ccsx_stage_wmeta")) return rc;
    if (!meta || !n_windows) { ccsx_set_error("ccsx_stage_wmeta: null argument"); return -1; }
    const Slot &S = h->slot[0];
    int32_t st = 0, nw = 0;
    HIPTRY(hipMemcpy(&st, S.P.zstat + z, 4, hipMemcpyDeviceToHost));
    HIPTRY(hipMemcpy(&nw, S.P.nwin + z, 4, hipMemcpyDeviceToHost));
    if (st != CCSX_SUCCESS) nw = 0;                      // (a ZMW that failed before the polish has no polished window)
    if (nw > cap) { ccsx_set_error("ccsx_stage_wmeta: buffer too small"); return -1; }
    if (nw > 0) {
        std::vector<int4> wm(nw);
        HIPTRY(hipMemcpy(wm.data(), S.P.wmeta + (size_t)(S.wb_off[z] - z), (size_t)nw * sizeof(int4), hipMemcpyDeviceToHost));
        for (int w = 0; w < nw; ++w) {
            meta[5 * w] = wm[w].x; meta[5 * w + 1] = wm[w].y & 255; meta[5 * w + 2] = wm[w].y >> 8; meta[5 * w + 3] = wm[w].z; meta[5 * w + 4] = wm[w].w;
        }
    }
    *n_windows = nw;
    return 0;
}

// ---- the heteroduplex finder: the third seam (include/ccsx.h).  Synchronous, on slot 0 like ccsx_upload / ccsx_run, so that the stage accessors report what it used.
void ccsx_hd_opts_default(ccsx_hd_opts *o)
{
    if (!o) return;
    o->min_strand_passes = 3; o->min_sites = 1; o->min_indel = 21; o->min_alt_frac = 0.5f; o->max_pvalue = 1e-3;   // DESIGN.md §2 "Heteroduplex rule": the study behind them
}

int ccsx_hd_rule_version(void) { return 1; }

int ccsx_hd_batch(ccsx_handle h, const ccsx_batch *b, const ccsx_drafts *drafts, const ccsx_hd_opts *o, ccsx_hd_report *out)
{
    if (!h || !b || !drafts || !out) { ccsx_set_error("ccsx_hd_batch: null argument"); return -1; }
    ccsx_hd_opts hd;
    if (hd_opts_check(o, &hd, "ccsx_hd_batch") || hd_report_check(out, b->n_zmw, "ccsx_hd_batch")) return -1;
    if (h->poisoned) { ccsx_set_error("ccsx_hd_batch: an earlier submit failed after work had been enqueued; destroy the handle"); return -2; }
    int rc = ccsx_upload(h, b);
    if (rc) return rc;
    Slot &S = h->slot[0];
    S.mode = CCSX_RUN_HD;                                    // (slot 0 is the finder's now: ccsx_run / ccsx_download refuse it until the next ccsx_upload)
    if ((rc = check_drafts(S, drafts, true))) return rc;
    if ((rc = hd_table(h)) || (rc = hd_attach(h, S, hd, 0, h->s_comp))) return rc;
    if ((rc = upload_drafts(S, drafts, h->s_comp))) return rc;
    HIPTRY(hipStreamSynchronize(h->s_comp));
    if ((rc = launch(h, S)) || (rc = ccsx_sync(h))) return rc;
    if ((rc = enqueue_hd_download(S, out, h->s_comp))) return rc;   // (status: k_hd_verdict's copy of it, written for every ZMW in this mode too)
    HIPTRY(hipStreamSynchronize(h->s_comp));
    return 0;
}

// ---- the model training's counts: the fourth seam (include/ccsx.h; DESIGN.md §2 "Model training").  Synchronous, on slot 0 like ccsx_hd_batch, and by the same path.
int ccsx_train_batch(ccsx_handle h, const ccsx_batch *b, const ccsx_drafts *drafts, ccsx_train_counts *out)
{
    const char *fn = "ccsx_train_batch";
    if (!h || !b || !drafts || !out) return refuse(fn, "null argument");
    if (out->reserved != 0) return refuse(fn, "reserved must be 0");
    if (out->n_zmw != b->n_zmw || !out->match || !out->stay || !out->del || !out->loglik || !out->n_pairs || !out->n_gated || !out->n_bases || !out->status)
        return refuse(fn, "counts arrays missing, or sized for another batch");
    if (h->poisoned) { ccsx_set_error("ccsx_train_batch: an earlier submit failed after work had been enqueued; destroy the handle"); return -2; }
    int rc = ccsx_upload(h, b);
    if (rc) return rc;
    Slot &S = h->slot[0];
    S.mode = CCSX_RUN_TRAIN;                                 // (slot 0 is the training's now: ccsx_run / ccsx_download refuse it until the next ccsx_upload)
    if ((rc = check_drafts(S, drafts, true))) return rc;
    const size_t n = (size_t)S.P.n_zmw;
    if (S.d_train.reserve((n + 1) * ((CCSX_NCTX * CCSX_NOBS * 2 + CCSX_NCTX + 1) * 8 + 3 * 4))) return -2;   // (k_train's launch zeroes it on the stream)
    S.P.train_tab = (int64_t *)S.d_train.p;
    S.P.train_ll = S.P.train_tab + n * (CCSX_NCTX * CCSX_NOBS * 2 + CCSX_NCTX);
    S.P.train_zi = (int32_t *)(S.P.train_ll + n);
    if ((rc = upload_drafts(S, drafts, h->s_comp))) return rc;
    HIPTRY(hipStreamSynchronize(h->s_comp));
    if ((rc = launch(h, S)) || (rc = ccsx_sync(h))) return rc;
    // the ZMW's table is [match 192 | stay 192 | del 16]: three strided copies, then the planes
    const size_t row = (CCSX_NCTX * CCSX_NOBS * 2 + CCSX_NCTX) * 8;
    if (n) {
        HIPTRY(hipMemcpy2DAsync(out->match, 192 * 8, S.P.train_tab, row, 192 * 8, n, hipMemcpyDeviceToHost, h->s_comp));
        HIPTRY(hipMemcpy2DAsync(out->stay, 192 * 8, S.P.train_tab + 192, row, 192 * 8, n, hipMemcpyDeviceToHost, h->s_comp));
        HIPTRY(hipMemcpy2DAsync(out->del, 16 * 8, S.P.train_tab + 384, row, 16 * 8, n, hipMemcpyDeviceToHost, h->s_comp));
        HIPTRY(hipMemcpyAsync(out->loglik, S.P.train_ll, n * 8, hipMemcpyDeviceToHost, h->s_comp));
        HIPTRY(hipMemcpyAsync(out->n_pairs, S.P.train_zi, n * 4, hipMemcpyDeviceToHost, h->s_comp));
        HIPTRY(hipMemcpyAsync(out->n_gated, S.P.train_zi + n, n * 4, hipMemcpyDeviceToHost, h->s_comp));
        HIPTRY(hipMemcpyAsync(out->n_bases, S.P.train_zi + 2 * n, n * 4, hipMemcpyDeviceToHost, h->s_comp));
        HIPTRY(hipMemcpyAsync(out->status, S.P.zstat, n * 4, hipMemcpyDeviceToHost, h->s_comp));   // the status after the cascade
    }
    HIPTRY(hipStreamSynchronize(h->s_comp));
    return 0;
}

// ---- pass orientation: the seam (include/ccsx.h; DESIGN.md §2 "Pass orientation").  Synchronous, on slot 0 like ccsx_hd_batch: upload, k_orient, the report.
void ccsx_orient_opts_default(ccsx_orient_opts *o)
{
    if (!o) return;
    o->min_votes = 16; o->ratio = 3;   // DESIGN.md §2 "Pass orientation": the study behind them
}

int ccsx_orient_rule_version(void) { return 1; }

static int orient_report_check(const ccsx_orient_report *out, int32_t n_reads, const char *fn)
{
    if (!out) { ccsx_set_error(std::string(fn) + ": null report"); return -1; }
    if (out->n_reads != n_reads || !out->strand || !out->call || !out->votes_same || !out->votes_opp) {
        ccsx_set_error(std::string(fn) + ": report arrays missing, or sized for another batch"); return -1;
    }
    return 0;
}

int ccsx_set_orient_opts(ccsx_handle h, const ccsx_orient_opts *opts)
{
    if (!h) { ccsx_set_error("ccsx_set_orient_opts: null handle"); return -1; }
    if (opts && orient_opts_check(opts, "ccsx_set_orient_opts")) return -1;
    if (opts) h->orient_opts = *opts; else ccsx_orient_opts_default(&h->orient_opts);
    return 0;
}

// the report of slot 0's staged batch on s_comp: what k_orient wrote, or — it did not run — every pass GIVEN with its own bit 0 (the slot's copy of the flags)
static int orient_download(ccsx_handle h, Slot &S, ccsx_orient_report *out)
{
    const size_t R = (size_t)S.P.n_reads;
    if (S.orient_ran) {
        HIPTRY(hipMemcpyAsync(out->strand, S.P.orient_rep8, R, hipMemcpyDeviceToHost, h->s_comp));
        HIPTRY(hipMemcpyAsync(out->call, S.P.orient_rep8 + R, R, hipMemcpyDeviceToHost, h->s_comp));
        HIPTRY(hipMemcpyAsync(out->votes_same, S.P.orient_votes, R * 4, hipMemcpyDeviceToHost, h->s_comp));
        HIPTRY(hipMemcpyAsync(out->votes_opp, S.P.orient_votes + R, R * 4, hipMemcpyDeviceToHost, h->s_comp));
        HIPTRY(hipStreamSynchronize(h->s_comp));
        return 0;
    }
    HIPTRY(hipMemcpyAsync(out->strand, S.P.flags, R, hipMemcpyDeviceToHost, h->s_comp));
    HIPTRY(hipStreamSynchronize(h->s_comp));
    for (size_t r = 0; r < R; ++r) { out->strand[r] &= 1; out->call[r] = CCSX_ORIENT_GIVEN; out->votes_same[r] = 0; out->votes_opp[r] = 0; }
    return 0;
}

int ccsx_orient_batch(ccsx_handle h, const ccsx_batch *b, const ccsx_orient_opts *opts, ccsx_orient_report *out)
{
    const char *fn = "ccsx_orient_batch";
    if (!out) return refuse(fn, "null report");
    if (!b) return refuse(fn, "null argument");
    ccsx_orient_opts o;
    if (opts) o = *opts; else ccsx_orient_opts_default(&o);
    if (orient_report_check(out, b->n_reads, fn) || orient_opts_check(&o, fn)) return -1;
    if (!h) return refuse(fn, "null argument");
    if (h->poisoned) { ccsx_set_error("ccsx_orient_batch: an earlier submit failed after work had been enqueued; destroy the handle"); return -2; }
    Wants W;
    W.orient = &o;
    int rc = upload_impl(h, b, W);
    if (rc) return rc;
    Slot &S = h->slot[0];
    S.mode = CCSX_RUN_ORIENT;                                // (slot 0 is the seam's now: ccsx_run / ccsx_download refuse it until the next ccsx_upload)
    if (S.orient_pending) {
        if ((rc = launch(h, S)) || (rc = ccsx_sync(h))) return rc;
        S.ran = false;                                       // (no stage but k_orient ran: the stage accessors other than ccsx_stage_orient have nothing to report)
    }
    return orient_download(h, S, out);
}

int ccsx_stage_orient(ccsx_handle h, ccsx_orient_report *out)
{
    const char *fn = "ccsx_stage_orient";
    if (!out) return refuse(fn, "null report");
    if (!h || !h->slot[0].staged) return refuse(fn, "no batch uploaded: a synchronous call first");
    Slot &S = h->slot[0];
    if (orient_report_check(out, S.P.n_reads, fn)) return -1;
    HIPTRY(hipSetDevice(h->device));
    HIPTRY(hipStreamSynchronize(h->s_draft));
    HIPTRY(hipStreamSynchronize(h->s_comp));
    return orient_download(h, S, out);
}

}  // extern "C"

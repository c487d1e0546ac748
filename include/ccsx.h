/*
 * ccsx.h — C ABI of the MI355X-native CCS per-ZMW consensus hot path.
 *
 * Drop-in boundary.  The reference (PacificBiosciences/ccs, docs-only mount)
 * publishes no plugin API; the only documented seam is the block diagram docs/img/ccs-impl.png:
 * "Draft Stage {GPU | CPU pool}" -> queue(ZMWs, Drafts, Windows) -> "Polish Stage {GPU | CPU pool}".
 * The entry points below are the GPU consumers of those two queues plus the fused path:
 *
 *   ccsx_consensus_*  : steps 2,3,4,8,9,10 of docs/how-does-ccs-work.md:34-112 for a batch of ZMWs
 *   ccsx_stage_*      : per-stage access (draft / align / polish) used by the parity tests
 *
 * Conventions
 *   - plain C, plain pointers and sizes; no C++/torch types cross this boundary.
 *   - every function returns 0 on success, <0 on a fatal error (HIP error, OOM, bad argument);
 *     text via ccsx_last_error().  Algorithmic failures are reported PER ZMW in status[]
 *     (one status per ZMW, the run continues: docs/faq/reports-aux-files.md:10-12,143-159).
 *   - the caller owns every input and output buffer; the library owns device memory and streams.
 *   - a handle is bound to one GPU and is not thread-safe: one handle per host worker per GPU
 *     (mirrors the reference's "-j" worker pool, docs/faq/parallelize.md:17).
 *   - there is NO CPU fallback: if no gfx950 device is usable, ccsx_create fails loudly.
 */
#ifndef CCSX_H
#define CCSX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CCSX_ABI_VERSION 6   /* v6: ccsx_opts.max_qv (was reserved), ccsx_runtime_switches() */
#define CCSX_SPEC_VERSION 8   /* DESIGN.md §2; bumped whenever a result-changing rule changes (oracle: ORC_SPEC_VERSION) */

/* ---- fixed constants of the algorithm specification ---- */
#define CCSX_BAND          64   /* DP band rows of the wide alignment (retry of the cascade, split alignment: one wave64) */
#define CCSX_POA_BAND      32   /* DP band rows of the POA (four graphs per wave64, two rows per lane)                    */
#define CCSX_MAX_PASSES    255  /* passes of a ZMW the engine uses (SPEC v5; k_polish works through them in groups of 32)               */
#define CCSX_MAXPRED       7    /* POA in-edge cap per vertex (a move is a nibble: slot * 2 + [deletion], 15 = insertion) */
#define CCSX_WIN_CORE      22   /* target window core size, docs/how-does-ccs-work.md:57-59      */
#define CCSX_WIN_OVERHANG  2    /* +-2 bp overlap, same citation                                 */
#define CCSX_JMAX          31   /* max template columns in a polish window                       */
#define CCSX_IMAX          63   /* max read bases of one subread inside a polish window          */
#define CCSX_MAX_ITER      8    /* polish iterations per window                                  */
#define CCSX_NCTX          16   /* dinucleotide contexts (prev base, cur base)                   */
#define CCSX_NOBS          12   /* emission outcomes: base(4) x pulse-width bin(3)               */

/* ---- per-ZMW status, mirrors docs/faq/reports-aux-files.md:143-159 (subset that this path can raise) ---- */
enum ccsx_status {
    CCSX_SUCCESS               = 0,
    CCSX_TOO_FEW_PASSES        = 1,  /* fewer usable subreads than opts.min_passes                    */
    CCSX_DRAFT_FAILURE         = 2,  /* POA produced no draft / vertex capacity exceeded              */
    CCSX_TOO_MANY_UNUSABLE     = 3,  /* <= 50 % of subreads map to the draft (accuracy-vs-passes.md:37-39).  The `ccs` driver counts it under "Reads failed
                                        polishing" (metrics TOO_MANY_UNUSABLE), and with --coverage-filters under "Insufficient draft cov" (INSUFFICIENT_SPANS) */
    CCSX_NON_CONVERGENT        = 4,  /* some window hit CCSX_MAX_ITER with favourable mutations left   */
    CCSX_TOO_SHORT             = 5,
    CCSX_TOO_LONG              = 6,
    CCSX_LOW_RQ                = 7,  /* predicted accuracy below opts.min_rq                          */
    CCSX_EMPTY_WINDOW          = 8,  /* EMPTY_WINDOW_DURING_POLISHING                                 */
    CCSX_CAPACITY              = 9,  /* the polished consensus outgrew its buffer (1.25 x longest subread + 64): reported, never truncated */
    CCSX_HETERODUPLEX          = 10, /* ccsx_hd_request.split: the finder's verdict was HETERODUPLEX, the ZMW was not polished (see there)    */
    /* the coverage screen's gate (ccsx_coverage_request.gate; without that request no ZMW ever gets one of these four) */
    CCSX_DRAFT_TOO_DIFFERENT   = 11, /* fewer than opts.min_passes full-length passes align to the draft; not polished                          */
    CCSX_INSUFFICIENT_SPANS    = 12, /* fewer than min_spans full-length passes reach every window of the draft; not polished                   */
    CCSX_COVERAGE_DROPS        = 13, /* some window is reached cleanly by too few of the passes; not polished                                   */
    CCSX_READS_FAILED_POLISHING = 14 /* the polish dropped too many of the (pass, window) segments the alignment gave it; no consensus          */
};

/* ---- Arrow model parameter blob (interface of docs/faq/chemistry.md:27-56 the "arrow" json files) ----
 * ctx = 4*prev_base + cur_base, bases A,C,G,T = 0..3, obs = base*3 + min(pw,3)-1.
 * transition weights are cubic polynomials in the SNR of the current base's channel:
 *   w = c0 + c1 s + c2 s^2 + c3 s^3, s = clamp(snr[cur], snr_lo, snr_hi), w = max(w, 1e-6)
 *   P(move) = w_move / (1 + w_branch + w_stick + w_del), P(match) = 1 / (1 + ...).            */
typedef struct ccsx_model {
    char  name[32];
    float snr_lo, snr_hi;
    float trans_poly[CCSX_NCTX][3][4];      /* [ctx][branch,stick,deletion][c0..c3]              */
    float em_match [CCSX_NCTX][CCSX_NOBS];  /* P(obs | match, ctx)  (sums to 1 over obs)         */
    float em_branch[CCSX_NCTX][3];          /* P(pw bin | branch, ctx) (base is the cognate)     */
    float em_stick [CCSX_NCTX][3];          /* P(pw bin | stick, ctx)  (base uniform over 3)     */
} ccsx_model;

/* ---- run options (CLI names from SURVEY.md App. C) ---- */
typedef struct ccsx_opts {
    int32_t max_poa_cov;     /* --maxPoaCoverage (docs/changelog.md:114): subreads threaded into the POA */
    int32_t min_passes;      /* --min-passes                                                    */
    int32_t top_passes;      /* at most this many of a ZMW's passes are used, the FIRST ones in batch order (0 or > CCSX_MAX_PASSES = all, up to CCSX_MAX_PASSES).  The reference's
                                --top-passes ("closest to the median length", docs/faq/accuracy-vs-passes.md:49-52) is a selection the
                                caller makes when it builds the batch: the `ccs` driver does (ccs_main.cpp finish_zmw)             */
    int32_t min_length;      /* --min-length                                                    */
    int32_t max_length;      /* --max-length                                                    */
    float   min_rq;          /* --min-rq                                                        */
    int32_t poa_slots;       /* concurrent POA graphs resident on the device (0 = auto)          */
    int32_t hifi_kinetics;   /* --hifi-kinetics (docs/faq/kinetics.md:8-18): per-strand averaged IPD / PW; needs batch.ipd */
    int32_t disable_heuristics; /* --disable-heuristics (docs/faq/low-complexity.md:15): no candidate filter, every position is polished */
    float   min_zscore;      /* a pass is dropped from a window when its z-score (log-likelihood vs the model's expectation for
                                the window template) is below this; 0 = gate off                                   */
    int32_t handles_per_device; /* handles the caller runs on this GPU (0/1 = one): each takes 1/N of the free HBM for its POA scratch */
    int32_t no_fallback_draft;  /* 1: a failed / unmappable first draft is final (default 0: one fallback draft, SPEC "fallback draft") */
    int32_t max_insertion_size; /* SPEC "trim large insertions" (docs/how-does-ccs-work.md:74-78, --max-insertion-size): a subread segment more
                                 * than this many bases longer than its window is cut down to the window's length before polishing;
                                 * 0 = the default 30, < 0 = never trim (such a segment then leaves the window when it exceeds 63 bases) */
    int32_t serial_stages;      /* 1: draft and polish stage of all batches on ONE compute stream (A/B switch; default 0: the draft stage
                                 * of batch k+1 runs on its own stream under the polish stage of batch k, docs/img/ccs-impl.png)            */
    int32_t max_qv;             /* largest per-base QV that is reported: every per-base error probability (and with it rq) is floored at 10^(-max_qv/10).
                                 * 0 = the default 50 (SPEC v7 "honest QVs": nothing measured on synthetic data supports a higher claim);
                                 * 93 = the reference's documented range (docs/faq/qv-binning.md:31 bins [40, 93]); values above 93 mean 93.  A deviation
                                 * from the reference's output that a caller can switch off: INTEGRATION.md "QV policy"                                  */
} ccsx_opts;

/* ---- input batch: SoA + CSR ---- */
typedef struct ccsx_batch {
    int32_t        n_zmw;
    int32_t        n_reads;      /* R = read_off[n_zmw]                                         */
    int64_t        n_bases;      /* base_off[R]                                                 */
    const int32_t *zmw_id;       /* [n_zmw]  hole number (zm tag)                               */
    const float   *snr;          /* [n_zmw][4] A,C,G,T (sn tag)                                 */
    const int32_t *read_off;     /* [n_zmw+1] first read of each ZMW                            */
    const int64_t *base_off;     /* [R+1] first base of each read                               */
    const uint8_t *bases;        /* [n_bases] codes 0..3 = A,C,G,T, native (sequenced) orientation; only the low two bits of
                                    a byte are used, so no input byte can index out of range on the device */
    const uint8_t *pw;           /* [n_bases] pulse width, CodecV1 code as stored in the pw:B,C tag (codes < 64 ARE the
                                    frame count, so the HMM's pulse-width bin min(pw,3) needs no decoding)        */
    const uint8_t *ipd;          /* [n_bases] inter-pulse duration, CodecV1 code (ip:B,C tag).  Unused by the HMM;
                                    may be NULL unless opts.hifi_kinetics is set                                   */
    const uint8_t *flags;        /* [R] bit0: pass is on the reverse strand (cx REVERSE_PASS)
                                        bit1: PARTIAL pass (not flanked by adapters on both sides: the first / last subread of the
                                              polymerase read).  Not used for the draft, not counted in np; aligned to the draft anchored
                                              at one end and used by the polish where it reaches (docs/faq/accuracy-vs-passes.md:26-29:
                                              ec ~ np + 1).  A ZMW's partial passes must FOLLOW its full-length passes.
                                        bit2: (partial only) the adapter is at the pass's END (cx ADAPTER_AFTER only), else at its start
                                        bit3: CCSX_PASS_STRAND_UNKNOWN: bit0 of this pass is a guess; the engine decides it against the ZMW's
                                              anchor pass before anything reads it ("Pass orientation" below).  A pass without it is never touched */
} ccsx_batch;
#define CCSX_PASS_STRAND_UNKNOWN 0x8

/* ---- results: caller-allocated; seq/qual/raw_qv are laid out at seq_off[z] (capacity layout
 *      from ccsx_result_layout), seq_len[z] bases valid ---- */
typedef struct ccsx_results {
    int32_t  n_zmw;
    int64_t  seq_capacity;       /* total elements in seq / qual / raw_qv                       */
    int64_t *seq_off;            /* [n_zmw+1] (filled by ccsx_result_layout)                    */
    int32_t *status;             /* [n_zmw] enum ccsx_status                                    */
    int32_t *seq_len;            /* [n_zmw]                                                     */
    uint8_t *seq;                /* [seq_capacity] codes 0..3                                   */
    uint8_t *qual;               /* [seq_capacity] phred 0..93                                  */
    float   *raw_qv;             /* [seq_capacity] un-rounded QV (may be NULL)                  */
    float   *rq;                 /* [n_zmw] predicted accuracy (rq tag)                         */
    int32_t *np;                 /* [n_zmw] passes used (np tag)                                */
    float   *ec;                 /* [n_zmw] effective coverage (ec tag)                         */
    int32_t *iters;              /* [n_zmw] total polish iterations over all windows            */
    int32_t *n_windows;          /* [n_zmw]                                                     */
    /* HiFi kinetics (opts.hifi_kinetics; any of these may be NULL).  CodecV1 codes, indexed like seq (orientation of
     * SEQ; a BAM writer that stores ri/rp in the reverse strand's own orientation reverses them).  Tags fi fp ri rp
     * fn rn of docs/faq/bam-output.md:13-23; with --by-strand the forward pair is the record's ip / pw.           */
    uint8_t *fi, *fp;            /* [seq_capacity] mean IPD / pulse width of the passes on SEQ's strand         */
    uint8_t *ri, *rp;            /* [seq_capacity] same for the passes on the opposite strand                   */
    int32_t *fn, *rn;            /* [n_zmw] full-length passes that align to the draft, on SEQ's strand (the backbone's) / on the other; filled with or
                                    without kinetics.  fn + rn is the aligned count; np is the mode over windows of the passes the polish used, so
                                    np <= fn + rn, equal unless most windows' gates drop an aligned pass */
} ccsx_results;

/* ---- per-kernel device timings of the last run, HIP events on the handle's stream (ms) ---- */
typedef struct ccsx_timings {
    float setup_ms, draft_ms, align_ms, polish_ms, stitch_ms, total_ms;
    int64_t polish_workgroups;   /* launched polish workgroups that had work                     */
    float queue_ms;              /* between the two stages: end of the draft stage -> start of the polish stage (the polish stream
                                    was still busy with the previous batch); total_ms includes it               */
    float reserved_;
    double start_ms, end_ms;     /* device time of the batch's first / last kernel since the handle's creation: over a run of
                                    tickets (end of the last - start of the first) is the time the kernels alone took     */
} ccsx_timings;

typedef struct ccsx_handle_s *ccsx_handle;

/* library / device */
int         ccsx_abi_version(void);
int         ccsx_spec_version(void);                    /* version of the algorithm specification the kernels implement:
                                                           golden vectors carry it, so SPEC drift fails loudly           */
const char *ccsx_build_flags(void);                     /* "" for the product library.  Anything else names the compile-time switches of an experimental
                                                           build (tuning overrides, timing-only variants that compute wrong results: those also make
                                                           ccsx_spec_version() negative).  tests/test_abi.py requires "" of the library it ships   */
const char *ccsx_runtime_switches(void);                /* the CCSX_* scheduling / debugging overrides found in this process's environment, "NAME=VALUE ..." ("" = none).
                                                           They never change a result, they change timings: a benchmark line states them (bench.py config.runtime_switches)
                                                           and tests/test_abi.py requires "" under a clean environment                                                       */
const char *ccsx_last_error(void);
int         ccsx_device_count(void);

/* model + options */
void        ccsx_model_default(ccsx_model *m);          /* synthetic parameter set "SYN-1"      */
void        ccsx_opts_default(ccsx_opts *o);

/* model parameter files and chemistry lookup (docs/faq/chemistry.md:27-56, docs/changelog.md:66,101).  The json schema is
 * this library's own ("ConsensusModelVersion": "ccsx-1"): the ccsx_model blob plus the (BindingKit, SequencingKit,
 * BasecallerVersion) triples it supports; floats round-trip exactly.                                                      */
int         ccsx_model_from_json(const char *json_text, ccsx_model *m);
int         ccsx_model_load(const char *path, ccsx_model *m);
/* writes at most cap-1 bytes + NUL, returns the bytes needed (call with buf = NULL to size); the triple may be NULL      */
int64_t     ccsx_model_to_json(const ccsx_model *m, const char *binding_kit, const char *sequencing_kit,
                               const char *basecaller_version, char *buf, int64_t cap);
/* $SMRT_CHEMISTRY_BUNDLE_DIR/arrow/ (every .json there; injected models take precedence), then the built-in set.  <0 with
 * "Unsupported chemistries found: (...)" when no model supports the triple (basecaller versions match on major.minor)    */
int         ccsx_model_for_chemistry(const char *binding_kit, const char *sequencing_kit, const char *basecaller_version,
                                     ccsx_model *m);

/* lifecycle: binds to GPU `device_ordinal`, creates a stream, copies the model */
int         ccsx_create(int device_ordinal, const ccsx_model *model, const ccsx_opts *opts, ccsx_handle *out);
int         ccsx_destroy(ccsx_handle h);

/* page-locked host memory for batch arrays (optional: any host memory works; pinned buffers upload by DMA at PCIe
 * rate instead of through the runtime's staging copy).  NULL on failure (ccsx_last_error). */
/* NUMA placement of a device's host threads on a multi-GPU node (docs/faq/parallelize.md:8-29): the device's NUMA node from its PCI address
 * (/sys/bus/pci/devices/<id>/numa_node; -1 = unknown / the platform reports none), and binding the CALLING thread to that node's CPUs (intersected with the
 * CPUs the process may use).  Bind a device's worker / packing threads BEFORE they allocate page-locked staging: first touch then puts the staging on the
 * device's node.  Both return the node, or -1 when nothing was (or could be) done — never an error: placement is an optimisation.  CCSX_NUMA=0 turns binding off. */
int         ccsx_pci_numa_node(const char *pci_bus_id);
int         ccsx_device_numa_node(int device);
int         ccsx_bind_thread_to_node(int node);
int         ccsx_bind_thread_to_device(int device);
void       *ccsx_alloc_pinned(size_t bytes);
void        ccsx_free_pinned(void *p);

/* result sizing: fills res->seq_off[0..n] and returns the total capacity needed (elements) */
int64_t     ccsx_result_layout(const ccsx_batch *b, int64_t *seq_off);

/* fused path, host buffers in / host buffers out (one synchronous call = upload + run + download) */
int         ccsx_consensus_batch(ccsx_handle h, const ccsx_batch *b, ccsx_results *res);

/* asynchronous pipeline (submit / wait tickets).  ccsx_submit enqueues upload -> kernels -> download of one
 * batch on the handle's streams (H2D, draft stage, polish stage, D2H) and returns; up to three batches are in flight, so the
 * copies of batch k+1 / k-1 and the draft stage of batch k+1 run under the polish stage of batch k.  The batch arrays and the result buffers should be
 * page-locked (ccsx_alloc_pinned).  Tickets complete in order.
 * Lifetime: a ticket's batch, results and drafts structs (and the arrays they point to) must stay valid until the ticket is RETIRED: when ccsx_wait returns,
 * when ccsx_poll first returns 1, when its slot is recycled (a later submit, or any synchronous call: ccsx_upload and the calls built on it), or when the
 * handle is destroyed, whichever comes first.  Retiring completes the host-side outputs (seq_off; the drafts' seq_off, win_off and backbone) and takes the
 * ticket's timings; afterwards the library never touches those structs again, and ccsx_ticket_timings reads only what was taken.  A synchronous call
 * recycles slot 0's ticket: ccsx_wait / ccsx_poll on it fail ("unknown or recycled ticket"); the other slots' tickets stay valid, their outputs complete. */
typedef int64_t ccsx_ticket;
int         ccsx_submit(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, ccsx_ticket *ticket);
int         ccsx_wait(ccsx_handle h, ccsx_ticket ticket);              /* results of that batch are in `res`   */
int         ccsx_poll(ccsx_handle h, ccsx_ticket ticket);              /* 1 done, 0 not yet, <0 error          */
int         ccsx_ticket_timings(ccsx_handle h, ccsx_ticket ticket, ccsx_timings *t);

/* ---- the two seams of the reference's block diagram (docs/img/ccs-impl.png: a GPU consumer on the DRAFT queue and one on the POLISH queue;
 * docs/faq/revio.md:35-53: Arrow runs a second time, for QVs only, on a sequence that was made elsewhere).  ccsx_consensus_batch / ccsx_submit are the two fused.
 *   ccsx_draft_batch   draft stage only: draft cascade (POA -> fallback POA -> last resort) incl. the alignments that drive it; the drafts, their window
 *                      bounds and per-ZMW statuses go to caller buffers.
 *   ccsx_polish_batch  alignment cascade + windowing + Arrow polish + QVs on CALLER-SUPPLIED drafts (a host that drafts on its CPU pool, e.g. with SPOA).  With
 *                      CCSX_QV_ONLY no mutation is applied: one scoring round, QVs / rq / np / ec for the sequence as given.
 * ccsx_polish_batch(ccsx_draft_batch(b)) returns byte for byte what ccsx_consensus_batch(b) returns (tests/test_gpu_parity.py).  A draft nothing maps to yields
 * a per-ZMW status (TOO_MANY_UNUSABLE, DRAFT_FAILURE for length 0 or a length beyond the slot), never an error of the call.                                   */
/* Lifetime and memory: with the TICKETED forms the arrays of a ccsx_drafts are read (ccsx_submit_polish) / written (ccsx_submit_draft) by
 * asynchronous copies: they must stay valid until the ticket is retired (see ccsx_submit), and they should be page-locked (ccsx_alloc_pinned) — a copy from / to
 * pageable memory blocks the submitting thread until the stage has finished, so "three in flight" degenerates to one at a time (correct, but serial).
 * As INPUT (ccsx_polish_batch / ccsx_submit_polish) only seq_off, len, seq and backbone are read; status, n_windows, win_bounds and win_off may be NULL.   */
typedef struct ccsx_drafts {
    int32_t  n_zmw;
    int64_t  seq_capacity;       /* elements in seq, from ccsx_draft_layout (= the capacity layout of ccsx_result_layout)               */
    int64_t  win_capacity;       /* elements in win_bounds, from ccsx_draft_layout                                                      */
    int64_t *seq_off;            /* [n_zmw+1] slot of every ZMW's draft in seq (capacity layout; ccsx_draft_layout fills it)            */
    int64_t *win_off;            /* [n_zmw+1] slot of every ZMW's window bounds in win_bounds (ccsx_draft_layout fills it)               */
    int32_t *status;             /* [n_zmw] out of ccsx_draft_batch: enum ccsx_status so far (SUCCESS = a usable draft); ignored as input */
    int32_t *len;                /* [n_zmw] draft length; 0 = none                                                                       */
    uint8_t *seq;                /* [seq_capacity] codes 0..3, len[z] bases at seq_off[z]                                                */
    int32_t *backbone;           /* [n_zmw] index (within the ZMW) of a pass that has the draft's orientation: the strand reference of the
                                    consensus, of fn / rn and of the kinetics planes (ccsx_draft_batch: the backbone pass of the generator
                                    that succeeded)                                                                                      */
    int32_t *n_windows;          /* [n_zmw] out of ccsx_draft_batch (may be NULL)                                                        */
    int32_t *win_bounds;         /* [win_capacity] out of ccsx_draft_batch (may be NULL): n_windows[z] + 1 core bounds at win_off[z]       */
} ccsx_drafts;
#define CCSX_QV_ONLY 1u          /* ccsx_polish_batch flag */
void        ccsx_draft_layout(const ccsx_batch *b, int64_t *seq_off, int64_t *win_off, int64_t *seq_capacity, int64_t *win_capacity);
int         ccsx_draft_batch(ccsx_handle h, const ccsx_batch *b, ccsx_drafts *drafts);
int         ccsx_polish_batch(ccsx_handle h, const ccsx_batch *b, const ccsx_drafts *drafts, ccsx_results *res, uint32_t flags);
/* the same with tickets (ccsx_wait / ccsx_poll / ccsx_ticket_timings as for ccsx_submit; the two kinds share the handle's three slots) */
int         ccsx_submit_draft(ccsx_handle h, const ccsx_batch *b, ccsx_drafts *drafts, ccsx_ticket *ticket);
int         ccsx_submit_polish(ccsx_handle h, const ccsx_batch *b, const ccsx_drafts *drafts, ccsx_results *res, uint32_t flags, ccsx_ticket *ticket);

/* split form used by the benchmark (inputs resident in HBM when the timed region starts).  ccsx_run / ccsx_download take slot 0 as ccsx_upload staged it:
 * after ccsx_hd_batch (or a seam's ticket on slot 0) they fail until the next ccsx_upload                                                                      */
int         ccsx_upload(ccsx_handle h, const ccsx_batch *b);           /* H2D + workspace sizing */
int         ccsx_run(ccsx_handle h);                                   /* all kernels, async     */
int         ccsx_sync(ccsx_handle h);                                  /* wait for the stream    */
int         ccsx_download(ccsx_handle h, ccsx_results *res);           /* D2H                    */
int         ccsx_get_timings(ccsx_handle h, ccsx_timings *t);

/* stage access for parity tests (valid after ccsx_run + ccsx_sync on the uploaded batch)        */
int         ccsx_stage_draft(ccsx_handle h, int32_t zmw_index, uint8_t *draft, int32_t cap, int32_t *len);
int         ccsx_stage_align(ccsx_handle h, int32_t read_index, int32_t *rstart, int32_t cap,
                             int32_t *valid, int32_t *score);
int         ccsx_stage_windows(ccsx_handle h, int32_t zmw_index, int32_t *bounds, int32_t cap, int32_t *n_windows);
/* ccsx_stage_align plus the pass's pile-up evidence: rstart / valid / score exactly as ccsx_stage_align reports them, and dirty[p] (p < draft length <= dirty_cap)
 * = 1 iff the pass's dirty bit of draft position p is set, unpacked on the host from the per-interval masks the alignment kernels leave (interval k = the positions
 * from window-edge column k - 1 up to edge column k, bit p - column(k - 1)): the bits as k_polish's candidate filter reads them for that pass.  Every position of a
 * split or partial pass is 1; dirty[] of a pass that is not valid is 0.  For parity tests (tests/test_align_gpu.py).                                            */
int         ccsx_stage_align_ev(ccsx_handle h, int32_t read_index, int32_t *rstart, int32_t cap, int32_t *valid, int32_t *score,
                                uint8_t *dirty, int32_t dirty_cap);
/* What k_polish left per window of ZMW zmw_index, copied from the device as it stands: meta[5 w .. 5 w + 4] = core length after the polish, usable reads of the last
 * round (after the alpha/beta and z-score gates) over all passes, the same over the full-length passes only, 1 if the window ended NON_CONVERGENT, scoring rounds.
 * cap counts windows.  A ZMW that failed before the polish reports 0 windows.  For parity tests (tests/test_filter_gpu.py).                                       */
int         ccsx_stage_wmeta(ccsx_handle h, int32_t zmw_index, int32_t *meta, int32_t cap, int32_t *n_windows);
/* The POA log: a per-pass witness of the draft stage, off by default.  ccsx_poa_log(h, 1) asks for it; it holds from the next batch the handle stages (any entry
 * point) until ccsx_poa_log(h, 0).  While it is on, k_poa_thread writes one record of CCSX_POA_LOG_WORDS int32 per (ZMW, draft generator, pass rr of the POA):
 *   [0] I              length of the pass (rr-th pass of the generator's order: backbone + rr, wrapping)
 *   [1] end score      best M[v][I] over the graph (NEG = -2^28 when no vertex holds row I in its band)
 *   [2] end position   topological position of the end cell's vertex before the pass is threaded, -1 when there is none
 *   [3] threaded       1 = the pass went into the graph; 0 = the gate refused it, or threading it would overflow the vertex capacity (the generator then fails)
 *   [4] vertices       of the graph after the pass
 * With the log off the kernel is given a null pointer, stores nothing, and every output is byte for byte what it is with the log on.
 * ccsx_stage_poa reads the log of the batch the handle ran last (any entry point, after it has been waited for): generator 0 = POA on pass 0, 1 = the fallback.
 * rec receives `*n_records` records indexed by rr (cap_records >= the most passes of a ZMW in the batch; else refused, with that number in `*n_records`); record 0 (the backbone: k_poa_init chains
 * it, no DP runs) and every pass the generator did not reach for this ZMW have I = -1 in all five words.  For parity tests (tests/test_poa_gpu.py).            */
#define CCSX_POA_LOG_WORDS 5
int         ccsx_poa_log(ccsx_handle h, int32_t on);
int         ccsx_stage_poa(ccsx_handle h, int32_t zmw_index, int32_t generator, int32_t *rec, int32_t cap_records, int32_t *n_records);

/* ---- the heteroduplex finder (docs/faq/mode-heteroduplex-filtering.md:25-33, docs/how-does-ccs-work.md:65-72; the rule: DESIGN.md §2 "Heteroduplex rule").
 * ccsx_hd_batch is the third seam beside ccsx_draft_batch and ccsx_polish_batch: on the caller's drafts it runs the polish seam's alignment cascade and window map,
 * then a strand-resolved substitution pileup and the large-indel test per window, and reduces them to one verdict per ZMW.  No polish runs.  Afterwards
 * ccsx_stage_draft / ccsx_stage_windows / ccsx_stage_align report what it used.  The rule has its own version (ccsx_hd_rule_version): it changes no result of
 * the consensus, so CCSX_SPEC_VERSION does not move.                                                                                                           */
#define CCSX_HD_MAX_SITES 16     /* sites listed per ZMW: the ones with the lowest columns, in column order                                                   */
#define CCSX_HD_WIN_SITES 8      /* substitution sites per window that can enter the list (the window's lowest columns); the counts cover all sites             */
typedef struct ccsx_hd_opts {
    int32_t min_strand_passes;   /* passes needed on EACH strand at a column / event (and for a DOUBLE_STRAND verdict)                                          */
    int32_t min_sites;           /* substitution sites that make a heteroduplex                                                                                */
    int32_t min_indel;           /* a length excess of at least this many bases over 1-3 windows is a large-indel event (1 ..  21)                                */
    float   min_alt_frac;        /* the alternative base's share of a strand's outcomes, on at least one strand                                                  */
    double  max_pvalue;          /* two-sided Fisher exact test of the alternative against the strands                                                          */
} ccsx_hd_opts;
enum ccsx_hd_verdict { CCSX_HD_UNTESTED = 0, CCSX_HD_DOUBLE_STRAND = 1, CCSX_HD_HETERODUPLEX = 2 };
typedef struct ccsx_hd_site {
    int32_t column;              /* draft column (substitution), first core column of the event's first window (large indel)                                    */
    int8_t  kind;                /* 0 substitution, 1 large insertion, 2 large deletion                                                                        */
    int8_t  alt;                 /* substitution: the alternative base 0..3; -1 for an indel                                                                    */
    uint8_t fwd_alt, fwd_n, rev_alt, rev_n;   /* the Fisher table: passes with the alternative / passes counted, per strand relative to the draft                */
    uint8_t pad_[2];
    double  p;
} ccsx_hd_site;
typedef struct ccsx_hd_report {
    int32_t n_zmw;
    int32_t *verdict;            /* [n_zmw] enum ccsx_hd_verdict                                                                                               */
    int32_t *n_sub_sites, *n_indel_sites, *n_listed;   /* [n_zmw]                                                                                               */
    double  *min_p;              /* [n_zmw] smallest p of any site, 1 when there is none                                                                        */
    ccsx_hd_site *sites;         /* [n_zmw * CCSX_HD_MAX_SITES]                                                                                                 */
    int32_t *status;             /* [n_zmw] enum ccsx_status after the alignment cascade (anything but SUCCESS: UNTESTED); may be NULL                          */
} ccsx_hd_report;
void        ccsx_hd_opts_default(ccsx_hd_opts *o);
int         ccsx_hd_rule_version(void);
int         ccsx_hd_batch(ccsx_handle h, const ccsx_batch *b, const ccsx_drafts *drafts, const ccsx_hd_opts *o, ccsx_hd_report *out);

/* ---- the pileup summary: per-base tags sa sm sx of docs/faq/bam-output.md:25-27 (the rule: DESIGN.md §2 "Pileup summary", its own version
 * ccsx_pileup_rule_version; no result of the consensus changes).  After a window has converged, every used pass with a usable segment there (avalid,
 * 0 <= n <= CCSX_IMAX: the passes the kinetics see) is aligned to the converged window template with the kinetics alignment; per consensus base
 * `coverage` = such passes, `matches` / `mismatches` = those whose alignment puts a read base on the base (DIAG) that agrees / differs.  matches +
 * mismatches <= coverage; coverage is constant over a window's core.  Planes are indexed like seq (orientation of SEQ, seq_off[z], seq_len[z] valid).
 * ccsx_consensus_pileup = ccsx_consensus_batch + the planes (synchronous, slot 0); ccsx_submit_pileup = ccsx_submit + the planes: the arrays of `pile`
 * follow the lifetime rule of `res` (see ccsx_submit) and should be page-locked.  Either works with or without opts.hifi_kinetics (one alignment feeds
 * both).  Without a pileup request nothing of it runs.  (The polish seam with planes, ccsx_submit_polish + pileup, is not offered yet.)             */
typedef struct ccsx_pileup {
    int64_t  seq_capacity;       /* elements in each plane: the capacity layout of ccsx_result_layout (= ccsx_results.seq_capacity)              */
    uint8_t *coverage;           /* [seq_capacity] passes covering the base (sa before run-length encoding)                                    */
    uint8_t *matches;            /* [seq_capacity] aligned matches (sm)                                                                        */
    uint8_t *mismatches;         /* [seq_capacity] aligned mismatches (sx)                                                                     */
} ccsx_pileup;
int         ccsx_pileup_rule_version(void);
int         ccsx_consensus_pileup(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, ccsx_pileup *pile);
int         ccsx_submit_pileup(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, ccsx_pileup *pile, ccsx_ticket *ticket);
/* the converged window templates of ZMW zmw_index after the last synchronous run that kept them (ccsx_consensus_pileup, or any synchronous run of a
 * handle with opts.hifi_kinetics): tpl[w * 32 + k] (k < J), meta[w * 3 + 0..2] = J, core start cs, core end ce (the core is tpl[cs, ce)); n_windows = 0
 * for a ZMW that failed before stitching.  passes_used = the ZMW's passes the engine used, backbone = the index (within the ZMW) of its strand reference.
 * For parity tests (tests/pileup_ref.py).                                                                                                             */
int         ccsx_stage_polished(ccsx_handle h, int32_t zmw_index, uint8_t *tpl, int32_t *meta, int32_t cap, int32_t *n_windows,
                                int32_t *passes_used, int32_t *backbone);

/* ---- optional outputs of the fused path beside the results: ccsx_extras (the structs above stay their pinned sizes; new outputs join this one).
 *   pile                      the pileup summary planes (as ccsx_submit_pileup), or NULL.
 *   tandem_len                [n_zmw] or NULL: per ZMW the longest run of sDUST-masked bases of its deciding draft (DESIGN.md §2 "Tandem repeats", rule
 *                             version ccsx_tandem_rule_version): symmetric DUST, W = 64, T = 20 (score > 2.0), on the first draft the alignment cascade
 *                             aligns passes to in this call (pass-0 POA draft, else the fallback or last-resort draft); 0 without such a draft.
 *   min_tandem_repeat_length  > 0: a ZMW with tandem_len >= this value runs with opts.disable_heuristics for itself only (--min-tandem-repeat-length of
 *                             docs/faq/low-complexity.md:8-18).  0: detection only (when tandem_len is given), no result changes.  < 0 is an error.
 *   reserved                  must be 0.
 * Detection runs when tandem_len is given or the threshold is > 0.  With a NULL ccsx_extras, or NULL pile and tandem_len and a threshold of 0, nothing new is
 * launched, reserved or copied: the call is ccsx_consensus_batch / ccsx_submit.  ccsx_submit_extras is ticketed like ccsx_submit: the arrays behind `pile`
 * and tandem_len follow the lifetime rule of `res` (they are written by the ticket's download) and should be page-locked; the ccsx_extras struct itself is
 * read during the call only.  ccsx_consensus_extras is the synchronous form (slot 0).  The draft and polish seams and ccsx_hd_batch take no extras.   */
typedef struct ccsx_extras {
    ccsx_pileup *pile;
    int32_t     *tandem_len;
    int32_t      min_tandem_repeat_length;
    int32_t      reserved;
} ccsx_extras;
int         ccsx_tandem_rule_version(void);
int         ccsx_consensus_extras(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const ccsx_extras *ex);
int         ccsx_submit_extras(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const ccsx_extras *ex, ccsx_ticket *ticket);

/* The finder in the fused path: ccsx_consensus_hd (synchronous, slot 0) and ccsx_submit_hd (ticketed like ccsx_submit) are ccsx_consensus_extras /
 * ccsx_submit_extras (ex may be NULL) plus the finder, whose three kernels run in the draft stage after the window map, on what k_polish is given: the ZMW's
 * final draft (pass-0 POA, fallback or last resort), its window bounds, its status after the cascade and the entry rows (DESIGN.md §2 "Heteroduplex rule").
 * The report equals ccsx_hd_batch's on the drafts of ccsx_draft_batch, field for field (report.status: the status after the cascade, before a split).
 *   opts      NULL = ccsx_hd_opts_default; the ranges of ccsx_hd_batch.
 *   report    required, sized for the batch; its arrays follow the lifetime rule of `res` (written by the ticket's download) and should be page-locked.
 *   split     0: detection only, every result is byte for byte that of the same call without a request.  1: a ZMW whose verdict is HETERODUPLEX is not
 *             polished: status CCSX_HETERODUPLEX, seq_len = n_windows = iters = 0, rq = ec = 0, np = fn + rn and fn / rn as the accounting counted them
 *             (the values of a ZMW that fails before polishing); its kinetics and pileup planes are not written.  Every other ZMW is as with split = 0.
 *   reserved  must be 0 (and split 0 or 1).
 * The request struct is read during the call only.  Per batch slot the finder's buffers take about 200 bytes per window slot (1.7 GB at 16384 ZMWs x 10 kb);
 * they are reserved by the first request on that slot.  Without a request nothing of the finder is launched, reserved or copied.  The draft and polish
 * seams and the ccsx_upload / ccsx_run form take no request.                                                                                             */
typedef struct ccsx_hd_request {
    const ccsx_hd_opts *opts;
    ccsx_hd_report     *report;
    int32_t             split;
    int32_t             reserved;
} ccsx_hd_request;
int         ccsx_consensus_hd(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const ccsx_extras *ex, const ccsx_hd_request *hd);
int         ccsx_submit_hd(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const ccsx_extras *ex, const ccsx_hd_request *hd, ccsx_ticket *ticket);

/* ---- adapter palindromes (docs/faq/fail-reads.md: fail class 0x20 "CCS adapter palindrome"; the rule: DESIGN.md §2 "Adapter palindromes", its own version
 * ccsx_fold_rule_version).  A missed adapter makes every pass read X . A . rc(X) through the hairpin; the engine polishes that into a confident consensus.  k_fold
 * self-aligns the ZMW's final draft (what k_polish is given: pass-0 POA, fallback or last resort) against its reverse complement with sampled 15-mers and votes on
 * the fold's anti-diagonal; integer arithmetic only.  Detection only: every result byte equals the same call without the request.
 *   ccsx_consensus_fold  synchronous (slot 0): ccsx_consensus_extras (ex may be NULL) + the report.
 *   ccsx_submit_fold     ticketed like ccsx_submit_extras: the report's arrays follow the lifetime rule of `res` (written by the ticket's download) and should be
 *                        page-locked; the request and options structs are read during the call only.
 * A NULL request or report, a report sized for another batch, nonzero reserved words or thresholds out of range are errors of the call: nothing is enqueued.
 * Without a request nothing of it is launched, reserved or copied.  With a ccsx_hd_request: ccsx_consensus_hd_requests / ccsx_submit_hd_requests.                                            */
typedef struct ccsx_fold_opts {
    int32_t max_occ;             /* a canonical 15-mer sampled more often than this is dropped everywhere (1 .. 64)                                              */
    int32_t min_hits;            /* hits in the winning pair of anti-diagonal bins (>= 1)                                                                        */
    int32_t min_arm;             /* bases the hits span on each arm (>= 1)                                                                                       */
    int32_t min_span_tenths;     /* the span covers at least this many tenths of the shorter arm (0 .. 10)                                                       */
    int32_t end_slack;           /* the shorter arm's hits reach its end of the draft within this many bases (>= 0)                                              */
} ccsx_fold_opts;
enum ccsx_fold_verdict { CCSX_FOLD_UNTESTED = 0, CCSX_FOLD_NONE = 1, CCSX_FOLD_PALINDROME = 2 };
typedef struct ccsx_fold_report {
    int32_t  n_zmw;
    int32_t *verdict;            /* [n_zmw] enum ccsx_fold_verdict (UNTESTED: the status after the cascade is not SUCCESS)                                        */
    int32_t *fold;               /* [n_zmw] fold centre in draft coordinates, -1 when there is no hit                                                             */
    int32_t *hits;               /* [n_zmw] hits in the winning pair of anti-diagonal bins                                                                        */
    int32_t *span;               /* [n_zmw] bases the winning hits span, the shorter of the two arms' extents (0 without a hit)                                   */
} ccsx_fold_report;
typedef struct ccsx_fold_request {
    const ccsx_fold_opts *opts;  /* NULL = ccsx_fold_opts_default                                                                                                 */
    ccsx_fold_report     *report;
    int32_t               reserved[2];   /* must be 0                                                                                                            */
} ccsx_fold_request;
void        ccsx_fold_opts_default(ccsx_fold_opts *o);
int         ccsx_fold_rule_version(void);
int         ccsx_consensus_fold(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const ccsx_extras *ex, const ccsx_fold_request *fold);
int         ccsx_submit_fold(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const ccsx_extras *ex, const ccsx_fold_request *fold, ccsx_ticket *ticket);

/* ---- adapter screen (docs/faq/fail-reads.md: fail classes 0x10 "adapter concatenation" and 0x40 "adapters close to either end"; the rule: DESIGN.md §2 "Adapter
 * screen", its own version ccsx_adapter_rule_version).  SMRTbell adapter sequence the instrument's adapter finder missed sits inside the read the engine polishes.
 * k_adapter searches the ZMW's final draft (what k_polish is given: pass-0 POA, fallback or last resort) for every caller-supplied adapter and its reverse
 * complement by unit-cost edit distance (semi-global, bit-parallel); integer arithmetic only.  Detection only: every result byte equals the same call without the
 * request.
 *   ccsx_consensus_screen  synchronous (slot 0): ccsx_consensus_fold + the adapter request; either request may be NULL (both NULL = ccsx_consensus_extras).
 *   ccsx_submit_screen     ticketed like ccsx_submit_fold: the reports' arrays follow the lifetime rule of `res` (written by the ticket's download) and should be
 *                          page-locked; the request, set and options structs are read during the call only.
 * A NULL report, a report sized for another batch, nonzero reserved words, options or pattern lengths out of range, a code above 3 or n_adapters outside 1 .. 8 are
 * errors of the call: nothing is enqueued.  Without a request nothing of it is launched, reserved or copied.  With a ccsx_hd_request: ccsx_consensus_hd_requests / ccsx_submit_hd_requests.     */
#define CCSX_ADAPTER_MAX_PATTERNS 8
#define CCSX_ADAPTER_MIN_LEN      16
#define CCSX_ADAPTER_MAX_LEN      64
#define CCSX_ADAPTER_MAX_HITS     16
#define CCSX_ADAPTER_CONCAT       1   /* verdict bit: n_hits >= min_copies and max_gap <= max_insert (fail class 0x10)                                          */
#define CCSX_ADAPTER_NEAR_END     2   /* verdict bit: a hit starts within end_slack of the draft's start or ends within end_slack of its end (fail class 0x40)  */
typedef struct ccsx_adapter_opts {
    int32_t max_dist_pct;        /* a search of m bases matches at up to floor(m * max_dist_pct / 100) edits (0 .. 30)                                           */
    int32_t min_copies;          /* CONCAT: at least this many hits (>= 1)                                                                                       */
    int32_t max_insert;          /* CONCAT: no stretch of the draft outside every hit is longer than this (>= 0)                                                 */
    int32_t end_slack;           /* NEAR_END: distance of a hit to an end of the draft (>= 0)                                                                    */
} ccsx_adapter_opts;
typedef struct ccsx_adapter_set {
    int32_t n_adapters;          /* 1 .. CCSX_ADAPTER_MAX_PATTERNS; search 2a = adapter a as given, search 2a + 1 = its reverse complement                       */
    int32_t len[CCSX_ADAPTER_MAX_PATTERNS];                        /* CCSX_ADAPTER_MIN_LEN .. CCSX_ADAPTER_MAX_LEN                                                */
    uint8_t seq[CCSX_ADAPTER_MAX_PATTERNS][CCSX_ADAPTER_MAX_LEN];  /* codes 0 .. 3 (A C G T)                                                                      */
} ccsx_adapter_set;
typedef struct ccsx_adapter_hit {
    int32_t start, end;          /* the shortest best match, draft[start, end)                                                                                   */
    uint8_t search, dist, pad_[2];
} ccsx_adapter_hit;
typedef struct ccsx_adapter_report {
    int32_t  n_zmw;
    int32_t *tested;             /* [n_zmw] 1: the status after the cascade is SUCCESS (verdict 0 then means clean); 0: untested                                  */
    int32_t *verdict;            /* [n_zmw] CCSX_ADAPTER_CONCAT | CCSX_ADAPTER_NEAR_END                                                                            */
    int32_t *n_hits;             /* [n_zmw] hits of all searches (not capped)                                                                                      */
    int32_t *n_listed;           /* [n_zmw] min(n_hits, CCSX_ADAPTER_MAX_HITS)                                                                                     */
    int32_t *covered;            /* [n_zmw] draft bases inside a hit                                                                                               */
    int32_t *max_gap;            /* [n_zmw] longest stretch of draft bases outside every hit (the draft's length without a hit)                                    */
    int32_t *first_start;        /* [n_zmw] smallest start (-1 without a hit)                                                                                      */
    int32_t *last_end;           /* [n_zmw] largest end (-1 without a hit)                                                                                         */
    int32_t *min_dist;           /* [n_zmw] smallest dist (255 without a hit)                                                                                      */
    ccsx_adapter_hit *hits;      /* [n_zmw * CCSX_ADAPTER_MAX_HITS] the first hits in increasing (end, search); zero beyond n_listed                               */
} ccsx_adapter_report;
typedef struct ccsx_adapter_request {
    const ccsx_adapter_set  *adapters;
    const ccsx_adapter_opts *opts;       /* NULL = ccsx_adapter_opts_default                                                                                     */
    ccsx_adapter_report     *report;
    int32_t                  reserved[2];   /* must be 0                                                                                                         */
} ccsx_adapter_request;
void        ccsx_adapter_opts_default(ccsx_adapter_opts *o);
int         ccsx_adapter_rule_version(void);
int         ccsx_adapter_set_default(ccsx_adapter_set *s);   /* the 45-base SMRTbell hairpin adapter; 0, or -1 for a NULL argument */
int         ccsx_consensus_screen(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const ccsx_extras *ex, const ccsx_fold_request *fold,
                                  const ccsx_adapter_request *adapters);
int         ccsx_submit_screen(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const ccsx_extras *ex, const ccsx_fold_request *fold,
                               const ccsx_adapter_request *adapters, ccsx_ticket *ticket);

/* ---- control screen (docs/faq/fail-reads.md: fail class 0x2 "control reads"; docs/faq/reports-aux-files.md "ZMW with control success / failure"; the rule:
 * DESIGN.md §2 "Control screen", its own version ccsx_control_rule_version).  A spike-in control molecule is polished into a confident consensus like any sample.
 * k_control looks every 15-mer of the ZMW's final draft (what k_polish is given: pass-0 POA, fallback or last resort) up, in both orientations, in an index of the
 * caller-supplied control sequence and votes on the diagonal; integer arithmetic only.  Detection only: every result byte equals the same call without the
 * request.  There is no built-in control sequence.
 *   ccsx_consensus_control  synchronous (slot 0): ccsx_consensus_screen + the control request; any of ex, fold, adapters and control may be NULL (all NULL =
 *                           ccsx_consensus_extras).
 *   ccsx_submit_control     ticketed like ccsx_submit_screen: the reports' arrays follow the lifetime rule of `res` (written by the ticket's download) and should
 *                           be page-locked; the request, sequence and options structs are read during the call only (every ticket carries its own index: tickets
 *                           in flight may screen for different controls).
 * A NULL report or control sequence, a report sized for another batch, nonzero reserved words, a length outside 64 .. 4096, a code above 3 or options out of range
 * are errors of the call: nothing is enqueued.  Without a request nothing of it is launched, reserved or copied.  With a ccsx_hd_request: ccsx_consensus_hd_requests / ccsx_submit_hd_requests. */
#define CCSX_CONTROL_MIN_LEN 64
#define CCSX_CONTROL_MAX_LEN 4096
typedef struct ccsx_control_opts {
    int32_t max_occ;             /* a 15-mer that occurs more often than this in the control is dropped from its index (1 .. 64)                                 */
    int32_t min_matched;         /* CONTROL: distinct control positions among the winning hits (>= 1)                                                            */
    int32_t min_ctl_tenths;      /* CONTROL: the winning hits span at least this many tenths of the control (0 .. 10)                                            */
    int32_t min_draft_tenths;    /* CONTROL: ... and of the draft (0 .. 10): the molecule is the control, it does not merely contain a stretch of it             */
} ccsx_control_opts;
typedef struct ccsx_control_seq {
    int32_t        len;          /* CCSX_CONTROL_MIN_LEN .. CCSX_CONTROL_MAX_LEN                                                                                 */
    int32_t        reserved;     /* must be 0                                                                                                                    */
    const uint8_t *seq;          /* codes 0 .. 3 (A C G T)                                                                                                       */
} ccsx_control_seq;
enum ccsx_control_verdict { CCSX_CONTROL_UNTESTED = 0, CCSX_CONTROL_NONE = 1, CCSX_CONTROL_FOUND = 2 };
typedef struct ccsx_control_report {
    int32_t  n_zmw;
    int32_t *verdict;            /* [n_zmw] enum ccsx_control_verdict (UNTESTED: the status after the cascade is not SUCCESS)                                     */
    int32_t *strand;             /* [n_zmw] 0: the draft reads as the control, 1: as its reverse complement, -1: no hit                                           */
    int32_t *hits;               /* [n_zmw] hits in the winning pair of diagonal bins                                                                             */
    int32_t *matched;            /* [n_zmw] distinct control positions among them                                                                                 */
    int32_t *ctl_start, *ctl_end;       /* [n_zmw] control bases the winning hits span                                                                            */
    int32_t *draft_start, *draft_end;   /* [n_zmw] draft bases they span, in the draft's own orientation for either strand                                        */
} ccsx_control_report;
typedef struct ccsx_control_request {
    const ccsx_control_seq  *control;
    const ccsx_control_opts *opts;       /* NULL = ccsx_control_opts_default                                                                                     */
    ccsx_control_report     *report;
    int32_t                  reserved[2];   /* must be 0                                                                                                         */
} ccsx_control_request;
void        ccsx_control_opts_default(ccsx_control_opts *o);
int         ccsx_control_rule_version(void);
int         ccsx_consensus_control(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const ccsx_extras *ex, const ccsx_fold_request *fold,
                                   const ccsx_adapter_request *adapters, const ccsx_control_request *control);
int         ccsx_submit_control(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const ccsx_extras *ex, const ccsx_fold_request *fold,
                                const ccsx_adapter_request *adapters, const ccsx_control_request *control, ccsx_ticket *ticket);

/* ---- coverage screen (docs/faq/reports-aux-files.md:28-35,77-97,149-155: "Coverage drops", "Insufficient draft cov", "Draft too different", "Reads failed
 * polishing"; the rule: DESIGN.md §2 "Coverage rule", its own version ccsx_coverage_rule_version; no result of the consensus changes).  When the draft lacks a
 * block of bases that some passes carry, those passes go through the split alignment, are trimmed, and the ZMW comes out SUCCESS with whichever allele the draft
 * took.  k_coverage counts, per window of the final draft (what k_polish is given), the passes that reach it and those that carry a block there, from the entry
 * rows the alignment cascade left; k_coverage_post adds, after the stitch, how many (pass, window) segments the polish used.  Integer arithmetic only.
 *   reach_w      passes r with avalid[r] and 0 <= n <= L_r, n = the pass's bases between the window's two edge columns (k_polish's segment test before the
 *                63-base limit and before trimming); long_w those of them with n > J_w + block (J_w = the window's columns incl. overhangs); clean_w = reach_w - long_w
 *   verdict      the first that holds: UNTESTED (the status after the cascade is not SUCCESS), DRAFT_TOO_DIFFERENT (np_aligned < opts.min_passes),
 *                INSUFFICIENT_SPANS (spans < min_spans), COVERAGE_DROPS (drop_windows >= 1), READS_FAILED_POLISHING (final status SUCCESS or LOW_RQ and
 *                (reach_sum - used_sum) * 100 > max_lost_percent * reach_sum), NONE
 *   gate         bit v (v = 2 .. 5) set: a ZMW with verdict v gets the status CCSX_DRAFT_TOO_DIFFERENT + (v - 2) and no consensus (seq_len 0).  Verdicts 2 .. 4
 *                are known before the polish: such a ZMW is not polished (n_windows = iters = 0, rq = ec = 0, np / fn / rn as the accounting counted them, as with
 *                ccsx_hd_request.split) and its used_sum / used_min stay 0.  Every other ZMW is byte for byte as without the request.  gate 0: detection only.
 * The request travels in a ccsx_requests (below).  A NULL report, a report sized for another batch, nonzero reserved words, percentages outside 0 .. 100, block
 * outside 1 .. 4096, min_spans outside 0 .. 255 or gate bits outside 2 .. 5 are errors of the call: nothing is enqueued.  The report's arrays follow the lifetime
 * rule of `res` and should be page-locked for the ticketed form; the request and options structs are read during the call only (every ticket carries its own
 * options and gate).  Per batch slot the screen takes 40 bytes per ZMW and one byte per window slot, reserved by the first request on that slot; without a request
 * nothing of it is launched, reserved or copied.  With a ccsx_hd_request: ccsx_consensus_hd_requests / ccsx_submit_hd_requests; the draft and polish seams take no request.                      */
typedef struct ccsx_coverage_opts {
    int32_t drop_percent;        /* a window drops when clean_w * 100 <= drop_percent * cov_max (0 .. 100)                                                        */
    int32_t block;               /* a reaching pass carries a block in a window when its segment is more than this many bases longer than the window (1 .. 4096);
                                    independent of opts.max_insertion_size                                                                                        */
    int32_t min_spans;           /* INSUFFICIENT_SPANS below this many spanning passes; 0 = the handle's opts.min_passes (0 .. 255)                                */
    int32_t max_lost_percent;    /* READS_FAILED_POLISHING when more than this share of the reaching (pass, window) segments was not used by the polish (0 .. 100)  */
} ccsx_coverage_opts;
enum ccsx_coverage_verdict {
    CCSX_COVERAGE_UNTESTED = 0, CCSX_COVERAGE_NONE = 1, CCSX_COVERAGE_DRAFT_TOO_DIFFERENT = 2, CCSX_COVERAGE_INSUFFICIENT_SPANS = 3,
    CCSX_COVERAGE_COVERAGE_DROPS = 4, CCSX_COVERAGE_READS_FAILED_POLISHING = 5
};
typedef struct ccsx_coverage_report {
    int32_t  n_zmw;
    int32_t *verdict;            /* [n_zmw] enum ccsx_coverage_verdict; every other plane of an UNTESTED ZMW is 0                                                  */
    int32_t *np_aligned;         /* [n_zmw] full-length passes that align to the draft (the accounting's np)                                                      */
    int32_t *spans;              /* [n_zmw] ... that also reach every window (a double-split pass with uncovered edge columns does not)                            */
    int32_t *cov_max;            /* [n_zmw] max over the windows of reach_w                                                                                       */
    int32_t *clean_min;          /* [n_zmw] min over the windows of clean_w                                                                                       */
    int32_t *drop_window;        /* [n_zmw] the first window with clean_w = clean_min                                                                             */
    int32_t *drop_windows;       /* [n_zmw] windows with clean_w * 100 <= drop_percent * cov_max                                                                  */
    int32_t *reach_sum;          /* [n_zmw] sum over the windows of reach_w                                                                                       */
    int32_t *used_sum;           /* [n_zmw] sum over the windows of the passes the polish used there (ec x n_windows); 0 for a ZMW that was not polished            */
    int32_t *used_min;           /* [n_zmw] min over the windows of the same; 0 for a ZMW that was not polished                                                   */
} ccsx_coverage_report;
typedef struct ccsx_coverage_request {
    const ccsx_coverage_opts *opts;      /* NULL = ccsx_coverage_opts_default                                                                                    */
    ccsx_coverage_report     *report;
    uint32_t                  gate;      /* bit mask, bit v for verdict v = 2 .. 5; 0 = detection only                                                           */
    int32_t                   reserved[2];   /* must be 0                                                                                                        */
} ccsx_coverage_request;
void        ccsx_coverage_opts_default(ccsx_coverage_opts *o);
int         ccsx_coverage_rule_version(void);

/* ---- every optional request of the fused path in one struct: the argument lists of the ccsx_consensus_* / ccsx_submit_* family stop growing here; a new request
 * joins this struct.  Every member may be NULL (all NULL, or a NULL ccsx_requests = ccsx_consensus_batch / ccsx_submit); reserved must be NULL.  The members mean
 * what they mean in ccsx_consensus_control / ccsx_submit_control, which forward to the same path and give the same results for the same members.
 *   ccsx_consensus_requests  synchronous (slot 0).
 *   ccsx_submit_requests     ticketed like ccsx_submit; the ccsx_requests struct itself is read during the call only.                                             */
typedef struct ccsx_requests {
    const ccsx_extras           *ex;
    const ccsx_fold_request     *fold;
    const ccsx_adapter_request  *adapters;
    const ccsx_control_request  *control;
    const ccsx_coverage_request *coverage;
    const void                  *reserved[3];
} ccsx_requests;
int         ccsx_consensus_requests(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const ccsx_requests *rq);
int         ccsx_submit_requests(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const ccsx_requests *rq, ccsx_ticket *ticket);

/* The finder beside the other requests: ccsx_consensus_hd_requests (synchronous, slot 0) and ccsx_submit_hd_requests (ticketed like ccsx_submit_requests) are
 * ccsx_consensus_requests / ccsx_submit_requests plus a ccsx_hd_request, which is a further argument as the barcode and represent requests are (struct
 * ccsx_requests keeps its layout).  rq may be NULL or carry any member: extras with pileup planes and tandem detection, fold, adapters, control, coverage.  With
 * only rq->ex set the call is ccsx_consensus_hd / ccsx_submit_hd, which forward to this path.  hd == NULL is an error of the call ("null request or report"), and
 * every check of ccsx_submit_hd holds, by the same messages; nothing is enqueued.  It is not combined with the hand-off, barcode or represent requests.
 * Who gives a ZMW its status in the draft stage (DESIGN.md §2 "In the fused path"), in this order:
 *   1. the draft screens (fold, adapters, control) run on every draft whose status after the cascade is SUCCESS, heteroduplex or not: detection only;
 *   2. the coverage screen's k_coverage, on the statuses the cascade left: its report does not depend on the finder.  With a gate bit for verdict 2 .. 4 the ZMW
 *      gets CCSX_DRAFT_TOO_DIFFERENT .. CCSX_COVERAGE_DROPS here;
 *   3. the finder, on every ZMW that is still SUCCESS: a ZMW the gate took is UNTESTED in the finder's report, and report.status holds its gate status.  Without
 *      a gate bit the finder's report is that of ccsx_consensus_hd.  With split = 1 a HETERODUPLEX ZMW gets CCSX_HETERODUPLEX.
 * So the coverage gate precedes the split, and no ZMW is given a status twice.  A CCSX_HETERODUPLEX ZMW keeps the pre-polish planes of its coverage report
 * (verdict, np_aligned, spans, cov_max, clean_min, drop_window, drop_windows, reach_sum) and has used_sum = used_min = 0, as every ZMW that was not polished;
 * verdict 5 (READS_FAILED_POLISHING) is never reached for it.  Nothing else about any request changes.                                                         */
int         ccsx_consensus_hd_requests(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const ccsx_requests *rq, const ccsx_hd_request *hd);
int         ccsx_submit_hd_requests(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const ccsx_requests *rq, const ccsx_hd_request *hd, ccsx_ticket *ticket);

/* ---- polisher hand-off (docs/faq/revio.md:28-53: the low-quality windows of the Arrow consensus go to a second, learned polisher; the rule: DESIGN.md §2
 * "Polisher hand-off", its own version ccsx_handoff_rule_version; no result of the consensus changes).  The consensus of every ZMW is cut into tiles of tile_len
 * positions; a tile whose summed `qual` bytes are below skip_above x its length is selected, and for the selected tiles every pass is laid out column by column
 * against the consensus — base, pulse width, inter-pulse duration, inserted bases — from the kinetics alignment of the pass's segments to the converged window
 * templates (k_tile_select, k_tile_scan, k_tile_rows after k_stitch).  Integers only; the selected tiles are numbered in (ZMW, tile) order by a scan.
 * Every array of ccsx_handoff_out may be host memory (page-locked preferred) or memory of the handle's device: each is copied with hipMemcpyDefault on the
 * download stream, follows the lifetime rule of `res`, and is complete when ccsx_wait (or the synchronous call) returns.  Every byte of the slots
 * g < min(counts[1], max_tiles) is written on every run; slots beyond are unspecified; nothing past an array's capacity is written.
 *   ccsx_consensus_handoff  synchronous (slot 0); copies the written slots only.
 *   ccsx_submit_handoff     ticketed like ccsx_submit; copies the WHOLE capacity of every array (max_tiles slots), since counts is not known when it is enqueued.
 * rq may be NULL or carry any of ccsx_requests' members.  Options and capacity belong to the ticket.  A NULL out or array, max_tiles < 1, options out of range
 * and nonzero reserved words are errors of the call: nothing is enqueued.                                                                                      */
typedef struct ccsx_handoff_opts {
    int32_t tile_len;            /* T: consensus positions per tile, 16 .. 128 [100]                                                                           */
    int32_t max_rows;            /* R: rows (passes) per tile, 1 .. 32 [20]                                                                                    */
    int32_t skip_above;          /* a tile is selected iff the sum of its qual bytes < skip_above x its length, 0 .. 94 [45]: 0 selects none, 94 all           */
    int32_t reserved;            /* must be 0                                                                                                                  */
} ccsx_handoff_opts;
typedef struct ccsx_handoff_out {
    int64_t  max_tiles;          /* capacity of the arrays below in tiles (>= 1)                                                                               */
    int32_t *counts;             /* [2] tiles of the batch, tiles selected (may exceed max_tiles: the tiles g >= max_tiles are not written)                    */
    int32_t *tile_zmw;           /* [max_tiles] ZMW index of slot g                                                                                            */
    int32_t *tile_start;         /* [max_tiles] first consensus position of the tile                                                                           */
    int32_t *tile_len;           /* [max_tiles] its length (<= T; only a ZMW's last tile is shorter)                                                           */
    int32_t *tile_qsum;          /* [max_tiles] sum of the qual bytes of its positions                                                                         */
    int32_t *tile_rows;          /* [max_tiles] min(R, valid passes of the ZMW)                                                                                */
    uint8_t *row_pass;           /* [max_tiles][R] the row's pass (index within the ZMW), 255 = no such row                                                    */
    uint8_t *row_strand;         /* [max_tiles][R] 0 = the strand of SEQ, 1 = the opposite strand (0 where there is no row)                                    */
    uint8_t *cells;              /* [max_tiles][R][T][4] (base, pw, ip, ins): base 0-3, 4 = no base of the pass on the column, 5 = no segment / row / column   */
} ccsx_handoff_out;
typedef struct ccsx_handoff_request {
    const ccsx_handoff_opts *opts;       /* NULL = ccsx_handoff_opts_default                                                                                     */
    const ccsx_handoff_out  *out;
    int64_t                  reserved[2];    /* must be 0                                                                                                        */
} ccsx_handoff_request;
void        ccsx_handoff_opts_default(ccsx_handoff_opts *o);
int         ccsx_handoff_rule_version(void);
int         ccsx_consensus_handoff(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const ccsx_requests *rq, const ccsx_handoff_request *ho);
int         ccsx_submit_handoff(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const ccsx_requests *rq, const ccsx_handoff_request *ho, ccsx_ticket *ticket);

/* ---- polisher hand-back (docs/faq/revio.md:35-51, steps 2 and 3: the refined windows are merged into the consensus, the read quality is calculated from the
 * merged per-base values, and Arrow runs once more, for QVs only; the rule: DESIGN.md §2 "Polisher hand-back", its own version ccsx_refine_rule_version).  The
 * second polisher's answer is a list of replace-intervals ("tiles") on the consensus of an earlier run, `base`: k_refine_check, k_refine_plan and k_refine_splice
 * splice them into the base sequence on the device, where k_draft_in of the same ticket finds a caller's draft, and the polish seam scores the result with
 * CCSX_QV_ONLY.  `res` is byte for byte what ccsx_polish_batch(h, b, drafts, res, CCSX_QV_ONLY) returns for drafts holding the spliced sequences, their lengths
 * and backbone[z]; res->rq is that run's own.  The read quality of the merged values, the codes and — when asked — the merged quals come back in the report.
 * Integers only except the one division of rq_merged; the same inputs give the same bytes on every run.
 *   b         the passes the base consensus was made from (staged again, as by ccsx_submit_polish)
 *   base      host arrays in the capacity layout of b (ccsx_result_layout); only seq_off, seq_len, seq and qual are read
 *   backbone  [n_zmw], host: per ZMW a pass that has the orientation of SEQ (ccsx_drafts.backbone; any hand-off row with row_strand 0 names one in row_pass);
 *             < 0 leaves the ZMW out (code SKIPPED)
 * The list of tiles must be nondecreasing in tile_zmw with every tile_zmw in [0, n_zmw); the tiles of a ZMW must be in increasing order and disjoint.  Tiles need
 * not coincide with the hand-off's tiling.  Every array of ccsx_refine_tiles may be host memory (page-locked preferred) or memory of the handle's device: each is
 * copied with hipMemcpyDefault on the upload stream; they, base and backbone belong to the ticket and stay valid until it is retired.  A ZMW with a negative code
 * has none of its tiles applied.  Errors of the call (nothing is enqueued, the handle stays usable): NULL arguments or report arrays, n_tiles < 0 or above 2^26,
 * stride outside 1 .. 256, n_tiles > 0 with a NULL tile array, nonzero reserved words, base or res not in the capacity layout of b.
 *   ccsx_refine_batch   synchronous: ccsx_submit_refine + ccsx_wait, as ccsx_polish_batch.
 *   ccsx_submit_refine  ticketed like ccsx_submit_polish.                                                                                                      */
#define CCSX_REFINE_SKIPPED        0   /* base.seq_len <= 0, or backbone < 0; the ZMW's tiles are ignored; refined draft of length 0                             */
#define CCSX_REFINE_RESCORED       1   /* no tile: the base sequence                                                                                            */
#define CCSX_REFINE_REFINED        2   /* every tile applied                                                                                                    */
#define CCSX_REFINE_BAD_TILE     (-1)  /* a tile with start < 0, len < 1, start + len > L, new_len < 0 or new_len > stride: the base sequence                   */
#define CCSX_REFINE_BAD_ORDER    (-2)  /* a tile that starts before its predecessor in the ZMW ends: the base sequence                                          */
#define CCSX_REFINE_BAD_SYMBOL   (-3)  /* a code > 3 or a qual > 93 among the first new_len entries of a tile: the base sequence                                */
#define CCSX_REFINE_TOO_LONG     (-4)  /* the spliced length exceeds the ZMW's slot: the base sequence                                                          */
#define CCSX_REFINE_EMPTY        (-5)  /* the spliced length is below 1: the base sequence                                                                      */
#define CCSX_REFINE_BAD_BACKBONE (-6)  /* backbone >= the ZMW's passes: refined draft of length 0                                                               */
#define CCSX_REFINE_BAD_LIST     (-7)  /* the list breaks its order somewhere (counts[2] > 0): no tile is applied anywhere, the base sequence                   */
typedef struct ccsx_refine_tiles {
    int64_t  n_tiles;            /* >= 0                                                                                                                       */
    int32_t  stride;             /* U: entries per row of new_seq / new_qual, 1 .. 256 [128]                                                                   */
    int32_t  reserved0;          /* must be 0                                                                                                                  */
    int32_t *tile_zmw;           /* [n_tiles]                                                                                                                  */
    int32_t *tile_start;         /* [n_tiles] first replaced position of the base sequence                                                                     */
    int32_t *tile_len;           /* [n_tiles] replaced positions (>= 1)                                                                                        */
    int32_t *new_len;            /* [n_tiles] replacement length, 0 .. U                                                                                       */
    uint8_t *new_seq;            /* [n_tiles][U] codes 0 .. 3; only the first new_len[g] entries of a row are read                                             */
    uint8_t *new_qual;           /* [n_tiles][U] phred 0 .. 93, likewise                                                                                       */
    int64_t  reserved[2];        /* must be 0                                                                                                                  */
} ccsx_refine_tiles;
typedef struct ccsx_refine_report {  /* host memory, complete when the ticket is retired                                                                       */
    int32_t *counts;             /* [3] ZMWs with code REFINED, tiles applied, list-order violations                                                           */
    int32_t *code;               /* [n_zmw] CCSX_REFINE_*                                                                                                      */
    int32_t *n_applied;          /* [n_zmw] tiles applied                                                                                                      */
    int32_t *new_len;            /* [n_zmw] length of the refined draft                                                                                        */
    float   *rq_merged;          /* [n_zmw] 1 - mean error probability of the merged quals (0 for a draft of length 0)                                         */
    uint8_t *qual_merged;        /* [seq_capacity] or NULL: the merged quals at seq_off[z], new_len[z] bytes; bytes beyond are unspecified                      */
} ccsx_refine_report;
void        ccsx_refine_tiles_init(ccsx_refine_tiles *t);   /* zeroes, stride 128 */
int         ccsx_refine_rule_version(void);
uint64_t    ccsx_refine_perr(int32_t q);                    /* round(10^(-q / 10) x 2^32) for q = 0 .. 93, else 0 */
int         ccsx_refine_batch(ccsx_handle h, const ccsx_batch *b, const ccsx_results *base, const int32_t *backbone, const ccsx_refine_tiles *tiles,
                              ccsx_results *res, ccsx_refine_report *report);
int         ccsx_submit_refine(ccsx_handle h, const ccsx_batch *b, const ccsx_results *base, const int32_t *backbone, const ccsx_refine_tiles *tiles,
                               ccsx_results *res, ccsx_refine_report *report, ccsx_ticket *ticket);

/* ---- pass orientation (docs/faq/mode-by-strand.md:16-18: the orientation of the reads "with respect to the one closest to the median length"; the rule:
 * DESIGN.md §2 "Pass orientation", its own version ccsx_orient_rule_version).  Opt-in per pass: flags bit 3 (CCSX_PASS_STRAND_UNKNOWN).  k_orient runs first in
 * the draft stage of every batch that carries the bit, on every path that stages a batch (the fused forms, the draft and polish seams, ccsx_hd_batch,
 * ccsx_train_batch): it votes every 13-mer position of a flagged pass, forward and reverse-complemented, against the exact set of the anchor's 13-mers, and writes
 * the resolved bit 0 (bit 3 cleared) where every later kernel reads it.  Integer counts only.  A batch without the bit launches nothing and is byte for byte
 * what it was.
 *   ccsx_orient_batch      the seam: synchronous, slot 0: upload, k_orient, the report's download — for callers that need the strands on the host before they
 *                          build batches.  opts NULL = ccsx_orient_opts_default.  ccsx_run / ccsx_download refuse slot 0 until the next ccsx_upload.
 *   ccsx_set_orient_opts   the options of every other path (NULL = the defaults), from the next staged batch on.
 *   ccsx_stage_orient      the report of the last synchronous run on slot 0 (as ccsx_stage_align_ev): what k_orient wrote, or every pass GIVEN with its own bit 0
 *                          when the batch carried no bit 3.
 * A NULL report, a report sized for another batch or options out of range are errors of the call: nothing is enqueued.                                         */
typedef struct ccsx_orient_opts {
    int32_t min_votes;           /* SAME / OPPOSITE: the winning orientation has at least this many votes (>= 1)                                               */
    int32_t ratio;               /* ... and at least ratio times the votes of the other one (2 .. 16)                                                          */
} ccsx_orient_opts;
enum ccsx_orient_call { CCSX_ORIENT_GIVEN = 0, CCSX_ORIENT_ANCHOR = 1, CCSX_ORIENT_SAME = 2, CCSX_ORIENT_OPPOSITE = 3, CCSX_ORIENT_UNDETERMINED = 4,
                        CCSX_ORIENT_NO_ANCHOR = 5 };
typedef struct ccsx_orient_report {
    int32_t  n_reads;
    uint8_t *strand;             /* [n_reads] the resolved bit 0                                                                                                */
    uint8_t *call;               /* [n_reads] enum ccsx_orient_call                                                                                             */
    int32_t *votes_same;         /* [n_reads] positions of the pass whose 13-mer is among the anchor's; 0 for GIVEN, ANCHOR and NO_ANCHOR                       */
    int32_t *votes_opp;          /* [n_reads] ... whose reverse-complemented 13-mer is                                                                          */
} ccsx_orient_report;
void        ccsx_orient_opts_default(ccsx_orient_opts *o);
int         ccsx_orient_rule_version(void);
int         ccsx_orient_batch(ccsx_handle h, const ccsx_batch *b, const ccsx_orient_opts *opts, ccsx_orient_report *out);
int         ccsx_set_orient_opts(ccsx_handle h, const ccsx_orient_opts *opts);
int         ccsx_stage_orient(ccsx_handle h, ccsx_orient_report *out);

/* ---- barcode calls (the rule: DESIGN.md §2 "Barcode calls", its own version ccsx_barcode_rule_version; the reference leaves demultiplexing to a separate CPU
 * tool, docs/faq/sqiie.md:104-105; no result of the consensus changes).  k_barcode looks for every barcode of a caller-supplied set at both ends of a read's final
 * consensus by unit-cost edit distance (semi-global, bit-parallel): end 0 is the first min(L, window) bases of the read, end 1 the first min(L, window) bases of
 * its reverse complement, so a barcode at the tail is given as it reads on the opposite strand.  Per end: the barcode of smallest distance (ties: the smallest
 * index), its distance, the smallest prefix of the window that attains it (clip), and the smallest distance of any other barcode (255 with a set of one).  An end
 * is called iff dist <= floor(m * max_dist_pct / 100) and second - dist >= min_margin, m the length of its barcode.  Integers only.  Detection only: nothing is
 * clipped, and every result byte equals the same call without the request.
 *   ccsx_barcode_reads_host  the rule on the calling thread, without a device: the reference of the tests.
 *   ccsx_barcode_reads       k_barcode on caller-supplied reads (HiFi reads from anywhere).  Synchronous.  It uses buffers of the handle's own and the polish stream:
 *                            no slot is staged or recycled (slot 0 and every ticket stay as they are, ccsx_run / ccsx_download keep working), and the call returns
 *                            after the tickets in flight have left the polish stream.
 *   ccsx_consensus_barcodes  synchronous (slot 0), as ccsx_consensus_requests: k_barcode runs on the polish stream after k_stitch, on res->seq / res->seq_len as they
 *                            are on the device.
 *   ccsx_submit_barcodes     ticketed like ccsx_submit_requests: the report's arrays follow the lifetime rule of `res` and should be page-locked; the request, set
 *                            and options structs are read during the call only (every ticket carries its own set and options).
 * rq may be NULL or carry any member of ccsx_requests.  The request is not combined with ccsx_handoff_request or ccsx_hd_request: no entry point takes both.
 * The two ccsx_barcode_reads forms: opts NULL = ccsx_barcode_opts_default; read z is the seq_len[z] codes 0 .. 3 at seq + seq_off[z] (only the low two bits of a byte are
 * read); seq_len[z] <= 0: untested.  Errors of the call (nothing is enqueued, reserved or launched): a null argument, n_barcodes outside 1 .. CCSX_BARCODE_MAX, a
 * length outside 8 .. 64, a code above 3, options out of range, a nonzero reserved word, a report sized for another batch (n_zmw != n) or with a NULL array, n < 0,
 * a negative seq_off.  Without a request nothing of it is launched, reserved or copied.                                                                        */
#define CCSX_BARCODE_MAX        384
#define CCSX_BARCODE_MIN_LEN    8
#define CCSX_BARCODE_MAX_LEN    64
#define CCSX_BARCODE_MAX_WINDOW 1024
typedef struct ccsx_barcode_opts {
    int32_t window;              /* bases of either end that are searched, 8 .. 1024 [64]                                                                        */
    int32_t max_dist_pct;        /* an end is called at up to floor(m * max_dist_pct / 100) edits, 0 .. 30 [15]                                                  */
    int32_t min_margin;          /* ... and when every other barcode is at least this many edits worse, 0 .. 64 [1]                                              */
} ccsx_barcode_opts;
typedef struct ccsx_barcode_set {
    int32_t n_barcodes;          /* 1 .. CCSX_BARCODE_MAX                                                                                                        */
    int32_t len[CCSX_BARCODE_MAX];                         /* CCSX_BARCODE_MIN_LEN .. CCSX_BARCODE_MAX_LEN; lengths may differ within a set                      */
    uint8_t seq[CCSX_BARCODE_MAX][CCSX_BARCODE_MAX_LEN];   /* codes 0 .. 3 (A C G T)                                                                             */
} ccsx_barcode_set;
typedef struct ccsx_barcode_report {
    int32_t  n_zmw;
    int32_t *tested;             /* [n_zmw] 1: seq_len > 0; 0: untested (idx -1, dist / second 255, clip 0, call 0, bq -1)                                        */
    int32_t *call;               /* [n_zmw] bit 0: end 0 (the head) is called, bit 1: end 1 (the tail)                                                            */
    int32_t *bq;                 /* [n_zmw] min over the called ends of floor(100 * (m - dist) / m); -1 without a called end                                      */
    int32_t *idx;                /* [n_zmw][2] per end: the barcode of smallest dist (ties: the smallest index)                                                   */
    int32_t *dist;               /* [n_zmw][2] its edit distance to the best substring of the window                                                             */
    int32_t *second;             /* [n_zmw][2] the smallest dist of any other barcode; 255 when n_barcodes == 1                                                   */
    int32_t *clip;               /* [n_zmw][2] the smallest j such that a substring ending at window position j attains dist                                      */
} ccsx_barcode_report;
typedef struct ccsx_barcode_request {
    const ccsx_barcode_opts *opts;       /* NULL = ccsx_barcode_opts_default                                                                                     */
    const ccsx_barcode_set  *set;
    ccsx_barcode_report     *report;
    int32_t                  reserved[2];   /* must be 0                                                                                                         */
} ccsx_barcode_request;
void        ccsx_barcode_opts_default(ccsx_barcode_opts *o);
int         ccsx_barcode_rule_version(void);
int         ccsx_barcode_reads_host(const ccsx_barcode_set *set, const ccsx_barcode_opts *opts, const uint8_t *seq, const int64_t *seq_off, const int32_t *seq_len,
                                    int32_t n, ccsx_barcode_report *report);
int         ccsx_barcode_reads(ccsx_handle h, const ccsx_barcode_set *set, const ccsx_barcode_opts *opts, const uint8_t *seq, const int64_t *seq_off,
                               const int32_t *seq_len, int32_t n, ccsx_barcode_report *report);
int         ccsx_consensus_barcodes(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const ccsx_requests *rq, const ccsx_barcode_request *bc);
int         ccsx_submit_barcodes(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const ccsx_requests *rq, const ccsx_barcode_request *bc, ccsx_ticket *ticket);

/* ---- representative reads (the rule: DESIGN.md §2 "Representative rule", its own version ccsx_represent_rule_version; the reference's --all mode,
 * docs/faq/mode-all.md:13-37: no productive ZMW is lost).  A ZMW that does not end in a polished consensus gets a representative sequence in the result planes
 * instead of seq_len 0: its final draft, or one of its subreads unaltered.  k_represent runs on the polish stream after k_stitch, before the download.  Per ZMW the
 * class is the first of these that holds (nall: its passes after the top_passes cut; nfull: those without flag bit 1; st: its final status; Ld: the length of the
 * final draft, the one k_polish is given):
 *   POLISHED  st is SUCCESS or LOW_RQ.  Nothing of the ZMW is touched.
 *   NONE      nall == 0, or st is TOO_SHORT or TOO_LONG (or a draft longer than its slot: never truncated).  Nothing of the ZMW is touched.
 *   DRAFT     Ld > 0, st is not TOO_FEW_PASSES, subread_fallback == 0: seq = the draft.
 *   SUBREAD   everything else: seq = a pass in native orientation (low two bits of its bytes), whatever its strand flag — of the full-length passes when
 *             nfull >= 1, else of all nall passes, the one of rank floor(|C| / 2) in (length, index within the ZMW) order.
 * Written for a DRAFT or SUBREAD ZMW, and nothing else: seq_len, seq, qual = 10 and raw_qv = 10.0 for every base, rq = -1, ec = 0; with `kinetics`, for a SUBREAD
 * ZMW, fi / fp = the pass's ipd / pw codes unaltered (ri / rp are not written; a DRAFT ZMW gets no kinetics).  status, np, fn, rn, iters and n_windows stay as
 * the engine left them: the status says why the ZMW was not polished.  Every byte of a POLISHED or NONE ZMW equals the same call without the request.
 *   ccsx_represent_host       the rule on the calling thread, without a device, on a results struct that holds a finished run (status as given, the drafts as
 *                             given: draft z is draft_len[z] codes at draft_seq + draft_off[z]); res->seq_off must be the capacity layout (ccsx_result_layout).
 *                             The reference of the tests.
 *   ccsx_consensus_represent  synchronous (slot 0), as ccsx_consensus_requests.
 *   ccsx_submit_represent     ticketed like ccsx_submit_requests: the report's arrays follow the lifetime rule of `res` and should be page-locked; the request
 *                             struct is read during the call only (every ticket carries its own flags).
 * rq may be NULL or carry any member of ccsx_requests except a coverage request with a gate (statuses 11 .. 14 are not combined with this request).  It is not
 * combined with ccsx_hd_request, ccsx_handoff_request or ccsx_barcode_request: no entry point takes both.  Errors of the call (nothing is enqueued, reserved or
 * launched): a null request or report, a report sized for another batch or with a NULL array, a nonzero reserved word, a flag other than 0 / 1, `kinetics`
 * without opts.hifi_kinetics or without batch.ipd.  Without a request nothing of it is launched, reserved or copied.                                          */
enum ccsx_represent_class { CCSX_REPRESENT_POLISHED = 0, CCSX_REPRESENT_NONE = 1, CCSX_REPRESENT_DRAFT = 2, CCSX_REPRESENT_SUBREAD = 3 };
typedef struct ccsx_represent_report {
    int32_t  n_zmw;
    int32_t *cls;                /* [n_zmw] enum ccsx_represent_class                                                                                            */
    int32_t *pass;               /* [n_zmw] SUBREAD: the representative pass, index within the ZMW; -1 otherwise                                                 */
} ccsx_represent_report;
typedef struct ccsx_represent_request {
    int32_t                subread_fallback;   /* 1: a ZMW that would be DRAFT is SUBREAD (the reference's --subread-fallback); 0 / 1                              */
    int32_t                kinetics;           /* 1: SUBREAD ZMWs get fi / fp (the reference's --all-kinetics); needs opts.hifi_kinetics and batch.ipd; 0 / 1      */
    ccsx_represent_report *report;
    int32_t                reserved[2];        /* must be 0                                                                                                        */
} ccsx_represent_request;
int         ccsx_represent_rule_version(void);
int         ccsx_represent_host(const ccsx_batch *b, const ccsx_opts *opts, const int32_t *status, const uint8_t *draft_seq, const int64_t *draft_off,
                                const int32_t *draft_len, const ccsx_represent_request *req, ccsx_results *res);
int         ccsx_consensus_represent(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const ccsx_requests *rq, const ccsx_represent_request *rep);
int         ccsx_submit_represent(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const ccsx_requests *rq, const ccsx_represent_request *rep,
                                  ccsx_ticket *ticket);

/* ---- segmentation of concatenated-array reads (the rule: DESIGN.md §2 "Segment rule", its own version ccsx_segment_rule_version; this build's own, the
 * reference documents none of it, as it documents none of the barcode calls; no result of the consensus changes).  A read of such a library is
 * A0 S1 A1 S2 .. SK AK or the reverse complement of the whole: A0 .. AK are the adapters of a caller-supplied ordered set, S1 .. SK the segments.  k_segment looks
 * for every adapter and its reverse complement over the whole read by unit-cost edit distance (search 2a: adapter a as given, search 2a + 1: its reverse
 * complement; a hit is what ccsx_adapter_hit defines, at up to floor(m * max_dist_pct / 100) edits), orders the hits by (dist, start, search, end), takes a hit
 * iff it intersects no hit taken before (the cuts), and classifies the pieces between neighbouring cuts: a piece of at least min_len bases between searches 2a
 * and 2(a + 1) is segment a, forward; one between searches 2(a + 1) + 1 and 2a + 1 is segment a, reverse; every other piece of positive length, the read's head
 * and tail included, is leftover.  More than CCSX_SEGMENT_MAX_HITS hits: overflow, no cuts and no segments.  Integers only.  Detection only: nothing is cut.
 *   ccsx_segment_reads_host  the rule on the calling thread, without a device: the reference of the tests.
 *   ccsx_segment_reads       k_segment on caller-supplied reads (HiFi reads from anywhere).  Synchronous.  It uses buffers of the handle's own and the polish stream:
 *                            no slot is staged or recycled, and the call returns after the tickets in flight have left the polish stream (as ccsx_barcode_reads).
 *   ccsx_consensus_segments  synchronous (slot 0), as ccsx_consensus_requests: k_segment runs on the polish stream after k_stitch, on res->seq / res->seq_len as they
 *                            are on the device.
 *   ccsx_submit_segments     ticketed like ccsx_submit_requests: the report's arrays follow the lifetime rule of `res` and should be page-locked; the request, set
 *                            and options structs are read during the call only (every ticket carries its own set and options).
 * rq may be NULL or carry any member of ccsx_requests.  The request is not combined with ccsx_hd_request, ccsx_handoff_request, ccsx_barcode_request or
 * ccsx_represent_request: no entry point takes both.  The two ccsx_segment_reads forms: opts NULL = ccsx_segment_opts_default; reads as for ccsx_barcode_reads.
 * Errors of the call (nothing is enqueued, reserved or launched): a null argument, n_adapters outside 2 .. CCSX_SEGMENT_MAX_ADAPTERS, a length outside 8 .. 64,
 * a code above 3, options out of range, a nonzero reserved word, a report sized for another batch (n_zmw != n) or with a NULL array, n < 0, a negative seq_off.
 * Without a request nothing of it is launched, reserved or copied.  ccsx_segment_chunk: the bases of one item of k_segment (the tests place hits at its edges). */
#define CCSX_SEGMENT_MAX_ADAPTERS 33
#define CCSX_SEGMENT_MIN_LEN      8
#define CCSX_SEGMENT_MAX_LEN      64
#define CCSX_SEGMENT_MAX_HITS     64
#define CCSX_SEGMENT_MAX_PIECES   64
typedef struct ccsx_segment_opts {
    int32_t max_dist_pct;        /* an adapter of m bases hits at up to floor(m * max_dist_pct / 100) edits, 0 .. 30 [15]                                        */
    int32_t min_len;             /* a piece shorter than this is no segment, 1 .. 65535 [50]                                                                     */
} ccsx_segment_opts;
typedef struct ccsx_segment_set {
    int32_t n_adapters;          /* 2 .. CCSX_SEGMENT_MAX_ADAPTERS, in array order                                                                               */
    int32_t len[CCSX_SEGMENT_MAX_ADAPTERS];                            /* CCSX_SEGMENT_MIN_LEN .. CCSX_SEGMENT_MAX_LEN; lengths may differ within a set          */
    uint8_t seq[CCSX_SEGMENT_MAX_ADAPTERS][CCSX_SEGMENT_MAX_LEN];      /* codes 0 .. 3 (A C G T)                                                                 */
} ccsx_segment_set;
typedef struct ccsx_segment_piece {
    int32_t start, end;          /* the segment is read[start, end): between its two cuts                                                                        */
    uint8_t index;               /* a: the segment between adapters a and a + 1                                                                                  */
    uint8_t reverse;             /* 0: as the set reads (adapter a on its left); 1: reverse complemented (adapter a + 1 on its left)                             */
    uint8_t dist_left, dist_right;   /* the edit distances of the cuts on its left and right                                                                     */
} ccsx_segment_piece;
typedef struct ccsx_segment_report {
    int32_t  n_zmw;
    int32_t *tested;             /* [n_zmw] 1: seq_len > 0; 0: untested (orient -1, everything else 0)                                                            */
    int32_t *overflow;           /* [n_zmw] 1: more than CCSX_SEGMENT_MAX_HITS hits (adapter junk): only tested and n_hits differ from an untested read           */
    int32_t *n_hits;             /* [n_zmw] every hit of every search, not capped                                                                                */
    int32_t *n_cuts;             /* [n_zmw] the hits taken by the selection                                                                                      */
    int32_t *n_segments;         /* [n_zmw]                                                                                                                      */
    int32_t *complete;           /* [n_zmw] 1: one orientation, segments 0 .. n_adapters - 2 each once, in array order                                           */
    int32_t *orient;             /* [n_zmw] -1: no segment; 0: all forward; 1: all reverse; 2: mixed                                                             */
    int32_t *leftover_bases;     /* [n_zmw] the bases of the pieces that are no segment                                                                          */
    ccsx_segment_piece *pieces;  /* [n_zmw][CCSX_SEGMENT_MAX_PIECES] the segments by increasing start; entries beyond n_segments are zero                        */
} ccsx_segment_report;
typedef struct ccsx_segment_request {
    const ccsx_segment_opts *opts;       /* NULL = ccsx_segment_opts_default                                                                                     */
    const ccsx_segment_set  *set;
    ccsx_segment_report     *report;
    int32_t                  reserved[2];   /* must be 0                                                                                                         */
} ccsx_segment_request;
void        ccsx_segment_opts_default(ccsx_segment_opts *o);
int         ccsx_segment_rule_version(void);
int         ccsx_segment_chunk(void);
int         ccsx_segment_reads_host(const ccsx_segment_set *set, const ccsx_segment_opts *opts, const uint8_t *seq, const int64_t *seq_off, const int32_t *seq_len,
                                    int32_t n, ccsx_segment_report *report);
int         ccsx_segment_reads(ccsx_handle h, const ccsx_segment_set *set, const ccsx_segment_opts *opts, const uint8_t *seq, const int64_t *seq_off,
                               const int32_t *seq_len, int32_t n, ccsx_segment_report *report);
int         ccsx_consensus_segments(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const ccsx_requests *rq, const ccsx_segment_request *sg);
int         ccsx_submit_segments(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const ccsx_requests *rq, const ccsx_segment_request *sg, ccsx_ticket *ticket);

/* ---- full-length cDNA reads (the rule: DESIGN.md §2 "cDNA rule", its own version ccsx_cdna_rule_version; this build's own, as the barcode and the segment rule
 * are: the reference leaves primer removal, the poly(A) tail and concatemers to separate CPU tools; no result of the consensus changes).  A cDNA molecule reads
 * 5p . transcript . poly(A) . rc(3p) on the sense strand, or the reverse complement of the whole.  The primers of a caller-supplied set are given as the oligos,
 * each with a role: 0 = 5', 1 = 3'.  k_cdna, per read c[0, L):
 *   ends      the barcode rule over the primers, whatever their role (window, max_dist_pct, min_margin as in ccsx_barcode_opts): idx, dist, second, clip per end.
 *   strand    both ends called with primers of different roles: the role of the head's primer (0: sense; 1: antisense, the transcript is the reverse complement
 *             of the read).  Otherwise strand -1, class NO_PRIMER, ONE_END or SAME_ROLE, and the rule ends: the later planes are 0, first_internal -1.
 *   insert    [clip[0], L - clip[1]) in the read's coordinates, ins_len bases; ins_len < 1: class SHORT and the rule ends in the same way.
 *   poly(A)   over the first K = min(polya_max, ins_len) insert bases counted from the 3' primer, x_k = 1 iff base k is A on the transcript strand:
 *             s_0 = 0, s_k = s_(k-1) + (x_k ? 1 : -polya_mismatch), M_k = max of s_0 .. s_k; k* = the smallest k with M_k - s_k > polya_xdrop (K + 1 without one);
 *             polya_len = the smallest k in [0, k*) that attains the maximum of s over [0, k*).
 *   internal  every primer and its reverse complement over the whole read, hits and starts as the segment rule defines them at floor(m * max_dist_pct / 100)
 *             edits; a hit is internal iff clip[0] <= start and end <= L - clip[1].  n_internal counts them (not capped), first_internal is their smallest start.
 *   class     trimmed = ins_len - polya_len: SHORT if trimmed < min_len, else CONCATEMER if n_internal > 0, else NO_TAIL if min_polya > 0 and polya_len <
 *             min_polya, else FULL_LENGTH.  Classes CONCATEMER .. FULL_LENGTH report the slice without primers and tail, [start, end) in the read's
 *             coordinates: strand 0 [clip[0], L - clip[1] - polya_len), strand 1 [clip[0] + polya_len, L - clip[1]); every other class 0, 0.
 * Integers only.  Detection only: nothing is clipped, and every result byte equals the same call without the request.
 *   ccsx_cdna_reads_host  the rule on the calling thread, without a device: the reference of the tests.
 *   ccsx_cdna_reads       k_cdna on caller-supplied reads (HiFi reads from anywhere).  Synchronous; buffers of the handle's own on the polish stream, no slot is
 *                         staged or recycled (as ccsx_barcode_reads).
 *   ccsx_consensus_cdna   synchronous (slot 0), as ccsx_consensus_requests: k_cdna runs on the polish stream after k_stitch, on res->seq / res->seq_len as they are
 *                         on the device.
 *   ccsx_submit_cdna      ticketed like ccsx_submit_requests: the report's arrays follow the lifetime rule of `res` and should be page-locked; the request, set
 *                         and options structs are read during the call only (every ticket carries its own set and options).
 * rq may be NULL or carry any member of ccsx_requests.  The request is not combined with ccsx_hd_request, ccsx_handoff_request, ccsx_barcode_request,
 * ccsx_segment_request or ccsx_represent_request: no entry point takes both.  The two ccsx_cdna_reads forms: opts NULL = ccsx_cdna_opts_default; reads as for
 * ccsx_barcode_reads.  Errors of the call (nothing is enqueued, reserved or launched): a null argument, n_primers outside 2 .. CCSX_CDNA_MAX_PRIMERS, a role above
 * 1, a set without a primer of each role, a length outside 8 .. 64, a code above 3, options out of range, a nonzero reserved word, a report sized for another batch
 * (n_zmw != n) or with a NULL array, n < 0, a negative seq_off.  Without a request nothing of it is launched, reserved or copied.                              */
#define CCSX_CDNA_MAX_PRIMERS 64
#define CCSX_CDNA_MIN_LEN     8
#define CCSX_CDNA_MAX_LEN     64
enum ccsx_cdna_class { CCSX_CDNA_NO_PRIMER = 0, CCSX_CDNA_ONE_END = 1, CCSX_CDNA_SAME_ROLE = 2, CCSX_CDNA_SHORT = 3, CCSX_CDNA_CONCATEMER = 4,
                       CCSX_CDNA_NO_TAIL = 5, CCSX_CDNA_FULL_LENGTH = 6 };
typedef struct ccsx_cdna_opts {
    int32_t window;              /* bases of either end that are searched for a primer, 8 .. 1024 [64]                                                           */
    int32_t max_dist_pct;        /* a primer of m bases is called, and hits inside the read, at up to floor(m * max_dist_pct / 100) edits, 0 .. 30 [15]           */
    int32_t min_margin;          /* an end is called when every other primer is at least this many edits worse, 0 .. 64 [1]                                      */
    int32_t polya_mismatch;      /* what a base other than A costs the poly(A) scan, 1 .. 8 [3]                                                                  */
    int32_t polya_xdrop;         /* the scan stops when its score lies more than this below its maximum, 0 .. 64 [3]                                             */
    int32_t polya_max;           /* insert bases the scan looks at, 16 .. 4096 [512]                                                                             */
    int32_t min_polya;           /* a read with a shorter tail is NO_TAIL, 0 .. 255; 0: a tail is not required [20]                                               */
    int32_t min_len;             /* a read whose insert without the tail is shorter is SHORT, 1 .. 65535 [50]                                                    */
} ccsx_cdna_opts;
typedef struct ccsx_cdna_set {
    int32_t n_primers;           /* 2 .. CCSX_CDNA_MAX_PRIMERS                                                                                                   */
    int32_t len[CCSX_CDNA_MAX_PRIMERS];                         /* CCSX_CDNA_MIN_LEN .. CCSX_CDNA_MAX_LEN; lengths may differ within a set                       */
    uint8_t role[CCSX_CDNA_MAX_PRIMERS];                        /* 0: a 5' primer, 1: a 3' primer; the set has at least one of each                              */
    uint8_t seq[CCSX_CDNA_MAX_PRIMERS][CCSX_CDNA_MAX_LEN];      /* codes 0 .. 3 (A C G T), the oligo as the vendor's primer file gives it                        */
} ccsx_cdna_set;
typedef struct ccsx_cdna_report {
    int32_t  n_zmw;
    int32_t *tested;             /* [n_zmw] 1: seq_len > 0; 0: untested (cls 0, strand -1, first_internal -1, idx -1, dist / second 255, everything else 0)       */
    int32_t *cls;                /* [n_zmw] enum ccsx_cdna_class                                                                                                 */
    int32_t *strand;             /* [n_zmw] 0: sense, 1: antisense, -1: classes NO_PRIMER, ONE_END, SAME_ROLE                                                    */
    int32_t *start, *end;        /* [n_zmw] the slice of classes CONCATEMER, NO_TAIL and FULL_LENGTH; 0, 0 otherwise                                             */
    int32_t *polya_len;          /* [n_zmw] the poly(A) bases next to the 3' primer                                                                              */
    int32_t *n_internal;         /* [n_zmw] primer hits inside the insert, not capped                                                                            */
    int32_t *first_internal;     /* [n_zmw] the smallest start among them; -1 without one                                                                        */
    int32_t *idx;                /* [n_zmw][2] per end: the primer of smallest dist (ties: the smallest index)                                                   */
    int32_t *dist;               /* [n_zmw][2] its edit distance to the best substring of the window                                                             */
    int32_t *second;             /* [n_zmw][2] the smallest dist of any other primer, of either role                                                             */
    int32_t *clip;               /* [n_zmw][2] the smallest j such that a substring ending at window position j attains dist                                      */
} ccsx_cdna_report;
typedef struct ccsx_cdna_request {
    const ccsx_cdna_opts *opts;          /* NULL = ccsx_cdna_opts_default                                                                                        */
    const ccsx_cdna_set  *set;
    ccsx_cdna_report     *report;
    int32_t               reserved[2];   /* must be 0                                                                                                            */
} ccsx_cdna_request;
void        ccsx_cdna_opts_default(ccsx_cdna_opts *o);
int         ccsx_cdna_rule_version(void);
int         ccsx_cdna_reads_host(const ccsx_cdna_set *set, const ccsx_cdna_opts *opts, const uint8_t *seq, const int64_t *seq_off, const int32_t *seq_len,
                                 int32_t n, ccsx_cdna_report *report);
int         ccsx_cdna_reads(ccsx_handle h, const ccsx_cdna_set *set, const ccsx_cdna_opts *opts, const uint8_t *seq, const int64_t *seq_off,
                            const int32_t *seq_len, int32_t n, ccsx_cdna_report *report);
int         ccsx_consensus_cdna(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const ccsx_requests *rq, const ccsx_cdna_request *cd);
int         ccsx_submit_cdna(ccsx_handle h, const ccsx_batch *b, ccsx_results *res, const ccsx_requests *rq, const ccsx_cdna_request *cd, ccsx_ticket *ticket);

/* ---- duplicate reads (the rule: DESIGN.md §2 "Duplicate rule", its own version ccsx_dup_rule_version; this build's own, as the barcode, the segment and the
 * cDNA rule are: the reference contains no duplicate rule; no result of the consensus changes).  The first analysis that looks across reads.  Integers only.
 *   signature  of a read c[0, L): untested (window = 0, everything but len 0) when L < window.  Otherwise, per end e (end 0: c forwards, end 1: its reverse
 *              complement, as the barcode rule's ends), the first `window` bases packed at 2 bits a base (base j: bits 2 (j % 32) of word j / 32), and the
 *              minimizer: the smallest ccsx_dup_hash(x) over the window - kmer + 1 k-mers x of the end, a k-mer packed with its first base most significant.
 *              ccsx_dup_hash is a bijection of 32-bit words, so equal minimizers are the same k-mer.
 *   bucket     the tested reads of equal key (min(mini[0], mini[1]), max(mini[0], mini[1])): a read and its reverse complement share a key.  A bucket of more
 *              than CCSX_DUP_MAX_BUCKET reads is overflowed: every read of it is reported CCSX_DUP_OVERFLOW and alone.
 *   D(a, b)    of two end windows: the minimum over the last row and the last column of their start-anchored unit-cost edit table,
 *              min(min_q ed(a, b[0, q)), min_p ed(a[0, p), b)).
 *   pair       two reads i, j of one bucket are duplicates iff group[i] == group[j], |Li - Lj| * 100 <= max_len_diff_pct * min(Li, Lj), and with
 *              kmax = window * max_dist_pct / 100 either D(e0i, e0j) <= kmax and D(e1i, e1j) <= kmax (same strand) or D(e0i, e1j) <= kmax and
 *              D(e1i, e0j) <= kmax (opposite strands).
 *   sets       the connected components of the pairs (single linkage).  The representative of a set is its member of largest score, ties: the smallest index.
 * No output depends on the order of anything.
 *   ccsx_dup_sign_reads_host / ccsx_dup_cluster_host   the rule on the calling thread, without a device: the reference of the tests.
 *   ccsx_dup_sign_reads / ccsx_dup_cluster             k_dup_sign; k_dup_keys, a device radix sort, k_dup_buckets and k_dup_verify.  Synchronous, on the polish
 *                                                      stream, in buffers of the handle's own grown on demand: no slot is staged or recycled and tickets in flight
 *                                                      complete untouched (as ccsx_barcode_reads).
 * opts NULL = ccsx_dup_opts_default; reads as for ccsx_barcode_reads (only the low two bits of a byte are read).  group / score NULL: all 0.  Errors of the call
 * (nothing is reserved or launched): a null argument, options out of range, kmer > window, n < 0 or n > CCSX_DUP_MAX_READS, a negative seq_off, a signature
 * whose window is neither 0 nor opts->window, a negative group, a report sized for another n or with a NULL array. */
#define CCSX_DUP_MAX_BUCKET 512
#define CCSX_DUP_MAX_READS  (1 << 24)
#define CCSX_DUP_UNTESTED   0
#define CCSX_DUP_TESTED     1
#define CCSX_DUP_OVERFLOW   2
typedef struct ccsx_dup_opts {
    int32_t window;              /* bases of each end that are compared, 16 .. 64 [32]                                                                           */
    int32_t kmer;                /* the minimizer's k, 8 .. 16 and <= window [12]                                                                                */
    int32_t max_dist_pct;        /* two end windows agree when D <= floor(window * max_dist_pct / 100), 0 .. 30 [10]                                             */
    int32_t max_len_diff_pct;    /* two reads agree in length when |Li - Lj| * 100 <= max_len_diff_pct * min(Li, Lj), 0 .. 20 [2]                                */
} ccsx_dup_opts;
typedef struct ccsx_dup_sig {    /* 48 bytes, no padding: every byte is written                                                                                  */
    uint64_t end[2][2];          /* [end][word]: the window at 2 bits a base; bits past the window are 0                                                         */
    uint32_t mini[2];            /* the minimizer of each end                                                                                                    */
    int32_t  len;                /* L (0 for seq_len <= 0)                                                                                                       */
    int32_t  window;             /* 0: untested; otherwise the window the signature was taken with                                                               */
} ccsx_dup_sig;
typedef struct ccsx_dup_report {
    int32_t  n;
    int32_t *status;             /* [n] CCSX_DUP_UNTESTED, CCSX_DUP_TESTED or CCSX_DUP_OVERFLOW                                                                   */
    int32_t *rep;                /* [n] the representative of the read's set; an untested read, an overflowed one and a singleton report themselves               */
    int32_t *set_size;           /* [n] the reads in the set                                                                                                      */
    int32_t *dup;                /* [n] 1 iff the read is tested and is not its set's representative                                                              */
} ccsx_dup_report;
void        ccsx_dup_opts_default(ccsx_dup_opts *o);
int         ccsx_dup_rule_version(void);
uint32_t    ccsx_dup_hash(uint32_t x);
int         ccsx_dup_sign_reads_host(const ccsx_dup_opts *opts, const uint8_t *seq, const int64_t *seq_off, const int32_t *seq_len, int32_t n, ccsx_dup_sig *sig);
int         ccsx_dup_sign_reads(ccsx_handle h, const ccsx_dup_opts *opts, const uint8_t *seq, const int64_t *seq_off, const int32_t *seq_len, int32_t n,
                                ccsx_dup_sig *sig);
int         ccsx_dup_cluster_host(const ccsx_dup_opts *opts, const ccsx_dup_sig *sig, const int32_t *group, const int32_t *score, int32_t n,
                                  ccsx_dup_report *report);
int         ccsx_dup_cluster(ccsx_handle h, const ccsx_dup_opts *opts, const ccsx_dup_sig *sig, const int32_t *group, const int32_t *score, int32_t n,
                             ccsx_dup_report *report);

/* ---- cell barcodes and UMIs (the rule: DESIGN.md §2 "Cell-tag rule", its own version ccsx_cell_rule_version; this build's own, as the barcode, the segment, the
 * cDNA and the duplicate rule are; no result of the consensus changes and ccsx_cdna_* is untouched).  A single-cell cDNA molecule carries, between one primer and
 * the transcript, a UMI and a cell barcode: T = umi_len + bc_len bases.  A field is packed into a uint32 at 2 bits a base, the first base most significant; fields
 * are read on the strand of the end they adjoin, going away from the primer (the orientation of the oligo primer . field . field).  k_cell, per read c[0, L):
 *   ends      the cDNA rule's ends and strand; a read at which that rule ends there (NO_PRIMER, ONE_END, SAME_ROLE, SHORT) has tag NONE.
 *   tag end   e_t = (strand == side) ? 0 : 1, p0 = clip[e_t]; ins_len < T: class SHORT, tag NONE.
 *   barcode   bc_raw = the bc_len bases of end e_t from p = p0 + (bc_first ? 0 : umi_len).  Without a whitelist or with bc_len 0: tag RAW, bc -1.  A member of the
 *             whitelist: EXACT.  Otherwise the candidates: kind 1, the 3 bc_len substitutions; kind 2 (indels only; the read lost a base), the first bc_len - 1
 *             bases with one base inserted at each of bc_len places; kind 3 (indels and ins_len >= T + 1 only; the read gained a base), bc_raw with one base
 *             deleted and the base at p + bc_len appended.  bc / bc_hi = the smallest / largest whitelist index the candidates reach: none ABSENT (-1, -1),
 *             two or more AMBIGUOUS, one CORRECTED with kind = the smallest kind that reaches it and shift = 0, -1, +1 for kinds 1, 2, 3.  Every status but
 *             CORRECTED has kind 0 and shift 0.
 *   umi       umi_len bases from bc_first ? p0 + bc_len + shift : p0.
 *   the rest  the cDNA rule's poly(A) scan, internal hits, class and slice with clip[e_t] widened by tag_clip = T + shift (ins_len - tag_clip < 1: SHORT).  The
 *             clip planes keep the primers' own clips.
 * A whitelist is a host object, an open-addressing table of uint64 slots (key << 32) | (index + 1), 0 = empty; slots = the smallest power of two >= 2 n and >= 64;
 * the first slot of key x is ccsx_cell_slot(x, slots) = ccsx_dup_hash(x) & (slots - 1), then linear probing.  The device copy belongs to the handle and is uploaded
 * when a call brings a whitelist whose serial differs from the resident one.
 *   ccsx_cell_reads_host  the rule on the calling thread, without a device: the reference of the tests.
 *   ccsx_cell_reads       k_cell on caller-supplied reads.  Synchronous; buffers of the handle's own on the polish stream, no slot is staged or recycled.
 * wl may be NULL (tags RAW).  Errors of the call (nothing is enqueued, reserved or launched): everything ccsx_cdna_reads refuses, a null design, T = 0, a field
 * length outside 0 .. 16, side / bc_first / indels outside 0 .. 1, a nonzero reserved word, a whitelist of another bc_len, a report sized for another batch or with
 * a NULL plane.  ccsx_cell_whitelist_create: codes [n][bc_len] of 0 .. 3; n 1 .. 2^23, bc_len 1 .. 16; NULL and the error set on a null argument, a code above 3,
 * or a duplicate barcode (the message names both indices).  ccsx_cell_whitelist_info: n, bc_len, the number of slots and the table itself, each where the
 * pointer is not NULL (the table lives as long as the whitelist).                                                                                               */
#define CCSX_CELL_MAX_FIELD 16
#define CCSX_CELL_MAX_WHITELIST (1 << 23)
enum ccsx_cell_tag { CCSX_CELL_NONE = 0, CCSX_CELL_RAW = 1, CCSX_CELL_EXACT = 2, CCSX_CELL_CORRECTED = 3, CCSX_CELL_AMBIGUOUS = 4, CCSX_CELL_ABSENT = 5 };
typedef struct ccsx_cell_design {
    int32_t umi_len;             /* 0 .. 16                                                                                                                      */
    int32_t bc_len;              /* 0 .. 16; umi_len + bc_len >= 1                                                                                               */
    int32_t side;                /* 0: the fields adjoin the 5' primer, 1: the 3' primer                                                                          */
    int32_t bc_first;            /* 1: the barcode is the field next to the primer, 0: the UMI is                                                                 */
    int32_t indels;              /* 1: candidates of kinds 2 and 3 are tried [1]                                                                                  */
    int32_t reserved[3];         /* must be 0                                                                                                                    */
} ccsx_cell_design;
typedef struct ccsx_cell_report {
    ccsx_cdna_report cdna;       /* the cDNA planes (cdna.n_zmw sizes the whole report); clip: the primers' own                                                   */
    int32_t  *tag;               /* [n_zmw] enum ccsx_cell_tag                                                                                                   */
    uint32_t *bc_raw;            /* [n_zmw] the barcode field as read; 0 with tag NONE or bc_len 0                                                               */
    int32_t  *bc, *bc_hi;        /* [n_zmw] the smallest and the largest whitelist index reached; -1 without one                                                  */
    int32_t  *kind, *shift;      /* [n_zmw] of a CORRECTED read; 0 otherwise                                                                                      */
    uint32_t *umi;               /* [n_zmw] the UMI field; 0 with tag NONE or umi_len 0                                                                           */
    int32_t  *tag_clip;          /* [n_zmw] T + shift, what the tag end's clip was widened by; 0 with tag NONE                                                    */
} ccsx_cell_report;
typedef struct ccsx_cell_whitelist ccsx_cell_whitelist;
void        ccsx_cell_design_default(ccsx_cell_design *d);       /* 12 U, 16 B, the 3' side, the barcode next to the primer, indels                               */
int         ccsx_cell_rule_version(void);
uint32_t    ccsx_cell_slot(uint32_t key, uint32_t slots);
ccsx_cell_whitelist *ccsx_cell_whitelist_create(const uint8_t *codes, int32_t n, int32_t bc_len);
void        ccsx_cell_whitelist_destroy(ccsx_cell_whitelist *wl);
int         ccsx_cell_whitelist_info(const ccsx_cell_whitelist *wl, int32_t *n, int32_t *bc_len, uint32_t *slots, const uint64_t **table);
int         ccsx_cell_reads_host(const ccsx_cdna_set *set, const ccsx_cdna_opts *opts, const ccsx_cell_design *design, const ccsx_cell_whitelist *wl,
                                 const uint8_t *seq, const int64_t *seq_off, const int32_t *seq_len, int32_t n, ccsx_cell_report *report);
int         ccsx_cell_reads(ccsx_handle h, const ccsx_cdna_set *set, const ccsx_cdna_opts *opts, const ccsx_cell_design *design, const ccsx_cell_whitelist *wl,
                            const uint8_t *seq, const int64_t *seq_off, const int32_t *seq_len, int32_t n, ccsx_cell_report *report);

/* ---- BGZF inflate on the device (the rule: DESIGN.md §2 "BGZF inflate", its own version ccsx_inflate_rule_version; nothing of the consensus changes).  A BGZF
 * block is an independent raw DEFLATE stream (RFC 1951) of at most 64 KiB of output: k_inflate decodes one stream per wave.  An inflater is its own object: its
 * own non-blocking stream, device buffers and page-locked staging; it shares nothing with a ccsx_handle and may run beside one.  It is not thread-safe: one
 * inflater per caller thread.  Two calls may be in flight (ccsx_inflate_submit / ccsx_inflate_wait); tickets complete in order.
 *   blocks[i]   in_off / in_len: the raw DEFLATE payload in src (the caller strips BGZF's header — 18 bytes as htslib writes it — and the 8-byte trailer);
 *               out_off / out_len: where its bytes go in dst; out_len (the trailer's ISIZE) <= CCSX_INFLATE_MAX_OUT.
 *   status[i]   enum ccsx_inflate_status.  A corrupt block is never an error of the call (as a failed ZMW is not, elsewhere in this ABI): the other blocks of the
 *               call are inflated.  The bytes of dst[out_off, out_off + out_len) of a block whose status is not OK are unspecified; no byte of dst outside the
 *               blocks' output ranges is written.  CRC32 stays with the caller.
 * Argument errors (< 0, ccsx_last_error) fail the call before anything is enqueued: a null argument, a block outside src or dst, overlapping output ranges,
 * out_len > CCSX_INFLATE_MAX_OUT, src_len / dst_len / n_blocks beyond the inflater's capacities, two tickets already in flight.
 * src and dst may be any host memory: the library copies through its own page-locked staging (a page-locked src / dst makes that host copy faster, nothing else).
 * src, blocks, dst and status must stay valid until the ticket is waited for.
 * The stream's priority is the device's lowest by default (CCSX_INFLATE_PRIO=high|low|none overrides; DESIGN.md §7 has the measurement).
 * ccsx_inflate_blocks_host runs the same decoder (inflate_core.h) on the calling thread, without a device: the reference of the tests.                        */
#define CCSX_INFLATE_MAX_OUT 65536
#ifndef CCSX_INFLATE_STATUS_DEFINED
#define CCSX_INFLATE_STATUS_DEFINED
enum ccsx_inflate_status {
    CCSX_INFLATE_OK                = 0,
    CCSX_INFLATE_TRUNCATED_INPUT   = 1,  /* the stream needs bits beyond in_len                                              */
    CCSX_INFLATE_BAD_BLOCK_TYPE    = 2,  /* BTYPE 3                                                                          */
    CCSX_INFLATE_BAD_STORED_LENGTH = 3,  /* LEN != ~NLEN                                                                     */
    CCSX_INFLATE_BAD_CODE_LENGTHS  = 4,  /* over- or under-subscribed code (except zlib's `max == 1` rule: a literal / length or a distance
                                            code of exactly one 1-bit codeword passes, its unused codeword reads as BAD_SYMBOL; the
                                            code-length code is strict), a repeat without a previous length or past the end, more than
                                            286 / 30 codes, no end-of-block code                                               */
    CCSX_INFLATE_BAD_SYMBOL        = 5,  /* a code that stands for no symbol (litlen 286/287, distance 30/31, unassigned)     */
    CCSX_INFLATE_BAD_DISTANCE      = 6,  /* a match reaches before the start of this stream's output                         */
    CCSX_INFLATE_OUTPUT_OVERRUN    = 7,  /* the stream holds more than out_len bytes                                          */
    CCSX_INFLATE_OUTPUT_SHORT      = 8   /* the final block ended before out_len bytes                                        */
};
#endif
typedef struct ccsx_inflater_s *ccsx_inflater;
typedef struct ccsx_deflate_block { int64_t in_off; int32_t in_len; int32_t out_len; int64_t out_off; } ccsx_deflate_block;
int         ccsx_inflate_rule_version(void);
int         ccsx_inflater_create(int device, int64_t max_in_bytes, int64_t max_out_bytes, int32_t max_blocks, ccsx_inflater *out);
int         ccsx_inflater_destroy(ccsx_inflater f);
int         ccsx_inflate_blocks(ccsx_inflater f, const uint8_t *src, int64_t src_len, const ccsx_deflate_block *blocks, int32_t n_blocks,
                                uint8_t *dst, int64_t dst_len, int32_t *status);                        /* synchronous: submit + wait */
int         ccsx_inflate_submit(ccsx_inflater f, const uint8_t *src, int64_t src_len, const ccsx_deflate_block *blocks, int32_t n_blocks,
                                uint8_t *dst, int64_t dst_len, int32_t *status, ccsx_ticket *ticket);
int         ccsx_inflate_wait(ccsx_inflater f, ccsx_ticket ticket);
int         ccsx_inflate_blocks_host(const uint8_t *src, int64_t src_len, const ccsx_deflate_block *blocks, int32_t n_blocks,
                                     uint8_t *dst, int64_t dst_len, int32_t *status);

/* ---- BGZF deflate on the device (the rule: DESIGN.md §2 "BGZF deflate", its own version ccsx_deflate_rule_version; nothing of the consensus changes).  The other
 * half of the inflater: a span of at most CCSX_DEFLATE_MAX_IN plain bytes becomes one raw DEFLATE stream (RFC 1951, the payload of a BGZF block) and its CRC32
 * (zlib polynomial, what the BGZF trailer holds): k_deflate encodes one span per workgroup.  The stream and the CRC are a pure function of the span's bytes and
 * the rule version: the device and ccsx_deflate_spans_host give the same bytes.  A deflater is its own object: its own non-blocking stream, device buffers and
 * page-locked staging; it shares nothing with a ccsx_handle or an inflater and may run beside them.  It is not thread-safe.  Two calls may be in flight
 * (ccsx_deflate_submit / ccsx_deflate_wait); tickets complete in order.
 *   spans[i]    in_off / in_len: the plain bytes in src, in_len <= CCSX_DEFLATE_MAX_IN; out_off / out_cap: where the stream goes in dst and how long it may be.
 *               ccsx_deflate_bound(in_len) is an out_cap that is never too small: the length of the stored form.
 *   out_len[i]  the stream's bytes; crc[i] the CRC32 of the span's plain bytes (set whatever the status).
 *   status[i]   enum ccsx_deflate_status.  A span whose stream does not fit its out_cap is OUTPUT_FULL, never an error of the call: its out_len is 0 and the bytes
 *               of its output range are unspecified.  No byte of dst outside the spans' output ranges is written.
 * Argument errors (< 0, ccsx_last_error) fail the call before anything is enqueued: a null argument, a span outside src or dst, overlapping output ranges,
 * in_len > CCSX_DEFLATE_MAX_IN, src_len / dst_len / n_spans beyond the deflater's capacities, two tickets already in flight.
 * src, spans, dst, out_len, crc and status must stay valid until the ticket is waited for.
 * ccsx_deflate_spans_host runs the same encoder (deflate_core.h) on the calling thread, without a device: the reference of the tests.  ccsx_deflate_crc is the
 * rule's CRC alone, on the host, for any length.                                                                                                              */
#define CCSX_DEFLATE_MAX_IN 65536
#ifndef CCSX_DEFLATE_STATUS_DEFINED
#define CCSX_DEFLATE_STATUS_DEFINED
enum ccsx_deflate_status {
    CCSX_DEFLATE_OK          = 0,
    CCSX_DEFLATE_OUTPUT_FULL = 1   /* the stream (coded or stored, whichever the rule picks) is longer than out_cap */
};
#endif
typedef struct ccsx_deflater_s *ccsx_deflater;
typedef struct ccsx_deflate_span { int64_t in_off; int32_t in_len; int32_t out_cap; int64_t out_off; } ccsx_deflate_span;
int         ccsx_deflate_rule_version(void);
int32_t     ccsx_deflate_bound(int32_t in_len);
int         ccsx_deflater_create(int device, int64_t max_in_bytes, int64_t max_out_bytes, int32_t max_spans, ccsx_deflater *out);
int         ccsx_deflater_destroy(ccsx_deflater f);
int         ccsx_deflate_spans(ccsx_deflater f, const uint8_t *src, int64_t src_len, const ccsx_deflate_span *spans, int32_t n_spans,
                               uint8_t *dst, int64_t dst_len, int32_t *out_len, uint32_t *crc, int32_t *status);   /* synchronous: submit + wait */
int         ccsx_deflate_submit(ccsx_deflater f, const uint8_t *src, int64_t src_len, const ccsx_deflate_span *spans, int32_t n_spans,
                                uint8_t *dst, int64_t dst_len, int32_t *out_len, uint32_t *crc, int32_t *status, ccsx_ticket *ticket);
int         ccsx_deflate_wait(ccsx_deflater f, ccsx_ticket ticket);
int         ccsx_deflate_spans_host(const uint8_t *src, int64_t src_len, const ccsx_deflate_span *spans, int32_t n_spans,
                                    uint8_t *dst, int64_t dst_len, int32_t *out_len, uint32_t *crc, int32_t *status);
uint32_t    ccsx_deflate_crc(const uint8_t *p, int64_t n);
int         ccsx_deflate_code_lengths(const uint32_t *freq, int32_t n, int32_t max_bits, uint8_t *lens);   /* the rule's code construction alone, host: the lengths
                                              (<= max_bits, 1 .. 15) of the 2 <= n <= 286 symbols with these counts, as one sub-block would get them; for the tests */
int32_t     ccsx_deflate_fill_spans(int device);      /* spans of one call that fill the device: its CUs x the workgroups of k_deflate a CU holds (1); < 0 on error */

/* ---- model training: Baum-Welch counts on the device, the M-step on the host (the rule: DESIGN.md §2 "Model training", its own version ccsx_train_rule_version;
 * no result of the consensus changes).  A pair is (window of a ZMW, pass): the window k_polish would cut on the caller's draft, the pass's segment between the
 * window's two entry rows.  Per pair the FULL forward and backward matrices are filled (no band), the pair is gated (alpha / beta agreement, opts.min_zscore), and
 * the posterior probability of every match, stay and deletion event of the window's core columns is added, in 2^-CCSX_TRAIN_FRAC fixed point, to the ZMW's
 * tables.  Every sum is an integer sum: the tables do not depend on the order or grouping in which pairs ran, and per-ZMW tables of several calls add exactly.
 *   ccsx_train_batch      the fourth seam beside ccsx_draft_batch, ccsx_polish_batch and ccsx_hd_batch: synchronous, slot 0.  On the caller's drafts — the truth
 *                         the passes are measured against: known templates, or a consensus the caller trusts — it runs the polish seam's alignment cascade and
 *                         window map, then k_train in place of the polish.  A ZMW whose status after the cascade is not SUCCESS contributes zeros.  Afterwards
 *                         ccsx_stage_draft / ccsx_stage_windows / ccsx_stage_align report what it used; ccsx_run and ccsx_download refuse slot 0 until the next
 *                         ccsx_upload.  A null argument, nonzero `reserved`, counts sized for another batch or a poisoned handle are errors of the call: nothing
 *                         is enqueued.  The count buffers (3.2 KB per ZMW) are reserved by the first call; without one nothing is reserved, launched or copied.
 *   ccsx_train_pair_host  the same rule for ONE pair on the calling thread, no device (train_core.h: the code the kernel shares): the reference of the tests.  The
 *                         template is given in the pass's orientation (the caller reverse-complements it and swaps the flanks for a reverse-strand pass), J =
 *                         1 .. CCSX_JMAX columns, core [cs, ce), left_flank 0 .. 3 or 4 = none; obs: n = 0 .. CCSX_IMAX codes 0 .. 11.  Adds to match[192],
 *                         stay[192], del[16], *loglik; returns 1 counted, 0 gated, < 0 bad argument (nothing added).
 *   stay[k][o]            holds both stay events of context k: outcome base = the context's current base is a branch, any other base a stick.
 * The fitter is the M-step, host only.  Emissions: a row's counts plus `pseudo` per cell, normalised; a row with fewer than min_events events keeps the starting
 * row.  Transitions: each ZMW's row of context k goes into the bin of clamp(snr[cur(k)], start.snr_lo, start.snr_hi) out of snr_bins equal bins over the start
 * model's range; per bin with at least min_events matches r_move = N_move / N_match (the model's w) for branch, stick and deletion, fitted at the bins' CENTRES by
 * least squares weighted with N_match, polynomial degree min(degree, populated bins - 1); a context without a populated bin keeps its polynomials.  The fitted
 * snr_lo / snr_hi are the centres of the first and last populated bin of any context (equal when one bin is populated; a start model with snr_lo == snr_hi is
 * accepted: every row is then in bin 0, at that point).  All accumulation is integer: the fitted model is a pure function of the
 * multiset of (counts row, SNR) pairs, whatever the order or grouping of ccsx_fitter_add.  ccsx_fitter_finish may be called more than once.                       */
#define CCSX_TRAIN_FRAC 32
typedef struct ccsx_train_counts {
    int32_t  n_zmw, reserved;          /* reserved must be 0 */
    int64_t *match, *stay;             /* [n_zmw][16][12] events x 2^CCSX_TRAIN_FRAC */
    int64_t *del;                      /* [n_zmw][16] */
    int64_t *loglik;                   /* [n_zmw] log2-likelihood of the counted pairs x 65536, range shift removed */
    int32_t *n_pairs, *n_gated, *n_bases, *status;   /* [n_zmw]; status = enum ccsx_status after the cascade (as ccsx_hd_report.status) */
} ccsx_train_counts;
int         ccsx_train_rule_version(void);
int         ccsx_train_batch(ccsx_handle h, const ccsx_batch *b, const ccsx_drafts *drafts, ccsx_train_counts *out);
int         ccsx_train_pair_host(const ccsx_model *m, const float snr[4], const uint8_t *tpl, int32_t J, int32_t left_flank, int32_t cs, int32_t ce,
                                 const uint8_t *obs, int32_t n, float min_zscore, int64_t match[192], int64_t stay[192], int64_t del[16], int64_t *loglik);
typedef struct ccsx_fit_opts {
    int32_t degree;                    /* polynomial degree of the transition weights, 0 .. 3 (default 1) */
    int32_t snr_bins;                  /* 4 .. 256 (default 64) */
    double  min_events;                /* events a row / matches a bin needs (default 200) */
    double  pseudo;                    /* added to every emission cell (default 0.5) */
} ccsx_fit_opts;
typedef struct ccsx_fit_report {
    int64_t pairs, gated, bases;       /* sums over everything added */
    double  loglik_per_base;           /* log2-likelihood per read base of the counted pairs, under the model the counts were made with */
    int32_t contexts_kept;             /* contexts whose match-emission row kept its starting values (fewer than min_events matches) */
    float   snr_lo, snr_hi;            /* of the fitted model */
    double  max_change;                /* largest |new - old| of any emission probability and of any transition weight at a populated bin's centre */
} ccsx_fit_report;
typedef struct ccsx_fitter_s *ccsx_fitter;
void        ccsx_fit_opts_default(ccsx_fit_opts *o);
int         ccsx_fitter_create(const ccsx_model *start, const ccsx_fit_opts *o, ccsx_fitter *out);   /* o NULL = the defaults */
int         ccsx_fitter_add(ccsx_fitter f, const ccsx_train_counts *c, const float *snr);            /* snr: [n_zmw][4] */
int         ccsx_fitter_finish(ccsx_fitter f, ccsx_model *out, ccsx_fit_report *rep);                /* rep may be NULL */
int         ccsx_fitter_destroy(ccsx_fitter f);

/* deterministic synthetic subread generator (SURVEY.md §8d / BASELINE.md §3).  Caller frees with ccsx_synth_free */
typedef struct ccsx_synth {
    ccsx_batch batch;            /* arrays are owned by this object                             */
    int64_t   *tpl_off;          /* [n_zmw+1] */
    uint8_t   *tpl;              /* true templates, codes 0..3, orientation of read 0           */
} ccsx_synth;
int         ccsx_synth_generate(int32_t n_zmw, int32_t first_zmw_id, int32_t passes_lo, int32_t passes_hi,
                                int32_t len_lo, int32_t len_hi, uint64_t seed, ccsx_synth **out);
void        ccsx_synth_free(ccsx_synth *s);

#ifdef __cplusplus
}
#endif
#endif /* CCSX_H */

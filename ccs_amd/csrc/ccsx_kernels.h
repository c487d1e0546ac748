// ccsx_kernels.h — kernel parameter block shared by ccsx_kernels.hip and ccsx_api.cpp
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "ccsx.h"
#include "barcode_core.h"
#include "segment_core.h"
#include "cdna_core.h"
#include "dup_core.h"
#include "cell_core.h"
#include "represent_core.h"

// bytes of POA scratch per vertex (ccsx_kernels.hip poa_slot, all by topological position): the 32-row score column of far-read columns 128, five 16-byte
// records (kinfo, column records x 2, overflow in-edges x 2), 16 move bytes (a nibble per band row), 3 words of consensus / band state, two flag bytes
#define CCSX_POA_BYTES_PER_VERTEX 238

// the floor of every reported per-base error probability for opts.max_qv (SPEC v7: Q50 = exactly 1e-5f; the oracle computes the same expression)
static inline float ccsx_perr_floor(int max_qv) { return max_qv == 50 ? 1e-5f : (float)pow(10.0, -(double)max_qv / 10.0); }

// words of stored moves per pass of a k_align16 quad: per block of 16 draft columns 16 move words (one per band row) + 2 words of band steps / edge flags = 18,
// rounded up so that a pass's words start on a 16-byte boundary.  ONE definition for the kernels (tb_stride) and the host's slot size.
#define CCSX_TB_WORDS_PER_BLOCK 18
static inline __host__ __device__ int ccsx_tb_blocks(int Ld) { return (Ld + 15) >> 4; }
static inline __host__ __device__ int ccsx_tb_stride(int Ld) { return (ccsx_tb_blocks(Ld) * CCSX_TB_WORDS_PER_BLOCK + 3) & ~3; }

// passes of a ZMW the engine uses, for opts.top_passes: <= 0 (all of them) and anything above CCSX_MAX_PASSES mean CCSX_MAX_PASSES (SPEC v5)
static inline __host__ __device__ int ccsx_top_passes(int top_passes) { return (top_passes <= 0 || top_passes > CCSX_MAX_PASSES) ? CCSX_MAX_PASSES : top_passes; }

struct KParams {
    int32_t n_zmw, n_reads;
    int32_t maxL_max;          // longest subread of the batch
    int32_t vcap_max;          // POA vertex capacity of the largest ZMW
    int32_t need_max;          // max window-edge columns per read (2 * window slots)
    int32_t max_reads;         // most passes of a ZMW in the batch (after the top_passes cap)
    int32_t qv_only;           // CCSX_QV_ONLY (ccsx_polish_batch): one scoring round, no mutation applied — QVs / rq of the sequence as given
    ccsx_opts opts;
    float perr_floor;          // 10^(-opts.max_qv / 10): floor of every reported per-base error probability (ccsx_perr_floor)
    const ccsx_model *model;   // device copy
    // ---- inputs (HBM resident after ccsx_upload)
    const float *snr;
    const int32_t *read_off;
    const int64_t *base_off;
    const uint8_t *bases, *pw, *flags;
    // ---- host-derived layout
    const int32_t *read_zmw;   // [R] owning ZMW of each read
    const int32_t *vcap;       // [n] POA vertex capacity
    const int32_t *dcap;       // [n] draft / consensus capacity
    const int64_t *seq_off;    // [n+1] offsets of draft and outputs (capacity layout)
    const int32_t *wb_off;     // [n+1] offsets into wbounds; window slots of z = wb_off[z+1]-wb_off[z]-1
    const int64_t *ent_off;    // [R] offsets into ent
    int32_t *wslot_zmw;        // [total window slots] compact map built on the device after the draft stage (k_wmap): owning ZMW of the i-th WINDOW
    int32_t *wstart;           // [n_zmw + 1] first compact index of every ZMW's windows; [n_zmw] = windows of the batch
    // ---- per-ZMW state
    float *tabME, *tabINS, *tabDL;
    float *tabZ;               // [n][32] z-score parameters per context: MU[16], VAR[16]
    uint8_t *draft;
    int32_t *draft_len, *nwin, *zstat, *nreads_used, *wbounds, *np;
    int32_t *nfull;            // [n] full-length passes among nreads_used (the partial passes follow them)
    int32_t *zref;             // [n] backbone pass (index within the ZMW) = orientation reference of draft and consensus; bit 8: a fallback
                               //     draft is requested (set by k_post), bit 9: the fallback draft has been made
    int32_t *ticket_poa, *ticket_align;   // 256-byte scratch block that also holds debug[] and phase[] (no tickets since the chunked launch)
    int32_t *debug;            // [4] first failed bounds check (CCSX_DEBUG_CHECKS builds)
    unsigned long long *phase; // [16] per-phase cycle sums (CCSX_PROFILE_PHASES builds)
    // ---- POA / alignment scratch (per resident slot)
    uint8_t *poa_scratch;
    size_t poa_slot_bytes;
    int32_t poa_slots;
    int32_t *align_scratch;
    size_t align_slot_i32;
    int32_t align_slots;
    uint8_t *avalid;
    int32_t *ascore;
    int32_t *ent;              // entry rows of every window-edge column, per read
    uint32_t *dmask;           // same indexing: pile-up dirty bits of the draft positions between two window-edge columns
    // ---- per-window polish outputs
    long long total_wslots;
    int32_t pw_obs_bytes, pw_gb_floats;   // k_polish dynamic LDS: observation codes, gamma/beta floats
    uint8_t *wseq;             // [wslots][32]
    float *wqv;                // [wslots][32]
    float *wsum;               // [wslots] sum of p_err over the core
    int4 *wmeta;               // [wslots] (core length, usable reads, non-convergent, iterations)
    // ---- results
    uint8_t *out_seq, *out_qual;
    float *out_raw;
    int32_t *out_status, *out_len, *out_iters, *out_nwin;
    float *out_rq, *out_ec;
    int32_t *out_fn, *out_rn;  // passes used per strand
    // ---- launch order (cost-sorted, longest first: the one-wave-per-ZMW / per-read kernels finish together)
    const int32_t *zmw_perm;   // [n_zmw]
    const int32_t *read_perm;  // [n_reads]
    const int32_t *quads;      // [n_quads] (first pass << 2 | passes - 1): up to four consecutive passes of one ZMW, longest first
    int32_t n_quads;
    int32_t *align_retry;      // [16 + n_reads]: [0] = count, [16..] = passes for the 64-row retry (appended by k_align16)
    // ---- HiFi kinetics (NULL unless opts.hifi_kinetics); kept at the end so the hot kernels' kernarg offsets do not move
    const uint8_t *ipd;
    uint8_t *wtpl;             // [wslots][32] converged window template incl. overhangs
    short2 *wtmeta;            // [wslots] (J, core start)
    uchar4 *wkin;              // [wslots][32] (fi, fp, ri, rp) codes of the core positions
    uint8_t *out_kin;          // 4 planes (fi, fp, ri, rp) of seq_off[n] bytes each
    long long kin_plane;       // plane stride = seq_off[n]
    // ---- caller-supplied drafts (ccsx_polish_batch: the polish seam of docs/img/ccs-impl.png); the bases are already in `draft`
    const int32_t *din_len;    // [n] draft length (0 = none)
    const int32_t *din_bb;     // [n] a pass of the ZMW that has the draft's orientation
    // ---- k_align16 / k_align16_tb: a quad's stored moves (4 passes x ccsx_tb_stride(draft length) words + the 4 final band starts, see below); align_slot_i32 / align_slots are the 64-row retry's and the split alignment's
    size_t align16_slot_i32;
    int32_t align16_slots;
    int32_t *retry_scratch;    // the 64-row retry's / split alignment's slots: behind k_align16's in the same buffer (the trace-backs run beside the next launch / the retry)
    int32_t align16_regions;   // 1, or 2 when the batch's quads take several launches: launch c uses region c & 1, so its trace-back runs under launch c + 1
    // ---- heteroduplex finder (ccsx_hd_batch, or a fused run with a ccsx_hd_request; NULL otherwise).  Per-window outputs use the compact window index of k_wmap
    ccsx_hd_opts hd;
    int32_t hd_split;          // fused run only: a HETERODUPLEX ZMW gets status CCSX_HETERODUPLEX and no windows (k_hd_verdict), the window map is rebuilt
    const double *hd_lf;       // [CCSX_HD_LF_N] log k! (host-built, DESIGN.md §2 "Heteroduplex rule")
    int32_t *hd_wcnt;          // [windows] substitution sites of the window
    ccsx_hd_site *hd_wrec;     // [windows][CCSX_HD_WIN_SITES] the window's sites with the lowest columns, in column order
    double *hd_wminp;          // [windows] smallest p of the window's sites (1 = none)
    ccsx_hd_site *hd_isite;    // [n][CCSX_HD_MAX_SITES] large-indel sites with the lowest (column, kind)
    int32_t *hd_zi;            // [6][n] verdict, sub sites, indel sites, listed, indel sites listed, status after the cascade (before a split)
    double *hd_minp;           // [n]
    ccsx_hd_site *hd_sites;    // [n][CCSX_HD_MAX_SITES]
    // ---- pileup summary (ccsx_consensus_pileup / ccsx_submit_pileup only; NULL otherwise).  Needs wtpl / wtmeta as kinetics does
    uchar4 *wpile;             // [wslots][32] (coverage, matches, mismatches, 0) of the core positions
    uint8_t *out_pile;         // 3 planes (coverage, matches, mismatches) of seq_off[n] bytes each
    long long pile_plane;      // plane stride = seq_off[n]
    // ---- tandem repeats (ccsx_consensus_extras / ccsx_submit_extras with tandem_len or min_tandem_repeat_length; NULL otherwise): DESIGN.md §2 "Tandem repeats"
    int32_t *tflag;            // [n] 0 = undecided; bit 0 = decided on the ZMW's deciding draft, bit 1 = flagged (its heuristics are off, as with opts.disable_heuristics)
    int32_t *tlen;             // [n] longest run of sDUST-masked draft positions of the deciding draft (0: none decided)
    int32_t min_tandem;        // flag threshold (<= 0: detect and report only)
    int32_t sdust_words;       // k_sdust's LDS mask: 32-bit words, enough for the longest draft that is aligned
    // ---- adapter palindromes (ccsx_consensus_fold / ccsx_submit_fold; NULL otherwise): DESIGN.md §2 "Adapter palindromes"
    ccsx_fold_opts fold;
    int32_t *fold_zi;          // [4][n] verdict, fold, hits, span
    int32_t fold_bins;         // k_fold's LDS histogram: anti-diagonal bins of the longest draft that is aligned (+ 1 empty bin)
    // ---- adapter screen (ccsx_consensus_screen / ccsx_submit_screen with an adapter request; NULL otherwise): DESIGN.md §2 "Adapter screen"
    ccsx_adapter_opts adapt;
    int32_t *adapt_zi;         // [9][n] tested, verdict, n_hits, n_listed, covered, max_gap, first_start, last_end, min_dist
    int32_t *adapt_hits;       // [n][CCSX_ADAPTER_MAX_HITS][3] start, end, search | dist << 8 (the bytes of ccsx_adapter_hit)
    int32_t adapt_words;       // k_adapter's two LDS bitmaps: 32-bit words each, enough for the longest draft that is aligned
    int32_t adapt_n;           // adapters (searches = 2 x)
    uint8_t adapt_len[CCSX_ADAPTER_MAX_PATTERNS];
    uint32_t adapt_seq[CCSX_ADAPTER_MAX_PATTERNS][4];   // 2 bits per base, base i at bits 2 (i & 15) of word i >> 4
    // ---- control screen (ccsx_consensus_control / ccsx_submit_control with a control request; NULL otherwise): DESIGN.md §2 "Control screen"
    ccsx_control_opts ctl;
    int32_t *ctl_zi;           // [8][n] verdict, strand, hits, matched, ctl_start, ctl_end, draft_start, draft_end
    const uint32_t *ctl_index; // [CCSX_CONTROL_INDEX_WORDS] the slot's own copy of the control's index (ccsx_control_index_build)
    int32_t ctl_len;           // M
    int32_t ctl_bins;          // k_control's two LDS histograms: diagonal bins each, enough for the longest draft that is aligned (+ 1 empty bin)
    // ---- model training (ccsx_train_batch; NULL otherwise): DESIGN.md §2 "Model training".  Zeroed on the stream before k_train
    int64_t *train_tab;        // [n][400] posterior event counts x 2^32: match[16][12], stay[16][12], del[16]
    int64_t *train_ll;         // [n] log2-likelihood of the counted pairs x 65536, range shift removed
    int32_t *train_zi;         // [3][n] counted pairs, gated pairs, read bases of the counted pairs
    // ---- coverage screen (ccsx_consensus_requests / ccsx_submit_requests with a coverage request; NULL otherwise): DESIGN.md §2 "Coverage rule"
    ccsx_coverage_opts cov;    // min_spans already resolved (0 = opts.min_passes)
    uint32_t cov_gate;         // bit v: a ZMW with verdict v = 2 .. 5 gets the status CCSX_DRAFT_TOO_DIFFERENT + (v - 2) and no consensus
    int32_t *cov_zi;           // [10][n] verdict, np_aligned, spans, cov_max, clean_min, drop_window, drop_windows, reach_sum, used_sum, used_min
    uint8_t *cov_reach;        // [wslots] reach_w of every window, indexed as wmeta is ((wb_off[z] - z) + w): k_coverage writes it, k_coverage_post reads it
    // ---- POA log (ccsx_poa_log; NULL otherwise): include/ccsx.h "The POA log".  Filled with -1 when the batch is staged
    int32_t *poa_log;          // [n][2 generators][poa_log_stride passes][CCSX_POA_LOG_WORDS], written by k_poa_thread
    int32_t poa_log_stride;    // = max_reads
    // ---- pass orientation (a batch with a CCSX_PASS_STRAND_UNKNOWN pass; NULL otherwise): DESIGN.md §2 "Pass orientation"
    ccsx_orient_opts orient;
    uint8_t *orient_flags;     // [R] = flags, writable: k_orient resolves bit 0 of the flagged passes in place and clears their bit 3
    const int32_t *orient_anchor;   // [n] the ZMW's anchor pass (index within the ZMW; host-built, layout()), -1 = no full-length pass
    uint32_t *orient_tab;      // [orient_wgs][orient_tab_words] one open-addressing table of 13-mer codes per resident workgroup (shared scratch of the handle)
    int32_t orient_tab_words;  // a power of two >= 2 x the 13-mer positions of the batch's longest anchor
    int32_t orient_wgs;        // workgroups of the launch (each walks the ZMWs blockIdx.x, blockIdx.x + orient_wgs, ...)
    uint8_t *orient_rep8;      // [2][R] strand, call
    int32_t *orient_votes;     // [2][R] votes_same, votes_opp
    // ---- polisher hand-off (ccsx_consensus_handoff / ccsx_submit_handoff; NULL otherwise): DESIGN.md §2 "Polisher hand-off".  Needs wtpl / wtmeta as kinetics does.
    // The tiles of ZMW z are indexed ccsx_handoff_tile_off(seq_off[z], z, T) + t
    ccsx_handoff_opts ho;
    int32_t ho_max_tiles;      // capacity of the output arrays in tiles
    int32_t *ho_zcnt;          // [2][n] tiles of the ZMW, selected tiles of the ZMW (k_tile_select)
    int32_t *ho_tslot;         // [tiles] k_tile_select: the selected tile's rank within its ZMW; k_tile_scan: its slot g; -1 = not selected or beyond the capacity
    int32_t *ho_tqsum;         // [tiles] sum of the tile's qual bytes
    int32_t *ho_woff;          // [wslots] offset of every window's core in SEQ, indexed as wmeta is
    int32_t *ho_counts;        // [2] tiles, selected tiles
    int32_t *ho_hdr;           // [5][max_tiles] tile_zmw, tile_start, tile_len, tile_qsum, tile_rows
    uint8_t *ho_rows;          // [2][max_tiles][R] row_pass, row_strand
    uchar4 *ho_cells;          // [max_tiles][R][T]
    // ---- barcode calls (ccsx_consensus_barcodes / ccsx_submit_barcodes; bc.rep NULL otherwise): DESIGN.md §2 "Barcode calls".  k_barcode's own parameters
    // (ccsx_barcode.hip): it reads out_seq / out_len after k_stitch
    BarcodeParams bc;
    // ---- segmentation (ccsx_consensus_segments / ccsx_submit_segments; sg.rep NULL otherwise): DESIGN.md §2 "Segment rule".  k_segment's own parameters
    // (ccsx_segment.hip): it reads out_seq / out_len after k_stitch
    SegmentParams sg;
    // ---- full-length cDNA reads (ccsx_consensus_cdna / ccsx_submit_cdna; cd.rep NULL otherwise): DESIGN.md §2 "cDNA rule".  k_cdna's own parameters
    // (ccsx_cdna.hip): it reads out_seq / out_len after k_stitch
    CdnaParams cd;
    // ---- representative reads (ccsx_consensus_represent / ccsx_submit_represent; rep.rep NULL otherwise): DESIGN.md §2 "Representative rule".  k_represent's own
    // parameters (ccsx_represent.hip): it reads the final draft and out_status and writes the result planes after k_stitch
    RepresentParams rep;
};
// first tile index of ZMW z whose outputs start at seq_off: consecutive ZMWs get disjoint ranges of at least ceil(capacity / T) tiles, with no table
static inline __host__ __device__ int64_t ccsx_handoff_tile_off(int64_t seq_off, int z, int T) { return seq_off / T + z; }
#define CCSX_TILE_SCAN_ZMWS 64   // ZMWs per workgroup of k_tile_scan
#define CCSX_COVERAGE_PLANES 10
#define CCSX_COVERAGE_PRE_GATE 0x1cu   // the gate bits of the verdicts k_coverage reaches before the polish (2, 3, 4)

// k_adapter (DESIGN.md §2 "Adapter screen"): draft bases a lane owns per search, its workgroup, the hit keys one pass buffers in LDS and the bitmaps' LDS bound
#define CCSX_ADAPTER_CHUNK     128
#define CCSX_ADAPTER_THREADS   256
#define CCSX_ADAPTER_BUF       1024
#define CCSX_ADAPTER_MAX_WORDS 6144   // 2 bitmaps x 24 KiB (drafts up to 196 kb) + 12.4 KB of static LDS stay within the 64 KiB a launch gets by default

// k_fold (DESIGN.md §2 "Adapter palindromes"): k-mer length, sampled positions that enter, and the LDS hash table of one pass over the samples
#define CCSX_FOLD_K        15
#define CCSX_FOLD_NS_MAX   8192
#define CCSX_FOLD_THREADS  256
#define CCSX_FOLD_SLOTS    2048    // open-addressing table of canonical codes
#define CCSX_FOLD_CAP      1536    // distinct codes and kept members one pass holds; beyond that the samples are split into more passes
#define CCSX_FOLD_MAX_BINS 6656    // the histogram's LDS bound (drafts up to 212 kb): with k_fold's 37.9 KB of static LDS a launch stays within the
                                   // 64 KiB it gets without raising its dynamic-LDS attribute (drafts are at most ~82 kb: 1.25 x 65535-base subreads)

// k_control (DESIGN.md §2 "Control screen"): the index of a control of M <= CCSX_CONTROL_MAX_LEN bases as the host builds it and every workgroup copies it to LDS.
//   words [0, 4096)     the codes of the kept 15-mers in increasing (code, position), padded with 0xffffffff (no code: a code has 30 bits)
//   words [4096, 6144)  their positions, 16 bits each, in the same order
//   words [6144, 7168)  a prefilter: bit (ccsx_fmix32(code) & 32767) is set for every kept code; a look-up that passes it still compares the exact code
#define CCSX_CONTROL_THREADS     256
#define CCSX_CONTROL_POS_WORD    CCSX_CONTROL_MAX_LEN
#define CCSX_CONTROL_FILTER_WORD (CCSX_CONTROL_MAX_LEN + CCSX_CONTROL_MAX_LEN / 2)
#define CCSX_CONTROL_FILTER_BITS 32768
#define CCSX_CONTROL_INDEX_WORDS (CCSX_CONTROL_FILTER_WORD + CCSX_CONTROL_FILTER_BITS / 32)
#define CCSX_CONTROL_MAX_BINS    4352   // per orientation; the histograms' LDS bound (drafts up to 274 kb): 2 x 17 KiB + k_control's 29.2 KB of static LDS stay
                                        // within the 64 KiB a launch gets by default
static inline __host__ __device__ uint32_t ccsx_fmix32(uint32_t h) { h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16; return h; }

// k_orient (DESIGN.md §2 "Pass orientation"): the anchor's 13-mer codes (26 bits) live in a per-workgroup table in global scratch, slot of a code's first
// probe = ccsx_fmix32(code) & (slots - 1), linear probing, slots = ccsx_orient_slots(M) for an anchor of M bases (load <= 1/2); in front of it an LDS bitmap of
// CCSX_ORIENT_FILTER_BITS bits, bit = ccsx_fmix32(code) >> CCSX_ORIENT_FILTER_SHIFT, which may only reject.
#define CCSX_ORIENT_K            13
#define CCSX_ORIENT_THREADS      256
#define CCSX_ORIENT_FILTER_BITS  262144   // 32 KiB of LDS: four workgroups per CU; an anchor of 10 kb sets 4 % of it, one of 65 535 bases 22 %
#define CCSX_ORIENT_FILTER_SHIFT 14       // the hash's top 18 bits
#define CCSX_ORIENT_MIN_SLOTS    64
#define CCSX_ORIENT_MAX_WGS      1024     // resident workgroups of a launch = tables of the scratch (256 CUs x 4)
#define CCSX_ORIENT_EMPTY        0xffffffffu
static inline __host__ __device__ int ccsx_orient_slots(int M)
{
    const int npos = M >= CCSX_ORIENT_K ? M - CCSX_ORIENT_K + 1 : 0;
    int s = CCSX_ORIENT_MIN_SLOTS;
    while (s < 2 * npos) s <<= 1;
    return s;
}

// k_sdust (DESIGN.md §2 "Tandem repeats"): window W bases, threshold T in tenths, dynamic LDS = two [64][64] word tables + two byte tables + the mask
#define CCSX_SDUST_W 64
#define CCSX_SDUST_T 20
#define CCSX_SDUST_TABLE_BYTES (2 * 64 * 64 * 4 + 2 * 64 * 64)

#define CCSX_HD_LF_N (2 * CCSX_MAX_PASSES + 1)   // log-factorials 0 .. 510; a Fisher table holds nf + nr <= CCSX_MAX_PASSES = 255 passes, so only 0 .. 255 are read
#define CCSX_HD_IMAX 49                          // rows of a segment the pileup aligns.  A last window has up to 30 template columns (core <= 28 + one overhang), so
                                                 // with min_indel 21 a segment of 50 rows exists: this clause, not |n - J| < min_indel, leaves it out of the pileup

// which stages ccsx_launch_all enqueues: the fused path, the draft stage alone (ccsx_draft_batch), alignment cascade + polish on caller-supplied drafts, or
// alignment cascade + the heteroduplex finder on caller-supplied drafts (ccsx_hd_batch), or alignment cascade + the training counts on caller-supplied drafts
// (ccsx_train_batch)
// or k_orient alone (ccsx_orient_batch)
enum { CCSX_RUN_FUSED = 0, CCSX_RUN_DRAFT = 1, CCSX_RUN_POLISH = 2, CCSX_RUN_HD = 3, CCSX_RUN_TRAIN = 4, CCSX_RUN_ORIENT = 5 };

// The stage events of a batch (Slot::ev, timing enabled), in the values they have always had — in time order POLISH_START lies between DRAFT_STAGE_DONE and
// POLISH_DONE.  ccsx_launch_all records each of them exactly once on every path, in time order, so that ccsx_timings may read all seven after any run.
enum ccsx_stage_event {
    CCSX_EV_START = 0,             // before the batch's first call; setup_ms runs from here
    CCSX_EV_TABLES_DONE = 1,       // after k_setup; draft_ms runs from here
    CCSX_EV_DRAFT_DONE = 2,        // after the first POA round (and its k_sdust); align_ms — cascade, accounting, the whole fallback rounds — runs from here
    CCSX_EV_DRAFT_STAGE_DONE = 3,  // after the draft stream's last kernel: the polish stream waits for it; queue_ms runs from here
    CCSX_EV_POLISH_DONE = 4,       // after polish and kinetics / pileup; stitch_ms runs from here
    CCSX_EV_END = 5,               // after the last kernel: total_ms ends here, and the download stream waits for it ("results ready")
    CCSX_EV_POLISH_START = 6,      // on the polish stream once DRAFT_STAGE_DONE has passed (it may have queued behind the previous batch); polish_ms runs from here
    CCSX_EV_COUNT
};
// The ordering events of a batch (Slot::ev_aux, no timing): what the draft stream and the second stream tell each other inside one ccsx_launch_all.
enum ccsx_order_event {
    CCSX_ORD_POA_FORK = 0,         // draft stream -> second stream: the second half-batch of the POA may start
    CCSX_ORD_FIRST_DP_DONE = 1,    // first half's first k_poa_dp done: the second half stays one DP behind
    CCSX_ORD_POA_JOIN = 2,         // second stream -> draft stream: the second half's draft is made
    CCSX_ORD_ALIGN16_DONE_0 = 3,   // k_align16 launch c done (c even): its trace-back may start on the second stream
    CCSX_ORD_ALIGN16_DONE_1 = 4,   // ... (c odd)
    CCSX_ORD_TB_DONE_0 = 5,        // the trace-back of launch c done (c even): the launch's scratch region is free, its entry rows are written
    CCSX_ORD_TB_DONE_1 = 6,        // ... (c odd)
    CCSX_ORD_COUNT
};

// where ccsx_launch_all enqueues: the draft stage on `draft`, the polish stage on `polish` (the same stream: serial stages), half of a large POA round and the
// trace-backs of k_align16 on `aux` (NULL, or ev_aux NULL: everything on `draft`).  ev: [CCSX_EV_COUNT], or NULL with one stream; ev_aux: [CCSX_ORD_COUNT]
struct ccsx_launch_queues {
    hipStream_t draft, polish, aux;
    hipEvent_t *ev, *ev_aux;
};
const char *ccsx_launch_all(const KParams &P, const ccsx_launch_queues &q, int mode);   // NULL, or the name of the launch that failed
const char *ccsx_barcode_launch(const BarcodeParams &B, hipStream_t st);                 // ccsx_barcode.hip: k_barcode, one workgroup per read; NULL, or what failed
const char *ccsx_segment_launch(const SegmentParams &G, hipStream_t st);                 // ccsx_segment.hip: k_segment, one workgroup per read; NULL, or what failed
const char *ccsx_cdna_launch(const CdnaParams &D, hipStream_t st);                       // ccsx_cdna.hip: k_cdna, one workgroup per read; NULL, or what failed
const char *ccsx_cell_launch(const CellParams &C, hipStream_t st);                       // ccsx_cell.hip: k_cell, one workgroup per read; NULL, or what failed
const char *ccsx_dup_sign_launch(const DupSignParams &S, hipStream_t st);                // ccsx_dup.hip: k_dup_sign, one wave per read; NULL, or what failed
const char *ccsx_dup_cluster_launch(const DupClusterParams &P, hipStream_t st);          // ccsx_dup.hip: k_dup_keys, the sort, k_dup_buckets, k_dup_verify; NULL, or what failed
size_t ccsx_dup_sort_bytes(int n);                                                       // ccsx_dup.hip: the sort's scratch for n pairs (no device work)
const char *ccsx_represent_launch(const RepresentParams &R, hipStream_t st);             // ccsx_represent.hip: k_represent, one workgroup per ZMW; NULL, or what failed
const char *ccsx_train_launch(const KParams &P, hipStream_t st, long long max_blocks);   // ccsx_train.hip: the count buffers zeroed + k_train; NULL, or what failed
int ccsx_kernel_is_experiment();         // built with -DCCSX_EXPERIMENT (timing studies: wrong results)
const char *ccsx_kernel_build_flags();   // "" for a product build; the experiment switches this translation unit was compiled with otherwise
int ccsx_polish_lds(int max_reads, int *obs_bytes, int *gb_floats);

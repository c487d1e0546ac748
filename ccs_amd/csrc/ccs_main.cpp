// ccs — `ccs [options] IN.subreads.bam OUT.bam` on MI355X (reference CLI: docs/index.md:52-64,
// docs/faq/parallelize.md:8-20; flag spellings from SURVEY.md App. C).
//
// Pipeline (the reference's docs/img/ccs-impl.png with the GPU consumers only):
//   reader thread   BGZF inflate on the -j pool -> subread records -> ZMW grouping -> step-1 filters
//                   (docs/how-does-ccs-work.md:19-32) -> SoA batches of --batch-size ZMWs
//   pack workers    SoA packing of a batch straight into page-locked staging (off the reader thread)
//   GPU workers     one per device, each owns ONE ccsx_handle and keeps up to three batches in flight through
//                   ccsx_submit / ccsx_wait: upload, kernels and download of consecutive batches overlap
//   writer          restores input order, writes hifi BAM records with tags rq np ec sn zm RG
//                   (docs/faq/bam-output.md:9-30), BGZF deflate on the pool, ccs_report.txt
//                   (docs/faq/reports-aux-files.md:16-72)
// There is no CPU consensus fallback: without a gfx950 device the program exits with an error.
#include <sched.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <cctype>
#include <cstring>
#include <fstream>
#include <chrono>
#include <cinttypes>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <mutex>
#include <queue>
#include <string>
#include <thread>
#include <vector>

#include "bam_io.h"
#include "ccsx.h"

using namespace bamio;

namespace {

// default cost budget of a batch per ZMW of --batch-size (round 4 used 400 kb: 8192 mixed ZMWs became TWO tickets, nothing overlapped, 2.1 k ZMWs/s)
constexpr long long kDefaultBasesPerZmw = 110000;

// ZMWs of the k-th ticket when --batch-size is not given.  The engine wants LARGE batches (one wave per POA graph: a draft stage of 1000 graphs takes nearly as
// long as one of 8000, the kernels being latency-bound), a short run wants several tickets in flight from the start: 1024, 1024, 2048, 2048, 4096, 4096, 8192, ...
// — a file of 8192 ZMWs still becomes five tickets, a long run works in tickets of 8192.
inline int auto_batch_zmws(long long k) { return k >= 6 ? 8192 : 1024 << (int)(k / 2); }

struct Options {
    std::string in, out, report;
    int threads = 0;
    double min_snr = 2.5;
    int batch = 0;                 // --batch-size; 0 = automatic: tickets ramp up from 1024 to 8192 ZMWs (see batch_limit)
    long long batch_bases = 0;     // cost budget of a batch in subread bases (0 = 110 kb x --batch-size): SURVEY.md 8e "batches of ~ constant cost"
    int chunk_i = 1, chunk_n = 1;
    int workers_per_gpu = 3;      // packing threads per device (one engine handle per device keeps three batches in flight)
    std::string model_file;       // --model-file: Arrow parameter json (else: chemistry of the BAM header -> bundle dir / built-in)
    std::vector<int> gpus;
    ccsx_opts o;
    bool all_gpus = false;
    std::string write_synth;      // "N,P,L[,seed]" -> write a synthetic subreads.bam to `out`
    bool dump = false;            // print one line per ZMW after the step-1 filters, no GPU
    bool gpu_inflate = false;     // --gpu-inflate: the BGZF blocks of IN are inflated by k_inflate (experimental)
    bool gpu_deflate = false;     // --gpu-deflate: the BGZF blocks of OUT.bam and the --fail-reads BAM are deflated by k_deflate (experimental)
    bool host_only = false;       // reader -> filters -> packing into staging, no engine and no output: what the host side alone sustains
    bool by_strand = false;       // --by-strand: one consensus per strand (docs/faq/mode-by-strand.md:8-23)
    bool no_partial = false;      // --no-partial-passes: drop the subreads that are not flanked by adapters on both sides (as round 2 did)
    bool qv_binning = false;      // --qv-binning: 7-bin per-base QVs after rq is computed (docs/faq/qv-binning.md:19-31)
    bool pileup = false;          // --pileup-summary: per-base tags sa sm sx (docs/faq/bam-output.md:25-27; opt-in here)
    int min_tandem = 0;           // --min-tandem-repeat-length: per-ZMW heuristics switch on sDUST (docs/faq/low-complexity.md:8-18; off here)
    bool suppress_reports = false; // --suppress-reports: no report / metrics files "per default" — a file that is NAMED is still written (docs/faq/sqiie.md:36-46)
    bool report_named = false, metrics_named = false;
    std::string metrics;          // --metrics-json (default <prefix>.zmw_metrics.json.gz)
    std::string report_json;      // --report-json: the ccs_report counts as JSON (docs/changelog.md:72, docs/faq/sqiie.md:42); written only when named
    std::string hifi_summary;     // --hifi-summary-json: the HiFi statistics block as JSON (docs/faq/sqiie.md:45); written only when named
    std::string log_file;         // --log-file: log lines go there instead of stderr (docs/faq/sqiie.md:40)
    double refresh_rate = 5.0;    // --refresh-rate: seconds between progress lines at --log-level INFO (docs/faq/reports-aux-files.md:176-177)
    int log_level = 1;
    std::string fail_reads;       // --fail-reads FAIL.bam: one representative read per ZMW without a HiFi read, with the ff tag (docs/faq/fail-reads.md)
    std::string adapters;         // --adapters FILE.fasta|default: screen the drafts for adapter sequence (fail classes 0x10, 0x40); needs --fail-reads
    ccsx_adapter_set adapter_set{};   // ... the set it names
    std::string control;          // --control FILE.fasta: screen the drafts for the spike-in control (fail class 0x2); control ZMWs leave the main output
    std::vector<uint8_t> control_codes;   // ... its bases
    ccsx_control_seq control_seq{};       // ... as the requests name them
    bool orient_passes = false;   // --orient-passes: subreads without cx direction bits are submitted strand-unknown (flags bit 3; DESIGN.md §2 "Pass orientation")
    bool coverage_filters = false;   // --coverage-filters: the coverage screen with all four gate bits (DESIGN.md §2 "Coverage rule"; off here)
    int cov_drop_percent = -1, cov_block = -1;   // --coverage-drop-percent / --coverage-block: overrides of ccsx_coverage_opts (-1: the default)
    ccsx_coverage_opts coverage_opts{};          // ... the options every ticket carries
    std::string barcodes;         // --barcodes FILE.fasta: call the barcodes of the set at both ends of every HiFi read (DESIGN.md §2 "Barcode calls"): tags bc, bq
    int barcode_window = -1;      // --barcode-window N: bases of either end that are searched (-1: the default)
    std::string barcode_counts;   // --barcode-counts FILE.tsv: reads per called pair
    std::shared_ptr<ccsx_barcode_set> barcode_set;   // ... the set it names, the record names, the options every ticket carries
    std::vector<std::string> barcode_names;
    ccsx_barcode_opts barcode_opts{};
    std::string segment_adapters; // --segment-adapters FILE.fasta: cut every HiFi read of a concatenated array into its segments (DESIGN.md §2 "Segment rule"): tags di, dl, dr
    int segment_min_length = -1;  // --segment-min-length N: a piece shorter than this is no segment (-1: the default)
    std::string segment_counts;   // --segment-counts FILE.tsv: reads per (segments, orientation, complete) class
    std::shared_ptr<ccsx_segment_set> segment_set;   // ... the set it names and the options every ticket carries
    ccsx_segment_opts segment_opts{};
    std::string cdna_primers;     // --cdna-primers FILE.fasta: keep the full-length cDNA reads, clipped of primers and poly(A) tail (DESIGN.md §2 "cDNA rule"): tags ts, pa, pr, pq
    int cdna_min_polya = -1;      // --cdna-min-polya N: a read with a shorter tail is not full-length; 0: a tail is not required (-1: the default)
    int cdna_min_length = -1;     // --cdna-min-length N: a read whose insert without the tail is shorter is not full-length (-1: the default)
    std::string cdna_counts;      // --cdna-counts FILE.tsv: reads per (class, strand)
    std::shared_ptr<ccsx_cdna_set> cdna_set;         // ... the set it names and the options every ticket carries
    ccsx_cdna_opts cdna_opts{};
    bool reads_bam = false;       // --reads-bam: one representative read per productive ZMW (the reference's --all, DESIGN.md §2 "Representative rule")
    bool reads_kinetics = false;  // --reads-bam-kinetics: --hifi-kinetics for the polished reads, fi / fp of the pass for the unaltered subreads (--all-kinetics)
    bool reads_fallback = false;  // --reads-bam-subread-fallback: a subread where an unpolished draft would be written (--subread-fallback)
    bool min_passes_set = false, min_rq_set = false, max_length_set = false;   // given on the command line (--reads-bam fixes them)
    int heteroduplexes = 0;       // --heteroduplexes split|drop: the finder in every ticket with the split (DESIGN.md §2 "Heteroduplex rule").  HD_SPLIT: a heteroduplex
                                  // ZMW is written as up to two single-strand reads (the reference's --hd-finder); HD_DROP: it yields no read (how-does-ccs-work.md:65-72)
    std::string fit_model;        // --fit-model OUT.json: the training mode (DESIGN.md §2 "Model training"): no consensus output
    int fit_iterations = 3;       // --fit-iterations: EM iterations over the file
    double fit_min_rq = 0.999;    // --fit-min-rq: a polished consensus is a truth to measure passes against from this predicted accuracy on
    long long fit_max_zmws = 0;   // --fit-max-zmws: ZMWs (after the step-1 filters) that are used, 0 = all
    int fit_degree = -1;          // --fit-degree: polynomial degree of the transition weights (-1: the fitter's default)
    bool mark_duplicates = false; // --mark-duplicates IN.bam OUT.bam: the duplicate mode (DESIGN.md §2 "Duplicate rule"): reads in, the same reads out, marked
    bool dup_remove = false;      // --dup-remove: duplicates are left out instead of marked
    bool dup_within_barcodes = false;   // --dup-within-barcodes: only reads of equal bc tag are compared
    int dup_window = -1, dup_kmer = -1, dup_max_dist_pct = -1, dup_max_len_diff_pct = -1;   // --dup-window ...: overrides of ccsx_dup_opts (-1: the default)
    std::string dup_counts;       // --dup-counts FILE.tsv: sets per set size
    ccsx_dup_opts dup_opts{};     // ... the options of the run
    bool dup_within_cells = false;   // --dup-within-cells: only reads of equal (CB, XM) tags are compared
    bool cell_reads = false;      // --cell-reads IN.bam OUT.bam: the cell-tag mode (DESIGN.md §2 "Cell-tag rule"): reads in, the full-length cDNA reads out, tagged
    std::string cell_design_text; // --cell-design STR: the fields in sense-strand order around T (T-12U-16B, 16B-10U-T)
    std::string cell_whitelist;   // --cell-whitelist FILE: one barcode of bc_len ACGT per line
    std::string cell_counts;      // --cell-counts FILE.tsv: reads per whitelist index, per tag status and per cDNA class
    bool cell_no_indels = false, cell_require_barcode = false;   // --cell-no-indels, --cell-require-barcode
    ccsx_cell_design cell_design{};   // ... the design, the whitelist's barcodes as read (CB is written from them) and the object made of them
    std::vector<uint8_t> cell_codes;
    std::shared_ptr<ccsx_cell_whitelist> cell_wl;
    std::vector<std::string> seen;   // every option of the command line, as given (--mark-duplicates and --cell-reads refuse what they do not take)
};

enum HdMode { HD_OFF = 0, HD_SPLIT = 1, HD_DROP = 2 };
enum HostStatus { HS_OK = 0, HS_POOR_SNR = 100, HS_NO_SUBREADS = 101, HS_TOO_FEW = 102, HS_TOO_LONG = 103, HS_ADAPTER_PALINDROME = 104, HS_ADAPTER_CONCAT = 105,
                  HS_ADAPTER_NEAR_END = 106, HS_CONTROL_SUCCESS = 107, HS_CONTROL_FAILURE = 108 };

struct ZmwIn {
    int32_t zm = 0;
    float snr[4] = {0, 0, 0, 0};
    std::vector<Subread> reads;   // after filters: full-length passes only
    int host_status = HS_OK;
    int64_t order = 0;
    int strand_tag = 0;           // --by-strand: 1 = /fwd, 2 = /rev
    int64_t polymerase_len = 0;   // zmw_metrics: bases of all subreads of the ZMW
    int32_t median_len = 0, n_full = 0;
    std::string fl_name;          // --fail-reads: the median-length full-length subread (ties: the first in file order), kept before the filters clear `reads`
    std::vector<uint8_t> fl_seq;
};

// page-locked staging of one GPU worker (bases / pw / ipd of the batch in flight), grown geometrically and reused
static bool g_plain_arenas = false;        // --host-only: ordinary memory (there may be no device to pin for)
struct Arena {
    uint8_t *p = nullptr;
    size_t cap = 0;
    bool plain = false;
    void release() { if (plain) std::free(p); else ccsx_free_pinned(p); p = nullptr; }
    uint8_t *reserve(size_t bytes)
    {
        if (bytes > cap) {
            release();
            cap = bytes + bytes / 4 + (1u << 20);
            plain = g_plain_arenas;
            p = plain ? (uint8_t *)std::malloc(cap) : (uint8_t *)ccsx_alloc_pinned(cap);
            if (!p) { cap = 0; throw std::runtime_error(plain ? std::string("staging: out of memory") : std::string("pinned staging: ") + ccsx_last_error()); }
        }
        return p;
    }
    ~Arena() { release(); }
};

struct Batch {
    int64_t index = 0;
    std::vector<ZmwIn> zmws;      // including host-failed ones (they are only counted)
    // SoA of the ZMWs with host_status == OK
    std::vector<int32_t> zmw_id, read_off;
    std::vector<float> snr;
    std::vector<int64_t> base_off;
    std::vector<uint8_t> flags;
    const uint8_t *bases = nullptr, *pw = nullptr, *ipd = nullptr;   // in the packing worker's pinned arena, valid during its engine call
    int64_t n_bases = 0;
    std::vector<int> slot;        // per zmws[]: index into the SoA or -1
    // results: views into the batch's page-locked output arena (asynchronous D2H), valid until the writer has emitted the batch
    std::vector<int64_t> seq_off;
    int32_t n = 0; int64_t cap = 0;
    int32_t *status = nullptr, *seq_len = nullptr, *np = nullptr, *iters = nullptr, *n_windows = nullptr, *fn = nullptr, *rn = nullptr;
    uint8_t *seq = nullptr, *qual = nullptr, *kin = nullptr;   // kin: 4 planes (fi, fp, ri, rp) of cap bytes each (--hifi-kinetics)
    uint8_t *pile = nullptr;      // 3 planes (coverage, matches, mismatches) of cap bytes each (--pileup-summary)
    int32_t *tlen = nullptr;      // longest sDUST-masked run of each ZMW's deciding draft (--min-tandem-repeat-length)
    int32_t *fold = nullptr;      // --fail-reads: the adapter-palindrome report (verdict, fold, hits, span; n each)
    float *rq = nullptr, *ec = nullptr;
    int dev = 0;                  // which device's packers / worker / staging pools handle the batch (index into the handle list)
    bool have_results = false;    // false: packing or the engine failed for this batch
    std::unique_ptr<struct Arena> in_arena, out_arena;
    ccsx_batch cb; ccsx_results cr; // the structs handed to ccsx_submit_control live as long as the ticket
    ccsx_pileup cp{};               // ... and so does the pileup the extras point to
    ccsx_extras ex{};               // (read during the call only)
    ccsx_fold_report frep{}; ccsx_fold_request freq{};   // --fail-reads (ccsx_fold_request: the report's arrays are in out_arena)
    ccsx_adapter_report arep{}; ccsx_adapter_request areq{};   // --adapters (ccsx_adapter_request: the report's arrays are in out_arena)
    ccsx_control_report crep{}; ccsx_control_request creq{};   // --control (ccsx_control_request: the report's arrays are in out_arena)
    ccsx_coverage_report vrep{}; ccsx_coverage_request vreq{}; // --coverage-filters (ccsx_coverage_request: the report's arrays are in out_arena)
    ccsx_cdna_report drep{}; ccsx_cdna_request dreq{};         // --cdna-primers (ccsx_cdna_request: the report's arrays are in out_arena)
    ccsx_segment_report srep{}; ccsx_segment_request sreq{};   // --segment-adapters (ccsx_segment_request: the report's arrays are in out_arena)
    ccsx_barcode_report brep{}; ccsx_barcode_request breq{};   // --barcodes (ccsx_barcode_request: the report's arrays are in out_arena)
    ccsx_represent_report rrep{}; ccsx_represent_request rreq{};   // --reads-bam (ccsx_represent_request: the report's arrays are in out_arena)
    ccsx_hd_report hrep{}; ccsx_hd_request hreq{};   // --heteroduplexes (ccsx_hd_request: the report's arrays are in out_arena)
    ccsx_requests reqs{};           // (read during the call only)
    // --heteroduplexes split: the single-strand batch made of this batch's HETERODUPLEX ZMWs (the GPU worker builds it when the ticket retires), and per SoA
    // slot s its two entities there: strand_slot[2 s] the forward strand's, strand_slot[2 s + 1] the reverse strand's, -1 = no such entity
    std::shared_ptr<Batch> strand;
    std::vector<int> strand_slot;
    Batch *parent = nullptr;        // of a single-strand batch: the batch that goes to the writer when this one's ticket has retired
};

template <class T> class Channel {
public:
    explicit Channel(size_t cap) : cap_(cap) {}
    void push(T v)
    {
        std::unique_lock<std::mutex> l(m_);
        cv_full_.wait(l, [this] { return q_.size() < cap_; });
        q_.push(std::move(v));
        cv_empty_.notify_one();
    }
    bool pop(T &v)
    {
        std::unique_lock<std::mutex> l(m_);
        cv_empty_.wait(l, [this] { return !q_.empty() || closed_; });
        if (q_.empty()) return false;
        v = std::move(q_.front()); q_.pop();
        cv_full_.notify_one();
        return true;
    }
    void close() { std::lock_guard<std::mutex> l(m_); closed_ = true; cv_empty_.notify_all(); }

private:
    std::queue<T> q_;
    size_t cap_;
    bool closed_ = false;
    std::mutex m_;
    std::condition_variable cv_full_, cv_empty_;
};

void usage()
{
    std::fprintf(stderr,
                 "ccs (MI355X) - generate HiFi reads from PacBio subreads\n"
                 "usage: ccs [options] IN.subreads.bam OUT.{bam,fastq.gz}\n"
                 "  -j, --num-threads N       host threads for BAM (de)compression [all usable: affinity / cgroup quota]\n"
                 "      --min-passes N        minimum full-length passes [3]\n"
                 "      --top-passes N        use at most the N passes closest to the median length [60]; 0 = unlimited (the engine takes up\n"
                 "                            to 255 passes per ZMW)\n"
                 "      --model-file F        Arrow model parameters (json); default: chosen by the chemistry in the BAM header from\n"
                 "                            $SMRT_CHEMISTRY_BUNDLE_DIR/arrow/*.json, then the built-in set\n"
                 "      --disable-heuristics  polish every position (no candidate filter)\n"
                 "      --max-insertion-size N  trim subread insertions longer than N bases relative to the draft [30]; 0 = never\n"
                 "      --min-snr F           minimum SNR of a ZMW [2.5]\n"
                 "      --min-length N        minimum draft length [10]\n"
                 "      --max-length N        maximum draft length [50000]\n"
                 "      --min-rq F            minimum predicted accuracy [0.99]\n"
                 "      --maxPoaCoverage N    subreads used for the draft [5]\n"
                 "      --by-strand           one consensus per strand, read names end in /fwd or /rev\n"
                 "      --heteroduplexes split|drop  run the heteroduplex finder on every draft (strand-biased substitutions, insertions / deletions of more\n"
                 "                            than 20 bases on one strand).  split: such a ZMW is written as up to two single-strand reads named /fwd and /rev, each\n"
                 "                            polished from its own strand's passes, in read groups of their own; ccs_report.txt gets a double-strand and a\n"
                 "                            single-strand column; with --fail-reads the single-strand reads go to F.bam with ff 0x4.  drop: such a ZMW yields\n"
                 "                            no read and is counted as 'Heteroduplex insertions'.  Not with --by-strand, --reads-bam, --barcodes, --fit-model,\n"
                 "                            --orient-passes [off]\n"
                 "      --orient-passes       the engine determines the strand of every subread whose cx tag carries no direction bit, against the ZMW's\n"
                 "                            subread closest to the median length; alternation is then only a prior for passes it cannot call [off]\n"
                 "      --no-partial-passes   do not use the first / last (one-adapter) subread of a ZMW in the polish\n"
                 "      --qv-binning          write 7-bin per-base QVs (Q3 Q10 Q17 Q22 Q27 Q35 Q40)\n"
                 "      --hifi-kinetics       averaged per-strand kinetics: tags fi fp fn ri rp rn (ip pw with --by-strand)\n"
                 "      --pileup-summary      per-base pileup tags: sa (run-length encoded coverage), sm (matches), sx (mismatches) [off]\n"
                 "      --min-tandem-repeat-length N  a ZMW whose draft holds a tandem repeat (sDUST) of >= N bases runs with --disable-heuristics\n"
                 "                            for itself only; N > 0 [off: the reference's default is 1000]\n"
                 "      --fail-reads F.bam    also write one read per ZMW that yields no HiFi read, with the ff tag: 0x1 below --min-rq, 0x20 adapter\n"
                 "                            palindrome (such reads leave the main output), 0x8 the median full-length subread of a ZMW without a consensus,\n"
                 "                            0x4 a single-strand read (--heteroduplexes split)\n"
                 "      --adapters F|default  with --fail-reads: screen every draft for the adapters of FASTA file F (up to 8 records of 16-64 bases) or for the\n"
                 "                            built-in SMRTbell adapter; reads made of adapter copies (ff 0x10) or with an adapter close to an end (ff 0x40)\n"
                 "                            leave the main output for F.bam [off]\n"
                 "      --reads-bam           one read per productive ZMW (the reference's --all): the polished read, or the unpolished draft, or an unaltered\n"
                 "                            subread, the last two with rq -1 and every QV 10; sets --min-passes 2, --min-rq 0 and the engine's maximum length\n"
                 "      --reads-bam-kinetics  with --reads-bam: --hifi-kinetics for the polished reads, fi fp (fn 1, rn 0) for the subreads (--all-kinetics)\n"
                 "      --reads-bam-subread-fallback  with --reads-bam: a subread where an unpolished draft would be written (--subread-fallback)\n"
                 "      --coverage-filters    screen every draft's windows for coverage drops: a ZMW whose passes disagree on a block of bases, that too few\n"
                 "                            passes span end to end, that too few passes align to, or that lost too many passes in the polish gets no\n"
                 "                            consensus and is counted as 'Coverage drops', 'Insufficient draft cov', 'Draft too different' or 'Reads\n"
                 "                            failed polishing' [off]\n"
                 "      --coverage-drop-percent N  with --coverage-filters: a window drops at N %% or less of the best window's passes, 0-100 [50]\n"
                 "      --coverage-block N    with --coverage-filters: a pass carries a block when its segment exceeds the window by more than N bases,\n"
                 "                            1-4096 [30]\n"
                 "      --control F.fasta     screen every draft for the spike-in control of FASTA file F (one record of 64-4096 bases); control ZMWs leave\n"
                 "                            the main output and are counted as 'ZMW with control success / failure'; with --fail-reads those with a\n"
                 "                            consensus are written to F.bam with ff 0x2 [off: there is no built-in control]\n"
                 "      --barcodes F.fasta    call the barcodes of FASTA file F (1-384 records of 8-64 bases) at both ends of every HiFi read, on the GPU: a read\n"
                 "                            with a barcode called at both ends gets the tags bc:B:S (the two record indices, head and tail; the tail's barcode\n"
                 "                            as it reads on the opposite strand) and bq:i; nothing is clipped; the reports gain a barcode block [off]\n"
                 "      --barcode-window N    with --barcodes: bases of either end that are searched, 8-1024 [64]\n"
                 "      --barcode-counts F.tsv  with --barcodes: one line per called pair of barcodes (the two record names, the reads), sorted by index pair\n"
                 "      --segment-adapters F.fasta  cut every HiFi read of a concatenated array (A0 S1 A1 .. SK AK, either strand) into its segments, on the GPU: F holds\n"
                 "                            the 2-33 adapters of 8-64 bases in array order; a HiFi read is replaced by one record per segment, named\n"
                 "                            <movie>/<zm>/ccs/<start>_<end>, with the tags di:i (segment index) and dl:i / dr:i (the adapters on its left and right);\n"
                 "                            a read without a segment is not written; the reports gain a segment block.  Not with --by-strand, --barcodes,\n"
                 "                            --reads-bam, --heteroduplexes, --fit-model [off]\n"
                 "      --segment-min-length N  with --segment-adapters: a piece shorter than N bases is no segment, 1-65535 [50]\n"
                 "      --cdna-primers F.fasta  keep the full-length cDNA reads (5p . transcript . poly(A) . rc(3p), either strand), found on the GPU: F holds the 2-64\n"
                 "                            primers of 8-64 bases as the oligos, each record's name ending in _5p or _3p; a HiFi read with a 5' primer at one end\n"
                 "                            and a 3' primer at the other, no primer inside and a poly(A) tail becomes one record without primers and tail, named\n"
                 "                            <movie>/<zm>/ccs/<start>_<end>, in the read's orientation, with the tags ts:A (+ sense, - antisense), pa:i (the poly(A)\n"
                 "                            bases removed), pr:B:C (the 5' and the 3' primer's numbers in F) and pq:i; every other read is counted, not written; the\n"
                 "                            reports gain a cDNA block.  Not with --by-strand, --barcodes, --segment-adapters, --reads-bam, --heteroduplexes, --fit-model\n"
                 "      --cdna-min-polya N    with --cdna-primers: a tail shorter than N bases is no tail, 0-255; 0: a tail is not required [20]\n"
                 "      --cdna-min-length N   with --cdna-primers: a read of fewer than N bases between primers and tail is not written, 1-65535 [50]\n"
                 "      --cdna-counts F.tsv   with --cdna-primers: one line per class and strand of reads (class, strand, the reads), sorted\n"
                 "      --segment-counts F.tsv  with --segment-adapters: one line per class of reads (segments per read, orientation, complete, the reads), sorted\n"
                 "      --metrics-json F      per-ZMW metrics [<OUT prefix>.zmw_metrics.json.gz]\n"
                 "      --suppress-reports    do not write the default ccs_report.txt / zmw_metrics.json.gz (files named explicitly are still written)\n"
                 "      --chunk i/N           process only the i-th of N ZMW chunks\n"
                 "      --batch-size N        ZMWs per GPU batch, at most [automatic: 1024, 1024, 2048, 2048, 4096, 4096, then 8192 per ticket]\n"
                 "      --batch-bases N       ... and at most N subread bases (estimated cost, SURVEY.md 8e: batches of about constant cost for mixed\n"
                 "                            pass counts / insert lengths) [110000 x batch-size: a 10-pass x 10 kb ZMW costs ~ 102 kb, so such a batch still\n"
                 "                            closes by count, while a Sequel-II-like mix (~ 200 kb per ZMW, 400 x spread) is cut into >= 6 tickets per 8192 ZMWs]\n"
                 "      --gpus a,b,..         device ordinals [0] ('all' = every visible device)\n"
                 "      --workers-per-gpu N   packing threads per device [3] (one engine handle per device, three batches in flight)\n"
                 "      --report-file F       ccs_report.txt path [<OUT prefix>.ccs_report.txt]\n"
                 "      --report-json F       the same counts as JSON (only when named)\n"
                 "      --hifi-summary-json F HiFi yield / length / quality statistics as JSON (only when named)\n"
                 "      --log-level L         ERROR|WARN|INFO [WARN]\n"
                 "      --log-file F          write log lines to F instead of stderr\n"
                 "      --refresh-rate S      seconds between progress lines at --log-level INFO [5]\n"
                 "      --max-qv Q            largest per-base QV reported; rq follows [50 = this build's calibrated cap; 93 = the reference's range]\n"
                 "      --gpu-inflate         inflate the BGZF blocks of IN on the GPU (k_inflate) instead of on the host threads; the CRC32 check, every\n"
                 "                            error and every output byte stay as they are [off; experimental]\n"
                 "      --gpu-deflate         deflate the BGZF blocks of OUT.bam and of the --fail-reads BAM on the GPU (k_deflate, with their CRC32) instead of on\n"
                 "                            the host threads; the records are the same, the compressed bytes are another valid BGZF encoding of them;\n"
                 "                            OUT.fastq.gz, the .pbi files and the metrics stay on the host [off; experimental]\n"
                 "  test helpers (not in the reference):\n"
                 "      --write-synthetic N,P,L[,seed]  write a synthetic subreads.bam to OUT (no IN)\n"
                 "      --dump-zmws                     list ZMWs after the step-1 filters (no GPU, no OUT)\n"
                 "      --host-only                     read, filter and pack IN into batch staging, no engine (no GPU, no OUT): host throughput\n"
                 "duplicate marking (ccs --mark-duplicates IN.bam OUT.bam; one GPU; IN: an unaligned BAM of reads, HiFi reads, segments or cDNA reads):\n"
                 "      --mark-duplicates     find the reads of IN that are the same molecule (DESIGN.md, Duplicate rule: equal end minimizers, end windows\n"
                 "                            within an edit distance, lengths within a tolerance; single linkage) and write every record of IN to OUT: a member\n"
                 "                            of a set of two or more gains ds:i (the set's size), a duplicate also FLAG 0x400 and du:Z (the name of the set's\n"
                 "                            representative, the member of largest rq).  No OUT.bam.pbi is written.  Not with any option of the consensus side,\n"
                 "                            --chunk or input from stdin: usage errors\n"
                 "      --dup-remove          leave the duplicates out of OUT instead of marking them\n"
                 "      --dup-within-barcodes only reads with equal bc tags are compared\n"
                 "      --dup-within-cells    only reads with equal CB and XM tags (cell barcode and UMI, as --cell-reads writes them) are compared; a read that\n"
                 "                            lacks either is compared with its like.  Not with --dup-within-barcodes\n"
                 "      --dup-window W        bases of each end that are compared, 16 .. 64 [32]\n"
                 "      --dup-kmer K          the minimizer's k, 8 .. 16 [12]\n"
                 "      --dup-max-dist-pct P  two end windows agree within floor(W * P / 100) edits, 0 .. 30 [10]\n"
                 "      --dup-max-len-diff-pct P  two reads agree in length within P percent of the shorter, 0 .. 20 [2]\n"
                 "      --dup-counts F.tsv    sets per set size\n"
                 "cell barcodes and UMIs (ccs --cell-reads IN.bam OUT.bam; one GPU; IN: an unaligned BAM of reads, HiFi reads or segments):\n"
                 "      --cell-reads          read the UMI and the cell barcode behind one cDNA primer of every read of IN, on the GPU (DESIGN.md, Cell-tag rule), and\n"
                 "                            write the full-length cDNA reads to OUT: the input record with SEQ, QUAL and every per-base B tag cut to the slice\n"
                 "                            without primers, fields and poly(A) tail (ri / rp from the other end), every other tag as it is, and the tags ts:A, pa:i,\n"
                 "                            pr:B:C, pq:i of --cdna-primers, XM:Z (the UMI), XC:Z (the barcode as read) and, for a barcode of the whitelist, exact or\n"
                 "                            corrected, CB:Z.  No OUT.bam.pbi is written.  Needs --cdna-primers and --cell-design; takes --cdna-min-polya,\n"
                 "                            --cdna-min-length, -j, --gpus with one device, --log-level, --log-file and --report-file; everything else: usage errors\n"
                 "      --cell-design STR     the fields in sense-strand order around the transcript T, each a length 1-16 and U (UMI) or B (barcode): T-12U-16B has\n"
                 "                            them at the 3' primer, the barcode next to it; 16B-10U-T at the 5' primer.  At most one U and one B, on one side of T\n"
                 "      --cell-whitelist F    the known barcodes, plain text, one of exactly the design's length per line, ACGT in either case (not compressed)\n"
                 "      --cell-no-indels      correct substitutions only [a lost or a gained base is corrected as well]\n"
                 "      --cell-require-barcode  write only reads whose barcode is in the whitelist, exact or corrected\n"
                 "      --cell-counts F.tsv   the reads written per whitelist index, sorted by index, then the reads of IN per tag status and per cDNA class\n"
                 "model training (ccs --fit-model OUT.json IN.subreads.bam; one GPU, no HiFi output):\n"
                 "      --fit-model OUT.json  fit the Arrow parameter set to the subreads of IN by EM and write it as a ccsx-1 json with the header's chemistry\n"
                 "                            triple: per iteration every batch is drafted and polished, the passes are measured against the polished reads of at\n"
                 "                            least --fit-min-rq (posterior event counts, k_train), and the fitter makes the next model.  Starts from the\n"
                 "                            chemistry's model or --model-file.  Not with a second positional, several GPUs, --chunk or any option of the\n"
                 "                            output side (--fail-reads, --by-strand, --control, --adapters, reports, tags, --gpu-inflate, --gpu-deflate): usage errors\n"
                 "      --fit-iterations N    EM iterations (default 3)\n"
                 "      --fit-min-rq X        predicted accuracy a polished read needs to serve as a truth (default 0.999)\n"
                 "      --fit-max-zmws N      use the first N ZMWs that pass the filters (default 0 = all)\n"
                 "      --fit-degree D        polynomial degree of the transition weights in the SNR, 0 .. 3 (default 1)\n");
}

// The FASTA files of --adapters, --barcodes, --segment-adapters and --control: min_records .. max_records records of min_bases .. max_bases bases each, ACGT in
// either case; CR, blanks and tabs at a line's end and empty lines are skipped.  names: the '>' lines, cut at 60 characters; codes: the bases as 0 .. 3.
// too_few: what is said of the first record of a file with fewer than min_records (> 1) records.  false + a message that names the record.
struct FastaLimits { size_t min_records, max_records, min_bases, max_bases; const char *too_few; };
struct FastaSet { std::vector<std::string> names; std::vector<std::vector<uint8_t>> codes; };
bool load_fasta_set(const std::string &path, const FastaLimits &lim, FastaSet &fa, std::string &err)
{
    std::ifstream f(path);
    if (!f) { err = "cannot open the file"; return false; }
    fa = FastaSet{};
    auto where = [&](size_t k) { return "record " + std::to_string(k + 1) + " (" + fa.names[k] + ")"; };
    std::string line;
    while (std::getline(f, line)) {
        while (!line.empty() && (line.back() == '\r' || line.back() == ' ' || line.back() == '\t')) line.pop_back();
        if (line.empty()) continue;
        if (line[0] == '>') {
            fa.names.push_back(line.substr(0, 60));
            fa.codes.emplace_back();
            if (fa.names.size() > lim.max_records) {
                err = where(fa.names.size() - 1) + ": more than " + (lim.max_records == 1 ? std::string("one record") : std::to_string(lim.max_records) + " records"); return false;
            }
            continue;
        }
        if (fa.names.empty()) { err = "sequence before the first '>' line"; return false; }
        const size_t a = fa.names.size() - 1;
        for (char c : line) {
            const int u = std::toupper((unsigned char)c);
            const int code = u == 'A' ? 0 : u == 'C' ? 1 : u == 'G' ? 2 : u == 'T' ? 3 : -1;
            if (code < 0) { err = where(a) + ": '" + std::string(1, c) + "' is not one of ACGT"; return false; }
            if (fa.codes[a].size() >= lim.max_bases) { err = where(a) + ": more than " + std::to_string(lim.max_bases) + " bases"; return false; }
            fa.codes[a].push_back((uint8_t)code);
        }
    }
    if (fa.names.empty()) { err = "no FASTA record"; return false; }
    if (fa.names.size() < lim.min_records) { err = where(0) + ": " + lim.too_few; return false; }
    for (size_t k = 0; k < fa.names.size(); ++k)
        if (fa.codes[k].size() < lim.min_bases) { err = where(k) + ": " + std::to_string(fa.codes[k].size()) + " bases, fewer than " + std::to_string(lim.min_bases); return false; }
    return true;
}
// the records as the len / seq of a pattern set of the C ABI (the limits given to load_fasta_set were the set's); the number of records
template <typename Set> int32_t fasta_patterns(const FastaSet &fa, Set &set)
{
    std::memset(&set, 0, sizeof set);
    for (size_t k = 0; k < fa.codes.size(); ++k) {
        set.len[k] = (int32_t)fa.codes[k].size();
        std::copy(fa.codes[k].begin(), fa.codes[k].end(), set.seq[k]);
    }
    return (int32_t)fa.codes.size();
}

// --adapters: "default" = the built-in set; otherwise a FASTA of 1 .. 8 records of 16 .. 64 bases
bool load_adapters(const std::string &path, ccsx_adapter_set &set, std::string &err)
{
    if (path == "default") return ccsx_adapter_set_default(&set) == 0;
    FastaSet fa;
    if (!load_fasta_set(path, {1, CCSX_ADAPTER_MAX_PATTERNS, CCSX_ADAPTER_MIN_LEN, CCSX_ADAPTER_MAX_LEN, nullptr}, fa, err)) return false;
    set.n_adapters = fasta_patterns(fa, set);
    return true;
}

// --barcodes: a FASTA of 1 .. 384 records of 8 .. 64 bases.  ids: the names up to their first blank, without the '>'
bool load_barcodes(const std::string &path, ccsx_barcode_set &set, std::vector<std::string> &ids, std::string &err)
{
    FastaSet fa;
    if (!load_fasta_set(path, {1, CCSX_BARCODE_MAX, CCSX_BARCODE_MIN_LEN, CCSX_BARCODE_MAX_LEN, nullptr}, fa, err)) return false;
    set.n_barcodes = fasta_patterns(fa, set);
    ids.clear();
    for (const std::string &n : fa.names) ids.push_back(n.substr(1, n.find_first_of(" \t", 1) == std::string::npos ? std::string::npos : n.find_first_of(" \t", 1) - 1));
    return true;
}

// --segment-adapters: a FASTA of 2 .. 33 records of 8 .. 64 bases, in array order
bool load_segment_adapters(const std::string &path, ccsx_segment_set &set, std::string &err)
{
    FastaSet fa;
    if (!load_fasta_set(path, {2, CCSX_SEGMENT_MAX_ADAPTERS, CCSX_SEGMENT_MIN_LEN, CCSX_SEGMENT_MAX_LEN, "the only record, an array has at least 2 adapters"}, fa, err)) return false;
    set.n_adapters = fasta_patterns(fa, set);
    return true;
}

// --cdna-primers: a FASTA of 2 .. 64 records of 8 .. 64 bases, the primers as the oligos.  A record's role is its name's ending, _5p or _3p, up to the first
// blank (the convention is recalled from the vendor's primer files, which are not in the reference mount, as bam_io.h says of the .pbi layout)
bool load_cdna_primers(const std::string &path, ccsx_cdna_set &set, std::string &err)
{
    FastaSet fa;
    if (!load_fasta_set(path, {2, CCSX_CDNA_MAX_PRIMERS, CCSX_CDNA_MIN_LEN, CCSX_CDNA_MAX_LEN, "the only record, a cDNA library has a 5' and a 3' primer"}, fa, err)) return false;
    set.n_primers = fasta_patterns(fa, set);
    int roles = 0;
    for (size_t k = 0; k < fa.names.size(); ++k) {
        const std::string id = fa.names[k].substr(0, fa.names[k].find_first_of(" \t"));
        const std::string end = id.size() >= 3 ? id.substr(id.size() - 3) : std::string();
        if (end != "_5p" && end != "_3p") { err = "record " + std::to_string(k + 1) + " (" + fa.names[k] + "): the name ends in neither _5p nor _3p"; return false; }
        set.role[k] = end == "_3p";
        roles |= 1 << set.role[k];
    }
    if (roles != 3) { err = "the file needs a _5p and a _3p record"; return false; }
    return true;
}

// --control: a FASTA of exactly one record of 64 .. 4096 bases
bool load_control(const std::string &path, std::vector<uint8_t> &codes, std::string &err)
{
    FastaSet fa;
    if (!load_fasta_set(path, {1, 1, CCSX_CONTROL_MIN_LEN, CCSX_CONTROL_MAX_LEN, nullptr}, fa, err)) return false;
    codes = fa.codes[0];
    return true;
}

// --cell-design: the fields in sense-strand order around T.  T first: the fields stand between the transcript and the 3' primer, the last one next to the primer;
// T last: between the 5' primer and the transcript, the first one next to the primer
bool parse_cell_design(const std::string &text, ccsx_cell_design &d, std::string &err)
{
    ccsx_cell_design_default(&d);
    d.umi_len = 0; d.bc_len = 0;
    std::vector<std::string> tok(1);
    for (char c : text) { if (c == '-') tok.emplace_back(); else tok.back().push_back(c); }
    size_t n_t = 0;
    for (const std::string &t : tok) n_t += t == "T";
    if (n_t != 1) { err = "the design names the transcript T once"; return false; }
    if (tok.size() < 2) { err = "the design has no field"; return false; }
    if (tok.front() != "T" && tok.back() != "T") { err = "fields on both sides of T are not supported"; return false; }
    d.side = tok.front() == "T" ? 1 : 0;
    char next_to_primer = 0;
    for (size_t k = 0; k < tok.size(); ++k) {
        const std::string &t = tok[k];
        if (t == "T") continue;
        const char kind = t.empty() ? 0 : t.back();
        char *end = nullptr;
        const long n = std::strtol(t.c_str(), &end, 10);
        if ((kind != 'U' && kind != 'B') || end != t.c_str() + t.size() - 1 || end == t.c_str() || n < 1 || n > CCSX_CELL_MAX_FIELD) {
            err = "field '" + t + "' is not a length 1 .. 16 and U or B"; return false;
        }
        int32_t &len = kind == 'U' ? d.umi_len : d.bc_len;
        if (len) { err = std::string("more than one ") + kind + " field"; return false; }
        len = (int32_t)n;
        if (d.side ? k + 1 == tok.size() : k == 0) next_to_primer = kind;
    }
    d.bc_first = next_to_primer == 'B';
    return true;
}

// --cell-whitelist: plain text, one barcode of exactly bc_len ACGT (either case) per line; blank lines are ignored; anything else names its line
bool load_cell_whitelist(const std::string &path, int bc_len, std::vector<uint8_t> &codes, std::string &err)
{
    if (bc_len < 1) { err = "the design has no barcode field"; return false; }
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) { err = "cannot read the file"; return false; }
    std::string line;
    size_t lineno = 0, n = 0;
    bool ok = true, more = true;
    while (ok && more) {
        line.clear();
        int c;
        while ((c = std::fgetc(f)) != EOF && c != '\n') line.push_back((char)c);
        more = c != EOF;
        ++lineno;
        if (lineno == 1 && line.size() >= 2 && (uint8_t)line[0] == 0x1f && (uint8_t)line[1] == 0x8b) { err = "line 1: compressed files are not read"; ok = false; break; }
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty()) continue;
        if ((int)line.size() != bc_len) { err = "line " + std::to_string(lineno) + ": not a barcode of " + std::to_string(bc_len) + " bases"; ok = false; break; }
        for (char ch : line) {
            static const char bases[] = "ACGTacgt";
            const char *at = ch ? std::strchr(bases, ch) : nullptr;
            if (!at) { err = "line " + std::to_string(lineno) + ": not ACGT"; ok = false; break; }
            codes.push_back((uint8_t)((at - bases) & 3));
        }
        if (ok && ++n > (size_t)CCSX_CELL_MAX_WHITELIST) { err = "line " + std::to_string(lineno) + ": more than 2^23 barcodes"; ok = false; }
    }
    std::fclose(f);
    if (ok && !n) { err = "the file holds no barcode"; ok = false; }
    return ok;
}

bool parse(int argc, char **argv, Options &o)
{
    ccsx_opts_default(&o.o);
    std::vector<std::string> pos;
    bool dash = false;
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto need = [&](const char *n) -> std::string { if (i + 1 >= argc) { std::fprintf(stderr, "missing value for %s\n", n); std::exit(2); } return argv[++i]; };
        // the value of option `a`, a whole number in lo .. hi; otherwise "ccs: <a> needs <what>, got '<value>'" and exit 2
        auto need_int = [&](long lo, long hi, const char *what) -> int {
            const std::string v = need(a.c_str());
            char *end = nullptr;
            const long n = std::strtol(v.c_str(), &end, 10);
            if (v.empty() || *end || n < lo || n > hi) { std::fprintf(stderr, "ccs: %s needs %s, got '%s'\n", a.c_str(), what, v.c_str()); std::exit(2); }
            return (int)n;
        };
        if (a.size() > 1 && a[0] == '-') o.seen.push_back(a);
        if (a == "-h" || a == "--help") { usage(); std::exit(0); }
        else if (a == "--version") { std::printf("ccs (ccs_amd, MI355X-native consensus path) abi %d spec %d\n", ccsx_abi_version(), ccsx_spec_version()); std::exit(0); }
        else if (a == "-j" || a == "--num-threads") o.threads = std::atoi(need("-j").c_str());
        else if (a == "--min-passes") { o.o.min_passes = std::atoi(need(a.c_str()).c_str()); o.min_passes_set = true; }
        else if (a == "--top-passes") o.o.top_passes = std::atoi(need(a.c_str()).c_str());
        else if (a == "--min-snr") o.min_snr = std::atof(need(a.c_str()).c_str());
        else if (a == "--min-length") o.o.min_length = std::atoi(need(a.c_str()).c_str());
        else if (a == "--max-length") { o.o.max_length = std::atoi(need(a.c_str()).c_str()); o.max_length_set = true; }
        else if (a == "--min-rq") { o.o.min_rq = (float)std::atof(need(a.c_str()).c_str()); o.min_rq_set = true; }
        else if (a == "--maxPoaCoverage") o.o.max_poa_cov = std::atoi(need(a.c_str()).c_str());
        else if (a == "--max-insertion-size") { const int v = std::atoi(need(a.c_str()).c_str()); o.o.max_insertion_size = v > 0 ? v : -1; }
        else if (a == "--max-qv") { const int v = std::atoi(need(a.c_str()).c_str()); o.o.max_qv = v < 1 ? 50 : (v > 93 ? 93 : v); }
        else if (a == "--batch-size") o.batch = std::atoi(need(a.c_str()).c_str());
        else if (a == "--batch-bases") o.batch_bases = std::atoll(need(a.c_str()).c_str());
        else if (a == "--report-file") { o.report = need(a.c_str()); o.report_named = true; }
        else if (a == "--workers-per-gpu") o.workers_per_gpu = std::max(1, std::atoi(need(a.c_str()).c_str()));
        else if (a == "--chunk") { if (std::sscanf(need(a.c_str()).c_str(), "%d/%d", &o.chunk_i, &o.chunk_n) != 2 || o.chunk_i < 1 || o.chunk_i > o.chunk_n) { std::fprintf(stderr, "bad --chunk\n"); return false; } }
        else if (a == "--gpus") { std::string v = need(a.c_str()); if (v == "all") o.all_gpus = true; else { size_t p = 0; while (p < v.size()) { o.gpus.push_back(std::atoi(v.c_str() + p)); p = v.find(',', p); if (p == std::string::npos) break; ++p; } } }
        else if (a == "--log-level") { std::string v = need(a.c_str()); o.log_level = v == "INFO" ? 2 : (v == "ERROR" ? 0 : 1); }
        else if (a == "--write-synthetic") o.write_synth = need(a.c_str());
        else if (a == "--dump-zmws") o.dump = true;
        else if (a == "--host-only") o.host_only = true;
        else if (a == "--gpu-inflate") o.gpu_inflate = true;
        else if (a == "--gpu-deflate") o.gpu_deflate = true;
        else if (a == "--by-strand") o.by_strand = true;
        else if (a == "--no-partial-passes") o.no_partial = true;
        else if (a == "--qv-binning") o.qv_binning = true;
        else if (a == "--hifi-kinetics") o.o.hifi_kinetics = 1;
        else if (a == "--pileup-summary") o.pileup = true;
        else if (a == "--min-tandem-repeat-length") o.min_tandem = need_int(1, 0x7fffffffL, "a positive number of bases");
        else if (a == "--suppress-reports") o.suppress_reports = true;
        else if (a == "--fail-reads") o.fail_reads = need(a.c_str());
        else if (a == "--adapters") o.adapters = need(a.c_str());
        else if (a == "--control") o.control = need(a.c_str());
        else if (a == "--barcodes") o.barcodes = need(a.c_str());
        else if (a == "--barcode-counts") o.barcode_counts = need(a.c_str());
        else if (a == "--cdna-primers") o.cdna_primers = need(a.c_str());
        else if (a == "--cdna-counts") o.cdna_counts = need(a.c_str());
        else if (a == "--cdna-min-polya") o.cdna_min_polya = need_int(0, 255, "a number in 0 .. 255");
        else if (a == "--cdna-min-length") o.cdna_min_length = need_int(1, 65535, "a number in 1 .. 65535");
        else if (a == "--segment-adapters") o.segment_adapters = need(a.c_str());
        else if (a == "--segment-counts") o.segment_counts = need(a.c_str());
        else if (a == "--segment-min-length") o.segment_min_length = need_int(1, 65535, "a number in 1 .. 65535");
        else if (a == "--barcode-window") o.barcode_window = need_int(CCSX_BARCODE_MIN_LEN, CCSX_BARCODE_MAX_WINDOW, "a number in 8 .. 1024");
        else if (a == "--coverage-filters") o.coverage_filters = true;
        else if (a == "--reads-bam") o.reads_bam = true;
        else if (a == "--reads-bam-kinetics") o.reads_kinetics = true;
        else if (a == "--reads-bam-subread-fallback") o.reads_fallback = true;
        else if (a == "--orient-passes") o.orient_passes = true;
        else if (a == "--heteroduplexes") {
            const std::string v = need(a.c_str());
            o.heteroduplexes = v == "split" ? HD_SPLIT : (v == "drop" ? HD_DROP : HD_OFF);
            if (!o.heteroduplexes) { std::fprintf(stderr, "ccs: --heteroduplexes needs 'split' or 'drop', got '%s'\n", v.c_str()); std::exit(2); }
        }
        else if (a == "--coverage-drop-percent" || a == "--coverage-block") {
            const bool pct = a == "--coverage-drop-percent";
            const std::string v = need(a.c_str());
            char *end = nullptr;
            const long n = std::strtol(v.c_str(), &end, 10);
            if (v.empty() || *end || n < (pct ? 0 : 1) || n > (pct ? 100 : 4096)) {
                std::fprintf(stderr, "ccs: %s needs a number in %s, got '%s'\n", a.c_str(), pct ? "0 .. 100" : "1 .. 4096", v.c_str()); std::exit(2);
            }
            (pct ? o.cov_drop_percent : o.cov_block) = (int)n;
        }
        else if (a == "--model-file") o.model_file = need(a.c_str());
        else if (a == "--fit-model") o.fit_model = need(a.c_str());
        else if (a == "--fit-iterations") o.fit_iterations = std::atoi(need(a.c_str()).c_str());
        else if (a == "--fit-min-rq") o.fit_min_rq = std::atof(need(a.c_str()).c_str());
        else if (a == "--fit-max-zmws") o.fit_max_zmws = std::atoll(need(a.c_str()).c_str());
        else if (a == "--fit-degree") o.fit_degree = std::atoi(need(a.c_str()).c_str());
        else if (a == "--mark-duplicates") o.mark_duplicates = true;
        else if (a == "--dup-remove") o.dup_remove = true;
        else if (a == "--dup-within-barcodes") o.dup_within_barcodes = true;
        else if (a == "--dup-within-cells") o.dup_within_cells = true;
        else if (a == "--cell-reads") o.cell_reads = true;
        else if (a == "--cell-design") o.cell_design_text = need(a.c_str());
        else if (a == "--cell-whitelist") o.cell_whitelist = need(a.c_str());
        else if (a == "--cell-counts") o.cell_counts = need(a.c_str());
        else if (a == "--cell-no-indels") o.cell_no_indels = true;
        else if (a == "--cell-require-barcode") o.cell_require_barcode = true;
        else if (a == "--dup-window") o.dup_window = need_int(16, 64, "a number in 16 .. 64");
        else if (a == "--dup-kmer") o.dup_kmer = need_int(8, 16, "a number in 8 .. 16");
        else if (a == "--dup-max-dist-pct") o.dup_max_dist_pct = need_int(0, 30, "a number in 0 .. 30");
        else if (a == "--dup-max-len-diff-pct") o.dup_max_len_diff_pct = need_int(0, 20, "a number in 0 .. 20");
        else if (a == "--dup-counts") o.dup_counts = need(a.c_str());
        else if (a == "--disable-heuristics") o.o.disable_heuristics = 1;
        else if (a == "--metrics-json") { o.metrics = need(a.c_str()); o.metrics_named = true; }
        else if (a == "--report-json") o.report_json = need(a.c_str());
        else if (a == "--hifi-summary-json") o.hifi_summary = need(a.c_str());
        else if (a == "--log-file") o.log_file = need(a.c_str());
        else if (a == "--refresh-rate") { o.refresh_rate = std::atof(need(a.c_str()).c_str()); if (!(o.refresh_rate >= 0.0)) o.refresh_rate = 0.0; }
        else if (a == "--all" || a == "--all-kinetics" || a == "--subread-fallback" || a == "--split-heteroduplexes" || a == "--hd-finder" || a == "--streamed") {
            // modes of the reference outside this path (OUT OF SCOPE rows): refused by name rather than as a typo
            std::fprintf(stderr, "ccs: %s is not supported by this build (the MI355X consensus path covers the default HiFi mode, --by-strand and --hifi-kinetics)\n", a.c_str());
            std::exit(2);
        }
        else if (a == "-") dash = true;                      // (stdin: no mode reads it; --mark-duplicates says so, the others know no such option)
        else if (!a.empty() && a[0] == '-') { std::fprintf(stderr, "unknown option %s\n", a.c_str()); return false; }
        else pos.push_back(a);
    }
    if (dash && !o.mark_duplicates && !o.cell_reads) { std::fprintf(stderr, "unknown option -\n"); return false; }
    if (!o.cell_reads && (!o.cell_design_text.empty() || !o.cell_whitelist.empty() || !o.cell_counts.empty() || o.cell_no_indels || o.cell_require_barcode)) {
        std::fprintf(stderr, "ccs: the --cell-* options need --cell-reads\n"); std::exit(2);
    }
    if (o.cell_reads) {                                      // a mode of its own, as --mark-duplicates: what it does not take is refused by name, before any input is opened
        static const char *const takes[] = {"--cell-reads", "--cell-design", "--cell-whitelist", "--cell-counts", "--cell-no-indels", "--cell-require-barcode",
                                            "--cdna-primers", "--cdna-min-polya", "--cdna-min-length", "-j", "--num-threads", "--gpus", "--log-level", "--log-file",
                                            "--report-file"};
        for (const std::string &a : o.seen) {
            bool ok = false;
            for (const char *t : takes) ok = ok || a == t;
            if (!ok) { std::fprintf(stderr, "ccs: --cell-reads combined with %s is not supported\n", a.c_str()); std::exit(2); }
        }
        if (dash) { std::fprintf(stderr, "ccs: --cell-reads: input from stdin (-) is not supported\n"); std::exit(2); }
        if (o.all_gpus || o.gpus.size() > 1) { std::fprintf(stderr, "ccs: --cell-reads runs on one GPU: --gpus with more than one device is not supported\n"); std::exit(2); }
        if (pos.size() != 2) { std::fprintf(stderr, "ccs: --cell-reads takes two positionals, IN.bam and OUT.bam\n"); std::exit(2); }
        if (o.cdna_primers.empty() || o.cell_design_text.empty()) { std::fprintf(stderr, "ccs: --cell-reads needs --cdna-primers and --cell-design\n"); std::exit(2); }
        std::string err;
        if (!parse_cell_design(o.cell_design_text, o.cell_design, err)) { std::fprintf(stderr, "ccs: --cell-design %s: %s\n", o.cell_design_text.c_str(), err.c_str()); std::exit(2); }
        if (o.cell_no_indels) o.cell_design.indels = 0;
        if (!o.cell_whitelist.empty()) {
            if (!load_cell_whitelist(o.cell_whitelist, o.cell_design.bc_len, o.cell_codes, err)) {
                std::fprintf(stderr, "ccs: --cell-whitelist %s: %s\n", o.cell_whitelist.c_str(), err.c_str()); std::exit(2);
            }
            o.cell_wl.reset(ccsx_cell_whitelist_create(o.cell_codes.data(), (int32_t)(o.cell_codes.size() / (size_t)o.cell_design.bc_len), o.cell_design.bc_len),
                            ccsx_cell_whitelist_destroy);
            if (!o.cell_wl) { std::fprintf(stderr, "ccs: --cell-whitelist %s: %s\n", o.cell_whitelist.c_str(), ccsx_last_error()); std::exit(2); }
        }
        if (o.cell_require_barcode && !o.cell_wl) { std::fprintf(stderr, "ccs: --cell-require-barcode needs --cell-whitelist\n"); std::exit(2); }
    }
    if (!o.mark_duplicates && (o.dup_remove || o.dup_within_barcodes || o.dup_within_cells || o.dup_window >= 0 || o.dup_kmer >= 0 || o.dup_max_dist_pct >= 0 ||
                               o.dup_max_len_diff_pct >= 0 || !o.dup_counts.empty())) {
        std::fprintf(stderr, "ccs: the --dup-* options need --mark-duplicates\n"); std::exit(2);
    }
    if (o.mark_duplicates) {                                 // a mode of its own: reads in, the same reads out.  It takes its own options, the threads, one device, the
        // log and the report file; every option of the consensus side is refused by name, before any input is opened
        static const char *const takes[] = {"--mark-duplicates", "--dup-remove", "--dup-within-barcodes", "--dup-within-cells", "--dup-window", "--dup-kmer", "--dup-max-dist-pct",
                                            "--dup-max-len-diff-pct", "--dup-counts", "-j", "--num-threads", "--gpus", "--log-level", "--log-file", "--report-file"};
        for (const std::string &a : o.seen) {
            bool ok = false;
            for (const char *t : takes) ok = ok || a == t;
            if (!ok) { std::fprintf(stderr, "ccs: --mark-duplicates combined with %s is not supported\n", a.c_str()); std::exit(2); }
        }
        if (dash) { std::fprintf(stderr, "ccs: --mark-duplicates reads IN twice: input from stdin (-) is not supported\n"); std::exit(2); }
        if (o.dup_within_cells && o.dup_within_barcodes) { std::fprintf(stderr, "ccs: --dup-within-cells combined with --dup-within-barcodes is not supported\n"); std::exit(2); }
        if (o.all_gpus || o.gpus.size() > 1) { std::fprintf(stderr, "ccs: --mark-duplicates runs on one GPU: --gpus with more than one device is not supported\n"); std::exit(2); }
        if (pos.size() != 2) { std::fprintf(stderr, "ccs: --mark-duplicates takes two positionals, IN.bam and OUT.bam\n"); std::exit(2); }
        ccsx_dup_opts_default(&o.dup_opts);
        if (o.dup_window >= 0) o.dup_opts.window = o.dup_window;
        if (o.dup_kmer >= 0) o.dup_opts.kmer = o.dup_kmer;
        if (o.dup_max_dist_pct >= 0) o.dup_opts.max_dist_pct = o.dup_max_dist_pct;
        if (o.dup_max_len_diff_pct >= 0) o.dup_opts.max_len_diff_pct = o.dup_max_len_diff_pct;
        if (o.dup_opts.kmer > o.dup_opts.window) { std::fprintf(stderr, "ccs: --dup-kmer %d is above --dup-window %d\n", o.dup_opts.kmer, o.dup_opts.window); std::exit(2); }
    }
    if (!o.cdna_primers.empty() && !o.cell_reads) {          // its own output mode: refused before any input is opened
        auto refuse = [](const char *what) { std::fprintf(stderr, "ccs: --cdna-primers combined with %s is not supported\n", what); std::exit(2); };
        if (o.by_strand) refuse("--by-strand");
        if (!o.barcodes.empty()) refuse("--barcodes");
        if (!o.segment_adapters.empty()) refuse("--segment-adapters");
        if (o.reads_bam) refuse("--reads-bam");
        if (o.heteroduplexes) refuse("--heteroduplexes");
        if (!o.fit_model.empty()) refuse("--fit-model");
    }
    if (!o.segment_adapters.empty()) {                       // its own output mode: refused before any input is opened
        auto refuse = [](const char *what) { std::fprintf(stderr, "ccs: --segment-adapters combined with %s is not supported\n", what); std::exit(2); };
        if (o.by_strand) refuse("--by-strand");
        if (!o.barcodes.empty()) refuse("--barcodes");
        if (o.reads_bam) refuse("--reads-bam");
        if (o.heteroduplexes) refuse("--heteroduplexes");
        if (!o.fit_model.empty()) refuse("--fit-model");
    }
    if (o.heteroduplexes) {                                  // its own output mode: the options that make another kind of record, or that need the strands on the host
        auto refuse = [](const char *what) { std::fprintf(stderr, "ccs: --heteroduplexes combined with %s is not supported\n", what); std::exit(2); };
        if (o.by_strand) refuse("--by-strand");
        if (o.reads_bam) refuse("--reads-bam");
        if (!o.barcodes.empty()) refuse("--barcodes");
        if (!o.fit_model.empty()) refuse("--fit-model");
        if (o.orient_passes) refuse("--orient-passes");      // (the host would need the strand bits the device resolved to split a ZMW's passes)
    }
    if ((o.reads_kinetics || o.reads_fallback) && !o.reads_bam) {
        std::fprintf(stderr, "ccs: --reads-bam-kinetics and --reads-bam-subread-fallback need --reads-bam\n"); std::exit(2);
    }
    if (o.reads_bam) {                                       // docs/faq/mode-all.md:13-37: the filters of the mode are fixed, and it is its own output mode
        auto fixed = [](const char *what) { std::fprintf(stderr, "ccs: %s can't be changed with --reads-bam (it sets --min-passes 2, --min-rq 0 and the engine's maximum length)\n", what); std::exit(2); };
        auto refuse = [](const char *what) { std::fprintf(stderr, "ccs: --reads-bam combined with %s is not supported\n", what); std::exit(2); };
        if (o.min_passes_set) fixed("--min-passes");
        if (o.min_rq_set) fixed("--min-rq");
        if (o.max_length_set) fixed("--max-length");
        if (o.by_strand) refuse("--by-strand");
        if (!o.fail_reads.empty()) refuse("--fail-reads");
        if (o.coverage_filters) refuse("--coverage-filters");
        if (!o.barcodes.empty()) refuse("--barcodes");
        if (!o.fit_model.empty()) refuse("--fit-model");
        o.o.min_passes = 2; o.o.min_rq = 0.0f;
        o.o.max_length = 65535 + 65535 / 4 + 64;             // the longest draft the engine holds: the slot of its longest subread
        if (o.reads_kinetics) o.o.hifi_kinetics = 1;
    }
    if (!o.fit_model.empty()) {                              // the training mode takes nothing of the output side: refused before any of those options is looked at
        auto refuse = [](const char *what) { std::fprintf(stderr, "ccs: --fit-model %s\n", what); std::exit(2); };
        if (!o.fail_reads.empty()) refuse("combined with --fail-reads is not supported");
        if (o.by_strand) refuse("combined with --by-strand is not supported");
        if (o.gpus.size() > 1) refuse("runs on one GPU: --gpus with more than one device is not supported");
        if (o.fit_iterations < 1 || o.fit_max_zmws < 0 || o.fit_degree > 3 || o.fit_degree < -1 || !(o.fit_min_rq >= 0.0 && o.fit_min_rq <= 1.0))
            refuse("options out of range (--fit-iterations >= 1, --fit-max-zmws >= 0, --fit-degree 0 .. 3, --fit-min-rq in [0, 1])");
        if (o.dump || o.host_only) refuse("combined with --dump-zmws or --host-only is not supported");
        // nothing of the output side runs in this mode: an option that would be ignored is refused, not dropped silently
        if (!o.control.empty() || !o.adapters.empty() || o.coverage_filters)
            refuse("runs no draft screen: --control, --adapters and --coverage-filters are not supported with it");
        if (o.gpu_inflate) refuse("combined with --gpu-inflate is not supported");
        if (o.gpu_deflate) refuse("combined with --gpu-deflate is not supported");
        if (o.report_named || o.metrics_named || !o.report_json.empty() || !o.hifi_summary.empty() || o.suppress_reports)
            refuse("writes no reports: --report-file, --metrics-json, --report-json, --hifi-summary-json and --suppress-reports are not supported with it");
        if (o.pileup || o.qv_binning || o.o.hifi_kinetics || o.min_tandem > 0)
            refuse("writes no reads: --pileup-summary, --qv-binning, --hifi-kinetics and --min-tandem-repeat-length are not supported with it");
        if (o.chunk_n > 1) refuse("reads the whole file: --chunk is not supported with it");
        if (!o.barcodes.empty()) refuse("writes no reads: --barcodes is not supported with it");
    }
    if (o.orient_passes && o.by_strand) {                    // the strands are split on the host, before the engine has seen a pass
        std::fprintf(stderr, "ccs: --orient-passes combined with --by-strand is not supported\n"); std::exit(2);
    }
    if (!o.fail_reads.empty()) {
        if (o.fail_reads.size() < 5 || o.fail_reads.compare(o.fail_reads.size() - 4, 4, ".bam") != 0) {
            std::fprintf(stderr, "ccs: --fail-reads needs a path ending in .bam, got '%s'\n", o.fail_reads.c_str()); std::exit(2);
        }
        if (o.by_strand) { std::fprintf(stderr, "ccs: --fail-reads combined with --by-strand is not supported\n"); std::exit(2); }
    }
    if (!o.adapters.empty()) {
        if (o.fail_reads.empty()) { std::fprintf(stderr, "ccs: --adapters needs --fail-reads (the reads it flags are written there)\n"); std::exit(2); }
        std::string err;
        if (!load_adapters(o.adapters, o.adapter_set, err)) { std::fprintf(stderr, "ccs: --adapters %s: %s\n", o.adapters.c_str(), err.c_str()); std::exit(2); }
    }
    if (o.barcodes.empty() && (o.barcode_window >= 0 || !o.barcode_counts.empty())) {
        std::fprintf(stderr, "ccs: --barcode-window and --barcode-counts need --barcodes\n"); std::exit(2);
    }
    if (!o.barcodes.empty()) {
        if (o.by_strand) { std::fprintf(stderr, "ccs: --barcodes combined with --by-strand is not supported\n"); std::exit(2); }
        std::string err;
        o.barcode_set = std::make_shared<ccsx_barcode_set>();
        if (!load_barcodes(o.barcodes, *o.barcode_set, o.barcode_names, err)) { std::fprintf(stderr, "ccs: --barcodes %s: %s\n", o.barcodes.c_str(), err.c_str()); std::exit(2); }
        ccsx_barcode_opts_default(&o.barcode_opts);
        if (o.barcode_window >= 0) o.barcode_opts.window = o.barcode_window;
    }
    if (o.segment_adapters.empty() && (o.segment_min_length >= 0 || !o.segment_counts.empty())) {
        std::fprintf(stderr, "ccs: --segment-min-length and --segment-counts need --segment-adapters\n"); std::exit(2);
    }
    if (!o.segment_adapters.empty()) {
        std::string err;
        o.segment_set = std::make_shared<ccsx_segment_set>();
        if (!load_segment_adapters(o.segment_adapters, *o.segment_set, err)) { std::fprintf(stderr, "ccs: --segment-adapters %s: %s\n", o.segment_adapters.c_str(), err.c_str()); std::exit(2); }
        ccsx_segment_opts_default(&o.segment_opts);
        if (o.segment_min_length >= 0) o.segment_opts.min_len = o.segment_min_length;
    }
    if (o.cdna_primers.empty() && (o.cdna_min_polya >= 0 || o.cdna_min_length >= 0 || !o.cdna_counts.empty())) {
        std::fprintf(stderr, "ccs: --cdna-min-polya, --cdna-min-length and --cdna-counts need --cdna-primers\n"); std::exit(2);
    }
    if (!o.cdna_primers.empty()) {
        std::string err;
        o.cdna_set = std::make_shared<ccsx_cdna_set>();
        if (!load_cdna_primers(o.cdna_primers, *o.cdna_set, err)) { std::fprintf(stderr, "ccs: --cdna-primers %s: %s\n", o.cdna_primers.c_str(), err.c_str()); std::exit(2); }
        ccsx_cdna_opts_default(&o.cdna_opts);
        if (o.cdna_min_polya >= 0) o.cdna_opts.min_polya = o.cdna_min_polya;
        if (o.cdna_min_length >= 0) o.cdna_opts.min_len = o.cdna_min_length;
    }
    if (!o.control.empty()) {
        std::string err;
        if (!load_control(o.control, o.control_codes, err)) { std::fprintf(stderr, "ccs: --control %s: %s\n", o.control.c_str(), err.c_str()); std::exit(2); }
        o.control_seq = ccsx_control_seq{(int32_t)o.control_codes.size(), 0, o.control_codes.data()};
    }
    if (!o.coverage_filters && (o.cov_drop_percent >= 0 || o.cov_block >= 0)) {
        std::fprintf(stderr, "ccs: --coverage-drop-percent and --coverage-block need --coverage-filters\n"); std::exit(2);
    }
    ccsx_coverage_opts_default(&o.coverage_opts);
    if (o.cov_drop_percent >= 0) o.coverage_opts.drop_percent = o.cov_drop_percent;
    if (o.cov_block >= 0) o.coverage_opts.block = o.cov_block;
    // --top-passes 0 = unlimited (docs/faq/accuracy-vs-passes.md:49-52); the engine takes up to CCSX_MAX_PASSES = 255 per ZMW (SPEC v5)
    if (o.o.top_passes <= 0) o.o.top_passes = CCSX_MAX_PASSES;
    if (o.o.top_passes > CCSX_MAX_PASSES) {
        std::fprintf(stderr, "ccs: warning: --top-passes %d: this engine uses at most %d passes per ZMW (those closest to the median length)\n", o.o.top_passes, CCSX_MAX_PASSES);
        o.o.top_passes = CCSX_MAX_PASSES;
    }
    if (!o.write_synth.empty()) { if (pos.size() != 1) return false; o.out = pos[0]; return true; }
    if (!o.fit_model.empty()) {                              // the training mode: one positional, one GPU, nothing of the output side
        auto refuse = [](const char *what) { std::fprintf(stderr, "ccs: --fit-model %s\n", what); std::exit(2); };
        if (pos.size() != 1) refuse("takes one positional, IN.subreads.bam: it writes OUT.json and no reads");
        o.in = pos[0]; if (o.batch < 0) o.batch = 0;
        return true;
    }
    if (o.dump || o.host_only) { if (pos.size() != 1) return false; o.in = pos[0]; if (o.batch < 0) o.batch = 0; return true; }
    if (pos.size() != 2) return false;
    o.in = pos[0]; o.out = pos[1];
    {
        std::string p = o.out; size_t d = p.rfind(".bam"); if (d == std::string::npos) d = p.rfind(".fastq.gz"); if (d != std::string::npos) p = p.substr(0, d);
        if (o.report.empty()) o.report = p + ".ccs_report.txt";
        if (o.metrics.empty()) o.metrics = p + ".zmw_metrics.json.gz";
    }
    if (o.batch < 0) o.batch = 0;
    return true;
}

// host threads the process may actually use: affinity mask and cgroup CPU quota (a container can expose 256 logical CPUs
// with a 16-CPU quota; over-subscribing the quota makes the BGZF pool slower, not faster)
int effective_cores()
{
    int n = (int)std::thread::hardware_concurrency();
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof(set), &set) == 0) { const int c = CPU_COUNT(&set); if (c > 0 && c < n) n = c; }
    auto quota = [](const char *path, bool v2) -> double {
        FILE *f = std::fopen(path, "r");
        if (!f) return 0.0;
        char a[64] = {0}; long long per = 100000, q = -1;
        double r = 0.0;
        if (v2) { if (std::fscanf(f, "%63s %lld", a, &per) >= 1 && std::strcmp(a, "max") != 0) r = std::atof(a) / (double)(per > 0 ? per : 100000); }
        else if (std::fscanf(f, "%lld", &q) == 1 && q > 0) {
            FILE *g = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r");
            if (g) { if (std::fscanf(g, "%lld", &per) != 1) per = 100000; std::fclose(g); }
            r = (double)q / (double)(per > 0 ? per : 100000);
        }
        std::fclose(f);
        return r;
    };
    double q = quota("/sys/fs/cgroup/cpu.max", true);
    if (q <= 0.0) q = quota("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", false);
    if (q > 0.0) { const int c = (int)std::ceil(q); if (c < n) n = c; }
    return n < 1 ? 1 : n;
}

std::string movie_of(const std::string &qname) { const size_t p = qname.find('/'); return p == std::string::npos ? qname : qname.substr(0, p); }

// ---- synthetic subreads.bam (test helper) ----------------------------------------------------------
int write_synthetic(const Options &o, ThreadPool &pool)
{
    int n = 0, P = 0, P2 = 0, L = 0, L2 = 0, partial = 0; unsigned long long seed = 1;   // n,passes,length[,seed[,1]]: a fifth field 1 = the first and the last
    // subread of every ZMW are PARTIAL passes (one adapter only, truncated at the polymerase read's start / end); passes and length may be
    // ranges LO-HI (uniform / log-uniform: the BASELINE configs[4] mix is 3-50,1000-25000)
    {
        std::vector<std::string> f;
        size_t a = 0;
        for (;;) { const size_t c = o.write_synth.find(',', a); f.push_back(o.write_synth.substr(a, c == std::string::npos ? c : c - a)); if (c == std::string::npos) break; a = c + 1; }
        auto span = [](const std::string &t, int &lo, int &hi) { const size_t d = t.find('-'); lo = std::atoi(t.c_str()); hi = d == std::string::npos ? lo : std::atoi(t.c_str() + d + 1); };
        if (f.size() < 3) { std::fprintf(stderr, "bad --write-synthetic\n"); return 2; }
        n = std::atoi(f[0].c_str()); span(f[1], P, P2); span(f[2], L, L2);
        if (f.size() > 3) seed = std::strtoull(f[3].c_str(), nullptr, 10);
        if (f.size() > 4) partial = std::atoi(f[4].c_str());
        if (n < 1 || P < 1 || P2 < P || L < 1 || L2 < L) { std::fprintf(stderr, "bad --write-synthetic\n"); return 2; }
    }
    ccsx_synth *s = nullptr;
    if (ccsx_synth_generate(n, 1000, P, P2, L, L2, seed, &s)) { std::fprintf(stderr, "%s\n", ccsx_last_error()); return 1; }
    BgzfWriter out(o.out, pool);
    const std::string movie = "m64000_synth";
    write_header(out, "@HD\tVN:1.6\tSO:unknown\tpb:5.0.0\n@RG\tID:synth001\tPL:PACBIO\tDS:READTYPE=SUBREAD;Ipd:CodecV1=ip;PulseWidth:CodecV1=pw;"
                      "BINDINGKIT=101-789-500;SEQUENCINGKIT=101-826-100;BASECALLERVERSION=5.0.0;FRAMERATEHZ=100.000000\tPU:" + movie + "\tPM:SEQUELII\n");
    const ccsx_batch &b = s->batch;
    RecordBuilder rb;
    PbiIndex pbi; std::vector<uint64_t> marks;
    for (int z = 0; z < b.n_zmw; ++z) {
        int64_t q = 0;
        for (int r = b.read_off[z]; r < b.read_off[z + 1]; ++r) {
            int64_t a = b.base_off[r], len = b.base_off[r + 1] - a;
            int cxa = 3;                                                          // ADAPTER_BEFORE | ADAPTER_AFTER
            if (partial && b.read_off[z + 1] - b.read_off[z] >= 3) {
                if (r == b.read_off[z]) { a += len / 2; len -= len / 2; cxa = 2; }               // sequencing started inside the insert
                else if (r == b.read_off[z + 1] - 1) { len = (6 * len) / 10; cxa = 1; }          // ... and ended inside it
            }
            const std::string name = movie + "/" + std::to_string(b.zmw_id[z]) + "/" + std::to_string(q) + "_" + std::to_string(q + len);
            rb.begin(name, b.bases + a, nullptr, (uint32_t)len);
            rb.tagZ("RG", "synth001");
            rb.tagi("zm", b.zmw_id[z]);
            rb.tagi("qs", (int32_t)q); rb.tagi("qe", (int32_t)(q + len));
            rb.tagf("rq", 0.8f);
            rb.tagBf("sn", b.snr + 4 * z, 4);
            rb.tagBC("ip", b.ipd + a, (uint32_t)len);
            rb.tagBC("pw", b.pw + a, (uint32_t)len);
            rb.tagC("cx", (uint8_t)(cxa | ((b.flags[r] & 1) ? 32 : 16)));    // adapters + FORWARD/REVERSE_PASS
            marks.push_back(out.mark());
            pbi.rg_id.push_back(0); pbi.q_start.push_back((int32_t)q); pbi.q_end.push_back((int32_t)(q + len)); pbi.hole.push_back(b.zmw_id[z]);
            pbi.read_qual.push_back(0.8f); pbi.ctxt.push_back((uint8_t)cxa);
            rb.finish(out);
            q += len + 45;
        }
    }
    out.close();
    for (uint64_t m : marks) pbi.file_offset.push_back((int64_t)out.virtual_offset(m));
    write_pbi(o.out + ".pbi", pool, pbi);
    ccsx_synth_free(s);
    return 0;
}

// ---- step-1 filters (docs/how-does-ccs-work.md:19-32) ----------------------------------------------
void finish_zmw(ZmwIn &z, const Options &o)
{
    for (auto &r : z.reads) z.polymerase_len += (int64_t)r.size() + 45;   // + adapter between consecutive subreads
    if (z.reads.empty()) { z.host_status = HS_NO_SUBREADS; return; }
    if (!o.fail_reads.empty()) {                                  // fail record 0x8: the median-length full-length subread (ties: the first in file order)
        std::vector<uint32_t> fl;
        for (auto &r : z.reads) if ((r.cx < 0) || ((r.cx & 3) == 3)) fl.push_back(r.len);
        if (!fl.empty()) {
            std::vector<uint32_t> s1 = fl;
            std::nth_element(s1.begin(), s1.begin() + s1.size() / 2, s1.end());
            const uint32_t m = s1[s1.size() / 2];
            for (auto &r : z.reads)
                if (((r.cx < 0) || ((r.cx & 3) == 3)) && r.len == m) { z.fl_name = r.name; z.fl_seq.resize(r.len); r.decode_bases(z.fl_seq.data()); break; }
        }
    }
    {
        std::vector<size_t> s0;
        for (auto &r : z.reads) s0.push_back(r.size());
        std::nth_element(s0.begin(), s0.begin() + s0.size() / 2, s0.end());
        z.median_len = (int32_t)s0[s0.size() / 2];
        for (auto &r : z.reads) z.n_full += ((r.cx < 0) || ((r.cx & 3) == 3)) ? 1 : 0;
    }
    float mn = z.snr[0];
    for (int c = 1; c < 4; ++c) mn = std::min(mn, z.snr[c]);
    if (mn < (float)o.min_snr) { z.host_status = HS_POOR_SNR; z.reads.clear(); return; }
    std::vector<size_t> lens;
    for (auto &r : z.reads) lens.push_back(r.size());
    std::vector<size_t> s = lens;
    std::nth_element(s.begin(), s.begin() + s.size() / 2, s.end());
    const double med = (double)s[s.size() / 2];
    std::vector<Subread> keep, part;
    bool any_len_ok = false;
    for (auto &r : z.reads) {
        const double l = (double)r.size();
        const bool full = (r.cx < 0) || ((r.cx & 3) == 3);       // flanked by adapters (docs/faq/accuracy-vs-passes.md:17-18)
        // partial passes (one adapter only: the first / last subread of the polymerase read) are not passes, but the polish uses them
        // where they reach (docs/faq/accuracy-vs-passes.md:26-29: ec ~ np + 1); they are shorter by nature: no lower length bound
        // (--reads-bam: a subread with no adapter flag at all is submitted as a partial pass too)
        const bool partial = !full && r.cx >= 0 && ((r.cx & 3) != 0 || o.reads_bam) && l >= 50.0 && l <= 2.0 * med && !o.no_partial;
        if (partial && !r.has_n) {
            // a subread inside [0.5, 2] x median is not a "Median length filter" case whatever its adapters (docs/faq/reports-aux-files.md:26-27:
            // that category means ALL subreads are outside); a ZMW with one-adapter subreads only ends as "Lacking full passes" 
            if (l >= 0.5 * med) any_len_ok = true;
            // the engine's subread limit and the --max-length margin hold for partial passes too: an over-long one is dropped, it never
            // fails the ZMW or the batch (a > 65535-base partial pass used to make ccsx_submit refuse the whole batch)
            if (r.size() > 65535 || l > 1.3 * (double)o.o.max_length + 1000.0) continue;
            r.partial = (uint8_t)((r.cx & 3) == 2 ? 6 : 2);      // cx ADAPTER_AFTER only: the adapter is at the pass's end
            part.push_back(std::move(r));
            continue;
        }
        if (l < 0.5 * med || l > 2.0 * med) continue;            // length filter
        any_len_ok = true;
        if (!full || r.has_n || r.size() == 0) continue;
        keep.push_back(std::move(r));
    }
    z.reads.swap(keep);
    if (!any_len_ok) { z.host_status = HS_NO_SUBREADS; z.reads.clear(); return; }
    // the engine handles subreads up to 65535 bases; longer inserts cannot pass --max-length (<= 50000) anyway
    for (auto &r : z.reads) if (r.size() > 65535 || (double)r.size() > 1.3 * (double)o.o.max_length + 1000.0) { z.host_status = HS_TOO_LONG; z.reads.clear(); return; }
    // --reads-bam: a ZMW with any subread left is submitted; the engine says TOO_FEW_PASSES and the representative rule picks a subread
    if ((int)z.reads.size() < o.o.min_passes && !(o.reads_bam && z.reads.size() + part.size() >= 1)) { z.host_status = HS_TOO_FEW; z.reads.clear(); return; }
    // --top-passes: "at most the top 60 full-length passes after sorting by median length" (docs/faq/accuracy-vs-passes.md:49-52):
    // the N passes whose length is closest to the median are kept, in their original order
    const size_t top = (size_t)o.o.top_passes;
    if (z.reads.size() > top) {
        std::vector<size_t> idx(z.reads.size());
        for (size_t i = 0; i < idx.size(); ++i) idx[i] = i;
        auto dist = [&](size_t i) { const double d = (double)z.reads[i].size() - med; return d < 0 ? -d : d; };
        std::stable_sort(idx.begin(), idx.end(), [&](size_t a, size_t b) { return dist(a) < dist(b); });
        idx.resize(top);
        std::sort(idx.begin(), idx.end());
        std::vector<Subread> sel;
        for (size_t i : idx) sel.push_back(std::move(z.reads[i]));
        z.reads.swap(sel);
    }
    // the engine wants a ZMW's partial passes behind its full-length passes; it uses at most CCSX_MAX_PASSES in all
    for (auto &r : part) if (z.reads.size() < (size_t)CCSX_MAX_PASSES) z.reads.push_back(std::move(r));
}

struct ArenaPool {                          // free list of page-locked arenas: a batch holds its staging until its results are written
    std::mutex m;
    std::vector<std::unique_ptr<Arena>> free_;
    std::unique_ptr<Arena> get()
    {
        std::lock_guard<std::mutex> l(m);
        if (free_.empty()) return std::unique_ptr<Arena>(new Arena());
        auto a = std::move(free_.back()); free_.pop_back();
        return a;
    }
    void put(std::unique_ptr<Arena> a) { if (a) { std::lock_guard<std::mutex> l(m); free_.push_back(std::move(a)); } }
};

// returns the passes packed strand-unknown (--orient-passes)
long long pack(Batch &b, Arena &arena)
{
    long long unknown = 0;
    b.read_off.assign(1, 0); b.base_off.assign(1, 0);
    b.slot.assign(b.zmws.size(), -1);
    int64_t total = 0;
    for (const ZmwIn &z : b.zmws) if (z.host_status == HS_OK) for (const Subread &r : z.reads) total += (int64_t)r.size();
    uint8_t *base = arena.reserve((size_t)3 * (size_t)total);
    uint8_t *bases = base, *pw = base + total, *ipd = base + 2 * total;
    int64_t at = 0;
    for (size_t i = 0; i < b.zmws.size(); ++i) {
        ZmwIn &z = b.zmws[i];
        if (z.host_status != HS_OK) continue;
        b.slot[i] = (int)b.zmw_id.size();
        b.zmw_id.push_back(z.zm);
        b.snr.insert(b.snr.end(), z.snr, z.snr + 4);
        for (size_t k = 0; k < z.reads.size(); ++k) {
            Subread &r = z.reads[k];
            const size_t L = r.size();
            r.decode_bases(bases + at); r.decode_pw(pw + at); r.decode_ip(ipd + at);      // the one and only decode: record -> staging
            at += (int64_t)L;
            b.flags.push_back((uint8_t)(r.strand | r.partial | (r.strand_unknown ? CCSX_PASS_STRAND_UNKNOWN : 0)));
            unknown += r.strand_unknown;
            b.base_off.push_back(at);
            r.keep.reset(); r.seq = r.pw_p = r.ip_p = nullptr;                              // the inflated bytes may go
        }
        b.read_off.push_back((int32_t)b.flags.size());
    }
    b.bases = bases; b.pw = pw; b.ipd = ipd; b.n_bases = total;
    return unknown;
}

struct Report {
    int64_t input = 0, pass = 0;
    std::map<std::string, int64_t> fail;
    std::vector<int32_t> lens; std::vector<float> rqs; std::vector<int32_t> nps;   // one entry per written read
    int64_t bases_q30 = 0;        // written bases with a phred QV >= 30 ("Base quality >=Q30 (bp)", docs/faq/reports-aux-files.md:66)
    int64_t rep_cls[4] = {0, 0, 0, 0};   // --reads-bam: submitted ZMWs per ccsx_represent_class (POLISHED, NONE, DRAFT, SUBREAD)
    int64_t tandem = 0;           // ZMWs flagged as tandem repeats (--min-tandem-repeat-length; docs/faq/reports-aux-files.md:22)
    int64_t fail_records = 0;     // records written to --fail-reads
    int64_t control = 0;          // ZMWs the control screen found (--control), whatever their final status
    int64_t coverage = 0;         // ZMWs the coverage screen's gate took (--coverage-filters)
    int64_t bc_tested = 0, bc_call[4] = {0, 0, 0, 0};           // --barcodes: HiFi reads tested, and by call: none, head only, tail only, both ends
    int64_t sg_tested = 0, sg_complete = 0, sg_with = 0, sg_without = 0, sg_overflow = 0, sg_written = 0, sg_leftover = 0;   // --segment-adapters, over the HiFi reads
    int64_t cd_tested = 0, cd_cls[7] = {0, 0, 0, 0, 0, 0, 0};     // --cdna-primers, over the HiFi reads: per class of the rule
    std::map<std::array<int, 2>, int64_t> cd_classes;             // ... reads per (class, strand)
    std::map<std::array<int, 3>, int64_t> sg_classes;             // ... reads per (segments per read, orientation, complete)
    std::map<std::pair<int, int>, int64_t> bc_pairs;              // ... reads per called pair (head, tail)
    int64_t hd_zmws = 0;          // --heteroduplexes: ZMWs the split took (split: written as single-strand reads; drop: the "Heteroduplex insertions" row)
    // --heteroduplexes split: the single-strand column of the report.  It counts reads, not ZMWs (mode-heteroduplex-filtering.md:86-90); `input`, `pass`, `fail`
    // and `tandem` above are then the double-strand column plus hd_zmws in `input`
    int64_t ss_input = 0, ss_pass = 0, ss_tandem = 0;
    std::map<std::string, int64_t> ss_fail;
    std::vector<uint8_t> ss;      // per written read, beside lens / rqs / nps: 1 = a single-strand read
    std::vector<int32_t> holes;   // ... and its ZMW
};

// cov: --coverage-filters.  Under it "Reads failed polishing" counts what the reference counts there, the reads lost while polishing; the engine's "more than
// half of the passes must map" rule is an end-to-end alignment rule and moves to "Insufficient draft cov"
const char *fail_label(int st, bool cov = false)
{
    switch (st) {
        case CCSX_COVERAGE_DROPS: return "Coverage drops";
        case CCSX_INSUFFICIENT_SPANS: return "Insufficient draft cov";
        case CCSX_DRAFT_TOO_DIFFERENT: return "Draft too different";
        case CCSX_READS_FAILED_POLISHING: return "Reads failed polishing";
        case CCSX_HETERODUPLEX: return "Heteroduplex insertions";
        case HS_POOR_SNR: return "Below SNR threshold";
        case HS_NO_SUBREADS: return "Median length filter";
        case HS_TOO_FEW: case CCSX_TOO_FEW_PASSES: return "Lacking full passes";
        case CCSX_DRAFT_FAILURE: return "Draft generation error";
        case CCSX_TOO_MANY_UNUSABLE: return cov ? "Insufficient draft cov" : "Reads failed polishing";
        case CCSX_NON_CONVERGENT: return "CCS did not converge";
        case CCSX_TOO_SHORT: return "Draft below --min-length";
        case CCSX_TOO_LONG: case HS_TOO_LONG: return "Draft above --max-length";
        case CCSX_LOW_RQ: return "CCS below minimum RQ";
        case CCSX_EMPTY_WINDOW: return "Empty coverage windows";
        case CCSX_CAPACITY: return "Consensus outgrew its buffer";
        case HS_ADAPTER_PALINDROME: return "CCS adapter palindrome";
        case HS_ADAPTER_CONCAT: return "CCS adapter concatenation";
        case HS_ADAPTER_NEAR_END: return "CCS adapter near end";
        case HS_CONTROL_SUCCESS: return "ZMW with control success";
        case HS_CONTROL_FAILURE: return "ZMW with control failure";
        default: return "Unknown error";
    }
}

const char *status_name(int st, bool cov = false)
{
    switch (st) {   // docs/faq/reports-aux-files.md:143-159
        case CCSX_COVERAGE_DROPS: return "COVERAGE_DROPS";
        case CCSX_INSUFFICIENT_SPANS: return "INSUFFICIENT_SPANS";
        case CCSX_DRAFT_TOO_DIFFERENT: return "TOO_FEW_PASSES_AFTER_DRAFT_ALIGNMENT";
        case CCSX_READS_FAILED_POLISHING: return "TOO_MANY_UNUSABLE";
        case CCSX_HETERODUPLEX: return "HETERODUPLEXES";
        case CCSX_SUCCESS: return "SUCCESS";
        case HS_POOR_SNR: return "POOR_SNR";
        case HS_NO_SUBREADS: return "NO_SUBREADS";
        case HS_TOO_FEW: case CCSX_TOO_FEW_PASSES: return "TOO_FEW_PASSES";
        case CCSX_DRAFT_FAILURE: return "DRAFT_FAILURE";
        case CCSX_TOO_MANY_UNUSABLE: return cov ? "INSUFFICIENT_SPANS" : "TOO_MANY_UNUSABLE";
        case CCSX_NON_CONVERGENT: return "NON_CONVERGENT";
        case CCSX_TOO_SHORT: return "TOO_SHORT";
        case CCSX_TOO_LONG: case HS_TOO_LONG: return "TOO_LONG";
        case CCSX_LOW_RQ: return "POOR_QUALITY";
        case CCSX_EMPTY_WINDOW: return "EMPTY_WINDOW_DURING_POLISHING";
        case CCSX_CAPACITY: return "CAPACITY";
        case HS_ADAPTER_PALINDROME: return "ADAPTER_PALINDROME";
        case HS_ADAPTER_CONCAT: return "ADAPTER_CONCATENATION";
        case HS_ADAPTER_NEAR_END: return "ADAPTER_NEAR_END";
        case HS_CONTROL_SUCCESS: return "CONTROL_SUCCESS";
        case HS_CONTROL_FAILURE: return "CONTROL_FAILURE";
        default: return "EXCEPTION_THROWN";
    }
}

// the rows of "Exclusive failed counts" this path can produce, in the order of docs/faq/reports-aux-files.md:24-46 (the rows of the subsystems
// outside this path, and without their options the heteroduplex, coverage, adapter and control classes, cannot occur and are not listed)
const char *const kFailOrder[] = {"Below SNR threshold", "Median length filter", "Lacking full passes", "Draft generation error",
                                  "Draft above --max-length", "Draft below --min-length", "Reads failed polishing", "Empty coverage windows",
                                  "CCS did not converge", "CCS below minimum RQ", "Consensus outgrew its buffer", "Unknown error"};

// the rows printed: with --coverage-filters the three coverage rows after "Lacking full passes", where the reference lists them; with --fail-reads also "CCS adapter palindrome" (now a failure) and "ZMW with full-length subread" (the 0x8 records), with --control the two
// control rows, where the reference lists them
std::vector<const char *> fail_order(const Options &o)
{
    std::vector<const char *> v;
    for (const char *k : kFailOrder) {
        if (!o.fail_reads.empty() && std::string(k) == "CCS below minimum RQ") {
            v.push_back("CCS adapter palindrome");
            if (!o.adapters.empty()) { v.push_back("CCS adapter concatenation"); v.push_back("CCS adapter near end"); }   // (--adapters: the screen's two classes)
            v.push_back("ZMW with full-length subread");
        }
        if (!o.control.empty() && std::string(k) == "CCS below minimum RQ") { v.push_back("ZMW with control failure"); v.push_back("ZMW with control success"); }
        v.push_back(k);
        if (o.heteroduplexes == HD_DROP && std::string(k) == "Lacking full passes") v.push_back("Heteroduplex insertions");   // (where the reference lists it)
        if (o.coverage_filters && std::string(k) == "Lacking full passes") { v.push_back("Coverage drops"); v.push_back("Insufficient draft cov"); v.push_back("Draft too different"); }
    }
    return v;
}

// statistics of one class of written reads (docs/faq/reports-aux-files.md:52-64: HiFi = predicted accuracy >= Q20, "<Q20", ">=Q30")
struct ReadClass {
    int64_t reads = 0, yield = 0, len_mean = 0, len_median = 0, n50 = 0, np_mean = 0;
    int qual_median = 0;
};

int rq_to_q(float rq) { return rq >= 1.0f ? 60 : (int)std::floor(-10.0 * std::log10(1.0 - (double)rq) + 1e-9); }

ReadClass classify(const Report &r, float rq_lo, float rq_hi)
{
    ReadClass c;
    std::vector<int32_t> len; std::vector<float> rq; int64_t nps = 0;
    for (size_t i = 0; i < r.lens.size(); ++i)
        if (r.rqs[i] >= rq_lo && r.rqs[i] < rq_hi) { len.push_back(r.lens[i]); rq.push_back(r.rqs[i]); nps += r.nps[i]; c.yield += r.lens[i]; }
    c.reads = (int64_t)len.size();
    if (len.empty()) return c;
    std::sort(len.begin(), len.end()); std::sort(rq.begin(), rq.end());
    c.len_mean = c.yield / c.reads;
    c.len_median = len[len.size() / 2];
    c.qual_median = rq_to_q(rq[rq.size() / 2]);
    c.np_mean = nps / c.reads;
    int64_t acc = 0;                                            // N50: the length L such that reads of length >= L hold half of the yield
    for (size_t i = len.size(); i-- > 0;) { acc += len[i]; if (2 * acc >= c.yield) { c.n50 = len[i]; break; } }
    return c;
}

std::string with_commas(int64_t v)                              // 63881 -> "63,881", as the reference prints its yield / length rows
{
    std::string d = std::to_string(v < 0 ? -v : v), o;
    for (size_t i = 0; i < d.size(); ++i) { if (i && (d.size() - i) % 3 == 0) o += ','; o += d[i]; }
    return v < 0 ? "-" + o : o;
}

void write_report(const Options &o, const Report &r)
{
    const int64_t failed = r.input - r.pass;
    auto pct = [](int64_t a, int64_t b) { return b ? 100.0 * (double)a / (double)b : 0.0; };
    const ReadClass hifi = classify(r, 0.99f, 2.0f), lowq = classify(r, -1.0f, 0.99f), q30 = classify(r, 0.999f, 2.0f);
    int64_t all_bases = 0;
    for (int32_t l : r.lens) all_bases += l;
    if (FILE *f = std::fopen(o.report.c_str(), "w")) {
        if (o.heteroduplexes == HD_SPLIT) {
            // the two columns of mode-heteroduplex-filtering.md:92-117: reads, not ZMWs.  Inputs: of the ZMWs; every other percentage: of its column's Inputs
            // (Passed, Failed, Tandem repeats) or of its column's Failed (the exclusive counts).  Rows, labels and order are this driver's
            const int64_t ds_in = r.input - r.hd_zmws, ds_fail = ds_in - r.pass, ss_failed = r.ss_input - r.ss_pass;
            auto row2 = [&](const char *label, int64_t a, double pa, int64_t b, double pb) {
                std::fprintf(f, "%-30s: %10" PRId64 " (%6.2f%%) %11" PRId64 " (%6.2f%%)\n", label, a, pa, b, pb);
            };
            std::fprintf(f, "%-30s  %20s %20s\n", "", "Double-Strand Reads", "Single-Strand Reads");
            row2("Inputs", ds_in, pct(ds_in, r.input), r.ss_input, pct(r.ss_input, r.input));
            std::fprintf(f, "\n");
            row2("Passed", r.pass, pct(r.pass, ds_in), r.ss_pass, pct(r.ss_pass, r.ss_input));
            row2("Failed", ds_fail, pct(ds_fail, ds_in), ss_failed, pct(ss_failed, r.ss_input));
            std::fprintf(f, "\n");
            if (o.min_tandem > 0) { row2("Tandem repeats", r.tandem, pct(r.tandem, ds_in), r.ss_tandem, pct(r.ss_tandem, r.ss_input)); std::fprintf(f, "\n"); }
            std::fprintf(f, "Exclusive failed counts\n");
            for (const char *k : fail_order(o)) {
                auto a = r.fail.find(k), b = r.ss_fail.find(k);
                const int64_t ca = a == r.fail.end() ? 0 : a->second, cb = b == r.ss_fail.end() ? 0 : b->second;
                if (ca == 0 && cb == 0 && std::string(k) == "Consensus outgrew its buffer") continue;
                row2(k, ca, pct(ca, ds_fail), cb, pct(cb, ss_failed));
            }
        } else {
        std::fprintf(f, "ZMWs input                    : %" PRId64 "\n\n", r.input);
        std::fprintf(f, "ZMWs pass filters             : %" PRId64 " (%.2f%%)\n", r.pass, pct(r.pass, r.input));
        std::fprintf(f, "ZMWs fail filters             : %" PRId64 " (%.2f%%)\n", failed, pct(failed, r.input));
        std::fprintf(f, "ZMWs shortcut filters         : 0 (0.00%%)\n\n");
        if (o.min_tandem > 0) std::fprintf(f, "ZMWs with tandem repeats      : %" PRId64 " (%.2f%%)\n\n", r.tandem, pct(r.tandem, r.input));
        if (!o.barcodes.empty()) {                               // over the HiFi reads of the main output (DESIGN.md §2 "Barcode calls")
            std::fprintf(f, "Barcode calls\n");
            std::fprintf(f, "%-30s: %" PRId64 "\n", "HiFi reads tested", r.bc_tested);
            static const char *const rows[4] = {"Barcodes at both ends", "Barcode at the head only", "Barcode at the tail only", "No barcode"};
            static const int which[4] = {3, 1, 2, 0};
            for (int k = 0; k < 4; ++k) std::fprintf(f, "%-30s: %" PRId64 " (%.2f%%)\n", rows[k], r.bc_call[which[k]], pct(r.bc_call[which[k]], r.bc_tested));
            std::fprintf(f, "\n");
        }
        if (!o.segment_adapters.empty()) {                       // over the HiFi reads the run would write without the option (DESIGN.md §2 "Segment rule")
            std::fprintf(f, "Segmentation\n");
            std::fprintf(f, "%-30s: %" PRId64 "\n", "HiFi reads tested", r.sg_tested);
            std::fprintf(f, "%-30s: %" PRId64 " (%.2f%%)\n", "Complete arrays", r.sg_complete, pct(r.sg_complete, r.sg_tested));
            std::fprintf(f, "%-30s: %" PRId64 " (%.2f%%)\n", "Reads with segments", r.sg_with, pct(r.sg_with, r.sg_tested));
            std::fprintf(f, "%-30s: %" PRId64 " (%.2f%%)\n", "Reads without segments", r.sg_without, pct(r.sg_without, r.sg_tested));
            std::fprintf(f, "%-30s: %" PRId64 " (%.2f%%)\n", "Reads with adapter overflow", r.sg_overflow, pct(r.sg_overflow, r.sg_tested));
            std::fprintf(f, "%-30s: %" PRId64 "\n", "Segments written", r.sg_written);
            std::fprintf(f, "%-30s: %" PRId64 "\n\n", "Leftover bases", r.sg_leftover);
        }
        if (!o.cdna_primers.empty()) {                           // over the HiFi reads the run would write without the option (DESIGN.md §2 "cDNA rule")
            static const char *const rows[7] = {"No primer", "Primer at one end only", "Both primers of one role", "Insert too short", "Concatemers", "No poly(A) tail",
                                                "Full-length reads written"};
            std::fprintf(f, "cDNA reads\n");
            std::fprintf(f, "%-30s: %" PRId64 "\n", "HiFi reads tested", r.cd_tested);
            for (int k = 6; k >= 0; --k) std::fprintf(f, "%-30s: %" PRId64 " (%.2f%%)\n", rows[k], r.cd_cls[k], pct(r.cd_cls[k], r.cd_tested));
            std::fprintf(f, "\n");
        }
        if (o.reads_bam) {                                       // DESIGN.md §2 "Representative rule": what the records of OUT are
            std::fprintf(f, "Representative reads\n");
            std::fprintf(f, "%-30s: %" PRId64 "\n", "Polished reads", r.rep_cls[CCSX_REPRESENT_POLISHED]);
            std::fprintf(f, "%-30s: %" PRId64 "\n", "Unpolished drafts", r.rep_cls[CCSX_REPRESENT_DRAFT]);
            std::fprintf(f, "%-30s: %" PRId64 "\n\n", "Unaltered subreads", r.rep_cls[CCSX_REPRESENT_SUBREAD]);
        }
        std::fprintf(f, "Exclusive failed counts\n");
        for (const char *k : fail_order(o)) {
            auto it = r.fail.find(k);
            const int64_t c = it == r.fail.end() ? 0 : it->second;
            if (c == 0 && std::string(k) == "Consensus outgrew its buffer") continue;      // (not a row of the reference: shown only when it happened)
            std::fprintf(f, "%-30s: %" PRId64 " (%.2f%%)\n", k, c, pct(c, failed));
        }
        }
        std::fprintf(f, "\n- - - - - - - - - - - - - - - : - - - - -\n\n");
        std::fprintf(f, "HiFi Reads                    : %s\n", with_commas(hifi.reads).c_str());
        std::fprintf(f, "HiFi Yield (bp)               : %s\n", with_commas(hifi.yield).c_str());
        std::fprintf(f, "HiFi Read Length (mean, bp)   : %s\n", with_commas(hifi.len_mean).c_str());
        std::fprintf(f, "HiFi Read Length (median, bp) : %s\n", with_commas(hifi.len_median).c_str());
        std::fprintf(f, "HiFi Read Length N50 (bp)     : %s\n", with_commas(hifi.n50).c_str());
        std::fprintf(f, "HiFi Read Quality (median)    : %d\n", hifi.qual_median);
        std::fprintf(f, "HiFi Number of Passes (mean)  : %" PRId64 "\n", hifi.np_mean);
        if (lowq.reads > 0) {                                    // reads below Q20 are written only under --min-rq < 0.99
            std::fprintf(f, "\n<Q20 Reads                    : %s\n", with_commas(lowq.reads).c_str());
            std::fprintf(f, "<Q20 Yield (bp)               : %s\n", with_commas(lowq.yield).c_str());
            std::fprintf(f, "<Q20 Read Length (mean, bp)   : %s\n", with_commas(lowq.len_mean).c_str());
            std::fprintf(f, "<Q20 Read Length (median, bp) : %s\n", with_commas(lowq.len_median).c_str());
            std::fprintf(f, "<Q20 Read Quality (median)    : %d\n", lowq.qual_median);
        }
        std::fprintf(f, "\n>=Q30 Reads                   : %s\n", with_commas(q30.reads).c_str());
        std::fprintf(f, ">=Q30 Yield (bp)              : %s\n", with_commas(q30.yield).c_str());
        std::fprintf(f, ">=Q30 Read Length (mean, bp)  : %s\n", with_commas(q30.len_mean).c_str());
        std::fprintf(f, ">=Q30 Read Length (median, bp): %s\n", with_commas(q30.len_median).c_str());
        std::fprintf(f, ">=Q30 Read Quality (median)   : %d\n", q30.qual_median);
        std::fprintf(f, "\nBase quality >=Q30 (bp)       : %s (%.1f%%)\n", with_commas(r.bases_q30).c_str(), pct(r.bases_q30, hifi.yield));
        std::fclose(f);
    }
}

// --report-json (docs/changelog.md:72 "JSON output of ccs_reports"; docs/faq/sqiie.md:42): the counts of ccs_report.txt, keyed by the row labels
void write_report_json(const Options &o, const Report &r)
{
    FILE *f = std::fopen(o.report_json.c_str(), "w");
    if (!f) { std::fprintf(stderr, "ccs: cannot write %s\n", o.report_json.c_str()); return; }
    std::fprintf(f, "{\n  \"zmws_input\": %" PRId64 ",\n  \"zmws_pass_filters\": %" PRId64 ",\n  \"zmws_fail_filters\": %" PRId64 ",\n  \"zmws_shortcut_filters\": 0,\n",
                 r.input, r.pass, r.input - r.pass);
    if (o.min_tandem > 0) std::fprintf(f, "  \"zmws_with_tandem_repeats\": %" PRId64 ",\n", r.tandem);
    if (!o.barcodes.empty())
        std::fprintf(f, "  \"barcode_calls\": {\"tested\": %" PRId64 ", \"both_ends\": %" PRId64 ", \"head_only\": %" PRId64 ", \"tail_only\": %" PRId64 ", \"none\": %" PRId64 "},\n",
                     r.bc_tested, r.bc_call[3], r.bc_call[1], r.bc_call[2], r.bc_call[0]);
    if (!o.segment_adapters.empty())
        std::fprintf(f, "  \"segmentation\": {\"tested\": %" PRId64 ", \"complete_arrays\": %" PRId64 ", \"with_segments\": %" PRId64 ", \"without_segments\": %" PRId64
                        ", \"overflow\": %" PRId64 ", \"segments_written\": %" PRId64 ", \"leftover_bases\": %" PRId64 "},\n",
                     r.sg_tested, r.sg_complete, r.sg_with, r.sg_without, r.sg_overflow, r.sg_written, r.sg_leftover);
    if (!o.cdna_primers.empty())
        std::fprintf(f, "  \"cdna_reads\": {\"tested\": %" PRId64 ", \"full_length\": %" PRId64 ", \"no_tail\": %" PRId64 ", \"concatemer\": %" PRId64 ", \"short\": %" PRId64
                        ", \"same_role\": %" PRId64 ", \"one_end\": %" PRId64 ", \"no_primer\": %" PRId64 "},\n",
                     r.cd_tested, r.cd_cls[6], r.cd_cls[5], r.cd_cls[4], r.cd_cls[3], r.cd_cls[2], r.cd_cls[1], r.cd_cls[0]);
    if (o.reads_bam)
        std::fprintf(f, "  \"representative_reads\": {\"polished\": %" PRId64 ", \"draft\": %" PRId64 ", \"subread\": %" PRId64 "},\n",
                     r.rep_cls[CCSX_REPRESENT_POLISHED], r.rep_cls[CCSX_REPRESENT_DRAFT], r.rep_cls[CCSX_REPRESENT_SUBREAD]);
    if (o.heteroduplexes == HD_SPLIT) {                       // the two columns of ccs_report.txt: reads, not ZMWs (zmws_pass_filters / zmws_fail_filters count ZMWs)
        const int64_t ds_in = r.input - r.hd_zmws;
        std::fprintf(f, "  \"double_strand_reads\": {\"inputs\": %" PRId64 ", \"passed\": %" PRId64 ", \"failed\": %" PRId64 ", \"tandem_repeats\": %" PRId64 "},\n",
                     ds_in, r.pass, ds_in - r.pass, r.tandem);
        std::fprintf(f, "  \"single_strand_reads\": {\"inputs\": %" PRId64 ", \"passed\": %" PRId64 ", \"failed\": %" PRId64 ", \"tandem_repeats\": %" PRId64
                        ", \"exclusive_failed_counts\": {", r.ss_input, r.ss_pass, r.ss_input - r.ss_pass, r.ss_tandem);
        bool first_ss = true;
        for (const char *k : fail_order(o)) {
            auto it = r.ss_fail.find(k);
            std::fprintf(f, "%s\"%s\": %" PRId64, first_ss ? "" : ", ", k, it == r.ss_fail.end() ? (int64_t)0 : it->second);
            first_ss = false;
        }
        std::fprintf(f, "}},\n");
    }
    std::fprintf(f, "  \"exclusive_failed_counts\": {");
    bool first = true;
    for (const char *k : fail_order(o)) {
        auto it = r.fail.find(k);
        std::fprintf(f, "%s\n    \"%s\": %" PRId64, first ? "" : ",", k, it == r.fail.end() ? (int64_t)0 : it->second);
        first = false;
    }
    std::fprintf(f, "\n  }\n}\n");
    std::fclose(f);
}

// --barcode-counts: one line per called pair of barcodes, in increasing (head index, tail index): the two record names and the HiFi reads
void write_barcode_counts(const Options &o, const Report &r)
{
    FILE *f = std::fopen(o.barcode_counts.c_str(), "w");
    if (!f) { std::fprintf(stderr, "ccs: cannot write %s\n", o.barcode_counts.c_str()); return; }
    for (const auto &kv : r.bc_pairs)
        std::fprintf(f, "%s\t%s\t%" PRId64 "\n", o.barcode_names[kv.first.first].c_str(), o.barcode_names[kv.first.second].c_str(), kv.second);
    std::fclose(f);
}

// --segment-counts: one line per class of HiFi reads, in increasing (segments per read, orientation, complete): those three and the reads.  orientation: -1 no
// segment, 0 forward, 1 reverse, 2 mixed
void write_segment_counts(const Options &o, const Report &r)
{
    FILE *f = std::fopen(o.segment_counts.c_str(), "w");
    if (!f) { std::fprintf(stderr, "ccs: cannot write %s\n", o.segment_counts.c_str()); return; }
    for (const auto &kv : r.sg_classes) std::fprintf(f, "%d\t%d\t%d\t%" PRId64 "\n", kv.first[0], kv.first[1], kv.first[2], kv.second);
    std::fclose(f);
}

// --cdna-counts: one line per (class, strand) of HiFi reads, in increasing order: the class's number and name, the strand (-1 unknown, 0 sense, 1 antisense) and
// the reads
void write_cdna_counts(const Options &o, const Report &r)
{
    static const char *const names[7] = {"NO_PRIMER", "ONE_END", "SAME_ROLE", "SHORT", "CONCATEMER", "NO_TAIL", "FULL_LENGTH"};
    FILE *f = std::fopen(o.cdna_counts.c_str(), "w");
    if (!f) { std::fprintf(stderr, "ccs: cannot write %s\n", o.cdna_counts.c_str()); return; }
    for (const auto &kv : r.cd_classes) std::fprintf(f, "%d\t%s\t%d\t%" PRId64 "\n", kv.first[0], names[kv.first[0]], kv.first[1], kv.second);
    std::fclose(f);
}

// --hifi-summary-json (docs/faq/sqiie.md:45 "summary JSON file for hifi statistics"): the statistics block of ccs_report.txt
void write_hifi_summary(const Options &o, const Report &r)
{
    FILE *f = std::fopen(o.hifi_summary.c_str(), "w");
    if (!f) { std::fprintf(stderr, "ccs: cannot write %s\n", o.hifi_summary.c_str()); return; }
    int64_t all_bases = 0;
    for (int32_t l : r.lens) all_bases += l;
    auto cls = [&](const char *name, const ReadClass &c, bool last) {
        std::fprintf(f, "  \"%s\": {\"reads\": %" PRId64 ", \"yield_bp\": %" PRId64 ", \"read_length_mean\": %" PRId64 ", \"read_length_median\": %" PRId64
                        ", \"read_length_n50\": %" PRId64 ", \"read_quality_median\": %d, \"number_of_passes_mean\": %" PRId64 "}%s\n",
                     name, c.reads, c.yield, c.len_mean, c.len_median, c.n50, c.qual_median, c.np_mean, last ? "" : ",");
    };
    std::fprintf(f, "{\n");
    cls("hifi", classify(r, 0.99f, 2.0f), false);
    cls("below_q20", classify(r, -1.0f, 0.99f), false);
    cls("q30_and_above", classify(r, 0.999f, 2.0f), false);
    std::fprintf(f, "  \"bases\": %" PRId64 ",\n  \"bases_q30_and_above\": %" PRId64 "\n}\n", all_bases, r.bases_q30);
    std::fclose(f);
}

// --gpu-inflate: the inflaters the reader's slab jobs share.  A job takes one (waits when all are busy: that pool thread then serves neither the record decode nor
// the output's deflate, which share the pool), inflates its slab with one synchronous call and hands it back.  COUNT = 4: a slab is one short kernel between two
// copies of a few MB, so four in flight keep the copy engines and the kernel overlapped.  The reader's look-ahead is what it is without the flag (2 * threads + 4
// slabs); it was not tuned for it.  A slab is ~1 MB of blocks and inflates to ~2.6 MB on subread BAMs (ratio 2 - 4 for BAM in general): MAX_OUT = 6 MB covers a
// ratio of 5.7; a slab beyond an inflater's capacities is declined and inflated on the host.  Page-locked memory: 4 inflaters x 2 call slots x 7 MB = 57 MB.
struct GpuInflaters {
    static constexpr int COUNT = 4;
    static constexpr int64_t MAX_IN = (1 << 20) + (1 << 16) + 64, MAX_OUT = 6 << 20;
    static constexpr int32_t MAX_BLOCKS = 4096;
    static_assert(sizeof(BgzfReader::Span) == sizeof(ccsx_deflate_block) && offsetof(BgzfReader::Span, out_off) == offsetof(ccsx_deflate_block, out_off) &&
                  offsetof(BgzfReader::Span, in_len) == offsetof(ccsx_deflate_block, in_len) && offsetof(BgzfReader::Span, out_len) == offsetof(ccsx_deflate_block, out_len),
                  "BgzfReader::Span is ccsx_deflate_block");
    std::vector<ccsx_inflater> all, free_;
    std::mutex m;
    std::condition_variable cv;
    ~GpuInflaters() { for (ccsx_inflater f : all) ccsx_inflater_destroy(f); }
    bool create(int device)
    {
        for (int i = 0; i < COUNT; ++i) {
            ccsx_inflater f = nullptr;
            if (ccsx_inflater_create(device, MAX_IN, MAX_OUT, MAX_BLOCKS, &f)) return false;
            all.push_back(f); free_.push_back(f);
        }
        return true;
    }
    bool inflate(const uint8_t *src, size_t src_len, const std::vector<BgzfReader::Span> &spans, uint8_t *dst, size_t dst_len, std::vector<int32_t> &status)
    {
        if ((int64_t)src_len > MAX_IN || (int64_t)dst_len > MAX_OUT || spans.size() > (size_t)MAX_BLOCKS) return false;
        ccsx_inflater f;
        { std::unique_lock<std::mutex> l(m); cv.wait(l, [this] { return !free_.empty(); }); f = free_.back(); free_.pop_back(); }
        const int rc = ccsx_inflate_blocks(f, src, (int64_t)src_len, reinterpret_cast<const ccsx_deflate_block *>(spans.data()), (int32_t)spans.size(), dst, (int64_t)dst_len, status.data());
        const std::string err = rc ? ccsx_last_error() : "";
        { std::lock_guard<std::mutex> l(m); free_.push_back(f); }
        cv.notify_one();
        if (rc) throw std::runtime_error("--gpu-inflate: " + err);
        return true;
    }
};

// --gpu-deflate: the one deflater the run's BGZF writers share (the HiFi BAM and the --fail-reads BAM; both are written by the writer thread, the only thread
// that calls this).  A ticket is as many raw 0xff00-byte blocks as fill the device: ccsx_deflate_fill_spans (CUs x resident workgroups of k_deflate), at least
// 256.  submit() copies the blocks into one source buffer, enqueues and returns; two tickets are in flight at most, so a third submit first waits for the oldest
// (its writer finds it done when it asks).  Every out_cap is ccsx_deflate_bound: no span can be OUTPUT_FULL.  After an error nothing more is sent to the device.
// Page-locked memory: 2 call slots x (16.7 + 16.7) MB = 67 MB at 256 blocks.
struct GpuDeflater : BgzfDeflateBackend {
    struct Call : BgzfDeflateCall {
        ccsx_ticket ticket = 0;
        bool waited = false, bad = false;                // bad: waited for, and the ticket failed (its owner must not write it)
        std::vector<uint8_t> src;
        std::vector<ccsx_deflate_span> spans;
        std::vector<int32_t> status;
    };
    ccsx_deflater f = nullptr;
    size_t blocks = 256;
    bool broken = false;
    long long n_tickets = 0, n_blocks = 0, n_in = 0, n_out = 0, us_submit = 0, us_wait = 0;
    std::deque<std::shared_ptr<Call>> inflight;      // oldest first
    static long long us_since(std::chrono::steady_clock::time_point t) { return (long long)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t).count(); }
    ~GpuDeflater() { if (f) ccsx_deflater_destroy(f); }
    bool create(int device)
    {
        const int32_t fill = ccsx_deflate_fill_spans(device);
        if (fill < 0) return false;
        blocks = (size_t)std::max<int32_t>(256, fill);
        return ccsx_deflater_create(device, (int64_t)blocks * 0xff00, (int64_t)blocks * ccsx_deflate_bound(0xff00), (int32_t)blocks, &f) == 0;
    }
    size_t ticket_blocks() const override { return blocks; }
    void wait_oldest()
    {
        std::shared_ptr<Call> c = inflight.front(); inflight.pop_front();
        const auto t0 = std::chrono::steady_clock::now();
        const int rc = ccsx_deflate_wait(f, c->ticket);
        us_wait += us_since(t0);
        c->waited = true;
        c->bad = rc != 0 || std::any_of(c->status.begin(), c->status.end(), [](int32_t st) { return st != CCSX_DEFLATE_OK; });
        if (rc) { broken = true; throw std::runtime_error(std::string("--gpu-deflate: ") + ccsx_last_error()); }
        for (size_t i = 0; i < c->status.size(); ++i) {
            if (c->status[i] != CCSX_DEFLATE_OK) { broken = true; throw std::runtime_error("--gpu-deflate: block " + std::to_string(i) + " of a ticket came back with status " + std::to_string(c->status[i])); }
            n_out += c->len[i];
        }
    }
    std::shared_ptr<BgzfDeflateCall> submit(const std::vector<std::shared_ptr<std::vector<uint8_t>>> &raw) override
    {
        if (broken) throw std::runtime_error("--gpu-deflate: the deflater failed earlier in this run");
        if (raw.size() > blocks) throw std::runtime_error("--gpu-deflate: a ticket of more blocks than the deflater holds");
        while (inflight.size() >= 2) wait_oldest();
        const auto t0 = std::chrono::steady_clock::now();
        auto c = std::make_shared<Call>();
        const size_t n = raw.size();
        size_t in = 0, out = 0;
        c->spans.resize(n); c->off.resize(n); c->len.assign(n, 0); c->crc.assign(n, 0); c->status.assign(n, -1);
        for (size_t i = 0; i < n; ++i) {
            const int32_t len = (int32_t)raw[i]->size(), cap = ccsx_deflate_bound(len);
            c->spans[i] = ccsx_deflate_span{(int64_t)in, len, cap, (int64_t)out};
            c->off[i] = (int64_t)out;
            in += (size_t)len; out += (size_t)cap;
        }
        c->src.resize(in); c->dst.resize(out);
        for (size_t i = 0; i < n; ++i) std::memcpy(c->src.data() + c->spans[i].in_off, raw[i]->data(), raw[i]->size());
        if (ccsx_deflate_submit(f, c->src.data(), (int64_t)in, c->spans.data(), (int32_t)n, c->dst.data(), (int64_t)out, c->len.data(), c->crc.data(), c->status.data(), &c->ticket)) {
            broken = true;
            throw std::runtime_error(std::string("--gpu-deflate: ") + ccsx_last_error());
        }
        inflight.push_back(c);
        ++n_tickets; n_blocks += (long long)n; n_in += (long long)in;
        us_submit += us_since(t0);
        return c;
    }
    void wait(BgzfDeflateCall &call) override
    {
        Call &c = static_cast<Call &>(call);
        while (!c.waited) {
            if (inflight.empty()) throw std::runtime_error("--gpu-deflate: a ticket that is not in flight");
            wait_oldest();
        }
        if (c.bad) throw std::runtime_error("--gpu-deflate: the deflater failed earlier in this run");
    }
};

}  // namespace

// ---- ccs --fit-model: EM over the packed batches of the file, serial, on one GPU (DESIGN.md §2 "Model training").  Per iteration a handle with the current
// model; per batch the draft seam, the polish seam, drafts made of the polished reads that are good enough to be a truth, the training counts on them, the
// fitter.  h0: the handle main() made with the start model (iteration 1 uses it; it is destroyed here, `h0` is cleared).  0, or 1 after an engine failure (no json).
static int fit_model(const Options &opt, ccsx_handle &h0, const ccsx_model &start, const std::vector<std::shared_ptr<Batch>> &batches, const std::string &bk,
              const std::string &sk, const std::string &bc)
{
    auto engine_failed = [&](const char *what) { std::fprintf(stderr, "ccs: --fit-model: %s: %s\n", what, ccsx_last_error()); return 1; };
    if (batches.empty()) { std::fprintf(stderr, "ccs: --fit-model: no ZMW of %s passes the filters\n", opt.in.c_str()); return 1; }
    const int dev = opt.gpus.empty() ? 0 : opt.gpus[0];
    ccsx_fit_opts fo; ccsx_fit_opts_default(&fo);
    if (opt.fit_degree >= 0) fo.degree = opt.fit_degree;
    ccsx_model cur = start;
    for (int it = 1; it <= opt.fit_iterations; ++it) {
        ccsx_handle h = h0; h0 = nullptr;
        if (!h && ccsx_create(dev, &cur, &opt.o, &h)) return engine_failed("ccsx_create");
        ccsx_fitter fit = nullptr;
        if (ccsx_fitter_create(&cur, &fo, &fit)) { ccsx_destroy(h); return engine_failed("ccsx_fitter_create"); }
        long long used = 0;
        int rc = 0;
        for (const auto &b : batches) {
            const int n = b->n;
            std::vector<int64_t> seq_off(n + 1), win_off(n + 1);
            int64_t scap = 0, wcap = 0;
            ccsx_draft_layout(&b->cb, seq_off.data(), win_off.data(), &scap, &wcap);
            std::vector<int32_t> i32((size_t)n * 16);
            std::vector<uint8_t> dseq((size_t)scap), rseq((size_t)scap), rqual((size_t)scap), tseq((size_t)scap);
            std::vector<float> f32((size_t)n * 2);
            int32_t *I = i32.data();
            ccsx_drafts dr{n, scap, 0, seq_off.data(), nullptr, I, I + n, dseq.data(), I + 2 * n, nullptr, nullptr};
            ccsx_results res{n, scap, seq_off.data(), I + 3 * n, I + 4 * n, rseq.data(), rqual.data(), nullptr, f32.data(), I + 5 * n, f32.data() + n, I + 6 * n, I + 7 * n};
            res.fn = I + 8 * n; res.rn = I + 9 * n;
            if (ccsx_draft_batch(h, &b->cb, &dr)) { rc = engine_failed("ccsx_draft_batch"); break; }
            if (ccsx_polish_batch(h, &b->cb, &dr, &res, 0)) { rc = engine_failed("ccsx_polish_batch"); break; }
            // the truths: the polished reads of the ZMWs that succeeded with rq >= --fit-min-rq, in the draft call's orientation; none for the rest
            ccsx_drafts tr{n, scap, 0, seq_off.data(), nullptr, nullptr, I + 10 * n, tseq.data(), I + 2 * n, nullptr, nullptr};
            for (int z = 0; z < n; ++z) {
                const bool ok = res.status[z] == CCSX_SUCCESS && (double)res.rq[z] >= opt.fit_min_rq && res.seq_len[z] > 0;
                tr.len[z] = ok ? res.seq_len[z] : 0;
                if (ok) { std::memcpy(tseq.data() + seq_off[z], rseq.data() + seq_off[z], (size_t)res.seq_len[z]); ++used; }
            }
            std::vector<int64_t> tab((size_t)n * 401);
            ccsx_train_counts tc{n, 0, tab.data(), tab.data() + (size_t)n * 192, tab.data() + (size_t)n * 384, tab.data() + (size_t)n * 400, I + 11 * n, I + 12 * n,
                                 I + 13 * n, I + 14 * n};
            if (ccsx_train_batch(h, &b->cb, &tr, &tc)) { rc = engine_failed("ccsx_train_batch"); break; }
            if (ccsx_fitter_add(fit, &tc, b->snr.data())) { rc = engine_failed("ccsx_fitter_add"); break; }
        }
        ccsx_model next;
        ccsx_fit_report rep{};
        if (!rc && ccsx_fitter_finish(fit, &next, &rep)) rc = engine_failed("ccsx_fitter_finish");
        ccsx_fitter_destroy(fit);
        ccsx_destroy(h);
        if (rc) return rc;
        if (opt.log_level >= 2)
            std::fprintf(stderr, "ccs: --fit-model iteration %d: %lld ZMWs used, %lld pairs, %lld gated, log2-likelihood per base %.5f, largest parameter change %.3g\n", it, used,
                         (long long)rep.pairs, (long long)rep.gated, rep.loglik_per_base, rep.max_change);
        if (rep.pairs == 0) { std::fprintf(stderr, "ccs: --fit-model: no pair was counted (no polished read reaches --fit-min-rq %.4f?)\n", opt.fit_min_rq); return 1; }
        cur = next;
    }
    const std::string name = ("fit-" + std::string(start.name, strnlen(start.name, sizeof(start.name)))).substr(0, sizeof(cur.name) - 1);   // (cut to 31 characters)
    std::memset(cur.name, 0, sizeof(cur.name));
    std::memcpy(cur.name, name.data(), name.size());
    const int64_t need = ccsx_model_to_json(&cur, bk.empty() ? nullptr : bk.c_str(), sk.empty() ? nullptr : sk.c_str(), bc.empty() ? nullptr : bc.c_str(), nullptr, 0);
    if (need <= 0) return engine_failed("ccsx_model_to_json");
    std::string text((size_t)need + 1, '\0');
    ccsx_model_to_json(&cur, bk.empty() ? nullptr : bk.c_str(), sk.empty() ? nullptr : sk.c_str(), bc.empty() ? nullptr : bc.c_str(), &text[0], need + 1);
    FILE *f = std::fopen(opt.fit_model.c_str(), "w");
    if (!f || std::fwrite(text.c_str(), 1, std::strlen(text.c_str()), f) != std::strlen(text.c_str()) || std::fclose(f)) {
        std::fprintf(stderr, "ccs: cannot write %s\n", opt.fit_model.c_str()); return 1;
    }
    return 0;
}

// ---- ccs --mark-duplicates IN.bam OUT.bam (DESIGN.md §2 "Duplicate rule", §7): the reads of an unaligned BAM in, the same records out, the duplicate sets
// marked.  Pass 1 streams the records and signs them on the device in bounded batches; per read it keeps the signature, a score (floor(rq * 10^6), 0 without
// the tag), a group (0, or the bc pair under --dup-within-barcodes) and the name, of which only the representatives' outlive the clustering.  One
// ccsx_dup_cluster call makes the sets.  Pass 2 reads IN again and writes every record through byte for byte; a member of a set of two or more gains ds:i (the
// set's size), a duplicate also FLAG 0x400 and du:Z (the representative's name) — or is left out under --dup-remove.  No .pbi is written for OUT.
struct DupTags { bool has_rq = false, has_bc = false, marked = false, has_cb = false, has_xm = false; float rq = 0.0f; uint32_t bc[2] = {0, 0}; std::string cb, xm; };
// the rq, bc, ds and du tags of a record body that parse_subread has accepted (every length in it has been checked there)
static DupTags dup_scan_tags(const uint8_t *p, uint32_t bs)
{
    DupTags g;
    const uint32_t l_name = p[8], n_cig = p[12] | (p[13] << 8), l_seq = rd32(p + 16);
    const uint8_t *t = p + 32 + l_name + 4 * n_cig + (l_seq + 1) / 2 + l_seq, *end = p + bs;
    while (t + 3 <= end) {
        const char t0 = (char)t[0], t1 = (char)t[1], ty = (char)t[2];
        t += 3;
        if ((t0 == 'd' && t1 == 's') || (t0 == 'd' && t1 == 'u')) g.marked = true;
        if (ty == 'Z' || ty == 'H') {
            const uint8_t *v = t;
            while (t < end && *t) ++t;
            if (ty == 'Z' && t0 == 'C' && t1 == 'B') { g.has_cb = true; g.cb.assign((const char *)v, (size_t)(t - v)); }
            if (ty == 'Z' && t0 == 'X' && t1 == 'M') { g.has_xm = true; g.xm.assign((const char *)v, (size_t)(t - v)); }
            ++t; continue;
        }
        if (ty == 'B') {
            const char st = (char)t[0];
            const uint32_t n = rd32(t + 1);
            const uint8_t *q = t + 5;
            if (t0 == 'b' && t1 == 'c' && (st == 'S' || st == 's') && n == 2) { g.has_bc = true; g.bc[0] = q[0] | (q[1] << 8); g.bc[1] = q[2] | (q[3] << 8); }
            t = q + (size_t)n * tag_value_size(st);
            continue;
        }
        if (t0 == 'r' && t1 == 'q' && ty == 'f') { std::memcpy(&g.rq, t, 4); g.has_rq = true; }
        t += tag_value_size(ty);
    }
    return g;
}

static int mark_duplicates(const Options &opt, ThreadPool &pool)
{
    auto failed = [](const std::string &what) { std::fprintf(stderr, "ccs: --mark-duplicates: %s\n", what.c_str()); return 1; };
    if (ccsx_device_count() <= 0) { std::fprintf(stderr, "ccs: no gfx950 GPU available (this build has no CPU path for the duplicate rule)\n"); return 1; }
    ccsx_model model; ccsx_model_default(&model);
    ccsx_opts eo; ccsx_opts_default(&eo);
    ccsx_handle h = nullptr;
    if (ccsx_create(opt.gpus.empty() ? 0 : opt.gpus[0], &model, &eo, &h)) { std::fprintf(stderr, "ccs: %s\n", ccsx_last_error()); return 1; }
    struct Closer { ccsx_handle h; ~Closer() { ccsx_destroy(h); } } closer{h};
    const ccsx_dup_opts &D = opt.dup_opts;
    typedef std::chrono::steady_clock Clock;                         // (the phases' wall clock, one line at --log-level INFO: tools/dup_bench.py reads it)
    auto seconds = [](Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double>(b - a).count(); };
    const Clock::time_point t_start = Clock::now();
    double sign_s = 0.0;

    // ---- pass 1: signatures in batches of at most kBatchReads reads or kBatchBases bases
    constexpr size_t kBatchReads = 16384, kBatchBases = (size_t)64 << 20;
    std::vector<ccsx_dup_sig> sig;
    std::vector<int32_t> score, group;
    std::vector<std::string> names;
    std::map<std::pair<std::string, std::string>, int32_t> cells;   // --dup-within-cells: the dense id, from 1, of every (CB, XM) pair seen
    std::string header_text;
    {
        BgzfReader in(opt.in, pool);
        BamHeader hdr; read_header(in, hdr);
        if (!hdr.refs.empty()) return failed("IN has reference sequences: aligned input is not supported");
        header_text = hdr.text;
        std::vector<uint8_t> seq;
        std::vector<int64_t> off;
        std::vector<int32_t> len;
        auto flush = [&]() -> bool {
            if (len.empty()) return true;
            const size_t at = sig.size();
            sig.resize(at + len.size());
            seq.push_back(0);                                        // (never empty: the call wants a pointer)
            const Clock::time_point t0 = Clock::now();
            const int rc = ccsx_dup_sign_reads(h, &D, seq.data(), off.data(), len.data(), (int32_t)len.size(), sig.data() + at);
            sign_s += seconds(t0, Clock::now());
            seq.clear(); off.clear(); len.clear();
            return rc == 0;
        };
        auto chunk = std::make_shared<RawChunk>();
        Subread r;
        while (read_raw_chunk(in, *chunk)) {
            for (const auto &rec : chunk->recs) {
                parse_subread(rec.first, rec.second, r);
                const DupTags g = dup_scan_tags(rec.first, rec.second);
                if (g.marked) return failed("read " + r.name + " already carries a ds or du tag: IN has been marked before");
                if (sig.size() + len.size() >= (size_t)CCSX_DUP_MAX_READS) return failed("more than " + std::to_string(CCSX_DUP_MAX_READS) + " reads");
                if (g.has_bc && g.bc[0] >= 32767u && opt.dup_within_barcodes) return failed("read " + r.name + ": a bc index above 32766");
                const double sc = g.has_rq && g.rq == g.rq ? std::floor((double)g.rq * 1e6) : 0.0;
                score.push_back((int32_t)std::min(2147483647.0, std::max(-2147483648.0, sc)));
                int32_t grp = opt.dup_within_barcodes && g.has_bc ? (int32_t)(1 + g.bc[0] * 65536u + g.bc[1]) : 0;
                if (opt.dup_within_cells && g.has_cb && g.has_xm) grp = cells.emplace(std::make_pair(g.cb, g.xm), (int32_t)cells.size() + 1).first->second;
                group.push_back(grp);
                names.push_back(r.name);
                off.push_back((int64_t)seq.size()); len.push_back((int32_t)r.len);
                seq.resize(seq.size() + r.len);
                if (r.len) r.decode_bases(seq.data() + seq.size() - r.len);
                if (len.size() >= kBatchReads || seq.size() >= kBatchBases) { if (!flush()) return failed(ccsx_last_error()); }
            }
            chunk = std::make_shared<RawChunk>();
        }
        if (!flush()) return failed(ccsx_last_error());
    }

    // ---- the sets: one call over everything kept
    const Clock::time_point t_pass1 = Clock::now();
    const int32_t n = (int32_t)sig.size();
    std::vector<int32_t> planes((size_t)n * 4 + 1);
    ccsx_dup_report rep{n, planes.data(), planes.data() + n, planes.data() + 2 * (size_t)n, planes.data() + 3 * (size_t)n};
    if (ccsx_dup_cluster(h, &D, sig.data(), group.data(), score.data(), n, &rep)) return failed(ccsx_last_error());
    const Clock::time_point t_cluster = Clock::now();
    int64_t tested = 0, untested = 0, overflowed = 0, sets = 0, dups = 0, largest = 0;
    std::map<int32_t, int64_t> by_size;
    for (int32_t z = 0; z < n; ++z) {
        if (rep.status[z] == CCSX_DUP_UNTESTED) { ++untested; continue; }
        if (rep.status[z] == CCSX_DUP_OVERFLOW) { ++overflowed; continue; }
        ++tested; dups += rep.dup[z];
        if (rep.rep[z] == z) { ++by_size[rep.set_size[z]]; sets += rep.set_size[z] >= 2; largest = std::max<int64_t>(largest, rep.set_size[z]); }
    }
    { std::vector<char> is_rep((size_t)n, 0);                         // only the names pass 2 writes stay
      for (int32_t z = 0; z < n; ++z) if (rep.dup[z]) is_rep[rep.rep[z]] = 1;
      for (int32_t z = 0; z < n; ++z) if (!is_rep[z]) std::string().swap(names[z]); }
    std::vector<ccsx_dup_sig>().swap(sig);

    // ---- pass 2: every record through, the members of a set marked
    int64_t written = 0;
    {
        BgzfReader in(opt.in, pool);
        BamHeader hdr; read_header(in, hdr);
        BgzfWriter out(opt.out, pool);
        write_header(out, header_text);
        auto chunk = std::make_shared<RawChunk>();
        std::vector<uint8_t> b;
        int32_t z = 0;
        while (read_raw_chunk(in, *chunk)) {
            for (const auto &rec : chunk->recs) {
                if (z >= n) return failed("IN changed between the two passes");
                const int32_t k = z++;
                if (rep.dup[k] && opt.dup_remove) continue;
                ++written;
                uint8_t b4[4];
                auto put32 = [&](uint32_t v) { for (int i = 0; i < 4; ++i) b4[i] = (uint8_t)(v >> (8 * i)); };
                if (rep.set_size[k] < 2) { put32(rec.second); out.write(b4, 4); out.write(rec.first, rec.second); continue; }
                b.assign(rec.first, rec.first + rec.second);
                if (rep.dup[k]) { const unsigned flag = (b[14] | (b[15] << 8)) | 0x400u; b[14] = (uint8_t)(flag & 0xff); b[15] = (uint8_t)(flag >> 8); }
                b.push_back('d'); b.push_back('s'); b.push_back('i');
                put32((uint32_t)rep.set_size[k]); b.insert(b.end(), b4, b4 + 4);
                if (rep.dup[k]) {
                    const std::string &nm = names[rep.rep[k]];
                    b.push_back('d'); b.push_back('u'); b.push_back('Z'); b.insert(b.end(), nm.begin(), nm.end()); b.push_back(0);
                }
                put32((uint32_t)b.size()); out.write(b4, 4); out.write(b.data(), b.size());
            }
            chunk = std::make_shared<RawChunk>();
        }
        if (z != n) return failed("IN changed between the two passes");
        out.close();
    }
    const Clock::time_point t_pass2 = Clock::now();

    // ---- the report block and the counts
    if (!opt.report.empty()) {
        FILE *f = std::fopen(opt.report.c_str(), "w");
        if (!f) { std::fprintf(stderr, "ccs: cannot write %s\n", opt.report.c_str()); return 1; }
        std::fprintf(f, "Duplicate marking (rule %d: window %d, kmer %d, max_dist_pct %d, max_len_diff_pct %d%s)\n", ccsx_dup_rule_version(), D.window, D.kmer,
                     D.max_dist_pct, D.max_len_diff_pct, opt.dup_within_barcodes ? ", within barcodes" : opt.dup_within_cells ? ", within cells" : "");
        std::fprintf(f, "Reads input                 : %lld\n", (long long)n);
        std::fprintf(f, "Reads tested                : %lld\n", (long long)tested);
        std::fprintf(f, "Reads untested              : %lld\n", (long long)untested);
        std::fprintf(f, "Reads in overflowed buckets : %lld\n", (long long)overflowed);
        std::fprintf(f, "Duplicate sets              : %lld\n", (long long)sets);
        std::fprintf(f, "Duplicates                  : %lld\n", (long long)dups);
        std::fprintf(f, "Largest set                 : %lld\n", (long long)largest);
        std::fprintf(f, "Reads written               : %lld\n", (long long)written);
        std::fclose(f);
    }
    if (!opt.dup_counts.empty()) {
        FILE *f = std::fopen(opt.dup_counts.c_str(), "w");
        if (!f) { std::fprintf(stderr, "ccs: cannot write %s\n", opt.dup_counts.c_str()); return 1; }
        std::fprintf(f, "set_size\tsets\n");
        for (const auto &kv : by_size) std::fprintf(f, "%d\t%lld\n", kv.first, (long long)kv.second);
        std::fclose(f);
    }
    if (opt.log_level >= 2)
        std::fprintf(stderr, "ccs: --mark-duplicates: %lld reads, %lld sets, %lld duplicates %s; pass 1 %.3f s (of which ccsx_dup_sign_reads %.3f s, the rest inflate, "
                             "parsing and base decoding), ccsx_dup_cluster %.3f s, pass 2 %.3f s (inflate, copy, deflate)\n", (long long)n, (long long)sets, (long long)dups,
                     opt.dup_remove ? "removed" : "marked", seconds(t_start, t_pass1), sign_s, seconds(t_pass1, t_cluster), seconds(t_cluster, t_pass2));
    return 0;
}

// ---- ccs --cell-reads IN.bam OUT.bam (DESIGN.md §2 "Cell-tag rule", §7): the reads of an unaligned BAM in, the full-length cDNA reads out.  One pass: the
// records are streamed in batches of at most kBatchReads reads or kBatchBases bases (the chunks that hold a batch's records stay until it is written), every batch
// is one ccsx_cell_reads call, and a FULL_LENGTH read is written as its input record cut to the slice, with the tags the rule gives.  No .pbi is written for OUT.
static std::string cell_field_text(uint32_t x, int n)
{
    std::string s((size_t)n, 'A');
    for (int j = 0; j < n; ++j) s[(size_t)j] = "ACGT"[(x >> (2 * (n - 1 - j))) & 3u];
    return s;
}

// a record body that parse_subread has accepted carries an XM, XC or CB tag
static bool cell_is_tagged(const uint8_t *p, uint32_t bs)
{
    const uint32_t l_name = p[8], n_cig = p[12] | (p[13] << 8), l_seq = rd32(p + 16);
    const uint8_t *t = p + 32 + l_name + 4 * n_cig + (l_seq + 1) / 2 + l_seq, *end = p + bs;
    while (t + 3 <= end) {
        const char t0 = (char)t[0], t1 = (char)t[1], ty = (char)t[2];
        if ((t0 == 'X' && (t1 == 'M' || t1 == 'C')) || (t0 == 'C' && t1 == 'B')) return true;
        t += 3;
        if (ty == 'Z' || ty == 'H') { while (t < end && *t) ++t; ++t; continue; }
        if (ty == 'B') { t += 5 + (size_t)rd32(t + 1) * tag_value_size((char)t[0]); continue; }
        t += tag_value_size(ty);
    }
    return false;
}

// the body of such a record with SEQ and QUAL cut to [from, to), every B tag of l_seq elements cut the same way (ri and rp, which run from the read's other end,
// to [l_seq - to, l_seq - from)) and every other tag byte for byte; the caller appends its tags
static void cell_cut_record(std::vector<uint8_t> &b, const uint8_t *p, uint32_t bs, uint32_t from, uint32_t to)
{
    const uint32_t l_name = p[8], n_cig = p[12] | (p[13] << 8), L = rd32(p + 16), n = to - from;
    const uint8_t *seq = p + 32 + l_name + 4 * n_cig, *qual = seq + (L + 1) / 2, *t = qual + L, *end = p + bs;
    auto put32 = [&](uint32_t v) { for (int i = 0; i < 4; ++i) b.push_back((uint8_t)(v >> (8 * i))); };
    auto nib = [&](uint32_t i) { return (uint8_t)((seq[i >> 1] >> ((i & 1) ? 0 : 4)) & 15); };
    b.assign(p, seq);
    for (int i = 0; i < 4; ++i) b[16 + (size_t)i] = (uint8_t)(n >> (8 * i));
    for (uint32_t i = 0; i < n; i += 2) b.push_back((uint8_t)((nib(from + i) << 4) | (i + 1 < n ? nib(from + i + 1) : 0)));
    b.insert(b.end(), qual + from, qual + to);
    while (t + 3 <= end) {
        const uint8_t *tag = t;
        const char t0 = (char)t[0], t1 = (char)t[1], ty = (char)t[2];
        t += 3;
        if (ty == 'Z' || ty == 'H') { while (t < end && *t) ++t; ++t; b.insert(b.end(), tag, t); continue; }
        if (ty == 'B') {
            const char st = (char)t[0];
            const uint32_t cnt = rd32(t + 1);
            const size_t es = tag_value_size(st);
            const uint8_t *q = t + 5;
            t = q + (size_t)cnt * es;
            if (cnt != L) { b.insert(b.end(), tag, t); continue; }
            const bool rev = t0 == 'r' && (t1 == 'i' || t1 == 'p');
            const uint32_t lo = rev ? L - to : from;
            b.insert(b.end(), tag, tag + 4);
            put32(n);
            b.insert(b.end(), q + (size_t)lo * es, q + (size_t)(lo + n) * es);
            continue;
        }
        t += tag_value_size(ty);
        b.insert(b.end(), tag, t);
    }
}

static int cell_reads(const Options &opt, ThreadPool &pool)
{
    auto failed = [](const std::string &what) { std::fprintf(stderr, "ccs: --cell-reads: %s\n", what.c_str()); return 1; };
    if (ccsx_device_count() <= 0) { std::fprintf(stderr, "ccs: no gfx950 GPU available (this build has no CPU path for the cell-tag rule)\n"); return 1; }
    ccsx_model model; ccsx_model_default(&model);
    ccsx_opts eo; ccsx_opts_default(&eo);
    ccsx_handle h = nullptr;
    if (ccsx_create(opt.gpus.empty() ? 0 : opt.gpus[0], &model, &eo, &h)) { std::fprintf(stderr, "ccs: %s\n", ccsx_last_error()); return 1; }
    struct Closer { ccsx_handle h; ~Closer() { ccsx_destroy(h); } } closer{h};
    const ccsx_cell_design &D = opt.cell_design;
    const ccsx_cdna_set &P = *opt.cdna_set;
    typedef std::chrono::steady_clock Clock;                         // (the phases' wall clock, one line at --log-level INFO: tools/cell_bench.py reads it)
    auto seconds = [](Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double>(b - a).count(); };
    const Clock::time_point t_start = Clock::now();
    double call_s = 0.0, write_s = 0.0;
    static const char *const cls_names[7] = {"NO_PRIMER", "ONE_END", "SAME_ROLE", "SHORT", "CONCATEMER", "NO_TAIL", "FULL_LENGTH"};
    static const char *const tag_names[6] = {"NONE", "RAW", "EXACT", "CORRECTED", "AMBIGUOUS", "ABSENT"};
    int64_t n_in = 0, written = 0, unlisted = 0, cls_n[7] = {0, 0, 0, 0, 0, 0, 0}, tag_n[6] = {0, 0, 0, 0, 0, 0};
    std::map<int32_t, int64_t> per_bc;

    constexpr size_t kBatchReads = 16384, kBatchBases = (size_t)64 << 20;
    BgzfReader in(opt.in, pool);
    BamHeader hdr; read_header(in, hdr);
    if (!hdr.refs.empty()) return failed("IN has reference sequences: aligned input is not supported");
    BgzfWriter out(opt.out, pool);
    write_header(out, hdr.text);
    std::vector<std::shared_ptr<RawChunk>> held;
    std::vector<std::pair<const uint8_t *, uint32_t>> recs;
    std::vector<uint8_t> seq, b;
    std::vector<int64_t> off;
    std::vector<int32_t> len, planes;
    auto flush = [&]() -> bool {
        const size_t n = len.size();
        if (n) {
            planes.assign(n * 24, 0);
            int32_t *q = planes.data();
            ccsx_cell_report rep{};
            rep.cdna = ccsx_cdna_report{(int32_t)n, q, q + n, q + 2 * n, q + 3 * n, q + 4 * n, q + 5 * n, q + 6 * n, q + 7 * n, q + 8 * n, q + 10 * n, q + 12 * n, q + 14 * n};
            q += 16 * n;
            rep.tag = q; rep.bc_raw = (uint32_t *)(q + n); rep.bc = q + 2 * n; rep.bc_hi = q + 3 * n; rep.kind = q + 4 * n; rep.shift = q + 5 * n;
            rep.umi = (uint32_t *)(q + 6 * n); rep.tag_clip = q + 7 * n;
            seq.push_back(0);                                        // (never empty: the call wants a pointer)
            const Clock::time_point t0 = Clock::now();
            const int rc = ccsx_cell_reads(h, &P, &opt.cdna_opts, &D, opt.cell_wl.get(), seq.data(), off.data(), len.data(), (int32_t)n, &rep);
            const Clock::time_point t1 = Clock::now();
            call_s += seconds(t0, t1);
            if (rc) return false;
            const ccsx_cdna_report &d = rep.cdna;
            for (size_t z = 0; z < n; ++z) {
                ++cls_n[d.cls[z]]; ++tag_n[rep.tag[z]];
                if (d.cls[z] != CCSX_CDNA_FULL_LENGTH) continue;
                const bool listed = rep.tag[z] == CCSX_CELL_EXACT || rep.tag[z] == CCSX_CELL_CORRECTED;
                if (opt.cell_require_barcode && !listed) { ++unlisted; continue; }
                cell_cut_record(b, recs[z].first, recs[z].second, (uint32_t)d.start[z], (uint32_t)d.end[z]);
                RecordBuilder rb;                                    // (the tags alone: ts, pa, pr and pq as --cdna-primers writes them)
                const int st = d.strand[z];
                const uint8_t pr[2] = {(uint8_t)d.idx[2 * z + st], (uint8_t)d.idx[2 * z + 1 - st]};
                int pq = 100;
                for (int e = 0; e < 2; ++e) { const int m = P.len[d.idx[2 * z + e]]; pq = std::min(pq, 100 * (m - d.dist[2 * z + e]) / m); }
                rb.tagA("ts", st ? '-' : '+'); rb.tagi("pa", d.polya_len[z]); rb.tagBC("pr", pr, 2); rb.tagi("pq", pq);
                if (D.umi_len > 0) rb.tagZ("XM", cell_field_text(rep.umi[z], D.umi_len));
                if (D.bc_len > 0) rb.tagZ("XC", cell_field_text(rep.bc_raw[z], D.bc_len));
                if (listed) {
                    const uint8_t *w = opt.cell_codes.data() + (size_t)rep.bc[z] * (size_t)D.bc_len;
                    std::string cb((size_t)D.bc_len, 'A');
                    for (int j = 0; j < D.bc_len; ++j) cb[(size_t)j] = "ACGT"[w[j] & 3];
                    rb.tagZ("CB", cb);
                    ++per_bc[rep.bc[z]];
                }
                b.insert(b.end(), rb.b.begin(), rb.b.end());
                uint8_t b4[4];
                for (int i = 0; i < 4; ++i) b4[i] = (uint8_t)((uint32_t)b.size() >> (8 * i));
                out.write(b4, 4); out.write(b.data(), b.size());
                ++written;
            }
            write_s += seconds(t1, Clock::now());
        }
        seq.clear(); off.clear(); len.clear(); recs.clear(); held.clear();
        return true;
    };
    auto chunk = std::make_shared<RawChunk>();
    Subread r;
    while (read_raw_chunk(in, *chunk)) {
        held.push_back(chunk);
        for (const auto &rec : chunk->recs) {
            parse_subread(rec.first, rec.second, r);
            if (cell_is_tagged(rec.first, rec.second)) return failed("read " + r.name + " already carries an XM, XC or CB tag: IN has been through --cell-reads before");
            ++n_in;
            recs.push_back(rec);
            off.push_back((int64_t)seq.size()); len.push_back((int32_t)r.len);
            seq.resize(seq.size() + r.len);
            if (r.len) r.decode_bases(seq.data() + seq.size() - r.len);
            if (len.size() >= kBatchReads || seq.size() >= kBatchBases) {
                // (the records of this chunk that follow belong to the next batch: the chunk is held again)
                if (!flush()) return failed(ccsx_last_error());
                held.push_back(chunk);
            }
        }
        chunk = std::make_shared<RawChunk>();
    }
    if (!flush()) return failed(ccsx_last_error());
    out.close();
    const Clock::time_point t_end = Clock::now();

    const std::string listed_text = opt.cell_wl ? std::to_string(opt.cell_codes.size() / (size_t)D.bc_len) + " barcodes" : std::string("no whitelist");
    if (!opt.report.empty()) {
        FILE *f = std::fopen(opt.report.c_str(), "w");
        if (!f) { std::fprintf(stderr, "ccs: cannot write %s\n", opt.report.c_str()); return 1; }
        std::fprintf(f, "Cell reads (rule %d: design %s, %s, indels %s; cDNA rule %d: min_polya %d, min_len %d)\n", ccsx_cell_rule_version(), opt.cell_design_text.c_str(),
                     listed_text.c_str(), D.indels ? "on" : "off", ccsx_cdna_rule_version(), opt.cdna_opts.min_polya, opt.cdna_opts.min_len);
        std::fprintf(f, "Reads input                 : %lld\n", (long long)n_in);
        for (int k = 0; k < 7; ++k) std::fprintf(f, "Class %-22s: %lld\n", cls_names[k], (long long)cls_n[k]);
        for (int k = 0; k < 6; ++k) std::fprintf(f, "Tag %-24s: %lld\n", tag_names[k], (long long)tag_n[k]);
        std::fprintf(f, "Full-length, no barcode     : %lld\n", (long long)unlisted);
        std::fprintf(f, "Reads written               : %lld\n", (long long)written);
        std::fclose(f);
    }
    if (!opt.cell_counts.empty()) {
        FILE *f = std::fopen(opt.cell_counts.c_str(), "w");
        if (!f) { std::fprintf(stderr, "ccs: cannot write %s\n", opt.cell_counts.c_str()); return 1; }
        std::fprintf(f, "index\tbarcode\treads\n");
        for (const auto &kv : per_bc) {
            std::string cb((size_t)D.bc_len, 'A');
            for (int j = 0; j < D.bc_len; ++j) cb[(size_t)j] = "ACGT"[opt.cell_codes[(size_t)kv.first * (size_t)D.bc_len + (size_t)j] & 3];
            std::fprintf(f, "%d\t%s\t%lld\n", kv.first, cb.c_str(), (long long)kv.second);
        }
        for (int k = 0; k < 6; ++k) std::fprintf(f, "tag\t%s\t%lld\n", tag_names[k], (long long)tag_n[k]);
        for (int k = 0; k < 7; ++k) std::fprintf(f, "class\t%s\t%lld\n", cls_names[k], (long long)cls_n[k]);
        std::fclose(f);
    }
    if (opt.log_level >= 2)
        std::fprintf(stderr, "ccs: --cell-reads: %lld reads, %lld written; %.3f s (of which ccsx_cell_reads %.3f s, cutting and writing %.3f s, the rest inflate, parsing "
                             "and base decoding)\n", (long long)n_in, (long long)written, seconds(t_start, t_end), call_s, write_s);
    return 0;
}

int main(int argc, char **argv)
{
    Options opt;
    if (!parse(argc, argv, opt)) { usage(); return 2; }
    if (!opt.log_file.empty() && !std::freopen(opt.log_file.c_str(), "w", stderr)) {      // --log-file (docs/faq/sqiie.md:40): every log line goes there
        std::printf("ccs: cannot write %s\n", opt.log_file.c_str());
        return 1;
    }
    int nthreads = opt.threads > 0 ? opt.threads : effective_cores();
    if (nthreads < 1) nthreads = 1;
    try {
        ThreadPool pool(nthreads);
        if (!opt.write_synth.empty()) return write_synthetic(opt, pool);
        if (opt.mark_duplicates) return mark_duplicates(opt, pool);
        if (opt.cell_reads) return cell_reads(opt, pool);

        // ---- --gpu-inflate: a free list of inflaters (declared before the reader, whose slab jobs use them)
        GpuInflaters gpu_inflaters;
        BgzfReader in(opt.in, pool);
        if (opt.gpu_inflate) {
            if ((opt.host_only || opt.dump) && ccsx_device_count() <= 0) {
                if (opt.log_level >= 2) std::fprintf(stderr, "ccs: --gpu-inflate ignored: no engine runs (--host-only, --dump-zmws) and no device is present\n");
            } else {
                if (ccsx_device_count() <= 0) { std::fprintf(stderr, "ccs: no gfx950 GPU available (this build has no CPU consensus path)\n"); return 1; }
                const int dev = opt.gpus.empty() ? 0 : opt.gpus[0];
                if (!gpu_inflaters.create(dev)) { std::fprintf(stderr, "ccs: %s\n", ccsx_last_error()); return 1; }
                if (opt.log_level >= 2) std::fprintf(stderr, "ccs: --gpu-inflate: %d inflaters on device %d\n", GpuInflaters::COUNT, dev);
                in.set_inflate_backend([&gpu_inflaters](const uint8_t *src, size_t src_len, const std::vector<BgzfReader::Span> &spans, uint8_t *dst, size_t dst_len,
                                                        std::vector<int32_t> &status) { return gpu_inflaters.inflate(src, src_len, spans, dst, dst_len, status); });
            }
        }
        BamHeader hdr; read_header(in, hdr);

        // ---- model parameters: --model-file, else by the chemistry triple of the header (docs/faq/chemistry.md:27-56);
        // "Abort if chemistry information is missing in BAM header" (docs/changelog.md:66)
        ccsx_model model;
        std::string chem_desc, chem_bk, chem_sk, chem_bc;   // (the triple: --fit-model writes it into OUT.json)
        if (!opt.dump && !opt.host_only) {
            auto ds_value = [&](const char *key) -> std::string {
                const size_t rg = hdr.text.find("@RG");
                const size_t k = rg == std::string::npos ? rg : hdr.text.find(std::string(key) + "=", rg);
                if (k == std::string::npos) return "";
                const size_t a = k + std::strlen(key) + 1, e = hdr.text.find_first_of(";\t\n", a);
                return hdr.text.substr(a, e == std::string::npos ? std::string::npos : e - a);
            };
            const std::string bk = ds_value("BINDINGKIT"), sk = ds_value("SEQUENCINGKIT"), bc = ds_value("BASECALLERVERSION");
            chem_bk = bk; chem_sk = sk; chem_bc = bc;
            if (!opt.model_file.empty()) {
                if (ccsx_model_load(opt.model_file.c_str(), &model)) { std::fprintf(stderr, "ccs: %s\n", ccsx_last_error()); return 1; }
                chem_desc = std::string(model.name) + " (" + opt.model_file + ")";
            } else {
                if (bk.empty() || sk.empty() || bc.empty()) {
                    std::fprintf(stderr, "ccs: missing chemistry information in the BAM header (@RG DS: BINDINGKIT, SEQUENCINGKIT, BASECALLERVERSION)\n");
                    return 1;
                }
                if (ccsx_model_for_chemistry(bk.c_str(), sk.c_str(), bc.c_str(), &model)) { std::fprintf(stderr, "ccs: %s\n", ccsx_last_error()); return 1; }
                chem_desc = std::string(model.name) + " for " + bk + "/" + sk + "/" + bc;
            }
            if (opt.log_level >= 2) std::fprintf(stderr, "ccs: consensus model %s\n", chem_desc.c_str());   // docs/changelog.md:101
        }

        // ---- devices (not needed for --dump-zmws): one engine handle per device
        std::vector<ccsx_handle> handles;
        if (!opt.dump && !opt.host_only) {
            const int ndev = ccsx_device_count();
            if (ndev <= 0) { std::fprintf(stderr, "ccs: no gfx950 GPU available (this build has no CPU consensus path)\n"); return 1; }
            if (opt.all_gpus && !opt.fit_model.empty() && ndev > 1) { std::fprintf(stderr, "ccs: --fit-model runs on one GPU: --gpus all names %d\n", ndev); return 2; }
            if (opt.all_gpus) for (int d = 0; d < ndev; ++d) opt.gpus.push_back(d);
            if (opt.gpus.empty()) opt.gpus.push_back(0);
            for (int d : opt.gpus) {
                // (the handle's page-locked layout arrays are allocated by the creating thread: create it from the device's NUMA node, then come back)
                cpu_set_t aff; const bool have_aff = sched_getaffinity(0, sizeof(aff), &aff) == 0;
                const int node = ccsx_bind_thread_to_device(d);
                ccsx_handle h = nullptr;
                const int rc_create = ccsx_create(d, &model, &opt.o, &h);
                if (have_aff) sched_setaffinity(0, sizeof(aff), &aff);
                if (rc_create) { std::fprintf(stderr, "ccs: %s\n", ccsx_last_error()); return 1; }
                if (opt.log_level >= 2) std::fprintf(stderr, "ccs: device %d: NUMA node %d%s\n", d, ccsx_device_numa_node(d), node >= 0 ? " (its threads and page-locked staging are bound to it)" : " (no binding)");
                handles.push_back(h);
            }
        }

        // ---- --gpu-deflate: one deflater on the first engine device, shared by the run's BAM writers (declared here: it outlives the writer thread)
        GpuDeflater gpu_deflater;
        const bool fastq_out = opt.out.size() > 9 && opt.out.compare(opt.out.size() - 9, 9, ".fastq.gz") == 0;
        bool use_gpu_deflate = false;
        if (opt.gpu_deflate) {
            if (opt.host_only || opt.dump) {
                if (opt.log_level >= 2) std::fprintf(stderr, "ccs: --gpu-deflate ignored: no engine runs (--host-only, --dump-zmws)\n");
            } else if (fastq_out && opt.fail_reads.empty()) {
                if (opt.log_level >= 2) std::fprintf(stderr, "ccs: --gpu-deflate ignored: OUT.fastq.gz is written by gzip on the host and no BAM is written\n");
            } else {
                const int dev = opt.gpus[0];
                if (!gpu_deflater.create(dev)) { std::fprintf(stderr, "ccs: %s\n", ccsx_last_error()); for (ccsx_handle h : handles) ccsx_destroy(h); return 1; }
                if (opt.log_level >= 2) std::fprintf(stderr, "ccs: --gpu-deflate: tickets of %zu blocks on device %d, two in flight\n", gpu_deflater.ticket_blocks(), dev);
                use_gpu_deflate = true;
            }
        }

        g_plain_arenas = opt.host_only;
        // Round 6 (NUMA): every device has its own packing threads, staging pools and queue to its worker, all bound to the device's NUMA node, so a batch's
        // page-locked staging is local to the GPU that uploads it.  The ZMW stream is still ONE queue (to_pack): a packer whose device queue is full stops
        // drawing from it, so the work flows to the devices that are free (dynamic, not an i/N split).
        const size_t ndev_q = std::max<size_t>(1, handles.size());
        Channel<std::shared_ptr<Batch>> to_pack(2 * ndev_q), to_writer(4 * ndev_q);
        std::vector<std::unique_ptr<Channel<std::shared_ptr<Batch>>>> to_gpu_q;
        for (size_t d = 0; d < ndev_q; ++d) to_gpu_q.emplace_back(new Channel<std::shared_ptr<Batch>>(2));
        std::string movie;
        const auto t_start = std::chrono::steady_clock::now();

        // an exception on any pipeline thread ends the run with a message and exit code 1 (the other threads are drained, not killed)
        std::atomic<int> failed{0};
        std::atomic<int> enough{0};                           // --fit-max-zmws: the training mode has the ZMWs it wants, the reader stops
        std::mutex err_m;
        std::string err_msg;
        auto fail = [&](const std::string &m) { std::lock_guard<std::mutex> l(err_m); if (!failed.exchange(1)) err_msg = m; };

        // ---- IN.bam.pbi: random access for --chunk, and the number of ZMWs ahead for the progress line.  --chunk i/N with N > 1
        // REQUIRES the index (docs/faq/parallelize.md:9-13): every job of a sharded run must partition the ZMWs the same way, so a
        // missing, unreadable or stale index is fatal instead of a silent switch to another scheme
        bool have_pbi = false, chunk_done = false;
        int64_t chunk_zmws = 0, total_zmws = -1;
        int pbi_first_hole = -1;                              // the ZMW the index promises at the seek target (a stale index is an error)
        int pbi_next_hole = -1;                               // ... and right after the chunk's last record (-1: the chunk ends the file)
        int64_t pbi_chunk_records = -1, seen_records = 0;     // records the index counts inside the chunk
        {
            PbiIndex pbi;
            bool ok = false;
            std::string why = "not found";
            try { ok = read_pbi(opt.in + ".pbi", pool, pbi); }
            catch (const std::exception &e) { why = e.what(); if (opt.chunk_n <= 1) std::fprintf(stderr, "ccs: warning: ignoring %s.pbi: %s\n", opt.in.c_str(), e.what()); }
            if (opt.chunk_n > 1 && !(ok && pbi.size() > 0))
                throw std::runtime_error("--chunk needs a usable " + opt.in + ".pbi (" + why + "): generate the index first (docs/faq/parallelize.md:9-13)");
            if (ok && pbi.size() > 0) {
                std::vector<size_t> first;                        // first record of every ZMW (consecutive records of one hole number)
                for (size_t i = 0; i < pbi.size(); ++i) if (i == 0 || pbi.hole[i] != pbi.hole[i - 1]) first.push_back(i);
                const int64_t Z = (int64_t)first.size();
                total_zmws = Z;
                if (opt.chunk_n > 1) {
                    const int64_t lo = (opt.chunk_i - 1) * Z / opt.chunk_n, hi = (int64_t)opt.chunk_i * Z / opt.chunk_n;
                    have_pbi = true; chunk_zmws = hi - lo; total_zmws = chunk_zmws;
                    if (chunk_zmws == 0) chunk_done = true;
                    else {
                        in.seek((uint64_t)pbi.file_offset[first[(size_t)lo]]); pbi_first_hole = pbi.hole[first[(size_t)lo]];
                        pbi_chunk_records = (int64_t)((hi < Z ? first[(size_t)hi] : pbi.size()) - first[(size_t)lo]);
                        pbi_next_hole = hi < Z ? pbi.hole[first[(size_t)hi]] : -1;
                    }
                    std::fprintf(stderr, "ccs: chunk %d/%d = ZMWs %" PRId64 "..%" PRId64 " of %" PRId64 " by random access (%s.pbi)\n", opt.chunk_i, opt.chunk_n, lo, hi, Z, opt.in.c_str());
                }
            }
        }

        // ---- reader
        long long rd_us[3] = {0, 0, 0};                  // framing (BGZF inflate wait), waiting for record decode, grouping + filters + queue
        std::thread reader([&] {
            try {
            ZmwIn cur; bool have = false;
            int64_t nz = 0, nb = 0;
            auto batch = std::make_shared<Batch>();
            long long batch_cost = 0;                        // subread bases of the ZMWs in `batch` that will reach the engine
            auto emit_zmw = [&](ZmwIn &zin) {
                finish_zmw(zin, opt);
                if (opt.dump) {
                    unsigned long long hsh = 1469598103934665603ull;       // FNV-1a over bases, pw, ip of the kept passes (reader self-check)
                    std::vector<uint8_t> tmp;
                    for (const Subread &r : zin.reads) for (int a = 0; a < 3; ++a) {
                        tmp.resize(r.size());
                        if (a == 0) r.decode_bases(tmp.data()); else if (a == 1) r.decode_pw(tmp.data()); else r.decode_ip(tmp.data());
                        for (uint8_t x : tmp) { hsh ^= x; hsh *= 1099511628211ull; }
                    }
                    std::printf("%d%s\t%d\t%zu\t%.2f,%.2f,%.2f,%.2f\t%016llx\n", zin.zm, zin.strand_tag == 1 ? "/fwd" : (zin.strand_tag == 2 ? "/rev" : ""), zin.host_status,
                                zin.reads.size(), zin.snr[0], zin.snr[1], zin.snr[2], zin.snr[3], hsh);
                }
                else {
                    // cost-binned batches: the engine's work grows with passes x length (= the subread bases), which spreads over
                    // ~400x in a Sequel-II-like mix; a batch closes at --batch-size ZMWs or --batch-bases bases, whichever comes first, so every
                    // ticket the GPU workers draw from the shared queue costs about the same (and its staging stays bounded)
                    long long cost = 0;
                    if (zin.host_status == HS_OK) for (const Subread &r : zin.reads) cost += (long long)r.size();
                    const int lim_zmws = opt.batch > 0 ? opt.batch : auto_batch_zmws(nb);
                    const long long lim_bases = opt.batch_bases > 0 ? opt.batch_bases : kDefaultBasesPerZmw * lim_zmws;
                    if (!batch->zmws.empty() && batch_cost + cost > lim_bases) { batch->index = nb++; to_pack.push(batch); batch = std::make_shared<Batch>(); batch_cost = 0; }
                    batch->zmws.push_back(std::move(zin));
                    batch_cost += cost;
                    if ((int)batch->zmws.size() >= (opt.batch > 0 ? opt.batch : auto_batch_zmws(nb))) { batch->index = nb++; to_pack.push(batch); batch = std::make_shared<Batch>(); batch_cost = 0; }
                }
            };
            auto flush_zmw = [&] {
                if (!have) return;
                // --chunk i/N: with IN.bam.pbi a contiguous range of ZMWs (the reader has seeked to its first record and stops after
                // its last ZMW: docs/faq/parallelize.md:9-13); without an index round-robin over the ZMWs of the whole file
                const bool mine = have_pbi ? (nz < chunk_zmws) : true;
                cur.order = nz++;
                if (have_pbi && nz >= chunk_zmws) chunk_done = true;
                if (mine) {
                    // strand of every pass: cx REVERSE_PASS (32) / FORWARD_PASS (16) when present, else consecutive subreads alternate — with
                    // --orient-passes only as a prior: such a pass is submitted strand-unknown and the engine decides
                    for (size_t k = 0; k < cur.reads.size(); ++k) {
                        Subread &r = cur.reads[k];
                        const bool given = r.cx >= 0 && (r.cx & 48);
                        r.strand = given ? (uint8_t)((r.cx & 32) ? 1 : 0) : (uint8_t)(k & 1);
                        r.strand_unknown = (opt.orient_passes && !given) ? 1 : 0;
                    }
                    if (!opt.by_strand) emit_zmw(cur);
                    else {                                   // each strand is treated as an individual entity (mode-by-strand.md:16-23)
                        ZmwIn f, rv;
                        f.zm = rv.zm = cur.zm; f.order = rv.order = cur.order; f.strand_tag = 1; rv.strand_tag = 2;
                        std::memcpy(f.snr, cur.snr, 16); std::memcpy(rv.snr, cur.snr, 16);
                        for (Subread &r : cur.reads) (r.strand ? rv : f).reads.push_back(std::move(r));
                        emit_zmw(f); emit_zmw(rv);
                    }
                }
                cur = ZmwIn(); have = false;
            };
            // this thread only frames records; decoding runs on the pool, results are consumed in order
            std::deque<std::future<std::vector<Subread>>> pending;
            auto consume = [&](std::vector<Subread> recs) {
                for (Subread &rec : recs) {
                    if (pbi_first_hole >= 0) {                       // first record after the seek
                        if (rec.zm != pbi_first_hole) throw std::runtime_error(opt.in + ".pbi does not match the BAM (stale index?): delete it or re-index");
                        pbi_first_hole = -1;
                    }
                    if (movie.empty()) movie = movie_of(rec.name);
                    if (chunk_done) break;                           // records of the next chunk that shared the last inflated run
                    if (!have || rec.zm != cur.zm) {
                        flush_zmw(); cur.zm = rec.zm; have = true;
                        if (chunk_done) {                            // the chunk's last ZMW has just ended: the index must agree on where
                            if (seen_records != pbi_chunk_records || rec.zm != pbi_next_hole)
                                throw std::runtime_error(opt.in + ".pbi does not match the BAM (record count / next ZMW of the chunk differ: stale index?)");
                            break;
                        }
                    }
                    ++seen_records;
                    if (rec.has_snr) std::memcpy(cur.snr, rec.snr, 16);
                    cur.reads.push_back(std::move(rec));
                }
            };
            for (;;) {
                auto raw = std::make_shared<RawChunk>();
                auto t0 = std::chrono::steady_clock::now();
                const bool more = !chunk_done && read_raw_chunk(in, *raw);
                rd_us[0] += std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
                if (failed || enough) break;                        // an engine / writer failure ends the run: stop feeding it (or --fit-max-zmws is reached)
                if (more) pending.push_back(pool.submit([raw] { return decode_chunk(std::shared_ptr<const RawChunk>(raw)); }));
                while (!pending.empty() && (!more || pending.size() > (size_t)(2 * pool.size() + 4))) {
                    t0 = std::chrono::steady_clock::now();
                    auto recs = pending.front().get();
                    auto t1 = std::chrono::steady_clock::now();
                    consume(std::move(recs)); pending.pop_front();
                    rd_us[1] += std::chrono::duration_cast<std::chrono::microseconds>(t1 - t0).count();
                    rd_us[2] += std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t1).count();
                }
                if (!more) break;
            }
            if (!chunk_done && !enough) {                          // (a finished chunk ends inside the next chunk's first ZMW)
                flush_zmw();
                if (have_pbi && (seen_records != pbi_chunk_records || pbi_next_hole != -1 || !chunk_done))
                    throw std::runtime_error(opt.in + ".pbi does not match the BAM (the file ends before the chunk does: stale index?)");
            }
            if (!opt.dump && !batch->zmws.empty()) { batch->index = nb++; to_pack.push(batch); }
            } catch (const std::exception &e) { fail(std::string("reading ") + opt.in + ": " + e.what()); }
            to_pack.close();
        });
        if (opt.dump) {
            reader.join();
            if (opt.log_level >= 2)
                std::fprintf(stderr, "ccs: reader thread: framing/inflate %.2f s, waiting for record decode %.2f s, grouping+filters+queue %.2f s\n",
                             rd_us[0] * 1e-6, rd_us[1] * 1e-6, rd_us[2] * 1e-6);
            if (failed) std::fprintf(stderr, "ccs: %s\n", err_msg.c_str());
            return failed ? 1 : 0;
        }

        // ---- pack workers: SoA packing off the reader thread, straight into page-locked staging; result views are carved from a
        // second page-locked arena (the downloads are asynchronous DMA)
        std::vector<std::unique_ptr<ArenaPool>> in_pools, out_pools;
        for (size_t d = 0; d < ndev_q; ++d) { in_pools.emplace_back(new ArenaPool()); out_pools.emplace_back(new ArenaPool()); }
        std::atomic<long long> unknown_passes{0};                          // --orient-passes: passes submitted strand-unknown
        std::atomic<long long> us_pack{0}, us_engine{0}, us_wait{0};       // summed over workers (--log-level INFO)
        auto now = [] { return std::chrono::steady_clock::now(); };
        auto us_since = [](std::chrono::steady_clock::time_point t) { return (long long)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t).count(); };
        const bool kin = opt.o.hifi_kinetics != 0;
        const bool fail_reads = !opt.fail_reads.empty();
        const bool screen = !opt.adapters.empty();                  // (needs fail_reads)
        const bool control = !opt.control.empty();
        const bool coverage = opt.coverage_filters;
        const bool barcodes = !opt.barcodes.empty();
        const bool segments = !opt.segment_adapters.empty();
        const bool cdna = !opt.cdna_primers.empty();
        static_assert(sizeof(ccsx_segment_piece) * CCSX_SEGMENT_MAX_PIECES == 192 * 4, "the segment list is carved as 192 words per ZMW");
        // The views of a staged batch's results and reports, carved from a page-locked arena of its device's pool, and the requests that point to them: every
        // ticket of the run is given the same (finder: plus the heteroduplex request, which the single-strand tickets of --heteroduplexes split do not carry)
        static_assert(sizeof(ccsx_hd_site) == 24, "the finder's site list is carved as 96 words per ZMW");
        auto carve_outputs = [&](const std::shared_ptr<Batch> &b, ArenaPool &out_pool, bool finder) {
            const int n = b->n;
            b->seq_off.resize(n + 1);
            const int64_t cap = ccsx_result_layout(&b->cb, b->seq_off.data());
            b->cap = cap;
            b->out_arena = out_pool.get();
            const size_t n4 = ((size_t)n * 4 + 63) & ~(size_t)63, c1 = ((size_t)cap + 63) & ~(size_t)63;
            uint8_t *o = b->out_arena->reserve((9 + (opt.min_tandem > 0 ? 1 : 0) + (fail_reads ? 4 : 0) + (screen ? 9 + 3 * CCSX_ADAPTER_MAX_HITS : 0) + (control ? 8 : 0) + (coverage ? 10 : 0) + (barcodes ? 11 : 0) + (segments ? 8 + 192 : 0) + (cdna ? 16 : 0) + (opt.reads_bam ? 2 : 0) + (finder ? 103 : 0)) * n4 + ((kin ? 6 : 2) + (opt.pileup ? 3 : 0)) * c1);
            auto take = [&](size_t bytes) { uint8_t *r = o; o += bytes; return r; };
            auto planes = [&](int k) { std::vector<int32_t *> v(k); for (auto &p : v) p = (int32_t *)take(n4); return v; };   // a report's k arrays
            b->status = (int32_t *)take(n4); b->seq_len = (int32_t *)take(n4); b->np = (int32_t *)take(n4); b->iters = (int32_t *)take(n4);
            b->n_windows = (int32_t *)take(n4); b->fn = (int32_t *)take(n4); b->rn = (int32_t *)take(n4);
            b->rq = (float *)take(n4); b->ec = (float *)take(n4);
            b->seq = take(c1); b->qual = take(c1);
            b->cr = ccsx_results{n, cap, b->seq_off.data(), b->status, b->seq_len, b->seq, b->qual, nullptr, b->rq, b->np, b->ec, b->iters, b->n_windows};
            b->cr.fn = b->fn; b->cr.rn = b->rn;
            if (kin) {
                b->kin = take(4 * c1);
                // planes are cap bytes apart in the library's result layout
                b->cr.fi = b->kin; b->cr.fp = b->kin + cap; b->cr.ri = b->kin + 2 * cap; b->cr.rp = b->kin + 3 * cap;
            }
            if (opt.pileup) {
                b->pile = take(3 * c1);
                b->cp = ccsx_pileup{cap, b->pile, b->pile + cap, b->pile + 2 * cap};
            }
            if (opt.min_tandem > 0) {
                b->tlen = (int32_t *)take(n4);
                b->ex = ccsx_extras{opt.pileup ? &b->cp : nullptr, b->tlen, opt.min_tandem, 0};
            } else if (opt.pileup) b->ex = ccsx_extras{&b->cp, nullptr, 0, 0};
            if (fail_reads) {
                const auto f = planes(4);
                b->fold = f[0];
                b->frep = ccsx_fold_report{n, f[0], f[1], f[2], f[3]};
                b->freq = ccsx_fold_request{nullptr, &b->frep, {0, 0}};
            }
            if (screen) {
                const auto a9 = planes(9);
                ccsx_adapter_hit *hits = (ccsx_adapter_hit *)take(3 * CCSX_ADAPTER_MAX_HITS * n4);
                b->arep = ccsx_adapter_report{n, a9[0], a9[1], a9[2], a9[3], a9[4], a9[5], a9[6], a9[7], a9[8], hits};
                b->areq = ccsx_adapter_request{&opt.adapter_set, nullptr, &b->arep, {0, 0}};
            }
            if (control) {
                const auto c8 = planes(8);
                b->crep = ccsx_control_report{n, c8[0], c8[1], c8[2], c8[3], c8[4], c8[5], c8[6], c8[7]};
                b->creq = ccsx_control_request{&opt.control_seq, nullptr, &b->crep, {0, 0}};
            }
            if (coverage) {
                const auto v = planes(10);
                b->vrep = ccsx_coverage_report{n, v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9]};
                b->vreq = ccsx_coverage_request{&opt.coverage_opts, &b->vrep, 0x3cu, {0, 0}};   // all four gate bits
            }
            if (barcodes) {                          // tested, call, bq: n each; idx, dist, second, clip: [n][2]
                const auto b3 = planes(3);
                int32_t *two[4];
                for (auto &q : two) q = (int32_t *)take(2 * n4);
                b->brep = ccsx_barcode_report{n, b3[0], b3[1], b3[2], two[0], two[1], two[2], two[3]};
                b->breq = ccsx_barcode_request{&opt.barcode_opts, opt.barcode_set.get(), &b->brep, {0, 0}};
            }
            if (segments) {                          // the eight planes: n each; the list: [n][64] of 12 bytes
                const auto g = planes(8);
                ccsx_segment_piece *list = (ccsx_segment_piece *)take(192 * n4);
                b->srep = ccsx_segment_report{n, g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7], list};
                b->sreq = ccsx_segment_request{&opt.segment_opts, opt.segment_set.get(), &b->srep, {0, 0}};
            }
            if (cdna) {                              // the eight planes: n each; idx, dist, second, clip: [n][2]
                const auto d = planes(8);
                int32_t *two[4];
                for (auto &q : two) q = (int32_t *)take(2 * n4);
                b->drep = ccsx_cdna_report{n, d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], two[0], two[1], two[2], two[3]};
                b->dreq = ccsx_cdna_request{&opt.cdna_opts, opt.cdna_set.get(), &b->drep, {0, 0}};
            }
            if (opt.reads_bam) {
                const auto r2 = planes(2);
                b->rrep = ccsx_represent_report{n, r2[0], r2[1]};
                b->rreq = ccsx_represent_request{opt.reads_fallback ? 1 : 0, opt.reads_kinetics ? 1 : 0, &b->rrep, {0, 0}};
            }
            if (finder) {                                // verdict, n_sub_sites, n_indel_sites, n_listed, status: n each; min_p: n doubles; sites: [n][16] of 24 bytes
                const auto h5 = planes(5);
                double *min_p = (double *)take(2 * n4);
                ccsx_hd_site *sites = (ccsx_hd_site *)take(96 * n4);
                b->hrep = ccsx_hd_report{n, h5[0], h5[1], h5[2], h5[3], min_p, sites, h5[4]};
                b->hreq = ccsx_hd_request{nullptr, &b->hrep, 1, 0};   // ccsx_hd_opts_default, split = 1
            }
            b->reqs = ccsx_requests{(opt.min_tandem > 0 || opt.pileup) ? &b->ex : nullptr, fail_reads ? &b->freq : nullptr, screen ? &b->areq : nullptr,
                                  control ? &b->creq : nullptr, coverage ? &b->vreq : nullptr, {nullptr, nullptr, nullptr}};
        };
        std::vector<std::thread> packers;
        const size_t n_packers = std::max<size_t>(1, handles.size()) * (size_t)opt.workers_per_gpu;
        std::vector<std::atomic<int>> packers_left(ndev_q);
        for (size_t d = 0; d < ndev_q; ++d) packers_left[d] = (int)(n_packers / ndev_q);
        for (size_t pk = 0; pk < n_packers; ++pk) packers.emplace_back([&, pk] {
            const int dev = (int)(pk % ndev_q);
            if (!handles.empty()) ccsx_bind_thread_to_device(opt.gpus[dev]);
            ArenaPool &in_pool = *in_pools[dev], &out_pool = *out_pools[dev];
            Channel<std::shared_ptr<Batch>> &to_gpu = *to_gpu_q[dev];
            std::shared_ptr<Batch> b;
            while (to_pack.pop(b)) {
                auto t0 = now();
                b->dev = dev;
                try {
                    b->in_arena = in_pool.get();
                    unknown_passes += pack(*b, *b->in_arena);
                    const int n = (int)b->zmw_id.size();
                    b->n = n;
                    if (n > 0 && !opt.host_only) {
                        b->cb = ccsx_batch{n, (int32_t)b->flags.size(), b->n_bases, b->zmw_id.data(), b->snr.data(), b->read_off.data(),
                                           b->base_off.data(), b->bases, b->pw, b->ipd, b->flags.data()};
                        carve_outputs(b, out_pool, opt.heteroduplexes != 0);
                    }
                } catch (const std::exception &e) { fail(std::string("packing a batch: ") + e.what()); b->n = -1; }
                us_pack += us_since(t0);
                to_gpu.push(b);
            }
            if (--packers_left[dev] == 0) to_gpu.close();
        });

        if (opt.host_only) {                                  // no engine: count what arrives, hand the staging back
            int64_t nz = 0, nzok = 0, nbases = 0, nbatches = 0;
            std::thread sink([&] {
                std::shared_ptr<Batch> b;
                while (to_gpu_q[0]->pop(b)) { ++nbatches; nz += (int64_t)b->zmws.size(); if (b->n > 0) { nzok += b->n; nbases += b->n_bases; } in_pools[0]->put(std::move(b->in_arena)); }
            });
            reader.join();
            for (auto &w : packers) w.join();
            sink.join();
            const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
            std::fprintf(stderr, "ccs: reader thread: framing/inflate %.2f s, waiting for record decode %.2f s, grouping+filters+queue %.2f s; packing (sum over %zu threads) %.2f s\n",
                         rd_us[0] * 1e-6, rd_us[1] * 1e-6, rd_us[2] * 1e-6, n_packers, us_pack.load() * 1e-6);
            std::printf("host-only: %" PRId64 " ZMWs read, %" PRId64 " packed (%" PRId64 " bases) in %.2f s = %.1f ZMWs/s on %d host threads + %zu pack threads; %" PRId64 " batches\n", nz, nzok, nbases, el,
                        nz / el, nthreads, n_packers, nbatches);
            if (failed) std::fprintf(stderr, "ccs: %s\n", err_msg.c_str());
            return failed ? 1 : 0;
        }

        if (!opt.fit_model.empty()) {                         // the training mode: keep the packed batches, iterate over them (fit_model below)
            std::vector<std::shared_ptr<Batch>> kept;
            long long have_zmws = 0;
            std::thread sink([&] {
                std::shared_ptr<Batch> b;
                while (to_gpu_q[0]->pop(b)) {
                    if (b->n <= 0 || enough) continue;
                    if (opt.fit_max_zmws > 0 && have_zmws + b->n >= opt.fit_max_zmws) {      // the batch's first ZMWs: the arrays are CSR, a prefix is a batch
                        const int n = (int)(opt.fit_max_zmws - have_zmws);
                        b->n = n; b->cb.n_zmw = n; b->cb.n_reads = b->read_off[n]; b->cb.n_bases = b->base_off[b->read_off[n]];
                        enough = 1;
                    }
                    have_zmws += b->n;
                    kept.push_back(b);
                }
            });
            reader.join();
            for (auto &w : packers) w.join();
            sink.join();
            int rc = failed ? 1 : 0;
            if (failed) std::fprintf(stderr, "ccs: %s\n", err_msg.c_str());
            else rc = fit_model(opt, handles[0], model, kept, chem_bk, chem_sk, chem_bc);
            if (handles[0]) ccsx_destroy(handles[0]);
            return rc;
        }

        // ---- GPU workers: one per device; up to three batches in flight through the asynchronous boundary
        struct { long long tickets = 0, zmws = 0; double draft = 0, polish = 0, queue = 0, total = 0, first = 0, last = 0; } eng;   // ticket timings, --log-level INFO
        decltype(eng) eng_ss;                                 // ... of the single-strand tickets (--heteroduplexes split)
        std::mutex eng_m;
        const bool hd_split = opt.heteroduplexes == HD_SPLIT;
        std::vector<std::thread> workers;
        for (size_t wd = 0; wd < handles.size(); ++wd) workers.emplace_back([&, wd] {
            ccsx_handle h = handles[wd];
            ccsx_bind_thread_to_device(opt.gpus[wd]);
            ArenaPool &in_pool = *in_pools[wd];
            Channel<std::shared_ptr<Batch>> &to_gpu = *to_gpu_q[wd];
            ArenaPool &out_pool = *out_pools[wd];
            std::deque<std::pair<ccsx_ticket, std::shared_ptr<Batch>>> inflight;
            // --heteroduplexes split: the HETERODUPLEX ZMWs of a retired batch as single-strand entities (api.split_strands, the split the reader makes for
            // --by-strand): per ZMW its forward passes as one entity, then its reverse passes as the next, both keeping zm and snr; within a strand the
            // full-length passes first, each group in batch order; a strand without passes yields no entity.  Copied from the batch's staging, which is still
            // held, into staging of its own (the pools hand out a new arena when none is free: nothing here waits for another batch).  nullptr: no such ZMW
            std::vector<std::shared_ptr<Batch>> strand_parents;    // the batches whose strand ticket is in flight (a strand batch names its parent, it does not own it)
            auto strand_batch = [&](Batch &b) -> std::shared_ptr<Batch> {
                std::vector<int> het;
                for (int s = 0; s < b.n; ++s) if (b.status[s] == CCSX_HETERODUPLEX) het.push_back(s);
                if (het.empty()) return nullptr;
                auto sb = std::make_shared<Batch>();
                sb->index = b.index; sb->dev = b.dev; sb->parent = &b;
                b.strand_slot.assign((size_t)2 * b.n, -1);
                std::vector<int> reads;                             // the passes of the new batch, as indices into b's
                sb->read_off.assign(1, 0); sb->base_off.assign(1, 0);
                int64_t total = 0;
                for (int s : het) for (int strand = 0; strand < 2; ++strand) {
                    const size_t before = reads.size();
                    for (int partial = 0; partial < 2; ++partial)
                        for (int r = b.read_off[s]; r < b.read_off[s + 1]; ++r)
                            if ((b.flags[r] & 1) == strand && ((b.flags[r] >> 1) & 1) == partial) reads.push_back(r);
                    if (reads.size() == before) continue;
                    b.strand_slot[2 * s + strand] = (int)sb->zmw_id.size();
                    sb->zmw_id.push_back(b.zmw_id[s]);
                    sb->snr.insert(sb->snr.end(), b.snr.begin() + 4 * s, b.snr.begin() + 4 * s + 4);
                    sb->read_off.push_back((int32_t)reads.size());
                }
                for (int r : reads) total += b.base_off[r + 1] - b.base_off[r];
                sb->in_arena = in_pool.get();
                uint8_t *base = sb->in_arena->reserve((size_t)3 * (size_t)total);
                uint8_t *planes[3] = {base, base + total, base + 2 * total};
                const uint8_t *from[3] = {b.bases, b.pw, b.ipd};
                int64_t at = 0;
                for (int r : reads) {
                    const int64_t o = b.base_off[r], L = b.base_off[r + 1] - o;
                    for (int k = 0; k < 3; ++k) std::memcpy(planes[k] + at, from[k] + o, (size_t)L);
                    at += L;
                    sb->flags.push_back(b.flags[r]);
                    sb->base_off.push_back(at);
                }
                sb->bases = planes[0]; sb->pw = planes[1]; sb->ipd = planes[2]; sb->n_bases = total;
                sb->n = (int)sb->zmw_id.size();
                sb->cb = ccsx_batch{sb->n, (int32_t)sb->flags.size(), sb->n_bases, sb->zmw_id.data(), sb->snr.data(), sb->read_off.data(),
                                    sb->base_off.data(), sb->bases, sb->pw, sb->ipd, sb->flags.data()};
                carve_outputs(sb, out_pool, false);
                return sb;
            };
            auto retire = [&] {
                auto t0 = now();
                auto fr = std::move(inflight.front()); inflight.pop_front();
                std::shared_ptr<Batch> b = fr.second;
                const bool is_strand = b->parent != nullptr;
                if (ccsx_wait(h, fr.first)) fail(std::string("consensus engine: ") + ccsx_last_error());
                else {
                    b->have_results = true;
                    ccsx_timings tm;
                    if (opt.log_level >= 2 && ccsx_ticket_timings(h, fr.first, &tm) == 0) {       // the engine's own device times of this ticket (HIP events)
                        std::lock_guard<std::mutex> l(eng_m);
                        auto &e = is_strand ? eng_ss : eng;
                        e.tickets += 1; e.zmws += b->n;
                        e.draft += tm.draft_ms + tm.align_ms; e.polish += tm.polish_ms; e.queue += tm.queue_ms; e.total += tm.total_ms;
                        if (e.tickets == 1 || tm.start_ms < e.first) e.first = tm.start_ms;
                        if (e.tickets == 1 || tm.end_ms > e.last) e.last = tm.end_ms;
                    }
                }
                // --heteroduplexes split: the second ticket.  The batch's HETERODUPLEX ZMWs become a single-strand batch while its staging is still held; that
                // batch is submitted as an ordinary ticket with the run's other requests and no finder, into the slot this retirement has just freed (at most
                // three in flight), and the batch goes to the writer when the strand ticket has retired: OUT keeps input order
                std::shared_ptr<Batch> sb;
                if (hd_split && !is_strand && b->have_results && !failed) {
                    try { sb = strand_batch(*b); }
                    catch (const std::exception &e) { fail(std::string("packing a single-strand batch: ") + e.what()); sb.reset(); b->have_results = false; }
                }
                in_pool.put(std::move(b->in_arena));                // inputs are on the device (and consumed): the staging is free again
                b->bases = b->pw = b->ipd = nullptr;
                if (sb) {
                    ccsx_ticket t = -1;
                    b->strand = sb;
                    if (ccsx_submit_requests(h, &sb->cb, &sb->cr, &sb->reqs, &t)) {
                        fail(std::string("consensus engine: ") + ccsx_last_error());
                        sb->have_results = false;
                        in_pool.put(std::move(sb->in_arena));
                    } else {
                        inflight.emplace_back(t, sb);
                        strand_parents.push_back(b);
                        us_engine += us_since(t0);
                        return;                                     // (the writer gets b when sb retires)
                    }
                }
                us_engine += us_since(t0);
                if (!is_strand) { to_writer.push(b); return; }
                // a retired strand ticket: its parent, which holds it, goes to the writer now
                for (auto &held : strand_parents) if (held.get() == b->parent) { auto p = held; held = strand_parents.back(); strand_parents.pop_back(); to_writer.push(p); return; }
            };
            std::shared_ptr<Batch> b;
            for (;;) {
                auto t0 = now();
                if (!to_gpu.pop(b)) break;
                us_wait += us_since(t0);
                if (b->n <= 0 || failed) {                          // nothing for the GPU (all ZMWs failed on the host), or the run is ending
                    if (b->n > 0 || b->n < 0) b->have_results = false;
                    while (!inflight.empty()) retire();             // keep batch order towards the writer cheap: drain first
                    in_pool.put(std::move(b->in_arena));
                    to_writer.push(b);
                    continue;
                }
                while (inflight.size() >= 3) retire();              // (a retirement may put a strand ticket into the slot it freed: --heteroduplexes split)
                t0 = now();
                ccsx_ticket t = -1;
                // the most general submit: NULL for the extras and for every request this run did not ask for (the narrower entry points stage the same)
                if (opt.heteroduplexes ? ccsx_submit_hd_requests(h, &b->cb, &b->cr, &b->reqs, &b->hreq, &t)
                    : opt.reads_bam ? ccsx_submit_represent(h, &b->cb, &b->cr, &b->reqs, &b->rreq, &t)
                                  : barcodes ? ccsx_submit_barcodes(h, &b->cb, &b->cr, &b->reqs, &b->breq, &t)
                                  : segments ? ccsx_submit_segments(h, &b->cb, &b->cr, &b->reqs, &b->sreq, &t)
                                  : cdna ? ccsx_submit_cdna(h, &b->cb, &b->cr, &b->reqs, &b->dreq, &t) : ccsx_submit_requests(h, &b->cb, &b->cr, &b->reqs, &t)) {
                    // a failed batch must never reach the writer looking like SUCCESS records: it carries no results,
                    // the run is marked failed and ends with exit code 1 and no output file
                    fail(std::string("consensus engine: ") + ccsx_last_error());
                    b->have_results = false;
                    while (!inflight.empty()) retire();
                    in_pool.put(std::move(b->in_arena));
                    to_writer.push(b);
                } else inflight.emplace_back(t, b);
                us_engine += us_since(t0);
            }
            while (!inflight.empty()) retire();
        });

        // ---- writer (restores batch order)
        Report rep;
        const bool fastq = opt.out.size() > 9 && opt.out.compare(opt.out.size() - 9, 9, ".fastq.gz") == 0;   // OUT.fastq.gz (docs/index.md:55-58)
        std::thread writer([&] {
            try {
            std::unique_ptr<BgzfWriter> outp;
            gzFile gzq = nullptr;
            if (fastq) { gzq = gzopen(opt.out.c_str(), "wb4"); if (!gzq) throw std::runtime_error("cannot create " + opt.out); }
            else outp.reset(new BgzfWriter(opt.out, pool));
            if (outp && use_gpu_deflate) outp->set_deflate_backend(&gpu_deflater);
            std::unique_ptr<BgzfWriter> failp;                      // --fail-reads: FAIL.bam under the main output's header, FAIL.bam.pbi beside it
            if (fail_reads) failp.reset(new BgzfWriter(opt.fail_reads, pool));
            if (failp && use_gpu_deflate) failp->set_deflate_backend(&gpu_deflater);
            PbiIndex fpbi; std::vector<uint64_t> fmarks;
            std::string fq;
            bool header_done = false;
            std::map<int64_t, std::shared_ptr<Batch>> hold;
            int64_t next = 0;
            RecordBuilder rb;
            PbiIndex pbi; std::vector<uint64_t> marks;             // OUT.bam.pbi: one entry per HiFi record
            std::vector<uint8_t> kin_rev;
            std::vector<uint32_t> sa_rle;
            std::shared_ptr<Batch> b;
            double last_progress = -1e30;
            std::string metrics = "{\n  \"zmws\": [\n";
            bool first_metric = true;
            const bool want_metrics = !opt.suppress_reports || opt.metrics_named;
            gzFile gzm = want_metrics ? gzopen(opt.metrics.c_str(), "wb") : nullptr;
            auto flush_metrics = [&](bool force) {
                if (gzm && (force || metrics.size() > (1u << 20))) { gzwrite(gzm, metrics.data(), (unsigned)metrics.size()); metrics.clear(); }
            };
            static const uint8_t qvbin[94] = {3,3,3,3,3,3,3, 10,10,10,10,10,10,10, 17,17,17,17,17,17, 22,22,22,22,22, 27,27,27,27,27,
                                              35,35,35,35,35,35,35,35,35,35, 40,40,40,40,40,40,40,40,40,40,40,40,40,40,40,40,40,40,40,40,40,40,40,40,40,40,40,40,40,40,
                                              40,40,40,40,40,40,40,40,40,40,40,40,40,40,40,40,40,40,40,40,40,40,40,40};
            static const char *const kStrandRG[2] = {"ccsamd02", "ccsamd03"};   // --heteroduplexes split: the read groups of the /fwd and the /rev reads
            // a CCS record of ZMW slot s as the main output writes it (tags the run asks for); the caller adds its own and finishes it.  to >= 0: the record of
            // the slice [from, to) of SEQ (--segment-adapters, --cdna-primers), named after it: SEQ, QUAL and every per-base tag are the slice, the scalar tags the read's
            auto build = [&](const ZmwIn &z, Batch &bt, int s, int32_t from = 0, int32_t to = -1) {
                const int64_t o = bt.seq_off[s] + from; const int32_t len = (to >= 0 ? to : bt.seq_len[s]) - from;
                const std::string qname = movie + "/" + std::to_string(z.zm) + "/ccs" + (z.strand_tag == 1 ? "/fwd" : (z.strand_tag == 2 ? "/rev" : "")) +
                                          (to >= 0 ? "/" + std::to_string(from) + "_" + std::to_string(to) : "");
                rb.begin(qname, bt.seq + o, bt.qual + o, (uint32_t)len);
                rb.tagZ("RG", hd_split && z.strand_tag ? kStrandRG[z.strand_tag - 1] : "ccsamd01");   // (--heteroduplexes split: a single-strand read names its strand's group)
                rb.tagf("ec", bt.ec[s]);
                rb.tagi("np", bt.np[s]);
                rb.tagf("rq", bt.rq[s]);
                rb.tagBf("sn", z.snr, 4);
                rb.tagi("zm", z.zm);
                if (opt.o.hifi_kinetics) {                      // docs/faq/kinetics.md:8-18, tag table docs/faq/bam-output.md:13-23
                    const size_t cap = (size_t)bt.cap;
                    const uint8_t *fi = bt.kin + o, *fp = fi + cap, *ri = fp + cap, *rp = ri + cap;
                    const uint32_t nf = bt.fn[s] > 0 ? (uint32_t)len : 0, nr = bt.rn[s] > 0 ? (uint32_t)len : 0;   // a strand without passes: empty lists
                    if (z.strand_tag) {                         // single-strand record: its own strand is the forward pair
                        rb.tagBC("ip", fi, nf); rb.tagBC("pw", fp, nf);
                    } else {
                        rb.tagBC("fi", fi, nf); rb.tagBC("fp", fp, nf); rb.tagi("fn", bt.fn[s]);
                        kin_rev.assign(ri, ri + nr); std::reverse(kin_rev.begin(), kin_rev.end());   // reverse strand: its own orientation (a slice: taken in SEQ coordinates first)
                        rb.tagBC("ri", kin_rev.data(), nr);
                        kin_rev.assign(rp, rp + nr); std::reverse(kin_rev.begin(), kin_rev.end());
                        rb.tagBC("rp", kin_rev.data(), nr); rb.tagi("rn", bt.rn[s]);
                    }
                }
                if (opt.pileup) {                               // docs/faq/bam-output.md:25-27; the rule: DESIGN.md §2 "Pileup summary"
                    const size_t cap = (size_t)bt.cap;
                    const uint8_t *cov = bt.pile + o;
                    sa_rle.clear();
                    for (int32_t q = 0; q < len;) {             // sa: <length>,<coverage>,... runs of equal coverage
                        int32_t e = q + 1;
                        while (e < len && cov[e] == cov[q]) ++e;
                        sa_rle.push_back((uint32_t)(e - q)); sa_rle.push_back(cov[q]);
                        q = e;
                    }
                    rb.tagBI("sa", sa_rle.data(), (uint32_t)sa_rle.size());
                    rb.tagBC("sm", cov + cap, (uint32_t)len);
                    rb.tagBC("sx", cov + 2 * cap, (uint32_t)len);
                }
            };
            auto put_fastq = [&](const std::string &qname, const Batch &bt, int64_t o, int32_t len) {
                fq.clear(); fq += '@'; fq += qname; fq += '\n';
                for (int32_t q = 0; q < len; ++q) fq += "ACGT"[bt.seq[o + q] & 3];
                fq += "\n+\n";
                for (int32_t q = 0; q < len; ++q) fq += (char)(33 + (bt.qual[o + q] > 93 ? 93 : bt.qual[o + q]));
                fq += '\n';
                if (gzwrite(gzq, fq.data(), (unsigned)fq.size()) != (int)fq.size()) throw std::runtime_error("short write (fastq.gz)");
            };
            // --reads-bam: the record of a ZMW that was not polished, its draft or one of its subreads as k_represent left it in the result planes (rq -1, no ec;
            // the subread's own ipd / pw as fi / fp with --reads-bam-kinetics: "as forward orientation", docs/faq/mode-all.md:24)
            auto put_representative = [&](const ZmwIn &z, Batch &bt, int s, bool subread) {
                const int64_t o = bt.seq_off[s]; const int32_t len = bt.seq_len[s];
                const std::string qname = movie + "/" + std::to_string(z.zm) + "/ccs";
                if (fastq) { put_fastq(qname, bt, o, len); return; }
                rb.begin(qname, bt.seq + o, bt.qual + o, (uint32_t)len);
                rb.tagi("zm", z.zm);
                rb.tagZ("RG", "ccsamd01");
                rb.tagBf("sn", z.snr, 4);
                rb.tagi("np", bt.np[s]);
                rb.tagf("rq", bt.rq[s]);
                if (opt.reads_kinetics && subread) {
                    rb.tagBC("fi", bt.kin + o, (uint32_t)len); rb.tagBC("fp", bt.kin + (size_t)bt.cap + o, (uint32_t)len);
                    rb.tagi("fn", 1); rb.tagi("rn", 0);
                }
                marks.push_back(outp->mark());
                pbi.rg_id.push_back(0); pbi.q_start.push_back(0); pbi.q_end.push_back(len); pbi.hole.push_back(z.zm);
                pbi.read_qual.push_back(bt.rq[s]); pbi.ctxt.push_back(0);
                rb.finish(*outp);
            };
            std::function<void(const ZmwIn &, Batch &, int, std::string *)> emit_one;
            auto emit = [&](Batch &bt) {
                if (!header_done) {
                    // --heteroduplexes split: three read groups (mode-heteroduplex-filtering.md:44-51): today's serves the double-strand reads, one each the
                    // /fwd and the /rev reads, with the kinetics keys their records use
                    std::string strand_rg;
                    for (int k = 0; hd_split && k < 2; ++k)
                        strand_rg += std::string("@RG\tID:") + kStrandRG[k] + "\tPL:PACBIO\tDS:READTYPE=CCS;STRAND=" + (k ? "REVERSE" : "FORWARD") +
                                     (opt.o.hifi_kinetics ? ";Ipd:CodecV1=ip;PulseWidth:CodecV1=pw" : "") + "\tPU:" + movie + "\tPM:SEQUELII\n";
                    const std::string text = "@HD\tVN:1.6\tSO:unknown\tpb:5.0.0\n@RG\tID:ccsamd01\tPL:PACBIO\tDS:READTYPE=CCS" +
                                             std::string(opt.o.hifi_kinetics && opt.by_strand ? ";Ipd:CodecV1=ip;PulseWidth:CodecV1=pw" : "") + "\tPU:" + movie +
                                             "\tPM:SEQUELII\n" + strand_rg + "@PG\tID:ccs\tPN:ccs\tVN:amd-mi355x-r1\tDS:Generate circular consensus sequences (ccs) from subreads.\n";
                    if (!fastq) write_header(*outp, text);
                    if (failp) write_header(*failp, text);
                }
                header_done = true;
                for (size_t i = 0; i < bt.zmws.size(); ++i) {
                    ++rep.input;
                    const ZmwIn &z = bt.zmws[i];
                    const int s = bt.slot[i];
                    // --heteroduplexes split: a ZMW the split took is written as its single-strand entities, /fwd before /rev, at the ZMW's place; each is a read
                    // of the single-strand column and an entry of the ZMW's "_strands" in the metrics file
                    std::string strands;
                    if (hd_split && s >= 0 && bt.have_results && z.host_status == HS_OK && bt.status[s] == CCSX_HETERODUPLEX) {
                        ++rep.hd_zmws;
                        for (int k = 0; k < 2 && bt.strand; ++k) {
                            const int ks = bt.strand_slot[2 * s + k];
                            if (ks < 0) continue;
                            ZmwIn sz;
                            sz.zm = z.zm; sz.strand_tag = k + 1; std::memcpy(sz.snr, z.snr, 16);
                            emit_one(sz, *bt.strand, ks, &strands);
                        }
                        strands = "[" + strands + "]";
                    }
                    emit_one(z, bt, s, strands.empty() ? nullptr : &strands);
                }
            };
            // One entity through the writer: ZMW `z` of batch bt at SoA slot s (s < 0: it failed on the host), or — z.strand_tag set under --heteroduplexes split —
            // one strand of a split ZMW, bt being the single-strand batch.  strands: of a split ZMW the JSON list of its strands (the ZMW itself writes its
            // metrics entry and nothing else), of a strand the list to append its entry to
            emit_one = [&](const ZmwIn &z, Batch &bt, int s, std::string *strands) {
                {                                                                  // (a block, so that the body stays where it stood as the body of emit's loop)
                    const bool ss = hd_split && z.strand_tag != 0;
                    int st = z.host_status;
                    if (st == HS_OK) st = bt.have_results ? bt.status[s] : -1;      // -1: EXCEPTION_THROWN / "Unknown error" (engine failure)
                    const int engine_st = st;
                    const bool split_zmw = !ss && strands != nullptr;              // its strands have been written: the metrics entry remains
                    // --fail-reads: a palindrome with a consensus is a failure of its own (DESIGN.md §2 "Adapter palindromes")
                    if (fail_reads && s >= 0 && bt.have_results && bt.fold[s] == CCSX_FOLD_PALINDROME && (st == CCSX_SUCCESS || st == CCSX_LOW_RQ))
                        st = HS_ADAPTER_PALINDROME;
                    // --adapters: a tested ZMW with a consensus and a verdict of the screen fails too; counted under the first that holds of palindrome,
                    // concatenation, near end (DESIGN.md §2 "Adapter screen")
                    const int abits = (screen && s >= 0 && bt.have_results && bt.arep.tested[s] && (engine_st == CCSX_SUCCESS || engine_st == CCSX_LOW_RQ)) ? bt.arep.verdict[s] : 0;
                    if (abits && st != HS_ADAPTER_PALINDROME) st = (abits & CCSX_ADAPTER_CONCAT) ? HS_ADAPTER_CONCAT : HS_ADAPTER_NEAR_END;
                    // --control: a ZMW the screen found is a control molecule whatever became of it afterwards, and is counted as one before any adapter class
                    // (DESIGN.md §2 "Control screen")
                    const bool pal = st == HS_ADAPTER_PALINDROME;
                    const bool ctl = control && s >= 0 && bt.have_results && bt.crep.verdict[s] == CCSX_CONTROL_FOUND;
                    if (ctl && !split_zmw) { st = engine_st == CCSX_SUCCESS ? HS_CONTROL_SUCCESS : HS_CONTROL_FAILURE; rep.control += ss ? 0 : 1; }
                    const bool tandem = opt.min_tandem > 0 && s >= 0 && bt.have_results && bt.tlen[s] >= opt.min_tandem;
                    if (!split_zmw) (ss ? rep.ss_tandem : rep.tandem) += tandem ? 1 : 0;
                    if (ss) {                                                      // a strand's entry in its ZMW's "_strands" (fields with a leading _ are implementation details: reports-aux-files.md:173)
                        char line[256];
                        const bool have = bt.have_results && bt.seq_len[s] > 0;
                        std::snprintf(line, sizeof(line), "%s{\"strand\": \"%s\", \"status\": \"%s\", \"predicted_accuracy\": %.6f, \"insert_size\": %d}",
                                      strands->empty() ? "" : ", ", z.strand_tag == 1 ? "fwd" : "rev", status_name(st, coverage), have ? bt.rq[s] : -1.0f, have ? bt.seq_len[s] : 0);
                        *strands += line;
                        ++rep.ss_input;
                    } else
                    if (want_metrics) {
                        const bool have = (s >= 0 && bt.have_results);
                        const int32_t isz = (have && bt.seq_len[s] > 0) ? bt.seq_len[s] : z.median_len;
                        char line[512];
                        std::snprintf(line, sizeof(line), "%s    {\"effective_coverage\": %.2f, \"has_tandem_repeat\": %s, \"insert_size\": %d, \"num_full_passes\": %d, "
                                      "\"polymerase_length\": %" PRId64 ", \"predicted_accuracy\": %.6f, \"status\": \"%s\", \"zmw\": \"%s/%d%s\"}",
                                      first_metric ? "" : ",\n", have ? bt.ec[s] : 0.0f, tandem ? "true" : "false", isz, have ? bt.np[s] : z.n_full, z.polymerase_len,
                                      (have && bt.seq_len[s] > 0) ? bt.rq[s] : -1.0f, status_name(st, coverage), movie.c_str(), z.zm,
                                      z.strand_tag == 1 ? "/fwd" : (z.strand_tag == 2 ? "/rev" : ""));
                        metrics += line; first_metric = false;
                        if (split_zmw) { metrics.pop_back(); metrics += ", \"_strands\": " + *strands + "}"; }
                        flush_metrics(false);
                    }
                    const int64_t o = s >= 0 ? bt.seq_off[s] : 0; const int32_t len = (s >= 0 && bt.have_results) ? bt.seq_len[s] : 0;
                    const int rcls = (opt.reads_bam && s >= 0 && bt.have_results) ? bt.rrep.cls[s] : CCSX_REPRESENT_NONE;
                    if (opt.reads_bam && s >= 0 && bt.have_results) ++rep.rep_cls[rcls & 3];
                    if (split_zmw) return;
                    if (st != CCSX_SUCCESS) {
                        if (st == CCSX_HETERODUPLEX) ++rep.hd_zmws;                 // (--heteroduplexes drop: no read; with --fail-reads the 0x8 rule below)
                        (ss ? rep.ss_fail : rep.fail)[fail_label(st, coverage)]++;
                        if ((rcls == CCSX_REPRESENT_DRAFT || rcls == CCSX_REPRESENT_SUBREAD) && len > 0) put_representative(z, bt, s, rcls == CCSX_REPRESENT_SUBREAD);
                        if (st >= CCSX_DRAFT_TOO_DIFFERENT && st <= CCSX_READS_FAILED_POLISHING) ++rep.coverage;
                        if (!fail_reads) return;
                        if ((engine_st == CCSX_LOW_RQ || pal || abits || ctl) && len > 0) {     // a consensus: as the main writer builds it, plus ff
                            if (opt.qv_binning) for (int32_t q = 0; q < len; ++q) { uint8_t &v = bt.qual[o + q]; v = qvbin[v > 93 ? 93 : v]; }
                            build(z, bt, s);
                            rb.tagi("ff", (engine_st == CCSX_LOW_RQ ? 0x1 : 0) | (ctl ? 0x2 : 0) | (ss ? 0x4 : 0) | (pal ? 0x20 : 0) | ((abits & CCSX_ADAPTER_CONCAT) ? 0x10 : 0) |
                                              ((abits & CCSX_ADAPTER_NEAR_END) ? 0x40 : 0));
                            fmarks.push_back(failp->mark());
                            fpbi.rg_id.push_back(ss ? z.strand_tag : 0); fpbi.q_start.push_back(0); fpbi.q_end.push_back(len); fpbi.hole.push_back(z.zm);
                            fpbi.read_qual.push_back(bt.rq[s]); fpbi.ctxt.push_back(0);
                            rb.finish(*failp); ++rep.fail_records;
                        } else if (!ss && !z.fl_seq.empty()) {      // no consensus, at least one full pass: the median full-length subread (a strand without a consensus writes nothing)
                            rep.fail["ZMW with full-length subread"]++;
                            const int32_t n = (int32_t)z.fl_seq.size();
                            rb.begin(z.fl_name, z.fl_seq.data(), nullptr, (uint32_t)n);
                            rb.tagZ("RG", "ccsamd01");
                            rb.tagi("np", z.n_full);
                            rb.tagf("rq", -1.0f);
                            rb.tagBf("sn", z.snr, 4);
                            rb.tagi("zm", z.zm);
                            rb.tagi("ff", 0x8);
                            fmarks.push_back(failp->mark());
                            fpbi.rg_id.push_back(0); fpbi.q_start.push_back(0); fpbi.q_end.push_back(n); fpbi.hole.push_back(z.zm);
                            fpbi.read_qual.push_back(-1.0f); fpbi.ctxt.push_back(0);
                            rb.finish(*failp); ++rep.fail_records;
                        }
                        return;
                    }
                    ++(ss ? rep.ss_pass : rep.pass);
                    if (opt.qv_binning) for (int32_t q = 0; q < len; ++q) { uint8_t &v = bt.qual[o + q]; v = qvbin[v > 93 ? 93 : v]; }   // after rq (qv-binning.md:19-21)
                    // "Base quality >=Q30 (bp)" is a statement about the HiFi yield (docs/faq/reports-aux-files.md:66: 62,526 of the 63,881 HiFi bases while <Q20 reads
                    // are present): only reads with rq >= 0.99 count, and the percentage is taken over their bases
                    if (ss && fail_reads) {                         // fail class 0x4 "Single-stranded CCS reads" (fail-reads.md): to FAIL.bam, not to OUT, not in the HiFi statistics
                        build(z, bt, s);
                        rb.tagi("ff", 0x4);
                        fmarks.push_back(failp->mark());
                        fpbi.rg_id.push_back(z.strand_tag); fpbi.q_start.push_back(0); fpbi.q_end.push_back(len); fpbi.hole.push_back(z.zm);
                        fpbi.read_qual.push_back(bt.rq[s]); fpbi.ctxt.push_back(0);
                        rb.finish(*failp); ++rep.fail_records;
                        return;
                    }
                    if (segments) {                                 // --segment-adapters: one record per segment in place of the read's (DESIGN.md §2 "Segment rule")
                        const ccsx_segment_report &g = bt.srep;
                        const int ns = g.tested[s] ? g.n_segments[s] : 0;
                        rep.sg_tested += g.tested[s] ? 1 : 0; rep.sg_complete += g.complete[s]; rep.sg_leftover += g.leftover_bases[s];
                        ++(g.overflow[s] ? rep.sg_overflow : ns ? rep.sg_with : rep.sg_without);
                        ++rep.sg_classes[{ns, g.orient[s], g.complete[s]}];
                        for (int k = 0; k < ns; ++k) {
                            const ccsx_segment_piece &p = g.pieces[(size_t)s * CCSX_SEGMENT_MAX_PIECES + k];
                            const int32_t plen = p.end - p.start;
                            if (bt.rq[s] >= 0.99f) for (int32_t q = p.start; q < p.end; ++q) rep.bases_q30 += bt.qual[o + q] >= 30 ? 1 : 0;
                            if (fastq) put_fastq(movie + "/" + std::to_string(z.zm) + "/ccs/" + std::to_string(p.start) + "_" + std::to_string(p.end), bt, o + p.start, plen);
                            else {
                                build(z, bt, s, p.start, p.end);
                                // (di, dl, dr: the tag names are recalled from the vendor's segmentation tool, which is not in the reference mount, as bam_io.h
                                // says of the .pbi layout; dl / dr: the adapters' numbers in the FASTA, as read left to right)
                                rb.tagi("di", p.index); rb.tagi("dl", p.index + (p.reverse ? 1 : 0)); rb.tagi("dr", p.index + (p.reverse ? 0 : 1));
                                marks.push_back(outp->mark());
                                pbi.rg_id.push_back(0); pbi.q_start.push_back(p.start); pbi.q_end.push_back(p.end); pbi.hole.push_back(z.zm);
                                pbi.read_qual.push_back(bt.rq[s]); pbi.ctxt.push_back(0);
                                rb.finish(*outp);
                            }
                            rep.lens.push_back(plen); rep.rqs.push_back(bt.rq[s]); rep.nps.push_back(bt.np[s]); rep.ss.push_back(ss); rep.holes.push_back(z.zm);
                            ++rep.sg_written;
                        }
                        return;
                    }
                    if (cdna) {                                     // --cdna-primers: the full-length read's slice in place of the read (DESIGN.md §2 "cDNA rule")
                        const ccsx_cdna_report &d = bt.drep;
                        rep.cd_tested += d.tested[s] ? 1 : 0; ++rep.cd_cls[d.cls[s]]; ++rep.cd_classes[{d.cls[s], d.strand[s]}];
                        if (d.cls[s] != CCSX_CDNA_FULL_LENGTH) return;
                        const int32_t from = d.start[s], to = d.end[s], plen = to - from;
                        if (bt.rq[s] >= 0.99f) for (int32_t q = from; q < to; ++q) rep.bases_q30 += bt.qual[o + q] >= 30 ? 1 : 0;
                        if (fastq) put_fastq(movie + "/" + std::to_string(z.zm) + "/ccs/" + std::to_string(from) + "_" + std::to_string(to), bt, o + from, plen);
                        else {
                            build(z, bt, s, from, to);
                            // (ts, pa, pr, pq: the tag names are this build's own.  pr: the 5' and the 3' primer's numbers in the FASTA; pq: the barcode rule's bq
                            // over the two ends, the smaller of floor(100 * (m - dist) / m))
                            const int st = d.strand[s];
                            const uint8_t pr[2] = {(uint8_t)d.idx[2 * s + st], (uint8_t)d.idx[2 * s + 1 - st]};
                            int pq = 100;
                            for (int e = 0; e < 2; ++e) { const int m = opt.cdna_set->len[d.idx[2 * s + e]]; pq = std::min(pq, 100 * (m - d.dist[2 * s + e]) / m); }
                            rb.tagA("ts", st ? '-' : '+'); rb.tagi("pa", d.polya_len[s]); rb.tagBC("pr", pr, 2); rb.tagi("pq", pq);
                            marks.push_back(outp->mark());
                            pbi.rg_id.push_back(0); pbi.q_start.push_back(from); pbi.q_end.push_back(to); pbi.hole.push_back(z.zm);
                            pbi.read_qual.push_back(bt.rq[s]); pbi.ctxt.push_back(0);
                            rb.finish(*outp);
                        }
                        rep.lens.push_back(plen); rep.rqs.push_back(bt.rq[s]); rep.nps.push_back(bt.np[s]); rep.ss.push_back(ss); rep.holes.push_back(z.zm);
                        return;
                    }
                    if (bt.rq[s] >= 0.99f) for (int32_t q = 0; q < len; ++q) rep.bases_q30 += bt.qual[o + q] >= 30 ? 1 : 0;
                    const std::string qname = movie + "/" + std::to_string(z.zm) + "/ccs" + (z.strand_tag == 1 ? "/fwd" : (z.strand_tag == 2 ? "/rev" : ""));
                    const bool bc_both = barcodes && bt.brep.tested[s] && bt.brep.call[s] == 3;   // --barcodes: counted over the HiFi reads, tagged at both ends called
                    if (barcodes && bt.brep.tested[s]) {
                        ++rep.bc_tested; ++rep.bc_call[bt.brep.call[s] & 3];
                        if (bc_both) ++rep.bc_pairs[{bt.brep.idx[2 * s], bt.brep.idx[2 * s + 1]}];
                    }
                    if (fastq) {
                        put_fastq(qname, bt, o, len);
                        rep.lens.push_back(len); rep.rqs.push_back(bt.rq[s]); rep.nps.push_back(bt.np[s]); rep.ss.push_back(ss); rep.holes.push_back(z.zm);
                        return;
                    }
                    build(z, bt, s);
                    if (bc_both) {
                        const uint16_t pair[2] = {(uint16_t)bt.brep.idx[2 * s], (uint16_t)bt.brep.idx[2 * s + 1]};
                        rb.tagBS("bc", pair, 2);
                        rb.tagi("bq", bt.brep.bq[s]);
                    }
                    marks.push_back(outp->mark());
                    pbi.rg_id.push_back(ss ? z.strand_tag : 0); pbi.q_start.push_back(0); pbi.q_end.push_back(len); pbi.hole.push_back(z.zm);
                    pbi.read_qual.push_back(bt.rq[s]); pbi.ctxt.push_back(0);
                    rb.finish(*outp);
                    rep.lens.push_back(len); rep.rqs.push_back(bt.rq[s]); rep.nps.push_back(bt.np[s]); rep.ss.push_back(ss); rep.holes.push_back(z.zm);
                }
            };
            while (to_writer.pop(b)) {
                hold[b->index] = b;
                while (!hold.empty() && hold.begin()->first == next) {
                    emit(*hold.begin()->second);
                    out_pools[hold.begin()->second->dev]->put(std::move(hold.begin()->second->out_arena));
                    if (hold.begin()->second->strand) out_pools[hold.begin()->second->dev]->put(std::move(hold.begin()->second->strand->out_arena));
                    hold.erase(hold.begin()); ++next;
                }
                const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
                if (opt.log_level >= 2 && el - last_progress >= opt.refresh_rate) {     // --refresh-rate (docs/faq/reports-aux-files.md:176-177)
                    last_progress = el;
                    if (total_zmws > 0 && rep.input > 0)               // with an index the number of ZMWs ahead is known: ETA (reports-aux-files.md:183-192)
                        std::fprintf(stderr, "%" PRId64 "/%.1f %" PRId64 "/%.1f ETA %.0f s\n", rep.input, rep.input / el * 60, rep.pass, rep.pass / el * 60,
                                     el * (double)(total_zmws - rep.input) / (double)rep.input);
                    else
                    std::fprintf(stderr, "%" PRId64 "/%.1f %" PRId64 "/%.1f\n", rep.input, rep.input / el * 60, rep.pass, rep.pass / el * 60);
                }
            }
            for (auto &kv : hold) emit(*kv.second);
            if (fastq) { if (gzclose(gzq) != Z_OK) throw std::runtime_error("short write (fastq.gz)"); }
            else {
                if (!header_done) write_header(*outp, "@HD\tVN:1.6\tSO:unknown\tpb:5.0.0\n@RG\tID:ccsamd01\tPL:PACBIO\tDS:READTYPE=CCS\tPU:unknown\n");
                outp->close();
                for (uint64_t m : marks) pbi.file_offset.push_back((int64_t)outp->virtual_offset(m));
                write_pbi(opt.out + ".pbi", pool, pbi);
            }
            if (failp) {
                if (!header_done) write_header(*failp, "@HD\tVN:1.6\tSO:unknown\tpb:5.0.0\n@RG\tID:ccsamd01\tPL:PACBIO\tDS:READTYPE=CCS\tPU:unknown\n");
                failp->close();
                for (uint64_t m : fmarks) fpbi.file_offset.push_back((int64_t)failp->virtual_offset(m));
                write_pbi(opt.fail_reads + ".pbi", pool, fpbi);
            }
            if (gzm) {
                metrics += "\n  ]";
                if (opt.reads_bam) metrics += ",\n  \"representative_reads\": {\"polished\": " + std::to_string(rep.rep_cls[CCSX_REPRESENT_POLISHED]) + ", \"draft\": " +
                                              std::to_string(rep.rep_cls[CCSX_REPRESENT_DRAFT]) + ", \"subread\": " + std::to_string(rep.rep_cls[CCSX_REPRESENT_SUBREAD]) + "}";
                metrics += "\n}\n"; flush_metrics(true); gzclose(gzm);
            }
            } catch (const std::exception &e) {
                fail(std::string("writing ") + opt.out + ": " + e.what());
                std::shared_ptr<Batch> drop;
                while (to_writer.pop(drop)) {}                   // keep the workers from blocking on a full queue
            }
        });

        reader.join();
        for (auto &w : packers) w.join();
        for (auto &w : workers) w.join();
        to_writer.close();
        writer.join();
        for (ccsx_handle h : handles) ccsx_destroy(h);
        if (!opt.suppress_reports || opt.report_named) write_report(opt, rep);
        if (!opt.report_json.empty()) write_report_json(opt, rep);            // named files are written even under --suppress-reports (docs/faq/sqiie.md:36-46
        if (!opt.barcode_counts.empty()) write_barcode_counts(opt, rep);
        if (!opt.segment_counts.empty()) write_segment_counts(opt, rep);
        if (!opt.cdna_counts.empty()) write_cdna_counts(opt, rep);
        if (!opt.hifi_summary.empty()) write_hifi_summary(opt, rep);          //  combines --suppress-reports with explicit report names)
        const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
        if (opt.log_level >= 2)
            std::fprintf(stderr, "ccs: reader thread: framing/inflate %.2f s, waiting for record decode %.2f s, grouping+filters+queue %.2f s\n",
                         rd_us[0] * 1e-6, rd_us[1] * 1e-6, rd_us[2] * 1e-6);
        if (opt.log_level >= 2)
            std::fprintf(stderr, "ccs: GPU workers (sum over %zu): waiting for input %.2f s, packing (pack threads) %.2f s, submit + wait %.2f s\n", handles.size(),
                         us_wait.load() * 1e-6, us_pack.load() * 1e-6, us_engine.load() * 1e-6);
        if (opt.log_level >= 2 && eng.tickets > 0 && handles.size() == 1) {
            const double k = 1000.0 / (double)std::max<long long>(eng.zmws, 1);
            std::fprintf(stderr, "ccs: engine (ticket timings, %lld tickets, %lld ZMWs): first kernel to last %.1f ms = %.2f ms per 1000 ZMWs; per 1000 ZMWs on the device: "
                                 "draft + align %.2f ms, polish %.2f ms, between the stages %.2f ms, ticket start to end %.2f ms\n",
                         eng.tickets, eng.zmws, eng.last - eng.first, (eng.last - eng.first) * k, eng.draft * k, eng.polish * k, eng.queue * k, eng.total * k);
        }
        if (opt.log_level >= 2 && eng_ss.tickets > 0 && handles.size() == 1) {
            const double k = 1000.0 / (double)std::max<long long>(eng_ss.zmws, 1);
            std::fprintf(stderr, "ccs: engine (single-strand tickets, %lld tickets, %lld strands): on the device %.1f ms in all; per 1000 strands: draft + align %.2f ms, polish %.2f ms, "
                                 "between the stages %.2f ms, ticket start to end %.2f ms\n",
                         eng_ss.tickets, eng_ss.zmws, eng_ss.total, eng_ss.draft * k, eng_ss.polish * k, eng_ss.queue * k, eng_ss.total * k);
        }
        if (opt.log_level >= 2 && hd_split) {                    // the DS / SS summary of mode-heteroduplex-filtering.md:72-82, over the reads of OUT
            // a ZMW is written when OUT holds a read of it; UMY: the bases of the longest read of every written ZMW; HiFi: reads of predicted accuracy >= Q20
            std::map<int32_t, std::pair<int32_t, int32_t>> longest[2];    // per ZMW: its longest read, its longest HiFi read; [0] DS, [1] SS
            int64_t reads[2] = {0, 0}, hifi_bases = 0;
            double q_sum = 0;
            for (size_t i = 0; i < rep.lens.size(); ++i) {
                auto &e = longest[rep.ss[i]][rep.holes[i]];
                e.first = std::max(e.first, rep.lens[i]);
                if (rep.rqs[i] >= 0.99f) { e.second = std::max(e.second, rep.lens[i]); ++reads[rep.ss[i]]; hifi_bases += rep.lens[i]; q_sum += rq_to_q(rep.rqs[i]); }
            }
            int64_t umy[2] = {0, 0}, hy[2] = {0, 0};
            for (int c = 0; c < 2; ++c) for (const auto &kv : longest[c]) { umy[c] += kv.second.first; hy[c] += kv.second.second; }
            const int64_t nr = reads[0] + reads[1];
            std::fprintf(stderr, "ZMWs Input    : %" PRId64 "\nZMWs Written  : %zu\n - DS / SS    : %zu / %zu\nUMY           : %" PRId64 " bases\n - DS / SS    : %" PRId64 " / %" PRId64 "\n"
                                 "HiFi Yield    : %" PRId64 " bases\n - DS / SS    : %" PRId64 " / %" PRId64 "\nHiFi Reads    : %" PRId64 "\n - DS / SS    : %" PRId64 " / %" PRId64 "\n"
                                 "HiFi Avg Size : %" PRId64 " bases\nHiFi Avg QV   : %.1f\n",
                         rep.input, longest[0].size() + longest[1].size(), longest[0].size(), longest[1].size(), umy[0] + umy[1], umy[0], umy[1], hy[0] + hy[1], hy[0], hy[1],
                         nr, reads[0], reads[1], nr ? hifi_bases / nr : 0, nr ? q_sum / (double)nr : 0.0);
        }
        if (opt.log_level >= 2 && use_gpu_deflate)
            std::fprintf(stderr, "ccs: --gpu-deflate: %lld tickets, %lld blocks, %.1f MB in, %.1f MB out; writer thread: staging + submit %.2f s, waiting for tickets %.2f s\n",
                         gpu_deflater.n_tickets, gpu_deflater.n_blocks, gpu_deflater.n_in * 1e-6, gpu_deflater.n_out * 1e-6, gpu_deflater.us_submit * 1e-6,
                         gpu_deflater.us_wait * 1e-6);
        if (opt.log_level >= 1)
            std::fprintf(stderr, "ccs: %" PRId64 " ZMWs in, %" PRId64 " HiFi reads out, %.2f s (%.1f ZMWs/s, %d host threads, %zu GPU worker%s)%s%s%s%s%s%s\n", rep.input, rep.pass, el,
                         rep.input / el, nthreads, handles.size(), handles.size() == 1 ? "" : "s",
                         opt.min_tandem > 0 ? (", " + std::to_string(rep.tandem) + " ZMWs with tandem repeats").c_str() : "",
                         opt.fail_reads.empty() ? "" : (", " + std::to_string(rep.fail_records) + " fail reads").c_str(),
                         control ? (", " + std::to_string(rep.control) + " control ZMWs").c_str() : "",
                         coverage ? (", " + std::to_string(rep.coverage) + " ZMWs failed the coverage filters").c_str() : "",
                         opt.heteroduplexes ? (", " + std::to_string(rep.hd_zmws) + " heteroduplex ZMWs " + (hd_split ? "split" : "dropped")).c_str() : "",
                         opt.reads_bam ? (", representative reads: " + std::to_string(rep.rep_cls[CCSX_REPRESENT_POLISHED]) + " polished, " + std::to_string(rep.rep_cls[CCSX_REPRESENT_DRAFT]) +
                                          " drafts, " + std::to_string(rep.rep_cls[CCSX_REPRESENT_SUBREAD]) + " subreads").c_str() : "");
        if (opt.log_level >= 1 && opt.orient_passes)
            std::fprintf(stderr, "ccs: --orient-passes: %lld passes submitted strand-unknown\n", unknown_passes.load());
        if (failed) {
            if (!err_msg.empty()) std::fprintf(stderr, "ccs: %s\n", err_msg.c_str());
            // no plausible-looking partial output after a failed run
            std::remove(opt.out.c_str());
            std::remove((opt.out + ".pbi").c_str());
            if (!opt.fail_reads.empty()) { std::remove(opt.fail_reads.c_str()); std::remove((opt.fail_reads + ".pbi").c_str()); }
            std::fprintf(stderr, "ccs: run failed, %s removed\n", opt.out.c_str());
        }
        return failed ? 1 : 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "ccs: %s\n", e.what());
        return 1;
    }
}

// ccsx_internal.h — shared between the host and device translation units of libccsx.so
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>

#include "ccsx.h"

void ccsx_set_error(const std::string &s);

// a HIP call of an entry point: its failure is the entry point's, -2 with the call and HIP's text as the error
#define HIPTRY(expr)                                                                                           \
    do {                                                                                                       \
        hipError_t e_ = (expr);                                                                                \
        if (e_ != hipSuccess) {                                                                                \
            ccsx_set_error(std::string(#expr) + ": " + hipGetErrorString(e_));                                 \
            return -2;                                                                                         \
        }                                                                                                      \
    } while (0)

// capacity of the draft / consensus of a ZMW whose longest subread has maxL bases
static inline int64_t ccsx_draft_cap(int64_t maxL) { return maxL + maxL / 4 + 64; }
// POA vertex capacity for the same ZMW
static inline int64_t ccsx_vertex_cap(int64_t maxL) { return (5 * maxL) / 2 + 256; }

// The capacity layout: everything a ZMW is given follows from its longest pass.  wcap: the words of its window bounds, one more than its window slots (cores are
// 19..25 columns: SPEC windows).  The engine's slots (ccsx_api.cpp) and the layouts a caller sizes its buffers by (ccsx_result_layout, ccsx_draft_layout) are this
// one definition.
struct ccsx_zmw_caps { int64_t maxL, dcap, vcap, wcap; };
static inline ccsx_zmw_caps ccsx_caps_of(int64_t maxL)
{
    const int64_t dcap = ccsx_draft_cap(maxL);
    return {maxL, dcap, ccsx_vertex_cap(maxL), dcap / (CCSX_WIN_CORE - 3) + 4};
}
// f(z, caps of ZMW z) for every ZMW of a batch, in order
template <typename F> static inline void ccsx_for_each_zmw_caps(const ccsx_batch *b, F f)
{
    for (int z = 0; z < b->n_zmw; ++z) {
        int64_t maxL = 0;
        for (int r = b->read_off[z]; r < b->read_off[z + 1]; ++r) maxL = std::max<int64_t>(maxL, b->base_off[r + 1] - b->base_off[r]);
        f(z, ccsx_caps_of(maxL));
    }
}

// ---- the analyses on final reads: barcode calls (ccsx_barcode_api.cpp; DESIGN.md §2 "Barcode calls"), segmentation (ccsx_segment_api.cpp; "Segment rule") and
// full-length cDNA reads (ccsx_cdna_api.cpp; "cDNA rule").  What every entry point of one shares; a refusal sets the error under the exported function's name
// `fn` and returns -1.  The packed set, the binding of its buffer and the report's layout are in barcode_core.h / segment_core.h / cdna_core.h; the path all take
// through a handle is ccsx_api.cpp's (struct Barcodes, struct Segments, struct Cdna).
// the set, the options (NULL: the defaults; the checked copy goes to *o) and a report for n reads
int ccsx_barcode_check(const ccsx_barcode_set *set, const ccsx_barcode_opts *opts, const ccsx_barcode_report *report, int64_t n, const char *fn, ccsx_barcode_opts *o);
int ccsx_segment_check(const ccsx_segment_set *set, const ccsx_segment_opts *opts, const ccsx_segment_report *report, int64_t n, const char *fn, ccsx_segment_opts *o);
int ccsx_cdna_check(const ccsx_cdna_set *set, const ccsx_cdna_opts *opts, const ccsx_cdna_report *report, int64_t n, const char *fn, ccsx_cdna_opts *o);
// caller-supplied reads, of either analysis: *bytes = the bytes of seq the reads cover (the largest seq_off[z] + seq_len[z] over the reads with seq_len[z] > 0)
int ccsx_check_reads(const uint8_t *seq, const int64_t *seq_off, const int32_t *seq_len, int32_t n, const char *fn, int64_t *bytes);

// ---- duplicate reads (ccsx_dup_api.cpp; DESIGN.md §2 "Duplicate rule"): the checks the host and the device form of each call share.  The checked options go to
// *o (opts NULL: the defaults); *bytes as ccsx_check_reads.  The cluster check reads every signature's window and every group.  A refusal sets the error under `fn`
// and returns -1.
int ccsx_dup_check_sign(const ccsx_dup_opts *opts, const uint8_t *seq, const int64_t *seq_off, const int32_t *seq_len, int32_t n, const ccsx_dup_sig *sig,
                        const char *fn, ccsx_dup_opts *o, int64_t *bytes);
int ccsx_dup_check_cluster(const ccsx_dup_opts *opts, const ccsx_dup_sig *sig, const int32_t *group, int32_t n, const ccsx_dup_report *report, const char *fn,
                           ccsx_dup_opts *o);

// ---- cell barcodes and UMIs (ccsx_cell_api.cpp; DESIGN.md §2 "Cell-tag rule"): the one check of ccsx_cell_reads_host and ccsx_cell_reads: everything
// ccsx_cdna_check refuses, then the design, the whitelist against the design (wl NULL: none) and the report's own planes
int ccsx_cell_check(const ccsx_cdna_set *set, const ccsx_cdna_opts *opts, const ccsx_cell_design *design, const ccsx_cell_whitelist *wl,
                    const ccsx_cell_report *report, int64_t n, const char *fn, ccsx_cdna_opts *o);

// ---- representative reads (ccsx_represent_api.cpp; DESIGN.md §2 "Representative rule"): the request against the batch it is for and the options of the run — flags,
// reserved words, the report's arrays and size, kinetics without opts.hifi_kinetics or batch.ipd.  A refusal sets the error under `fn` and returns -1.
int ccsx_represent_check(const ccsx_represent_request *req, const ccsx_batch *b, const ccsx_opts *opts, const char *fn);

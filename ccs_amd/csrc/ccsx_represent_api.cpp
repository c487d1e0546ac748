// ccsx_represent_api.cpp — the host side of the representative reads that needs no device (DESIGN.md §2 "Representative rule"): the request's checks, which every
// entry point shares, and ccsx_represent_host, the rule on the calling thread (represent_core.h: the same class and the same order as the kernel's).  The entry
// points that take a handle are in ccsx_api.cpp.
#include <cstring>
#include <string>
#include <vector>

#include "ccsx.h"
#include "ccsx_internal.h"
#include "represent_core.h"

int ccsx_represent_rule_version(void) { return 1; }

int ccsx_represent_check(const ccsx_represent_request *req, const ccsx_batch *b, const ccsx_opts *opts, const char *fn)
{
    const std::string f(fn);
    if (!req) { ccsx_set_error(f + ": null represent request"); return -1; }
    if (!b || !opts) { ccsx_set_error(f + ": null argument"); return -1; }
    if (req->reserved[0] != 0 || req->reserved[1] != 0) { ccsx_set_error(f + ": represent request: reserved must be 0"); return -1; }
    if ((req->subread_fallback & ~1) || (req->kinetics & ~1)) { ccsx_set_error(f + ": represent request: subread_fallback and kinetics must be 0 or 1"); return -1; }
    if (!req->report) { ccsx_set_error(f + ": null represent report"); return -1; }
    if (req->report->n_zmw != b->n_zmw || !req->report->cls || !req->report->pass) {
        ccsx_set_error(f + ": represent report arrays missing, or sized for another batch"); return -1;
    }
    if (req->kinetics && !opts->hifi_kinetics) { ccsx_set_error(f + ": represent request: kinetics needs opts.hifi_kinetics"); return -1; }
    if (req->kinetics && !b->ipd) { ccsx_set_error(f + ": represent request: kinetics needs batch.ipd"); return -1; }
    return 0;
}

int ccsx_represent_host(const ccsx_batch *b, const ccsx_opts *opts, const int32_t *status, const uint8_t *draft_seq, const int64_t *draft_off,
                        const int32_t *draft_len, const ccsx_represent_request *req, ccsx_results *res)
{
    if (ccsx_represent_check(req, b, opts, __func__)) return -1;
    const std::string f(__func__);
    const int n = b->n_zmw;
    if (!res || (n > 0 && (!status || !draft_off || !draft_len))) { ccsx_set_error(f + ": null argument"); return -1; }
    if (res->n_zmw != n || !res->seq_off || !res->seq_len || !res->seq || !res->qual || !res->rq || !res->ec) {
        ccsx_set_error(f + ": results: missing arrays, or sized for another batch"); return -1;
    }
    if (n > 0 && (!b->read_off || !b->base_off || !b->flags || (b->n_bases > 0 && (!b->bases || !b->pw)))) { ccsx_set_error(f + ": batch: missing arrays"); return -1; }
    int bad = -1;                                                    // res->seq_off against the capacity layout: nothing is written outside a ZMW's slot
    int64_t at = 0;
    ccsx_for_each_zmw_caps(b, [&](int z, const ccsx_zmw_caps &c) {
        if (bad < 0 && (res->seq_off[z] != at || res->seq_off[z + 1] != at + c.dcap)) bad = z;
        at += c.dcap;
    });
    if (bad >= 0 || res->seq_capacity < at) { ccsx_set_error(f + ": results: seq_off is not the capacity layout of this batch (ccsx_result_layout)"); return -1; }
    for (int z = 0; z < n; ++z) {
        if (draft_len[z] > 0 && (!draft_seq || draft_off[z] < 0)) { ccsx_set_error(f + ": ZMW " + std::to_string(z) + ": a draft without bases"); return -1; }
    }
    ccsx_represent_report *rep = req->report;
    std::vector<int> len;
    for (int z = 0; z < n; ++z) {
        const int r0 = b->read_off[z], nall = ccsx_rp_nall(b->read_off[z + 1] - r0, opts->top_passes);
        const int64_t so = res->seq_off[z], slot = res->seq_off[z + 1] - so;
        const int cls = ccsx_rp_class(status[z], nall, draft_len[z], slot, req->subread_fallback);
        rep->cls[z] = cls; rep->pass[z] = -1;
        if (cls == CCSX_REPRESENT_POLISHED || cls == CCSX_REPRESENT_NONE) continue;
        const uint8_t *src;
        int L, pick = -1;
        if (cls == CCSX_REPRESENT_DRAFT) { src = draft_seq + draft_off[z]; L = draft_len[z]; }
        else {
            int nfull = 0, nc = 0;
            len.assign((size_t)nall, 0);
            for (int q = 0; q < nall; ++q) { nfull += (b->flags[r0 + q] & 2) ? 0 : 1; len[q] = (int)(b->base_off[r0 + q + 1] - b->base_off[r0 + q]); }
            for (int q = 0; q < nall; ++q) nc += ccsx_rp_member(b->flags[r0 + q], nfull);
            for (int i = 0; i < nall && pick < 0; ++i) {
                if (!ccsx_rp_member(b->flags[r0 + i], nfull)) continue;
                int rank = 0;
                for (int q = 0; q < nall; ++q) rank += ccsx_rp_member(b->flags[r0 + q], nfull) && ccsx_rp_before(len[q], q, len[i], i);
                if (rank == nc / 2) pick = i;
            }
            rep->pass[z] = pick;
            src = b->bases + b->base_off[r0 + pick]; L = len[pick];
        }
        for (int i = 0; i < L; ++i) { res->seq[so + i] = src[i] & 3; res->qual[so + i] = CCSX_REPRESENT_QV; }
        if (res->raw_qv) for (int i = 0; i < L; ++i) res->raw_qv[so + i] = (float)CCSX_REPRESENT_QV;
        if (req->kinetics && pick >= 0) {
            const int64_t bo = b->base_off[r0 + pick];
            if (res->fi && L > 0) std::memcpy(res->fi + so, b->ipd + bo, (size_t)L);
            if (res->fp && L > 0) std::memcpy(res->fp + so, b->pw + bo, (size_t)L);
        }
        res->seq_len[z] = L; res->rq[z] = -1.0f; res->ec[z] = 0.0f;
    }
    return 0;
}

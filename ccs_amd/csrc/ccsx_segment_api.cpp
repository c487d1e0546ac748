// ccsx_segment_api.cpp — the host side of the segmentation that needs no device (DESIGN.md §2 "Segment rule"): defaults, the argument checks every entry point
// shares, and ccsx_segment_reads_host, the rule on the calling thread (segment_core.h: the same walks, key, selection and
// classification as the kernel's).  The entry points that take a handle are in ccsx_api.cpp.
#include <algorithm>
#include <string>
#include <vector>

#include "ccsx.h"
#include "ccsx_internal.h"
#include "segment_core.h"

void ccsx_segment_opts_default(ccsx_segment_opts *o)
{
    if (!o) return;
    o->max_dist_pct = 15; o->min_len = 50;   // DESIGN.md §2 "Segment rule": min_len is the engine's own lower bound for a pass
}

int ccsx_segment_rule_version(void) { return 1; }
int ccsx_segment_chunk(void) { return CCSX_SEGMENT_CHUNK; }

int ccsx_segment_check(const ccsx_segment_set *set, const ccsx_segment_opts *opts, const ccsx_segment_report *report, int64_t n, const char *fn, ccsx_segment_opts *o)
{
    const std::string f(fn);
    if (!set) { ccsx_set_error(f + ": null segment set"); return -1; }
    if (!report) { ccsx_set_error(f + ": null segment report"); return -1; }
    if (opts) *o = *opts; else ccsx_segment_opts_default(o);
    if (o->max_dist_pct < 0 || o->max_dist_pct > 30 || o->min_len < 1 || o->min_len > 65535) {
        ccsx_set_error(f + ": segment options out of range (0 <= max_dist_pct <= 30; 1 <= min_len <= 65535)"); return -1;
    }
    if (set->n_adapters < 2 || set->n_adapters > CCSX_SEGMENT_MAX_ADAPTERS) { ccsx_set_error(f + ": n_adapters outside 2 .. 33"); return -1; }
    for (int a = 0; a < set->n_adapters; ++a) {
        if (set->len[a] < CCSX_SEGMENT_MIN_LEN || set->len[a] > CCSX_SEGMENT_MAX_LEN) {
            ccsx_set_error(f + ": adapter " + std::to_string(a) + ": length outside 8 .. 64"); return -1;
        }
        for (int i = 0; i < set->len[a]; ++i)
            if (set->seq[a][i] > 3) { ccsx_set_error(f + ": adapter " + std::to_string(a) + ": code above 3"); return -1; }
    }
    if (report->n_zmw != n || !report->tested || !report->overflow || !report->n_hits || !report->n_cuts || !report->n_segments || !report->complete ||
        !report->orient || !report->leftover_bases || !report->pieces) {
        ccsx_set_error(f + ": segment report arrays missing, or sized for another batch"); return -1;
    }
    return 0;
}

int ccsx_segment_reads_host(const ccsx_segment_set *set, const ccsx_segment_opts *opts, const uint8_t *seq, const int64_t *seq_off, const int32_t *seq_len,
                            int32_t n, ccsx_segment_report *report)
{
    ccsx_segment_opts o;
    int64_t bytes;
    if (ccsx_segment_check(set, opts, report, n, __func__, &o) || ccsx_check_reads(seq, seq_off, seq_len, n, __func__, &bytes)) return -1;
    const int A = set->n_adapters, S = 2 * A;
    std::vector<unsigned long long> packed(ccsx_sg_set_words(A), 0ull);
    ccsx_sg_pack(set, packed.data());
    SegmentParams G{};
    G.n_adapters = A;
    ccsx_sg_bind(G, packed.data());
    const SegmentOut out = ccsx_sg_out(*report);
    std::vector<unsigned long long> keys;
    for (int z = 0; z < n; ++z) {
        const int L = seq_len[z];
        ccsx_segment_piece *list = out.pieces + (size_t)z * CCSX_SEGMENT_MAX_PIECES;
        for (int i = 0; i < CCSX_SEGMENT_MAX_PIECES; ++i) ccsx_sg_zero_piece(list[i]);
        if (L <= 0) { ccsx_sg_put_empty(out, (size_t)z, 0, 0, 0); continue; }
        const uint8_t *c = seq + seq_off[z];
        const auto base = [&](int j) { return (int)(c[j] & 3); };
        int n_hits = 0;
        keys.clear();
        for (int s = 0; s < S; ++s) {
            const unsigned long long *w = &G.masks[(size_t)s * CCSX_SG_MASK_WORDS];
            const int m = G.len[s];
            ccsx_sg_walk(w[0], w[1], w[2], w[3], m, ccsx_sg_k(m, o.max_dist_pct), L, 0, L, base, [&](int end, int dist) {
                if (n_hits++ < CCSX_SEGMENT_MAX_HITS) keys.push_back(ccsx_sg_key(dist, ccsx_sg_start([&](int b) { return w[4 + b]; }, m, dist, end, base), s, end));
            });
        }
        if (n_hits > CCSX_SEGMENT_MAX_HITS) { ccsx_sg_put_empty(out, (size_t)z, 1, 1, n_hits); continue; }
        std::sort(keys.begin(), keys.end());
        SegmentHit cuts[CCSX_SEGMENT_MAX_HITS];
        const int nc = ccsx_sg_select(keys.data(), n_hits, cuts);
        ccsx_sg_put(out, (size_t)z, n_hits, ccsx_sg_pieces(cuts, nc, L, A, o.min_len, list));
    }
    return 0;
}

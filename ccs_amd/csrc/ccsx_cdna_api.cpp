// ccsx_cdna_api.cpp — the host side of the cDNA analysis that needs no device (DESIGN.md §2 "cDNA rule"): defaults, the argument checks every entry point shares,
// and ccsx_cdna_reads_host, the rule on the calling thread (cdna_core.h with barcode_core.h and segment_core.h: the same walks, keys, scan and classes as the
// kernel's), the whole read walked from its first base.  The entry points that take a handle are in ccsx_api.cpp.
#include <string>
#include <vector>

#include "ccsx.h"
#include "ccsx_internal.h"
#include "cdna_core.h"

void ccsx_cdna_opts_default(ccsx_cdna_opts *o)
{
    if (!o) return;
    o->window = 64; o->max_dist_pct = 15; o->min_margin = 1;        // the barcode rule's
    o->polya_mismatch = 3; o->polya_xdrop = 3; o->polya_max = 512; o->min_polya = 20;   // DESIGN.md §2 "cDNA rule": profiles/cdna_study.txt
    o->min_len = 50;                                                // the segment rule's
}

int ccsx_cdna_rule_version(void) { return 1; }

int ccsx_cdna_check(const ccsx_cdna_set *set, const ccsx_cdna_opts *opts, const ccsx_cdna_report *report, int64_t n, const char *fn, ccsx_cdna_opts *o)
{
    const std::string f(fn);
    if (!set) { ccsx_set_error(f + ": null cdna set"); return -1; }
    if (!report) { ccsx_set_error(f + ": null cdna report"); return -1; }
    if (opts) *o = *opts; else ccsx_cdna_opts_default(o);
    if (o->window < 8 || o->window > CCSX_BARCODE_MAX_WINDOW || o->max_dist_pct < 0 || o->max_dist_pct > 30 || o->min_margin < 0 || o->min_margin > 64 ||
        o->polya_mismatch < 1 || o->polya_mismatch > 8 || o->polya_xdrop < 0 || o->polya_xdrop > 64 || o->polya_max < 16 || o->polya_max > 4096 ||
        o->min_polya < 0 || o->min_polya > 255 || o->min_len < 1 || o->min_len > 65535) {
        ccsx_set_error(f + ": cdna options out of range (8 <= window <= 1024; 0 <= max_dist_pct <= 30; 0 <= min_margin <= 64; 1 <= polya_mismatch <= 8; "
                           "0 <= polya_xdrop <= 64; 16 <= polya_max <= 4096; 0 <= min_polya <= 255; 1 <= min_len <= 65535)");
        return -1;
    }
    if (set->n_primers < 2 || set->n_primers > CCSX_CDNA_MAX_PRIMERS) { ccsx_set_error(f + ": n_primers outside 2 .. 64"); return -1; }
    int roles = 0;
    for (int b = 0; b < set->n_primers; ++b) {
        if (set->role[b] > 1) { ccsx_set_error(f + ": primer " + std::to_string(b) + ": role above 1"); return -1; }
        roles |= 1 << set->role[b];
        if (set->len[b] < CCSX_CDNA_MIN_LEN || set->len[b] > CCSX_CDNA_MAX_LEN) {
            ccsx_set_error(f + ": primer " + std::to_string(b) + ": length outside 8 .. 64"); return -1;
        }
        for (int i = 0; i < set->len[b]; ++i)
            if (set->seq[b][i] > 3) { ccsx_set_error(f + ": primer " + std::to_string(b) + ": code above 3"); return -1; }
    }
    if (roles != 3) { ccsx_set_error(f + ": the primer set needs a primer of role 0 (5') and one of role 1 (3')"); return -1; }
    if (report->n_zmw != n || !report->tested || !report->cls || !report->strand || !report->start || !report->end || !report->polya_len || !report->n_internal ||
        !report->first_internal || !report->idx || !report->dist || !report->second || !report->clip) {
        ccsx_set_error(f + ": cdna report arrays missing, or sized for another batch"); return -1;
    }
    return 0;
}

int ccsx_cdna_reads_host(const ccsx_cdna_set *set, const ccsx_cdna_opts *opts, const uint8_t *seq, const int64_t *seq_off, const int32_t *seq_len, int32_t n,
                         ccsx_cdna_report *report)
{
    ccsx_cdna_opts o;
    int64_t bytes;
    if (ccsx_cdna_check(set, opts, report, n, __func__, &o) || ccsx_check_reads(seq, seq_off, seq_len, n, __func__, &bytes)) return -1;
    const int P = set->n_primers;
    std::vector<unsigned long long> packed(ccsx_cd_set_words(P), 0ull);
    ccsx_cd_pack(set, packed.data());
    CdnaParams D{};
    D.n_primers = P;
    ccsx_cd_bind(D, packed.data());
    const CdnaOut out = ccsx_cd_out(*report);
    for (int z = 0; z < n; ++z) {
        const int L = seq_len[z];
        if (L <= 0) { ccsx_cd_put_untested(out, (size_t)z); continue; }
        const uint8_t *c = seq + seq_off[z];
        const auto base = [&](int j) { return (int)(c[j] & 3); };
        const int W = L < o.window ? L : o.window;
        CdnaEnds e;
        for (int end = 0; end < 2; ++end) {                        // step 1: the barcode rule over the primers
            int best = 0x7fffffff, dist[CCSX_CDNA_MAX_PRIMERS], clip[CCSX_CDNA_MAX_PRIMERS];
            for (int b = 0; b < P; ++b) {
                const unsigned long long *w = D.masks + (size_t)2 * b * CCSX_SG_MASK_WORDS;
                const BarcodeHit h = ccsx_bc_walk(w[0], w[1], w[2], w[3], (int)D.len[b], W, [&](int j) { return ccsx_bc_base(c, L, end, j); });
                dist[b] = h.dist; clip[b] = h.clip;
                const int key = ccsx_bc_key(h.dist, b);
                if (key < best) best = key;
            }
            e.idx[end] = best & 0xffff; e.dist[end] = best >> 16; e.clip[end] = clip[e.idx[end]]; e.second[end] = 255;
            for (int b = 0; b < P; ++b) if (b != e.idx[end] && dist[b] < e.second[end]) e.second[end] = dist[b];
            ccsx_cd_put_end(out, (size_t)z, end, e.idx[end], e.dist[end], e.second[end], e.clip[end]);
        }
        CdnaRead r;
        int ins_len;
        if (ccsx_cd_orient(e, D.len, D.role, L, o, &r, &ins_len)) {
            r.polya_len = ccsx_cd_polya(ccsx_cd_polya_k(ins_len, o), o, [&](int k) { return ccsx_cd_is_a(r.strand, L, e.clip[0], e.clip[1], k, base); });
            for (int s = 0; s < 2 * P; ++s) {                       // step 5: the segment rule's hits, the whole read from its first base
                const unsigned long long *w = D.masks + (size_t)s * CCSX_SG_MASK_WORDS;
                const int m = D.len[s >> 1];
                ccsx_sg_walk(w[0], w[1], w[2], w[3], m, ccsx_sg_k(m, o.max_dist_pct), L, 0, L, base, [&](int end, int dist) {
                    const int start = ccsx_sg_start([&](int b) { return w[4 + b]; }, m, dist, end, base);
                    if (!ccsx_cd_internal(start, end, L, e.clip[0], e.clip[1])) return;
                    ++r.n_internal;
                    if (r.first_internal < 0 || start < r.first_internal) r.first_internal = start;
                });
            }
            ccsx_cd_finish(&r, e, L, ins_len, o);
        }
        ccsx_cd_put_read(out, (size_t)z, 1, r);
    }
    return 0;
}

// ccsx_barcode_api.cpp — the host side of the barcode calls that needs no device (DESIGN.md §2 "Barcode calls"): defaults, the argument checks every entry point
// shares, and ccsx_barcode_reads_host, the rule on the calling thread (barcode_core.h: the same walk and the same call as
// the kernel's).  The entry points that take a handle are in ccsx_api.cpp.
#include <string>
#include <vector>

#include "ccsx.h"
#include "ccsx_internal.h"
#include "barcode_core.h"

void ccsx_barcode_opts_default(ccsx_barcode_opts *o)
{
    if (!o) return;
    o->window = 64; o->max_dist_pct = 15; o->min_margin = 1;   // DESIGN.md §2 "Barcode calls": the study behind them (profiles/barcode_study.txt)
}

int ccsx_barcode_rule_version(void) { return 1; }

int ccsx_barcode_check(const ccsx_barcode_set *set, const ccsx_barcode_opts *opts, const ccsx_barcode_report *report, int64_t n, const char *fn, ccsx_barcode_opts *o)
{
    const std::string f(fn);
    if (!set) { ccsx_set_error(f + ": null barcode set"); return -1; }
    if (!report) { ccsx_set_error(f + ": null barcode report"); return -1; }
    if (opts) *o = *opts; else ccsx_barcode_opts_default(o);
    if (o->window < CCSX_BARCODE_MIN_LEN || o->window > CCSX_BARCODE_MAX_WINDOW || o->max_dist_pct < 0 || o->max_dist_pct > 30 || o->min_margin < 0 || o->min_margin > 64) {
        ccsx_set_error(f + ": barcode options out of range (8 <= window <= 1024; 0 <= max_dist_pct <= 30; 0 <= min_margin <= 64)"); return -1;
    }
    if (set->n_barcodes < 1 || set->n_barcodes > CCSX_BARCODE_MAX) { ccsx_set_error(f + ": n_barcodes outside 1 .. 384"); return -1; }
    for (int b = 0; b < set->n_barcodes; ++b) {
        if (set->len[b] < CCSX_BARCODE_MIN_LEN || set->len[b] > CCSX_BARCODE_MAX_LEN) {
            ccsx_set_error(f + ": barcode " + std::to_string(b) + ": length outside 8 .. 64"); return -1;
        }
        for (int i = 0; i < set->len[b]; ++i)
            if (set->seq[b][i] > 3) { ccsx_set_error(f + ": barcode " + std::to_string(b) + ": code above 3"); return -1; }
    }
    if (report->n_zmw != n || !report->tested || !report->call || !report->bq || !report->idx || !report->dist || !report->second || !report->clip) {
        ccsx_set_error(f + ": barcode report arrays missing, or sized for another batch"); return -1;
    }
    return 0;
}

int ccsx_check_reads(const uint8_t *seq, const int64_t *seq_off, const int32_t *seq_len, int32_t n, const char *fn, int64_t *bytes)
{
    const std::string f(fn);
    *bytes = 0;
    if (n < 0) { ccsx_set_error(f + ": n must be >= 0"); return -1; }
    if (n > 0 && (!seq_off || !seq_len)) { ccsx_set_error(f + ": null argument"); return -1; }
    for (int32_t z = 0; z < n; ++z) {
        if (seq_len[z] <= 0) continue;
        if (seq_off[z] < 0) { ccsx_set_error(f + ": read " + std::to_string(z) + ": negative seq_off"); return -1; }
        *bytes = std::max<int64_t>(*bytes, seq_off[z] + seq_len[z]);
    }
    if (*bytes > 0 && !seq) { ccsx_set_error(f + ": null argument"); return -1; }
    return 0;
}

int ccsx_barcode_reads_host(const ccsx_barcode_set *set, const ccsx_barcode_opts *opts, const uint8_t *seq, const int64_t *seq_off, const int32_t *seq_len,
                            int32_t n, ccsx_barcode_report *report)
{
    ccsx_barcode_opts o;
    int64_t bytes;
    if (ccsx_barcode_check(set, opts, report, n, __func__, &o) || ccsx_check_reads(seq, seq_off, seq_len, n, __func__, &bytes)) return -1;
    const int nb = set->n_barcodes;
    std::vector<unsigned long long> packed(ccsx_bc_set_words(nb), 0ull);
    std::vector<int> dist((size_t)nb);
    ccsx_bc_pack(set, packed.data());
    BarcodeParams B{};
    B.n_barcodes = nb;
    ccsx_bc_bind(B, packed.data());
    const BarcodeOut out = ccsx_bc_out(*report);
    for (int z = 0; z < n; ++z) {
        const int L = seq_len[z];
        if (L <= 0) { ccsx_bc_put_untested(out, z); continue; }
        const uint8_t *c = seq + seq_off[z];
        const int W = std::min(L, o.window);
        int idx[2], d[2], s2[2], m[2];
        for (int e = 0; e < 2; ++e) {
            int best = 0x7fffffff, clip = 0;
            for (int b = 0; b < nb; ++b) {
                const unsigned long long *k = &B.masks[(size_t)b * 4];
                const BarcodeHit h = ccsx_bc_walk(k[0], k[1], k[2], k[3], (int)B.len[b], W, [&](int j) { return ccsx_bc_base(c, L, e, j); });
                dist[b] = h.dist;
                if (ccsx_bc_key(h.dist, b) < best) { best = ccsx_bc_key(h.dist, b); clip = h.clip; }
            }
            idx[e] = best & 0xffff; d[e] = best >> 16; m[e] = B.len[idx[e]]; s2[e] = 255;
            for (int b = 0; b < nb; ++b) if (b != idx[e]) s2[e] = std::min(s2[e], dist[b]);
            out.idx[2 * z + e] = idx[e]; out.dist[2 * z + e] = d[e]; out.second[2 * z + e] = s2[e]; out.clip[2 * z + e] = clip;
        }
        int call, bq;
        ccsx_bc_read_call(d, s2, m, o, &call, &bq);
        out.tested[z] = 1; out.call[z] = call; out.bq[z] = bq;
    }
    return 0;
}

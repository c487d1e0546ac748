// ccsx_dup_api.cpp — the host side of the duplicate reads that needs no device (DESIGN.md §2 "Duplicate rule"): defaults, the argument checks every entry point
// shares, and ccsx_dup_sign_reads_host / ccsx_dup_cluster_host, the rule on the calling thread (dup_core.h: the same signature, the same walks and the same
// predicate as the kernels').  The entry points that take a handle are in ccsx_api.cpp.
#include <algorithm>
#include <numeric>
#include <string>
#include <vector>

#include "ccsx.h"
#include "ccsx_internal.h"
#include "dup_core.h"

void ccsx_dup_opts_default(ccsx_dup_opts *o)
{
    if (!o) return;
    o->window = 32; o->kmer = 12; o->max_dist_pct = 10; o->max_len_diff_pct = 2;   // DESIGN.md §2 "Duplicate rule": the study behind them (profiles/dup_study.txt)
}

int ccsx_dup_rule_version(void) { return 1; }

uint32_t ccsx_dup_hash(uint32_t x) { return ccsx_dup_hash32(x); }

int ccsx_dup_check_opts(const ccsx_dup_opts *opts, const char *fn, ccsx_dup_opts *o)
{
    if (opts) *o = *opts; else ccsx_dup_opts_default(o);
    if (o->window < 16 || o->window > 64 || o->kmer < 8 || o->kmer > 16 || o->kmer > o->window || o->max_dist_pct < 0 || o->max_dist_pct > 30 ||
        o->max_len_diff_pct < 0 || o->max_len_diff_pct > 20) {
        ccsx_set_error(std::string(fn) + ": duplicate options out of range (16 <= window <= 64; 8 <= kmer <= 16, kmer <= window; 0 <= max_dist_pct <= 30; "
                                         "0 <= max_len_diff_pct <= 20)");
        return -1;
    }
    return 0;
}

int ccsx_dup_check_sign(const ccsx_dup_opts *opts, const uint8_t *seq, const int64_t *seq_off, const int32_t *seq_len, int32_t n, const ccsx_dup_sig *sig,
                        const char *fn, ccsx_dup_opts *o, int64_t *bytes)
{
    const std::string f(fn);
    if (ccsx_dup_check_opts(opts, fn, o)) return -1;
    if (n > CCSX_DUP_MAX_READS) { ccsx_set_error(f + ": n above CCSX_DUP_MAX_READS"); return -1; }
    if (ccsx_check_reads(seq, seq_off, seq_len, n, fn, bytes)) return -1;
    if (n > 0 && !sig) { ccsx_set_error(f + ": null argument"); return -1; }
    return 0;
}

int ccsx_dup_check_cluster(const ccsx_dup_opts *opts, const ccsx_dup_sig *sig, const int32_t *group, int32_t n, const ccsx_dup_report *report, const char *fn,
                           ccsx_dup_opts *o)
{
    const std::string f(fn);
    if (ccsx_dup_check_opts(opts, fn, o)) return -1;
    if (n < 0) { ccsx_set_error(f + ": n must be >= 0"); return -1; }
    if (n > CCSX_DUP_MAX_READS) { ccsx_set_error(f + ": n above CCSX_DUP_MAX_READS"); return -1; }
    if (!report || (n > 0 && !sig)) { ccsx_set_error(f + ": null argument"); return -1; }
    if (report->n != n || !report->status || !report->rep || !report->set_size || !report->dup) {
        ccsx_set_error(f + ": duplicate report arrays missing, or sized for another n"); return -1;
    }
    for (int32_t z = 0; z < n; ++z) {
        if (sig[z].window != 0 && sig[z].window != o->window) {
            ccsx_set_error(f + ": signature " + std::to_string(z) + ": taken with another window"); return -1;
        }
        if (group && group[z] < 0) { ccsx_set_error(f + ": read " + std::to_string(z) + ": negative group"); return -1; }
    }
    return 0;
}

int ccsx_dup_sign_reads_host(const ccsx_dup_opts *opts, const uint8_t *seq, const int64_t *seq_off, const int32_t *seq_len, int32_t n, ccsx_dup_sig *sig)
{
    ccsx_dup_opts o;
    int64_t bytes;
    if (ccsx_dup_check_sign(opts, seq, seq_off, seq_len, n, sig, __func__, &o, &bytes)) return -1;
    for (int32_t z = 0; z < n; ++z) sig[z] = seq_len[z] >= o.window ? ccsx_dup_sign(seq + seq_off[z], seq_len[z], o) : ccsx_dup_sig_untested(seq_len[z]);
    return 0;
}

int ccsx_dup_cluster_host(const ccsx_dup_opts *opts, const ccsx_dup_sig *sig, const int32_t *group, const int32_t *score, int32_t n, ccsx_dup_report *report)
{
    ccsx_dup_opts o;
    if (ccsx_dup_check_cluster(opts, sig, group, n, report, __func__, &o)) return -1;
    const DupOut out = ccsx_dup_out(*report);
    std::vector<unsigned long long> key((size_t)n);
    std::vector<int32_t> order((size_t)n);
    for (int32_t z = 0; z < n; ++z) key[z] = ccsx_dup_key(sig[z]);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return key[a] < key[b]; });
    std::vector<int> par, cnt, rep;
    std::vector<DupEnds> ends;
    for (int32_t p0 = 0, p1; p0 < n; p0 = p1) {
        const unsigned long long k0 = key[order[p0]];
        for (p1 = p0 + 1; p1 < n && key[order[p1]] == k0; ++p1) {}
        const int m = p1 - p0;
        const int32_t *zs = &order[p0];                              // the bucket's reads, in index order
        if (k0 == CCSX_DUP_KEY_UNTESTED || m == 1 || m > CCSX_DUP_MAX_BUCKET) {
            const int st = k0 == CCSX_DUP_KEY_UNTESTED ? CCSX_DUP_UNTESTED : m == 1 ? CCSX_DUP_TESTED : CCSX_DUP_OVERFLOW;
            for (int t = 0; t < m; ++t) ccsx_dup_put_alone(out, zs[t], st);
            continue;
        }
        par.resize(m); cnt.assign(m, 0); rep.assign(m, -1); ends.resize(m);
        for (int t = 0; t < m; ++t) { par[t] = t; ends[t] = ccsx_dup_ends(&sig[zs[t]].end[0][0]); }
        auto find = [&](int x) { while (par[x] != x) x = par[x] = par[par[x]]; return x; };
        for (int j = 1; j < m; ++j)
            for (int i = 0; i < j; ++i) {
                const int zi = zs[i], zj = zs[j];
                if (!ccsx_dup_may_pair(sig[zi].len, group ? group[zi] : 0, sig[zj].len, group ? group[zj] : 0, o)) continue;
                const int a = find(i), b = find(j);
                if (a == b || !ccsx_dup_ends_agree(ends[i], ends[j], o)) continue;     // (already one set: a pair more changes nothing)
                par[std::max(a, b)] = std::min(a, b);                // (the root of a set is its smallest member)
            }
        for (int t = 0; t < m; ++t) {                                // (in index order: the first of the largest score stays)
            const int r = find(t);
            ++cnt[r];
            if (rep[r] < 0 || (score ? score[zs[t]] : 0) > (score ? score[zs[rep[r]]] : 0)) rep[r] = t;
        }
        for (int t = 0; t < m; ++t) {
            const int r = find(t), z = zs[t], zr = zs[rep[r]];
            out.status[z] = CCSX_DUP_TESTED; out.rep[z] = zr; out.set_size[z] = cnt[r]; out.dup[z] = zr != z;
        }
    }
    return 0;
}

// ccsx_cell_api.cpp — the host side of the cell-tag analysis that needs no device (DESIGN.md §2 "Cell-tag rule"): the default design, the whitelist's builder, the
// argument check both forms of the call share, and ccsx_cell_reads_host, the rule on the calling thread (cell_core.h over cdna_core.h: the same walks, fields,
// candidates, probes and classes as the kernel's).  ccsx_cell_reads, which takes a handle, is in ccsx_api.cpp.
#include <atomic>
#include <new>
#include <string>
#include <vector>

#include "ccsx.h"
#include "ccsx_internal.h"
#include "cell_core.h"

void ccsx_cell_design_default(ccsx_cell_design *d)
{
    if (!d) return;
    *d = ccsx_cell_design{12, 16, 1, 1, 1, {0, 0, 0}};
}

int ccsx_cell_rule_version(void) { return 1; }

uint32_t ccsx_cell_slot(uint32_t key, uint32_t slots) { return ccsx_cl_slot(key, slots); }

ccsx_cell_whitelist *ccsx_cell_whitelist_create(const uint8_t *codes, int32_t n, int32_t bc_len)
{
    static std::atomic<uint64_t> serial{0};
    const std::string f(__func__);
    if (!codes) { ccsx_set_error(f + ": null codes"); return nullptr; }
    if (n < 1 || n > CCSX_CELL_MAX_WHITELIST) { ccsx_set_error(f + ": n outside 1 .. 2^23"); return nullptr; }
    if (bc_len < 1 || bc_len > CCSX_CELL_MAX_FIELD) { ccsx_set_error(f + ": bc_len outside 1 .. 16"); return nullptr; }
    const uint32_t slots = ccsx_cl_n_slots(n);
    unsigned long long *table = new (std::nothrow) unsigned long long[slots]();
    ccsx_cell_whitelist *wl = new (std::nothrow) ccsx_cell_whitelist{n, bc_len, slots, 0, table};
    if (!table || !wl) { delete[] table; delete wl; ccsx_set_error(f + ": out of memory"); return nullptr; }
    for (int32_t k = 0; k < n; ++k) {
        const uint8_t *c = codes + (size_t)k * bc_len;
        for (int i = 0; i < bc_len; ++i)
            if (c[i] > 3) { ccsx_set_error(f + ": barcode " + std::to_string(k) + ": code above 3"); ccsx_cell_whitelist_destroy(wl); return nullptr; }
        const uint32_t x = ccsx_cl_pack(bc_len, [&](int j) { return (int)c[j]; });
        uint32_t s = ccsx_cl_slot(x, slots);
        for (; table[s]; s = (s + 1u) & (slots - 1u))
            if ((uint32_t)(table[s] >> 32) == x) {
                ccsx_set_error(f + ": barcodes " + std::to_string((uint32_t)table[s] - 1u) + " and " + std::to_string(k) + " are the same");
                ccsx_cell_whitelist_destroy(wl);
                return nullptr;
            }
        table[s] = ((unsigned long long)x << 32) | (unsigned long long)(uint32_t)(k + 1);
    }
    wl->serial = ++serial;
    return wl;
}

void ccsx_cell_whitelist_destroy(ccsx_cell_whitelist *wl)
{
    if (!wl) return;
    delete[] wl->table;
    delete wl;
}

int ccsx_cell_whitelist_info(const ccsx_cell_whitelist *wl, int32_t *n, int32_t *bc_len, uint32_t *slots, const uint64_t **table)
{
    if (!wl) { ccsx_set_error(std::string(__func__) + ": null whitelist"); return -1; }
    if (n) *n = wl->n;
    if (bc_len) *bc_len = wl->bc_len;
    if (slots) *slots = wl->slots;
    if (table) *table = (const uint64_t *)wl->table;
    return 0;
}

int ccsx_cell_check(const ccsx_cdna_set *set, const ccsx_cdna_opts *opts, const ccsx_cell_design *design, const ccsx_cell_whitelist *wl,
                    const ccsx_cell_report *report, int64_t n, const char *fn, ccsx_cdna_opts *o)
{
    const std::string f(fn);
    if (!report) { ccsx_set_error(f + ": null cell report"); return -1; }
    if (!design) { ccsx_set_error(f + ": null cell design"); return -1; }
    if (ccsx_cdna_check(set, opts, &report->cdna, n, fn, o)) return -1;
    const ccsx_cell_design &d = *design;
    if (d.umi_len < 0 || d.umi_len > CCSX_CELL_MAX_FIELD || d.bc_len < 0 || d.bc_len > CCSX_CELL_MAX_FIELD) {
        ccsx_set_error(f + ": cell design: a field length outside 0 .. 16"); return -1;
    }
    if (d.umi_len + d.bc_len < 1) { ccsx_set_error(f + ": cell design: umi_len + bc_len must be at least 1"); return -1; }
    if (d.side < 0 || d.side > 1 || d.bc_first < 0 || d.bc_first > 1 || d.indels < 0 || d.indels > 1) {
        ccsx_set_error(f + ": cell design: side, bc_first and indels are 0 or 1"); return -1;
    }
    if (d.reserved[0] != 0 || d.reserved[1] != 0 || d.reserved[2] != 0) { ccsx_set_error(f + ": cell design: reserved must be 0"); return -1; }
    if (wl && wl->bc_len != d.bc_len) {
        ccsx_set_error(f + ": the whitelist's barcodes have " + std::to_string(wl->bc_len) + " bases, the design's " + std::to_string(d.bc_len)); return -1;
    }
    if (!report->tag || !report->bc_raw || !report->bc || !report->bc_hi || !report->kind || !report->shift || !report->umi || !report->tag_clip) {
        ccsx_set_error(f + ": cell report arrays missing"); return -1;
    }
    return 0;
}

int ccsx_cell_reads_host(const ccsx_cdna_set *set, const ccsx_cdna_opts *opts, const ccsx_cell_design *design, const ccsx_cell_whitelist *wl,
                         const uint8_t *seq, const int64_t *seq_off, const int32_t *seq_len, int32_t n, ccsx_cell_report *report)
{
    ccsx_cdna_opts o;
    int64_t bytes;
    if (ccsx_cell_check(set, opts, design, wl, report, n, __func__, &o) || ccsx_check_reads(seq, seq_off, seq_len, n, __func__, &bytes)) return -1;
    const ccsx_cell_design &d = *design;
    const int P = set->n_primers, T = d.umi_len + d.bc_len, b = d.bc_len;
    std::vector<unsigned long long> packed(ccsx_cd_set_words(P), 0ull);
    ccsx_cd_pack(set, packed.data());
    CdnaParams D{};
    D.n_primers = P;
    ccsx_cd_bind(D, packed.data());
    const CellOut out = ccsx_cl_out(*report);
    for (int z = 0; z < n; ++z) {
        const int L = seq_len[z];
        CellTag t = ccsx_cl_none();
        if (L <= 0) { ccsx_cd_put_untested(out.cd, (size_t)z); ccsx_cl_put_tag(out, (size_t)z, t); continue; }
        const uint8_t *c = seq + seq_off[z];
        const auto base = [&](int j) { return (int)(c[j] & 3); };
        const int W = L < o.window ? L : o.window;
        CdnaEnds e;
        for (int end = 0; end < 2; ++end) {                        // step 1: the cDNA rule's ends
            int best = 0x7fffffff, dist[CCSX_CDNA_MAX_PRIMERS], clip[CCSX_CDNA_MAX_PRIMERS];
            for (int p = 0; p < P; ++p) {
                const unsigned long long *w = D.masks + (size_t)2 * p * CCSX_SG_MASK_WORDS;
                const BarcodeHit h = ccsx_bc_walk(w[0], w[1], w[2], w[3], (int)D.len[p], W, [&](int j) { return ccsx_bc_base(c, L, end, j); });
                dist[p] = h.dist; clip[p] = h.clip;
                const int key = ccsx_bc_key(h.dist, p);
                if (key < best) best = key;
            }
            e.idx[end] = best & 0xffff; e.dist[end] = best >> 16; e.clip[end] = clip[e.idx[end]]; e.second[end] = 255;
            for (int p = 0; p < P; ++p) if (p != e.idx[end] && dist[p] < e.second[end]) e.second[end] = dist[p];
            ccsx_cd_put_end(out.cd, (size_t)z, end, e.idx[end], e.dist[end], e.second[end], e.clip[end]);
        }
        CdnaRead r;
        int ins_len;
        if (ccsx_cd_orient(e, D.len, D.role, L, o, &r, &ins_len)) {
            if (ins_len < T) r.cls = CCSX_CDNA_SHORT;              // step 2
            else {
                const int e_t = ccsx_cl_tag_end(r.strand, d), p0 = e.clip[e_t], p = ccsx_cl_bc_at(p0, d);
                const auto tb = [&](int j) { return ccsx_bc_base(c, L, e_t, j); };
                t.bc_raw = ccsx_cl_pack(b, [&](int j) { return tb(p + j); });
                t.tag = CCSX_CELL_RAW;
                if (b > 0 && wl) {                                 // step 4
                    const int exact = ccsx_cl_probe(wl->table, wl->slots, t.bc_raw);
                    if (exact >= 0) { t.tag = CCSX_CELL_EXACT; t.bc = t.bc_hi = exact; }
                    else {
                        const int has_next = ins_len >= T + 1, next = has_next ? tb(p + b) : 0;
                        int lo = 0x7fffffff, hi = -1, kind_lo = 0;
                        for (int i = 0; i < ccsx_cl_n_candidates(b); ++i) {
                            int kind;
                            const uint32_t x = ccsx_cl_candidate(t.bc_raw, b, next, d.indels, has_next, i, &kind);
                            if (!kind) continue;
                            const int w = ccsx_cl_probe(wl->table, wl->slots, x);
                            if (w < 0) continue;
                            if (w < lo || (w == lo && kind < kind_lo)) { lo = w; kind_lo = kind; }
                            if (w > hi) hi = w;
                        }
                        ccsx_cl_decide(&t, hi < 0 ? -1 : lo, hi, kind_lo);
                    }
                }
                const int u = ccsx_cl_umi_at(p0, t.shift, d);
                t.umi = ccsx_cl_pack(d.umi_len, [&](int j) { return tb(u + j); });   // step 5
                t.tag_clip = T + t.shift;
                const CdnaEnds w = ccsx_cl_widen(e, e_t, t.tag_clip);               // step 6
                const int ins2 = ins_len - t.tag_clip;
                if (ins2 < 1) r.cls = CCSX_CDNA_SHORT;
                else {
                    r.polya_len = ccsx_cd_polya(ccsx_cd_polya_k(ins2, o), o, [&](int k) { return ccsx_cd_is_a(r.strand, L, w.clip[0], w.clip[1], k, base); });
                    for (int s = 0; s < 2 * P; ++s) {
                        const unsigned long long *m = D.masks + (size_t)s * CCSX_SG_MASK_WORDS;
                        const int len = D.len[s >> 1];
                        ccsx_sg_walk(m[0], m[1], m[2], m[3], len, ccsx_sg_k(len, o.max_dist_pct), L, 0, L, base, [&](int end, int dist) {
                            const int start = ccsx_sg_start([&](int code) { return m[4 + code]; }, len, dist, end, base);
                            if (!ccsx_cd_internal(start, end, L, w.clip[0], w.clip[1])) return;
                            ++r.n_internal;
                            if (r.first_internal < 0 || start < r.first_internal) r.first_internal = start;
                        });
                    }
                    ccsx_cd_finish(&r, w, L, ins2, o);
                }
            }
        }
        ccsx_cd_put_read(out.cd, (size_t)z, 1, r);
        ccsx_cl_put_tag(out, (size_t)z, t);
    }
    return 0;
}

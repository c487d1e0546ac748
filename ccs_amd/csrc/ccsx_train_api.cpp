// ccsx_train_api.cpp — the host side of the model training that needs no device (DESIGN.md §2 "Model training"): the counting rule for one pair
// (ccsx_train_pair_host, the code k_train shares through train_core.h) and the fitter, the M-step.  ccsx_train_batch itself lives in ccsx_api.cpp with the
// other seams.
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "ccsx_internal.h"
#include "train_core.h"

namespace {

int bad(const char *fn, const char *what) { ccsx_set_error(std::string(fn) + ": " + what); return -1; }

typedef __int128 acc_t;                                     // sums of 2^-32 fixed-point counts: a run of 10^12 events per cell is 2^72
inline long double events(acc_t v) { return (long double)v / 4294967296.0L; }

// least squares of y on 1, u, .., u^d with weights w (normal equations in long double; u is centred and scaled to [-1, 1], so they are well conditioned)
void wls(const std::vector<long double> &u, const std::vector<long double> &y, const std::vector<long double> &w, int d, long double a[4])
{
    long double N[4][5] = {};
    for (size_t q = 0; q < u.size(); ++q) {
        long double pw[7] = {1.0L};
        for (int m = 1; m <= 2 * d; ++m) pw[m] = pw[m - 1] * u[q];
        for (int r = 0; r <= d; ++r) {
            for (int c = 0; c <= d; ++c) N[r][c] += w[q] * pw[r + c];
            N[r][d + 1] += w[q] * pw[r] * y[q];
        }
    }
    for (int c = 0; c <= d; ++c) {                         // Gaussian elimination, partial pivoting
        int p = c;
        for (int r = c + 1; r <= d; ++r) if (fabsl(N[r][c]) > fabsl(N[p][c])) p = r;
        if (p != c) for (int k = 0; k <= d + 1; ++k) { const long double t = N[c][k]; N[c][k] = N[p][k]; N[p][k] = t; }
        for (int r = c + 1; r <= d; ++r) {
            const long double f = N[c][c] != 0.0L ? N[r][c] / N[c][c] : 0.0L;
            for (int k = c; k <= d + 1; ++k) N[r][k] -= f * N[c][k];
        }
    }
    for (int m = 0; m < 4; ++m) a[m] = 0.0L;
    for (int r = d; r >= 0; --r) {
        long double s = N[r][d + 1];
        for (int c = r + 1; c <= d; ++c) s -= N[r][c] * a[c];
        a[r] = N[r][r] != 0.0L ? s / N[r][r] : 0.0L;
    }
}

}  // namespace

struct ccsx_fitter_s {
    ccsx_model start;
    ccsx_fit_opts o;
    std::vector<acc_t> match, stay;                         // [16][12] over every row added
    std::vector<acc_t> bins;                                // [16][snr_bins][4]: matches, branches, sticks, deletions of the rows in the bin
    acc_t loglik = 0;
    int64_t pairs = 0, gated = 0, bases = 0;
};

extern "C" {

int ccsx_train_rule_version(void) { return 1; }

int ccsx_train_pair_host(const ccsx_model *m, const float snr[4], const uint8_t *tpl, int32_t J, int32_t left_flank, int32_t cs, int32_t ce, const uint8_t *obs,
                         int32_t n, float min_zscore, int64_t match[192], int64_t stay[192], int64_t del[16], int64_t *loglik)
{
    const char *fn = "ccsx_train_pair_host";
    if (!m || !snr || !tpl || !match || !stay || !del || !loglik || (n > 0 && !obs)) return bad(fn, "null argument");
    if (J < 1 || J > CCSX_JMAX) return bad(fn, "J outside 1 .. 31");
    if (n < 0 || n > CCSX_IMAX) return bad(fn, "n outside 0 .. 63");
    if (left_flank < 0 || left_flank > 4) return bad(fn, "left_flank outside 0 .. 4");
    if (cs < 0 || ce < cs || ce > J) return bad(fn, "core outside the template");
    for (int j = 0; j < J; ++j) if (tpl[j] > 3) return bad(fn, "template code above 3");
    for (int i = 0; i < n; ++i) if (obs[i] >= CCSX_NOBS) return bad(fn, "observation code above 11");
    ccsx_tr_tables T;
    for (int k = 0; k < CCSX_NCTX; ++k) ccsx_tr_tables_ctx(m, snr, k, &T);
    return ccsx_tr_pair_host(T, tpl, J, left_flank, cs, ce, obs, n, min_zscore, match, stay, del, loglik);
}

void ccsx_fit_opts_default(ccsx_fit_opts *o)
{
    if (!o) return;
    o->degree = 1; o->snr_bins = 64; o->min_events = 200.0; o->pseudo = 0.5;
}

int ccsx_fitter_create(const ccsx_model *start, const ccsx_fit_opts *o, ccsx_fitter *out)
{
    const char *fn = "ccsx_fitter_create";
    if (!start || !out) return bad(fn, "null argument");
    ccsx_fit_opts fo;
    if (o) fo = *o; else ccsx_fit_opts_default(&fo);
    if (fo.degree < 0 || fo.degree > 3 || fo.snr_bins < 4 || fo.snr_bins > 256 || !(fo.min_events >= 0.0) || !(fo.pseudo >= 0.0) || !std::isfinite(fo.min_events) ||
        !std::isfinite(fo.pseudo)) return bad(fn, "options out of range (0 <= degree <= 3; 4 <= snr_bins <= 256; min_events, pseudo >= 0)");
    if (!(start->snr_hi >= start->snr_lo)) return bad(fn, "the start model's SNR range is not lo <= hi");   // (lo == hi: a model fitted at one SNR; every row is in bin 0)
    ccsx_fitter_s *f = new (std::nothrow) ccsx_fitter_s;
    if (!f) return bad(fn, "out of memory");
    f->start = *start; f->o = fo;
    f->match.assign(CCSX_NCTX * CCSX_NOBS, 0); f->stay.assign(CCSX_NCTX * CCSX_NOBS, 0);
    f->bins.assign((size_t)CCSX_NCTX * fo.snr_bins * 4, 0);
    *out = f;
    return 0;
}

int ccsx_fitter_destroy(ccsx_fitter f) { delete f; return 0; }

int ccsx_fitter_add(ccsx_fitter f, const ccsx_train_counts *c, const float *snr)
{
    const char *fn = "ccsx_fitter_add";
    if (!f || !c || !snr) return bad(fn, "null argument");
    if (c->n_zmw < 0 || c->reserved != 0 || !c->match || !c->stay || !c->del || !c->loglik || !c->n_pairs || !c->n_gated || !c->n_bases)
        return bad(fn, "counts arrays missing or reserved not 0");
    const int nb = f->o.snr_bins;
    const double lo = (double)f->start.snr_lo, hi = (double)f->start.snr_hi;
    for (int z = 0; z < c->n_zmw; ++z) {
        const int64_t *mt = c->match + (size_t)z * 192, *sy = c->stay + (size_t)z * 192, *dl = c->del + (size_t)z * 16;
        for (int q = 0; q < 192 + 16; ++q) if ((q < 192 ? (mt[q] | sy[q]) : dl[q - 192]) < 0) return bad(fn, "negative count");
    }
    for (int z = 0; z < c->n_zmw; ++z) {
        const int64_t *mt = c->match + (size_t)z * 192, *sy = c->stay + (size_t)z * 192, *dl = c->del + (size_t)z * 16;
        for (int k = 0; k < CCSX_NCTX; ++k) {
            const int cur = k & 3;
            double s = (double)snr[(size_t)z * 4 + cur];
            if (!(s >= lo)) s = lo;                         // (a NaN goes to the low end)
            if (s > hi) s = hi;
            int b = hi > lo ? (int)std::floor((s - lo) / (hi - lo) * (double)nb) : 0;
            if (b < 0) b = 0;
            if (b > nb - 1) b = nb - 1;
            acc_t *B = &f->bins[((size_t)k * nb + b) * 4];
            for (int o = 0; o < CCSX_NOBS; ++o) {
                const int e = k * CCSX_NOBS + o;
                f->match[e] += mt[e]; f->stay[e] += sy[e];
                B[0] += mt[e];
                B[o / 3 == cur ? 1 : 2] += sy[e];
            }
            B[3] += dl[k];
        }
        f->loglik += c->loglik[z]; f->pairs += c->n_pairs[z]; f->gated += c->n_gated[z]; f->bases += c->n_bases[z];
    }
    return 0;
}

int ccsx_fitter_finish(ccsx_fitter f, ccsx_model *out, ccsx_fit_report *rep)
{
    if (!f || !out) return bad("ccsx_fitter_finish", "null argument");
    const ccsx_model &S = f->start;
    ccsx_model M = S;
    const int nb = f->o.snr_bins;
    const long double minev = (long double)f->o.min_events, ps = (long double)f->o.pseudo;
    const double lo = (double)S.snr_lo, hi = (double)S.snr_hi;
    auto centre = [&](int b) { return hi > lo ? lo + ((double)b + 0.5) * (hi - lo) / (double)nb : lo; };   // (a range of one point: the point)
    double change = 0.0;
    auto moved = [&](double a, double b) { const double d = std::fabs(a - b); if (d > change) change = d; };
    int kept = 0, first = nb, last = -1;
    for (int k = 0; k < CCSX_NCTX; ++k) {
        const int cur = k & 3;
        // ---- emissions
        long double tm = 0.0L, tb = 0.0L, ts = 0.0L, br[3], sk[3] = {0.0L, 0.0L, 0.0L};
        for (int o = 0; o < CCSX_NOBS; ++o) tm += events(f->match[k * CCSX_NOBS + o]);
        for (int p = 0; p < 3; ++p) {
            br[p] = events(f->stay[k * CCSX_NOBS + cur * 3 + p]); tb += br[p];
            acc_t s = 0;
            for (int b = 0; b < 4; ++b) if (b != cur) s += f->stay[k * CCSX_NOBS + b * 3 + p];
            sk[p] = events(s); ts += sk[p];
        }
        if (tm >= minev && tm > 0.0L) for (int o = 0; o < CCSX_NOBS; ++o) M.em_match[k][o] = (float)((events(f->match[k * CCSX_NOBS + o]) + ps) / (tm + 12.0L * ps));
        else ++kept;
        if (tb >= minev && tb > 0.0L) for (int p = 0; p < 3; ++p) M.em_branch[k][p] = (float)((br[p] + ps) / (tb + 3.0L * ps));
        if (ts >= minev && ts > 0.0L) for (int p = 0; p < 3; ++p) M.em_stick[k][p] = (float)((sk[p] + ps) / (ts + 3.0L * ps));
        // ---- transitions: the populated bins of this context
        std::vector<int> pop;
        for (int b = 0; b < nb; ++b) {
            const long double nm = events(f->bins[((size_t)k * nb + b) * 4]);
            if (nm >= minev && nm > 0.0L) pop.push_back(b);
        }
        if (pop.empty()) continue;
        if (pop.front() < first) first = pop.front();
        if (pop.back() > last) last = pop.back();
        const int d = std::min<int>(f->o.degree, (int)pop.size() - 1);
        const long double x0 = ((long double)centre(pop.front()) + (long double)centre(pop.back())) * 0.5L;
        long double xs = ((long double)centre(pop.back()) - (long double)centre(pop.front())) * 0.5L;
        if (!(xs > 0.0L)) xs = 1.0L;
        for (int mv = 0; mv < 3; ++mv) {
            std::vector<long double> u, y, w;
            for (int b : pop) {
                const acc_t *B = &f->bins[((size_t)k * nb + b) * 4];
                const long double nm = events(B[0]);
                u.push_back(((long double)centre(b) - x0) / xs); y.push_back(events(B[1 + mv]) / nm); w.push_back(nm);
            }
            long double a[4];
            wls(u, y, w, d, a);
            // p(x) = sum a_m ((x - x0) / xs)^m, expanded in x
            long double c[4] = {0.0L, 0.0L, 0.0L, 0.0L}, t[4] = {1.0L, 0.0L, 0.0L, 0.0L};   // t = ((x - x0) / xs)^m as a polynomial in x
            for (int m = 0; m <= d; ++m) {
                for (int q = 0; q < 4; ++q) c[q] += a[m] * t[q];
                long double nx[4] = {0.0L, 0.0L, 0.0L, 0.0L};
                for (int q = 0; q < 4; ++q) { nx[q] += t[q] * (-x0 / xs); if (q + 1 < 4) nx[q + 1] += t[q] / xs; }
                for (int q = 0; q < 4; ++q) t[q] = nx[q];
            }
            for (int q = 0; q < 4; ++q) M.trans_poly[k][mv][q] = (float)c[q];
            for (int b : pop) {
                const double x = centre(b);
                auto ev = [&](const float *p) { double v = ((p[3] * x + p[2]) * x + p[1]) * x + p[0]; return v < 1e-6 ? 1e-6 : v; };
                moved(ev(M.trans_poly[k][mv]), ev(S.trans_poly[k][mv]));
            }
        }
    }
    for (int k = 0; k < CCSX_NCTX; ++k) {
        for (int o = 0; o < CCSX_NOBS; ++o) moved(M.em_match[k][o], S.em_match[k][o]);
        for (int p = 0; p < 3; ++p) { moved(M.em_branch[k][p], S.em_branch[k][p]); moved(M.em_stick[k][p], S.em_stick[k][p]); }
    }
    if (last >= first && last >= 0) { M.snr_lo = (float)centre(first); M.snr_hi = (float)centre(last); }   // nothing is extrapolated
    *out = M;
    if (rep) {
        rep->pairs = f->pairs; rep->gated = f->gated; rep->bases = f->bases;
        rep->loglik_per_base = f->bases > 0 ? (double)((long double)f->loglik / 65536.0L / (long double)f->bases) : 0.0;
        rep->contexts_kept = kept; rep->snr_lo = M.snr_lo; rep->snr_hi = M.snr_hi; rep->max_change = change;
    }
    return 0;
}

}  // extern "C"

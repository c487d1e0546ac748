// train_sanitize — the host path of the model training (ccs_amd/csrc/train_core.h through ccsx_train_pair_host, and the fitter of ccsx_train_api.cpp) under
// AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU.  Every buffer handed to the rule is a heap block of exactly the documented size (J template bytes,
// n observation codes, 192 + 192 + 16 table words), so one access out of range is a report.  Random pairs over the whole argument range (J = 1 .. 31, n = 0 .. 63,
// every flank, cores at the template's ends, SNR far outside the range), the bad arguments, then the fitter on the accumulated tables in every grouping.
// Exit 0 = every call returned what its arguments ask for and every fitted row is a distribution; a sanitizer report aborts.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ccsx_internal.h"

static std::string g_err;
void ccsx_set_error(const std::string &s) { g_err = s; }

#include "ccsx_train_api.cpp"

static uint64_t g_s = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { g_s ^= g_s << 13; g_s ^= g_s >> 7; g_s ^= g_s << 17; return (uint32_t)(g_s >> 32); }
static double unif() { return rnd() / 4294967296.0; }

static ccsx_model make_model(int variant)
{
    ccsx_model m;
    memset(&m, 0, sizeof(m));
    snprintf(m.name, sizeof(m.name), "SAN-%d", variant);
    m.snr_lo = 4.0f; m.snr_hi = variant ? 14.0f : 20.0f;
    for (int k = 0; k < CCSX_NCTX; ++k) {
        for (int mv = 0; mv < 3; ++mv) {
            m.trans_poly[k][mv][0] = (float)(0.02 + 0.08 * unif()); m.trans_poly[k][mv][1] = (float)(-2e-3 + 4e-3 * unif());
            m.trans_poly[k][mv][2] = variant ? (float)(1e-4 * unif()) : 0.0f; m.trans_poly[k][mv][3] = variant ? (float)(-1e-5 * unif()) : 0.0f;   // (may go negative: the 1e-6 floor)
        }
        double s = 0.0, e[CCSX_NOBS];
        for (int o = 0; o < CCSX_NOBS; ++o) { e[o] = (o / 3 == (k & 3) ? 8.0 : 0.2) * (0.5 + unif()); s += e[o]; }
        for (int o = 0; o < CCSX_NOBS; ++o) m.em_match[k][o] = (float)(e[o] / s);
        for (int which = 0; which < 2; ++which) {
            double t = 0.0, p[3];
            for (int b = 0; b < 3; ++b) { p[b] = 0.2 + unif(); t += p[b]; }
            for (int b = 0; b < 3; ++b) (which ? m.em_stick : m.em_branch)[k][b] = (float)(p[b] / t);
        }
    }
    return m;
}

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "train_sanitize: line %d: %s (%s)\n", __LINE__, #c, g_err.c_str()); exit(3); } } while (0)

int main(int argc, char **argv)
{
    const long pairs = argc > 1 ? atol(argv[1]) : 20000;
    long counted = 0, gated = 0;
    for (int variant = 0; variant < 2; ++variant) {
        const ccsx_model m = make_model(variant);
        const int NZ = 24;
        std::vector<int64_t> match((size_t)NZ * 192), stay((size_t)NZ * 192), del((size_t)NZ * 16), ll(NZ);
        std::vector<int32_t> np(NZ), ng(NZ), nbs(NZ), st(NZ);
        std::vector<float> snr((size_t)NZ * 4);
        for (int z = 0; z < NZ; ++z) for (int c = 0; c < 4; ++c) snr[z * 4 + c] = z == 0 ? -3.0f : (z == 1 ? 1e6f : (float)(3.0 + 18.0 * unif()));
        for (long q = 0; q < pairs; ++q) {
            const int z = (int)(rnd() % NZ);
            const int J = 1 + (int)(rnd() % 31), n = (q % 97 == 0) ? 63 : (q % 89 == 0 ? 0 : (int)(rnd() % 64));
            int cs = (int)(rnd() % (J + 1)), ce = (int)(rnd() % (J + 1));
            if (ce < cs) { const int t = cs; cs = ce; ce = t; }
            if (q % 5 == 0) { cs = 0; ce = J; }
            uint8_t *tpl = (uint8_t *)malloc((size_t)J), *obs = (uint8_t *)malloc(n ? (size_t)n : 1);
            for (int j = 0; j < J; ++j) tpl[j] = (uint8_t)(rnd() & 3);
            // a segment that follows the template (so that most pairs are counted), stretched or shrunk to n bases
            for (int i = 0; i < n; ++i) { const int j = n > 1 ? (int)((long)i * (J - 1) / (n - 1)) : 0; obs[i] = (uint8_t)((unif() < 0.05 ? (rnd() & 3) : tpl[j]) * 3 + rnd() % 3); }
            int64_t *mt = (int64_t *)calloc(192, 8), *sy = (int64_t *)calloc(192, 8), *dl = (int64_t *)calloc(16, 8), *lk = (int64_t *)calloc(1, 8);
            const int rc = ccsx_train_pair_host(&m, &snr[z * 4], tpl, J, (int)(rnd() % 5), cs, ce, obs, n, q & 1 ? -3.4f : 0.0f, mt, sy, dl, lk);
            REQUIRE(rc == 0 || rc == 1);
            int64_t sum = 0;
            for (int e = 0; e < 192; ++e) { REQUIRE(mt[e] >= 0 && sy[e] >= 0); sum += mt[e]; match[z * 192 + e] += mt[e]; stay[z * 192 + e] += sy[e]; }
            for (int k = 0; k < 16; ++k) { REQUIRE(dl[k] >= 0); sum += dl[k]; del[z * 16 + k] += dl[k]; }
            if (rc == 1) {
                ++counted; np[z] += 1; nbs[z] += n; ll[z] += *lk;
                REQUIRE(std::llabs(sum - ((int64_t)(ce - cs) << 32)) <= ((int64_t)(ce - cs) << 32) / 10000 + 64 * 64);   // every core column is left once
            } else { ++gated; ng[z] += 1; REQUIRE(sum == 0 && *lk == 0); }
            free(tpl); free(obs); free(mt); free(sy); free(dl); free(lk);
        }
        // bad arguments: refused, nothing touched
        {
            uint8_t tpl[4] = {0, 1, 2, 3}, obs[2] = {0, 11}, bad_obs[2] = {0, 12}, bad_tpl[4] = {0, 1, 4, 3};
            int64_t mt[192] = {0}, sy[192] = {0}, dl[16] = {0}, lk = 0;
            REQUIRE(ccsx_train_pair_host(&m, &snr[0], tpl, 4, 4, 0, 4, obs, 64, 0.0f, mt, sy, dl, &lk) < 0);
            REQUIRE(ccsx_train_pair_host(&m, &snr[0], tpl, 32, 4, 0, 4, obs, 2, 0.0f, mt, sy, dl, &lk) < 0);
            REQUIRE(ccsx_train_pair_host(&m, &snr[0], tpl, 0, 4, 0, 0, obs, 2, 0.0f, mt, sy, dl, &lk) < 0);
            REQUIRE(ccsx_train_pair_host(&m, &snr[0], tpl, 4, 5, 0, 4, obs, 2, 0.0f, mt, sy, dl, &lk) < 0);
            REQUIRE(ccsx_train_pair_host(&m, &snr[0], tpl, 4, 4, 3, 2, obs, 2, 0.0f, mt, sy, dl, &lk) < 0);
            REQUIRE(ccsx_train_pair_host(&m, &snr[0], tpl, 4, 4, 0, 5, obs, 2, 0.0f, mt, sy, dl, &lk) < 0);
            REQUIRE(ccsx_train_pair_host(&m, &snr[0], tpl, 4, 4, 0, 4, bad_obs, 2, 0.0f, mt, sy, dl, &lk) < 0);
            REQUIRE(ccsx_train_pair_host(&m, &snr[0], bad_tpl, 4, 4, 0, 4, obs, 2, 0.0f, mt, sy, dl, &lk) < 0);
            REQUIRE(ccsx_train_pair_host(nullptr, &snr[0], tpl, 4, 4, 0, 4, obs, 2, 0.0f, mt, sy, dl, &lk) < 0);
            REQUIRE(ccsx_train_pair_host(&m, &snr[0], tpl, 4, 4, 0, 4, nullptr, 0, 0.0f, mt, sy, dl, &lk) >= 0);
            for (int e = 0; e < 192; ++e) REQUIRE(sy[e] == 0);
        }
        // the fitter: every degree and bin count, the rows in one call and one by one in reverse
        for (int degree = 0; degree <= 3; ++degree) for (int bins : {4, 64, 256}) {
            ccsx_fit_opts o; ccsx_fit_opts_default(&o); o.degree = degree; o.snr_bins = bins; o.min_events = 20.0;
            ccsx_fitter f1 = nullptr, f2 = nullptr;
            REQUIRE(ccsx_fitter_create(&m, &o, &f1) == 0 && ccsx_fitter_create(&m, &o, &f2) == 0);
            ccsx_train_counts all{NZ, 0, match.data(), stay.data(), del.data(), ll.data(), np.data(), ng.data(), nbs.data(), st.data()};
            REQUIRE(ccsx_fitter_add(f1, &all, snr.data()) == 0);
            for (int z = NZ - 1; z >= 0; --z) {
                ccsx_train_counts one{1, 0, &match[z * 192], &stay[z * 192], &del[z * 16], &ll[z], &np[z], &ng[z], &nbs[z], &st[z]};
                REQUIRE(ccsx_fitter_add(f2, &one, &snr[z * 4]) == 0);
            }
            ccsx_model a, b; ccsx_fit_report ra, rb;
            REQUIRE(ccsx_fitter_finish(f1, &a, &ra) == 0 && ccsx_fitter_finish(f2, &b, &rb) == 0 && ccsx_fitter_finish(f2, &b, nullptr) == 0);
            int64_t sum_np = 0;
            for (int z = 0; z < NZ; ++z) sum_np += np[z];
            REQUIRE(memcmp(&a, &b, sizeof(a)) == 0 && ra.pairs == sum_np && rb.pairs == sum_np && ra.max_change == rb.max_change);
            REQUIRE(a.snr_lo >= m.snr_lo && a.snr_hi <= m.snr_hi && a.snr_lo <= a.snr_hi);
            for (int k = 0; k < CCSX_NCTX; ++k) {
                double s = 0.0;
                for (int ob = 0; ob < CCSX_NOBS; ++ob) { REQUIRE(a.em_match[k][ob] > 0.0f && std::isfinite(a.em_match[k][ob])); s += a.em_match[k][ob]; }
                REQUIRE(std::fabs(s - 1.0) < 1e-6);
                for (int mv = 0; mv < 3; ++mv) for (int c = 0; c < 4; ++c) REQUIRE(std::isfinite(a.trans_poly[k][mv][c]));
            }
            REQUIRE(ccsx_fitter_destroy(f1) == 0 && ccsx_fitter_destroy(f2) == 0);
        }
        ccsx_fit_opts bad; ccsx_fit_opts_default(&bad); bad.snr_bins = 3;
        ccsx_fitter f = nullptr;
        REQUIRE(ccsx_fitter_create(&m, &bad, &f) < 0 && f == nullptr && ccsx_fitter_create(nullptr, nullptr, &f) < 0 && ccsx_fitter_destroy(nullptr) == 0);
    }
    printf("train_sanitize: %ld pairs counted, %ld gated, 24 fits: clean\n", counted, gated);
    return counted > pairs / 2 ? 0 : 3;
}

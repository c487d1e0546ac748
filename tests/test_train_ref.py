"""The model training without a device (DESIGN.md §2 "Model training"): the counting rule on the host (ccsx_train_pair_host, the code k_train shares through
train_core.h) against the float64 restatement of tests/train_ref.py, the fitter against known models, and two EM iterations on sampled data.

Bounds (none is fitted to what the code gives):
  per (pair, table entry)   |host - ref| <= 3 LIK_TOL ref + cells 2^-33: LIK_TOL = 2e-5 is arrow_ref.py's bound of one float32 likelihood, and each of the three
                            float32 factors alpha, beta, 1 / L carries it; the second term is the fixed-point conversion, half a step per contributing cell.
  per pair                  sum match + sum del = ce - cs within the same bound (every core column is left exactly once, by a match or a deletion).
  emissions                 |fit - true| <= pseudo / N, N = the matches per context at each of the 12 SNR values (the issue's bound as it stands).  It holds with room for
                            float32: a match row holds 12 N events, so the pseudo-count moves a cell by pseudo |1 - 12 p| / (12 N + 12 pseudo) <= (11 / 12) pseudo / N; a
                            stay row holds 12 N w events, moved by pseudo |1 - 3 p| / (12 N w + 3 pseudo) <= pseudo / (6 N w), and the known model's weights are >= 0.28.
  transition weights        at every populated bin's centre within sum |c_i| s^i 2^-23 + 1e-9: the four coefficients' own float32 rounding, from the TRUE ones.
"""
import numpy as np
import pytest

from ccs_amd import api
import arrow_ref as A
import train_ref as T

FRAC = 2.0 ** 32
STEP = 2.0 ** -33


def _perturbed():
    return api.model_from_json(A.perturbed_model_json(api.model_to_json(api.default_model())))


def _stretch(rng, t, n):
    """n bases that follow template t: surplus bases are copies of the base they follow (branch events), missing ones are dropped; one substitution now and then"""
    b = [int(x) for x in t]
    while len(b) < n:
        at = int(rng.integers(0, len(b))); b.insert(at, b[at])
    while len(b) > n:
        del b[int(rng.integers(0, len(b)))]
    b = np.array(b, np.int64)
    if n:
        sub = rng.random(n) < 0.03
        b = np.where(sub, (b + rng.integers(1, 4, n)) & 3, b)
    return A.obs_codes(b, rng.integers(1, 4, n) if n else np.zeros(0, np.int64))


def _lab(seed=11):
    """[(model name, snr, pairs)]: J = 5, 22, 26, 30, 31; n = 0, 1, 30, 63, J and J -+ up to 30; both strands; with and without a left flank; the core with overhangs
    and the whole template; SNR below, inside and above the range; both models"""
    rng = np.random.default_rng(seed)
    groups = []
    for name in ("default", "perturbed"):
        for snr in ((2.0, 3.0, 2.5, 3.5), (9.0, 12.0, 8.0, 10.0), (25.0, 30.0, 22.0, 40.0)):
            pairs = []
            for J in (5, 22, 26, 30, 31):
                for q, n in enumerate(sorted({0, 1, 30, 63, J, max(0, J - 30), min(63, J + 30), max(0, J - 4), J + 6, J + 1})):
                    for rev in (0, 1):
                        t = rng.integers(0, 4, J).astype(np.uint8)
                        lf, rf = (int(rng.integers(0, 4)) if (q + rev) & 1 else 4), (int(rng.integers(0, 4)) if q & 2 else 4)
                        cs, ce = ((0, J) if (q % 3 == 0 or J < 6) else (2, J - 2))
                        to, lfo, cso, ceo = T.oriented(t, lf, rf, cs, ce, rev)
                        pairs.append(T.make_pair(to, lfo, cso, ceo, _stretch(rng, to, n)))
            if snr[0] < 4.0:
                # the longest segments a window can count: n = 63 as ONE block of copies of a base, one pulse-width bin throughout (branch events where they are
                # cheapest; most sites still fall below 1e-30, which is the gate's to say)
                for J in (30, 31):
                    t = rng.integers(0, 4, J).astype(np.uint8)
                    for at in range(1, J - 1, 3):
                        for pwb in (1, 2, 3):
                            seg = np.concatenate([t[:at], np.full(63 - J, t[at]), t[at:]])
                            pairs.append(T.make_pair(t, 4, 2, J - 2, A.obs_codes(seg, np.full(63, pwb))))
            groups.append((name, snr, pairs))
    return groups


@pytest.fixture(scope="module")
def models(built):
    return {"default": api.default_model(), "perturbed": _perturbed()}


def check_tables(host, ref, q):
    """host = (match, stay, del) int64, ref = e_step's output, q = the pair's index there (or a slice summed by the caller): the per-entry bound"""
    worst = 0.0
    for h, r, c in ((host[0], ref["match"][q], ref["cells_m"][q]), (host[1], ref["stay"][q], ref["cells_s"][q]), (host[2], ref["dele"][q], ref["cells_d"][q])):
        err = np.abs(h / FRAC - r); bound = 3 * A.LIK_TOL * r + c * STEP
        assert np.all(err <= bound), (float(err.max()), float(bound[np.argmax(err - bound)]))
        assert np.all(h[c == 0] == 0)
        worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
    return worst


def test_host_rule_against_float64(models):
    counted, worst, seen = 0, 0.0, dict(n63=0, n0=0, skew26=0, J31=0, noflank=0, whole=0)
    for name, snr, pairs in _lab():
        m = models[name]
        ref = T.e_step([A.tables64(m, snr)], pairs)
        for q, p in enumerate(pairs):
            n, J = len(p["obs"]), len(p["tpl"])
            rc, mt, st, dl, ll = api.train_pair_host(m, snr, p["tpl"].astype(np.uint8), p["lf"], p["cs"], p["ce"], p["obs"].astype(np.uint8))
            scaled = ref["log2L"][q] + 2 * n
            if scaled > A.LOG2_TINY + 0.01: assert rc == 1, (name, snr, J, n, scaled)
            if scaled < A.LOG2_TINY - 0.01: assert rc == 0, (name, snr, J, n, scaled)
            if rc != 1:
                assert not mt.any() and not st.any() and not dl.any() and ll[0] == 0
                continue
            counted += 1
            worst = max(worst, check_tables((mt, st, dl), ref, q))
            tot = (mt.sum() + dl.sum()) / FRAC
            cells = int(ref["cells_m"][q].sum() + ref["cells_d"][q].sum())
            assert abs(tot - (p["ce"] - p["cs"])) <= 3 * A.LIK_TOL * (p["ce"] - p["cs"]) + cells * STEP, (tot, p["ce"] - p["cs"])
            assert abs(ll[0] / 65536.0 - ref["log2L"][q]) <= 2e-5 + A.LIK_TOL / np.log(2.0) + 2.0 ** -17     # det_log2's accuracy, the likelihood's, half a step
            if n == 0: assert not mt.any() and not st.any() and dl.sum() > 0
            seen["n63"] += n == 63; seen["n0"] += n == 0; seen["skew26"] += abs(n - J) >= 26; seen["J31"] += J == 31
            seen["noflank"] += p["lf"] == 4; seen["whole"] += p["cs"] == 0 and p["ce"] == J
    print(f"\n[train host rule] counted pairs {counted}, largest error / bound {worst:.3f}, seen {seen}")
    assert counted > 300 and all(v > 0 for v in seen.values()), seen


def test_bad_arguments_add_nothing(models):
    m = models["default"]; rng = np.random.default_rng(3)
    t = rng.integers(0, 4, 26).astype(np.uint8); obs = _stretch(rng, t, 64)
    out = (np.zeros((16, 12), np.int64), np.zeros((16, 12), np.int64), np.zeros(16, np.int64), np.zeros(1, np.int64))
    snr = (8.0,) * 4
    calls = [dict(tpl=t, left_flank=4, cs=2, ce=24, obs=obs),                      # n = 64
             dict(tpl=t, left_flank=5, cs=2, ce=24, obs=obs[:20]), dict(tpl=t, left_flank=4, cs=2, ce=27, obs=obs[:20]),
             dict(tpl=t, left_flank=4, cs=5, ce=4, obs=obs[:20]), dict(tpl=t, left_flank=4, cs=2, ce=24, obs=obs[:20], J=32),
             dict(tpl=t, left_flank=4, cs=0, ce=0, obs=obs[:20], J=0), dict(tpl=t, left_flank=4, cs=2, ce=24, obs=obs[:20], n=-1),
             dict(tpl=t + 4, left_flank=4, cs=2, ce=24, obs=obs[:20]), dict(tpl=t, left_flank=4, cs=2, ce=24, obs=obs[:20] + 12)]
    for kw in calls:
        rc = api.train_pair_host(m, snr, out=out, **kw)[0]
        assert rc < 0, kw
        assert api.lib().ccsx_last_error()
    assert not any(a.any() for a in out)
    assert api.train_pair_host(m, snr, t, 4, 2, 24, obs[:26], out=out)[0] == 1 and out[0].any()
    assert api.lib().ccsx_train_rule_version() == 1


# ---- the fitter
def _known_model(cubic):
    """SYN-1's emissions reweighted, transition weights linear or cubic in the SNR (float32 coefficients; every weight lies in 0.28 .. 0.6 over the range, so a stay
    row holds at least a quarter of the events of a match row)"""
    rng = np.random.default_rng(21)
    m = api.default_model()
    tp = np.zeros((16, 3, 4), np.float32)
    tp[:, :, 0] = rng.uniform(0.3, 0.5, (16, 3)); tp[:, :, 1] = rng.uniform(-1e-3, 2e-3, (16, 3))
    if cubic:
        tp[:, :, 2] = rng.uniform(-5e-5, 1e-4, (16, 3)); tp[:, :, 3] = rng.uniform(-1e-6, 3e-6, (16, 3))
    for key, w in (("em_match", 12), ("em_branch", 3), ("em_stick", 3)):
        e = np.array(getattr(m, key), np.float64) * rng.uniform(0.7, 1.4, (16, w))
        e = (e / e.sum(1, keepdims=True)).astype(np.float32)
        for k in range(16):
            for o in range(w): getattr(m, key)[k][o] = float(e[k, o])
    for k in range(16):
        for mv in range(3):
            for c in range(4): m.trans_poly[k][mv][c] = float(tp[k, mv, c])
    return m


def _expected_counts(true, snrs, N):
    """one row per SNR value (all four channels alike): N matches per context and what the model expects beside them, converted to fixed point"""
    S = T.model_ns(true)
    tc = api.TrainCounts.allocate(len(snrs))
    for z, s in enumerate(snrs):
        w = np.maximum(((S.trans_poly[:, :, 3] * s + S.trans_poly[:, :, 2]) * s + S.trans_poly[:, :, 1]) * s + S.trans_poly[:, :, 0], 1e-6)
        for k in range(16):
            cur = k & 3
            tc.match[z, k] = np.floor(N * S.em_match[k] * FRAC + 0.5)
            for b in range(4):
                ev = N * w[k, 0] * S.em_branch[k] if b == cur else N * w[k, 1] * S.em_stick[k] / 3.0
                tc.stay[z, k, 3 * b:3 * b + 3] = np.floor(ev * FRAC + 0.5)
            tc.del_[z, k] = np.floor(N * w[k, 2] * FRAC + 0.5)
        tc.n_pairs[z] = 10; tc.n_bases[z] = 1000; tc.loglik[z] = -2300 * 65536
    return tc


def _weights(m, s):
    p = np.array(m.trans_poly, np.float64)
    return np.maximum(((p[:, :, 3] * s + p[:, :, 2]) * s + p[:, :, 1]) * s + p[:, :, 0], 1e-6)


@pytest.mark.parametrize("cubic", [False, True])
def test_fitter_recovers_a_known_model(built, cubic):
    start, true = api.default_model(), _known_model(cubic)
    o = api.fit_opts_default(); o.degree = 3 if cubic else 1
    assert (o.snr_bins, o.min_events, o.pseudo) == (64, 200.0, 0.5)
    cen = T.bin_centres(float(start.snr_lo), float(start.snr_hi), 64)
    bins = np.arange(2, 62, 5); snrs = cen[bins]; N = 1.0e6
    assert len(snrs) == 12
    tc = _expected_counts(true, snrs, N)
    fit, rep = api.Fitter(start, o).add(tc, np.repeat(snrs[:, None], 4, 1)).finish()
    St, Sf = T.model_ns(true), T.model_ns(fit)
    assert min(_weights(true, s).min() for s in snrs) >= 0.28 and max(_weights(true, s).max() for s in snrs) <= 0.6
    for key in ("em_match", "em_branch", "em_stick"):
        err = np.abs(getattr(Sf, key) - getattr(St, key))
        print(f"[train fitter] {key}: largest error {err.max():.3g}, bound {o.pseudo / N:.3g}")
        assert np.all(err <= o.pseudo / N), key
    tp = np.abs(St.trans_poly)
    for s in snrs:
        bound = tp[:, :, 0] + tp[:, :, 1] * s + tp[:, :, 2] * s ** 2 + tp[:, :, 3] * s ** 3
        assert np.all(np.abs(_weights(fit, s) - _weights(true, s)) <= bound * 2.0 ** -23 + 1e-9), s
    if not cubic: assert not Sf.trans_poly[:, :, 2:].any()
    assert rep.contexts_kept == 0 and rep.pairs == 120 and rep.bases == 12000 and abs(rep.loglik_per_base + 2.3) < 1e-12
    assert rep.snr_lo == np.float32(cen[2]) and rep.snr_hi == np.float32(cen[57]) and fit.snr_lo == rep.snr_lo and fit.snr_hi == rep.snr_hi
    # the float64 restatement of the M-step agrees with the library on the same rows
    ref, info = T.m_step(start, tc.match / FRAC, tc.stay / FRAC, tc.del_ / FRAC, np.repeat(snrs[:, None], 4, 1), degree=o.degree)
    assert info["kept"] == 0 and all(len(info["populated"][k]) == 12 for k in range(16))
    for s in snrs: assert np.allclose(_weights(ref, s), _weights(fit, s), rtol=0, atol=1e-7)
    assert np.allclose(ref.em_match, Sf.em_match, rtol=0, atol=2.0 ** -23)


def test_fitter_is_order_independent(built):
    start, true = api.default_model(), _known_model(True)
    rng = np.random.default_rng(8)
    snr = rng.uniform(3.0, 22.0, (40, 4)).astype(np.float32)
    tc = _expected_counts(true, snr[:, 0].astype(np.float64), 3.0e3)
    for a in (tc.match, tc.stay, tc.del_): a[...] = (a * rng.uniform(0.5, 1.5, a.shape)).astype(np.int64)
    o = api.fit_opts_default(); o.degree = 2
    text = lambda f: api.model_to_json(f.finish()[0])
    one = text(api.Fitter(start, o).add(tc, snr))
    order = np.arange(40)[::-1]
    assert text(api.Fitter(start, o).add(tc.rows(order), snr[order])) == one
    f3 = api.Fitter(start, o)
    for part in (order[25:], order[:7], order[7:25]): f3.add(tc.rows(part), snr[part])
    assert text(f3) == one
    assert one != api.model_to_json(start)


def test_fitter_on_sparse_data(built):
    start, true = api.default_model(), _known_model(False)
    cen = T.bin_centres(float(start.snr_lo), float(start.snr_hi), 64)
    o = api.fit_opts_default()
    # fewer than min_events anywhere: everything is the start's
    tc = _expected_counts(true, cen[[10, 20]], 60.0)
    fit, rep = api.Fitter(start, o).add(tc, np.repeat(cen[[10, 20], None], 4, 1)).finish()
    assert rep.contexts_kept == 16 and bytes(fit) == bytes(start) and rep.max_change == 0.0
    # one populated bin: degree 0, a range of that one centre, emissions fitted
    tc = _expected_counts(true, cen[[30]], 1.0e5)
    fit, rep = api.Fitter(start, o).add(tc, np.repeat(cen[[30], None], 4, 1)).finish()
    Sf = T.model_ns(fit)
    assert rep.contexts_kept == 0 and not Sf.trans_poly[:, :, 1:].any()
    assert np.all(np.abs(Sf.trans_poly[:, :, 0] - _weights(true, cen[30])) <= _weights(true, cen[30]) * 2.0 ** -23 + 1e-9)
    assert fit.snr_lo == fit.snr_hi == np.float32(cen[30])
    # such a model is a start like any other (the next EM iteration, a restart from its file): every row goes to its one point, whatever the ZMW's SNR
    tc2 = _expected_counts(true, cen[[8, 50]], 1.0e5)
    again, rep2 = api.Fitter(fit, o).add(tc2, np.repeat(cen[[8, 50], None], 4, 1)).finish()
    assert again.snr_lo == again.snr_hi == fit.snr_lo and rep2.contexts_kept == 0 and not T.model_ns(again).trans_poly[:, :, 1:].any()
    mean_w = 0.5 * (_weights(true, cen[8]) + _weights(true, cen[50]))
    assert np.all(np.abs(T.model_ns(again).trans_poly[:, :, 0] - mean_w) <= mean_w * 2.0 ** -22 + 1e-9)
    ref2, _ = T.m_step(fit, tc2.match / FRAC, tc2.stay / FRAC, tc2.del_ / FRAC, np.repeat(cen[[8, 50], None], 4, 1))
    assert np.allclose(ref2.trans_poly, T.model_ns(again).trans_poly, rtol=0, atol=1e-7) and ref2.snr_lo == ref2.snr_hi == float(fit.snr_lo)
    # two populated bins among three: the range is theirs, the thin bin does not count
    sn = cen[[12, 40, 55]]
    tc = _expected_counts(true, sn, 1.0e5)
    for a in (tc.match, tc.stay, tc.del_): a[2] //= 1000                   # 100 matches at the third SNR value
    fit, rep = api.Fitter(start, o).add(tc, np.repeat(sn[:, None], 4, 1)).finish()
    assert fit.snr_lo == np.float32(cen[12]) and fit.snr_hi == np.float32(cen[40]) and rep.snr_hi == fit.snr_hi
    for key in ("em_match", "em_branch", "em_stick"):
        rows = np.array(getattr(fit, key), np.float32).astype(np.float64)
        assert np.all(np.abs(rows.sum(1) - 1.0) <= 4 * 2.0 ** -23), key
    text = api.model_to_json(fit, ("b", "s", "5.0"))
    assert api.model_to_json(api.model_from_json(text), ("b", "s", "5.0")) == text
    # arguments
    with pytest.raises(RuntimeError): api.Fitter(start, api.FitOpts(4, 64, 200.0, 0.5))
    with pytest.raises(RuntimeError): api.Fitter(start, api.FitOpts(1, 3, 200.0, 0.5))
    bad = _expected_counts(true, cen[[5]], 10.0); bad.match[0, 0, 0] = -1
    with pytest.raises(RuntimeError): api.Fitter(start, o).add(bad, np.repeat(cen[[5], None], 4, 1))


# ---- EM without a device
def _sampled_pairs(true, seed=4):
    """16 ZMWs x 1000 bases x 8 passes sampled from `true` at three SNR settings, cut on the generating path: (pairs, snr[16, 4])"""
    rng = np.random.default_rng(seed)
    settings = ((6.0, 7.0, 6.5, 7.5), (9.0, 10.5, 9.5, 10.0), (12.0, 13.5, 12.5, 13.0))
    pairs, snr = [], []
    for z in range(16):
        s = settings[z % 3]; snr.append(s)
        t = rng.integers(0, 4, 1000).astype(np.uint8)
        passes = []
        for r in range(8):
            rev = r & 1
            obs, enter = T.sample_pass(true, s, A.revcomp(t) if rev else t, 4, rng)
            passes.append((rev, obs, enter))
        pairs += T.cut_pairs(t, passes, z)
    return pairs, np.array(snr, np.float32)


def _ll(model, pairs, snr):
    tabs = [A.tables64(model, s) for s in snr]
    r = T.e_step(tabs, pairs, want_counts=False)
    return float(r["log2L"].sum() / sum(len(p["obs"]) for p in pairs))


def _zmw_rows(ref, pairs, n):
    zi = np.array([p["z"] for p in pairs])
    m, s, d = np.zeros((n, 16, 12)), np.zeros((n, 16, 12)), np.zeros((n, 16))
    np.add.at(m, zi, ref["match"]); np.add.at(s, zi, ref["stay"]); np.add.at(d, zi, ref["dele"])
    return m, s, d


def test_em_without_a_device(built):
    true, start = _perturbed(), api.default_model()
    pairs, snr = _sampled_pairs(true)
    nb = sum(len(p["obs"]) for p in pairs)
    assert len(pairs) > 5000
    ll_true, ll_start = _ll(true, pairs, snr), _ll(start, pairs, snr)
    # the reference EM first: it must itself satisfy both statements
    cur, lls = T.model_ns(start), [ll_start]
    for it in range(2):
        ref = T.e_step([A.tables64(cur, s) for s in snr], pairs)
        assert abs(ref["log2L"].sum() / nb - lls[-1]) < 1e-12
        cur, _ = T.m_step(cur, *_zmw_rows(ref, pairs, 16), snr, degree=1)
        lls.append(_ll(cur, pairs, snr))
    print(f"\n[train em] {len(pairs)} pairs, {nb} bases; LL true {ll_true:.5f}; reference EM {[round(x, 5) for x in lls]}")
    assert lls[0] < lls[1] < lls[2] and ll_true - lls[2] <= 0.05 * (ll_true - ll_start), (lls, ll_true)
    # the library: ccsx_train_pair_host + the fitter
    model, lib_lls = start, [ll_start]
    o = api.fit_opts_default(); o.degree = 1
    for it in range(2):
        tc = api.TrainCounts.allocate(16)
        for p in pairs:
            z = p["z"]
            rc = api.train_pair_host(model, snr[z], p["tpl"].astype(np.uint8), p["lf"], p["cs"], p["ce"], p["obs"].astype(np.uint8),
                                     out=(tc.match[z], tc.stay[z], tc.del_[z], tc.loglik[z:z + 1]))[0]
            assert rc >= 0
            tc.n_pairs[z] += rc == 1; tc.n_gated[z] += rc == 0; tc.n_bases[z] += len(p["obs"]) if rc == 1 else 0
        model, rep = api.Fitter(model, o).add(tc, snr).finish()
        if rep.gated == 0: assert abs(rep.loglik_per_base - lib_lls[-1]) < 1e-4
        lib_lls.append(_ll(model, pairs, snr))
    print(f"[train em] library EM {[round(x, 5) for x in lib_lls]}, gated pairs of the last iteration {rep.gated}")
    assert lib_lls[0] < lib_lls[1] < lib_lls[2] and ll_true - lib_lls[2] <= 0.05 * (ll_true - ll_start), (lib_lls, ll_true)

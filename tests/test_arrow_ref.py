"""The CPU restatement's Arrow polish (oracle/ccs_oracle.c: fill, score_mut, polish_window_impl, orc_zparams) against the plain float64
restatement of tests/arrow_ref.py, at the window limits.  A seeded "window lab" makes (template, reads, strands, flanks, core) for named
families; every family asserts that it produced what it is named for, prints its case counts and the share of (lane, read) pairs it had to
leave out because the reference itself puts the mutated likelihood below TINY_P (cap: 2 %).

Bounds (none of them fitted to what the oracle gives):
  likelihood of a read, oracle / reference - 1:            2e-5   (tests/test_oracle_hmm.py)
  likelihood of a (lane, read) pair:                       3e-5   (tests/test_oracle_hmm.py)
  log2-gain of a lane summed over n reads (banded mode):   n * (2 * 2e-5 + 2 * 3e-5 / ln 2 + 2^-17)
      = det_log2's asserted accuracy twice, the two likelihood tolerances in log2 units, half a fixed-point step
  p_err of a core base: the image of that bound under s = sum 2^min(d, 20), p = s / (1 + s), widened by 5e-6 relative for the float32
      evaluation (det_exp2 is asserted to 2e-6 by tests/test_oracle_hmm.py::test_det_log2_exp2_accuracy; at most 12 terms, one division);
      a floor is a float32 value: 3e-7 = two units in its last place

Measured here (python -m pytest tests/test_arrow_ref.py -q -s -m "not gpu"; every family prints its own figures and where its largest gap is):
  left-out share of (lane, read) pairs: skew 1.82 %, limits 0.02 %, every other family 0
  full vs banded float64 reference, largest |log2 L_full - log2 L_banded| over the usable (lane, read) pairs / pairs beyond 1e-6 relative:
      limits 7.3 / 171 of 6275 (case I0_I64, lane 197), skew 1.7e-04 / 8, reverse 5.3e-04 / 14, deep 2.2e-03 / 117, snr 1.9e-06 / 1, ends 1.1e-06 / 0, homopolymer 5.6e-04 / 14
  lanes on which the two modes disagree about delta > MUT_EPS: 0 in every family (asserted)
  So the pair-by-pair agreement of the two modes that DESIGN.md §2 "Banded link" suggests does not hold in the ordinary families either, while no decision moves;
  the oracle is therefore held to the BANDED reference everywhere and to the full one on the pairs where the reference's own modes agree within 1e-6.
  |I - J| = 40 cannot be made usable: 32 inserted bases cost about 2^-91 (scaled) at the low end of the SNR range, TINY_P is 2^-99.7; the family reaches 30
  (usable: 4 .. 17, 22, 26, 30).  Likewise J = 31 with I = 5 (26 deletions, 2^-112): the smallest usable read of a J = 31 window has I = 8 (asserted: <= 10).
  CPU time of the float64 reference: about 0.1 s per 6-read window for both modes, 2 s for 96 reads; the module runs in 40 - 80 s depending on the machine.
Sensitivity (shown once, scratch copies): orc_set_score_band(2) and a reverse-strand insertion column moved by one each fail every family that has such reads;
orc_set_fill_margins(0, 0) fails limits (case I0_I64); orc_set_score_clip(0) is noticed by no family.
"""
import numpy as np
import pytest

from ccs_amd import api
import arrow_ref as A
import oracle_lib as O

LIK_TOL, MUT_TOL = A.LIK_TOL, A.MUT_TOL
PER_READ = A.PER_READ
SNR0 = (9.0, 16.0, 8.0, 13.0)
LEFT_OUT_CAP = 0.02


def _perturbed_model():
    return api.model_from_json(A.perturbed_model_json(api.model_to_json(api.default_model())))


_MODELS = {}


def _model(name):
    if name not in _MODELS:
        _MODELS[name] = api.default_model() if name == "default" else _perturbed_model()
    return _MODELS[name]


# ------------------------------------------------------------------ the window lab
def _obs(rng, bases):
    b = np.asarray(bases, np.int64)
    return (b * 3 + rng.integers(0, 3, len(b))).astype(np.uint8)


def _noisy(rng, t, p):
    r = []
    for b in t:
        while rng.random() < p: r.append(int(rng.integers(0, 4)))
        if rng.random() < p: continue
        r.append(int(b) if rng.random() > p / 2 else int(rng.integers(0, 4)))
    return np.array(r, np.int64)


def _read(rng, tpl, rev, p=0.04, block=None, cut=None, stutter=0, pwc=None):
    """bases of one read of `tpl` in native orientation: optional inserted block (at, bases), deleted stretch (at, n), noise p"""
    t = [int(b) for b in tpl]
    if block is not None: t = t[:block[0]] + [int(b) for b in block[1]] + t[block[0]:]
    if cut is not None: t = t[:cut[0]] + t[cut[0] + cut[1]:]
    if stutter: t = [b for k, b in enumerate(t) for _ in range(2 if k < stutter else 1)]      # every one of the first `stutter` bases twice: branch events
    t = np.array(t, np.int64)
    if rev: t = 3 - t[::-1]
    o = _obs(rng, _noisy(rng, t, p) if p > 0 else t)[:70]
    return o if pwc is None else (o // 3 * 3 + pwc).astype(np.uint8)       # pwc: one pulse-width bin for the whole read


def _case(name, tpl, reads, strands, lf=4, rf=4, cs=2, ce=None, snr=SNR0, model="default", max_qv=50):
    tpl = np.asarray(tpl, np.uint8)
    return dict(name=name, tpl=tpl, reads=reads, strands=list(strands), lf=lf, rf=rf, cs=cs, ce=len(tpl) - 2 if ce is None else ce, snr=snr, model=model, max_qv=max_qv)


def lab(family, seed=7):
    rng = np.random.default_rng([seed, sum(map(ord, family))])
    T = lambda J: rng.integers(0, 4, J).astype(np.uint8)
    out = []
    if family == "limits":
        t = T(31)
        # 32 inserted bases are affordable (scaled likelihood above TINY_P) only as branch events at the low end of the SNR range: ~ 2^-91 there, 2^-100 at typical SNR
        dbl = lambda k: np.array([b for j, b in enumerate(t) for _ in range(3 if j == 30 and k < 3 else 2)], np.uint8)
        out.append(_case("J31_I63", t, [(3 * A.revcomp(dbl(k)) if k & 1 else 3 * dbl(k)).astype(np.uint8) + k % 3 for k in range(6)] + [_read(rng, t, 0) for _ in range(3)],
                         [0, 1, 0, 1, 0, 1, 0, 0, 0], lf=2, rf=1, snr=(4.0,) * 4))
        out.append(_case("J31_I5", t, [_read(rng, t, 0, p=0.0, cut=(3, 26)), _read(rng, t, 1, p=0.0, cut=(2, 26))] + [_read(rng, t, k & 1) for k in range(4)], [0, 1, 0, 1, 0, 1], lf=0, rf=3))
        # 26 deleted columns cost 2^-112 (deletion ~ 2^-4.3 each at the low end of the SNR range): I = 5 cannot stay above TINY_P (2^-99.7); about 22 deletions can
        out.append(_case("J31_smallI", t, [_read(rng, t, k & 1, p=0.0, cut=(4 + k % 3, 23 - k // 3), pwc=k % 3) for k in range(15)], [k & 1 for k in range(15)], lf=0, rf=3, snr=(4.0,) * 4))
        t = T(5)
        out.append(_case("J5", t, [_read(rng, t, k & 1, p=0.02) for k in range(6)], [k & 1 for k in range(6)], cs=1, ce=4, lf=3))
        t = T(24)
        # (read 1: I = J, but its first 12 bases twice and the last 12 missing - a path 12 rows off the diagonal the fill band is laid around)
        out.append(_case("I0_I64", t, [np.zeros(0, np.uint8), _read(rng, t, 0, p=0.0, stutter=24)[:24], _obs(rng, rng.integers(0, 4, 64))] + [_read(rng, t, k & 1) for k in range(4)],
                         [0, 0, 0, 0, 1, 0, 1], lf=1, rf=2))
    elif family == "skew":
        for where in ("first", "middle", "last"):
            for n in (4, 9, 17, 22, 26, 30, 40):
                J = int(rng.integers(20, 24 if n == 40 else 27)); t = T(J)
                at = {"first": 0, "middle": J // 2, "last": J - 1}[where]      # (the model has no stay behind the last column: the last place a block can be emitted is before it)
                blk = rng.integers(0, 4, n) if n < 17 else np.full(n, t[at])   # long blocks: copies of the base that follows (branch events), or no read stays above TINY_P
                reads = [_read(rng, t, k & 1, p=0.02 if n < 17 else 0.0, block=(at, blk), pwc=None if n < 17 else k)[:63] for k in range(3)] + [_read(rng, t, k & 1, p=0.03) for k in range(3)]
                out.append(_case(f"ins{n}_{where}", t, reads, [0, 1, 0, 0, 1, 0], lf=int(rng.integers(0, 5)), rf=int(rng.integers(0, 5)), snr=SNR0 if n < 22 else (4.0,) * 4))
            for n in (4, 8, 14):
                J = int(rng.integers(26, 32)); t = T(J)
                at = {"first": 0, "middle": (J - n) // 2, "last": J - n}[where]
                reads = [_read(rng, t, k & 1, p=0.02, cut=(at, n)) for k in range(3)] + [_read(rng, t, k & 1, p=0.03) for k in range(3)]
                out.append(_case(f"del{n}_{where}", t, reads, [0, 1, 0, 0, 1, 0], lf=int(rng.integers(0, 5)), rf=int(rng.integers(0, 5))))
    elif family == "reverse":
        for k in range(3):
            t = T(int(rng.integers(18, 30)))
            out.append(_case(f"allrev{k}", t, [_read(rng, t, 1) for _ in range(5)], [1] * 5, lf=int(rng.integers(0, 5)), rf=int(rng.integers(0, 5))))
            st = [int(rng.integers(0, 2)) for _ in range(7)]; st[0], st[1] = 0, 1
            out.append(_case(f"mixed{k}", t, [_read(rng, t, s) for s in st], st, lf=int(rng.integers(0, 5)), rf=int(rng.integers(0, 5))))
    elif family == "deep":
        for n in (33, 64, 96):
            t = T(24)
            out.append(_case(f"identical{n}", t, [_read(rng, t, k & 1, p=0.0) for k in range(n)], [k & 1 for k in range(n)], lf=1, rf=0))
            out.append(_case(f"noisy{n}", t, [_read(rng, t, k & 1, p=0.05) for k in range(n)], [k & 1 for k in range(n)], lf=3, rf=4, max_qv=93))
            alt = t.copy(); alt[12] = (alt[12] + 1) & 3; alt = np.delete(alt, 7)                # the reads disagree about two columns: error probabilities that no floor hides
            out.append(_case(f"split{n}", t, [_read(rng, alt if (k // 2) % 2 == 0 else t, k & 1, p=0.02) for k in range(n)], [k & 1 for k in range(n)], lf=2, rf=1, max_qv=93))
    elif family == "snr":
        m0 = api.default_model()
        lo, hi = float(m0.snr_lo), float(m0.snr_hi)
        for k, (snr, model) in enumerate([((lo - 1.5,) * 4, "default"), ((hi + 3.0,) * 4, "default"), ((lo, hi, lo, hi), "default"), ((lo + 0.7, hi - 0.9, 7.3, 11.1), "default"),
                                          ((4.0, 15.0, 9.5, 13.9), "perturbed"), (SNR0, "perturbed")]):
            t = T(int(rng.integers(16, 28)))
            st = [j & 1 for j in range(6)]
            out.append(_case(f"snr{k}", t, [_read(rng, t, s) for s in st], st, lf=int(rng.integers(0, 5)), rf=int(rng.integers(0, 5)), snr=snr, model=model))
    elif family == "ends":
        for lf in range(5):
            rf = (lf * 2 + 1) % 5
            t = T(int(rng.integers(8, 24))); J = len(t)
            st = [j & 1 for j in range(5)]
            out.append(_case(f"flank{lf}{rf}", t, [_read(rng, t, s, p=0.05) for s in st], st, lf=lf, rf=rf, cs=0 if lf == 4 else 2, ce=J if rf == 4 else J - 2))
    elif family == "homopolymer":
        def tr(pre, unit, n, post): return np.array(list(pre) + list(unit) * n + list(post), np.uint8)
        for name, t, lf, rf in [("hp9_closed", tr([1, 2, 3, 1, 0, 2, 1], [3], 9, [0, 1, 2, 0, 3, 1, 2]), 0, 1), ("hp12_open", tr([], [2], 12, [0, 1, 3, 0, 2, 1, 3, 0, 1, 0]), 4, 1),
                              ("di10_closed", tr([0, 3, 1, 3, 0], [1, 2], 5, [0, 0, 3, 1, 2, 3]), 3, 2), ("di14_open", tr([2, 0, 3, 1, 0, 3], [0, 1], 7, []), 1, 4),
                              ("hp7_below", tr([1, 2, 3, 1, 0, 2, 1], [3], 7, [0, 1, 2, 0, 3, 1, 2]), 0, 1)]:
            for n, q in ((6, 50), (12, 93), (12, 50)):
                st = [j & 1 for j in range(n)]
                out.append(_case(f"{name}_np{n}_q{q}", t, [_read(rng, t, s, p=0.0 if q == 93 else 0.03) for s in st], st, lf=lf, rf=rf, max_qv=q))
    else:
        raise KeyError(family)
    return out


FAMILIES = ["limits", "skew", "reverse", "deep", "snr", "ends", "homopolymer"]


# ------------------------------------------------------------------ one case: oracle against reference
def _orient(c, rev):
    """template and left flank a read of this strand is scored against"""
    if not rev: return c["tpl"], c["lf"]
    return A.revcomp(c["tpl"]), (3 - c["rf"] if c["rf"] < 4 else 4)


def _run_case(c):
    m = _model(c["model"])
    snr = np.array(c["snr"], np.float32)
    t32 = O.tables(m, snr); t64 = A.tables64(m, snr)
    tpl, reads, st, lf, rf = c["tpl"], c["reads"], c["strands"], c["lf"], c["rf"]
    ok_len = [len(r) <= A.IMAX for r in reads]
    rr = [r for r, k in zip(reads, ok_len) if k]; ss = [s for s, k in zip(st, ok_len) if k]
    gb = A.read_gains(t64, tpl, lf, rf, rr, ss, banded=True)
    gf = A.read_gains(t64, tpl, lf, rf, rr, ss, banded=False)
    use = A.usable(gb, rr)
    return dict(m=m, t32=t32, t64=t64, rr=rr, ss=ss, gb=gb, gf=gf, use=use, refused=len(reads) - len(rr))


def _check_case(c, S):
    """every assertion of the module docstring on one lab case; S collects the family's counts"""
    X = _run_case(c)
    t32, t64, rr, ss, gb, gf, use = X["t32"], X["t64"], X["rr"], X["ss"], X["gb"], X["gf"], X["use"]
    tpl, lf, rf, J = c["tpl"], c["lf"], c["rf"], len(c["tpl"])
    valid = gb["valid"]; ms = np.flatnonzero(valid)
    n = int(use.sum())
    # -- the window as the oracle polishes it (one scoring round on the template as given)
    out = O.polish_window(*t32, tpl, c["cs"], c["ce"], lf, rf, c["reads"], c["strands"], max_qv=c["max_qv"], qv_only=True)
    assert out["nvalid"] == n, (c["name"], out["nvalid"], n)
    S["reads"] += len(c["reads"]); S["usable"] += n; S["refused"] += X["refused"]
    # -- per read: base likelihood (full sum, alpha and beta), every valid lane (banded; full where the two modes agree)
    scaled = gb["mut"] + 2 * np.array([len(r) for r in rr])[:, None]
    with np.errstate(invalid="ignore"):
        gap = np.abs(gf["mut"] - gb["mut"])
    for r in np.flatnonzero(use):
        t, fl = _orient(c, ss[r]); I = len(rr[r])
        la, lb = A.loglik(t64, t, fl, rr[r])
        assert abs(la - lb) < 1e-9                                    # alpha(I,J) == beta(0,0) in float64 itself
        assert abs(la - gf["base"][r]) < 1e-9                         # the vectorised recurrence is the scalar one
        a, b = O.window_likelihood(*t32, t, fl, rr[r])
        lbd = gb["base"][r]                                            # the same sum over the paths the fill band of v6 keeps
        assert abs(a / 2.0 ** (lbd + 2 * I) - 1) < LIK_TOL and abs(b / 2.0 ** (lbd + 2 * I) - 1) < LIK_TOL, (c["name"], r, a, b, lbd)
        if abs(2.0 ** (la - lbd) - 1) <= 1e-6:
            assert abs(a / 2.0 ** (la + 2 * I) - 1) < LIK_TOL and abs(b / 2.0 ** (la + 2 * I) - 1) < LIK_TOL, (c["name"], r, a, b, la)
        else:
            S["base_beyond_1e6"] += 1; S["base_maxgap"] = max(S["base_maxgap"], la - lbd)
        one = O.polish_window(*t32, tpl, c["cs"], c["ce"], lf, rf, [rr[r]], [ss[r]], qv_only=True)["delta"]
        for mm in ms:
            S["pairs"] += 1
            if not scaled[r, mm] > A.LOG2_TINY:
                S["left_out"] += 1; continue
            d_ref = gb["d"][r, mm]
            # a single-base mutation moves a usable read's likelihood by a few events, far from 2^+-100: the +-100 clamp can bind only where the mutated likelihood is
            # below TINY_P, and those pairs were left out above; a lab case that comes near the clamp is news and is looked at, not absorbed
            assert abs(d_ref) < A.DQ_CLAMP - PER_READ, (c["name"], r, int(mm), float(d_ref))
            assert abs(one[mm] - d_ref) <= PER_READ, (c["name"], "read", r, "lane", int(mm), float(one[mm]), float(d_ref))
            if float(gap[r, mm]) > S["maxgap"]: S["maxgap"], S["maxgap_at"] = float(gap[r, mm]), (c["name"], J, len(rr[r]), int(mm))
            S["disagree_1e6"] += int(abs(2.0 ** (gf["mut"][r, mm] - gb["mut"][r, mm]) - 1) > 1e-6)
            S["touch"] += int(gb["touch"][r, mm]); S["clip"] += int(gb["clip"][r, mm])
        if not ss[r]:                                                  # the forward-strand hook: the likelihood of the lane itself
            for mm in ms:
                if not scaled[r, mm] > A.LOG2_TINY: continue
                res, v, ty, cc, x = O.mutation_likelihood(*t32, tpl, lf, rr[r], int(mm))
                assert v and (ty, cc, x) == (gb["type"][mm], gb["c"][mm], gb["x"][mm])
                assert abs(res / 2.0 ** scaled[r, mm] - 1) < MUT_TOL, (c["name"], r, int(mm))
                if abs(2.0 ** (gf["mut"][r, mm] - gb["mut"][r, mm]) - 1) <= 1e-6:
                    assert abs(res / 2.0 ** (gf["mut"][r, mm] + 2 * len(rr[r])) - 1) < MUT_TOL
    # -- summed over the reads
    d_b = A.deltas(t64, tpl, lf, rf, rr, ss, gains=gb); d_f = A.deltas(t64, tpl, lf, rf, rr, ss, gains=gf)
    bound = n * PER_READ
    clean = np.zeros(256, bool)
    for mm in ms:
        ok = n > 0 and bool(np.all(scaled[use, mm] > A.LOG2_TINY)) and bool(np.all(np.abs(gb["d"][use, mm]) < A.DQ_CLAMP - PER_READ))
        clean[mm] = ok
        if not ok: continue
        S["lanes"] += 1
        assert abs(out["delta"][mm] - d_b[mm]) <= bound, (c["name"], "lane", int(mm), float(out["delta"][mm]), float(d_b[mm]), bound)
        if abs(d_b[mm] - A.MUT_EPS) > bound:
            assert (out["delta"][mm] > np.float32(A.MUT_EPS)) == (d_b[mm] > A.MUT_EPS)
            S["decisions"] += 1
        S["mode_decisions_differ"] += int((d_f[mm] > A.MUT_EPS) != (d_b[mm] > A.MUT_EPS))
    assert not out["delta"][~valid].any()
    # -- QVs of the core
    ph, pf, qv, fl = A.perr(d_b, valid, tpl, lf, rf, c["cs"], c["ce"], n, c["max_qv"])
    assert len(out["perr"]) == c["ce"] - c["cs"] and np.array_equal(out["seq"], tpl[c["cs"]:c["ce"]])
    for k, col in enumerate(range(c["cs"], c["ce"])):
        lanes_c = [s * 32 + col for s in range(8)] + ([s * 32 + J for s in range(4, 8)] if col == J - 1 else [])
        lanes_c = [mm for mm in lanes_c if valid[mm]]
        if n and not all(clean[mm] for mm in lanes_c): continue
        p_lo, p_hi = A.p_bounds(d_b, lanes_c, bound)
        p = float(out["perr"][k])
        if fl[k] >= p_hi:
            assert abs(p / fl[k] - 1) < A.FLOOR_F32, (c["name"], col, p, fl[k])          # a floor that binds on both sides IS the value
            S["floored"] += 1
            S["tract_floor"] += int(fl[k] > A.p_min(c["max_qv"]) * (1 + 1e-9))
        else:
            assert max(p_lo, fl[k] * (1 - A.FLOOR_F32)) <= p <= max(p_hi, fl[k] * (1 + A.FLOOR_F32)), (c["name"], col, p, p_lo, p_hi, fl[k])
            S["bounded"] += 1
        S["bases"] += 1
        assert abs(float(out["qv"][k]) - min(93.0, max(0.0, -10 * np.log10(p)))) < 1e-4
    return X, out


def _stats():
    return dict(reads=0, usable=0, refused=0, pairs=0, left_out=0, lanes=0, decisions=0, bases=0, floored=0, tract_floor=0, maxgap=0.0, disagree_1e6=0,
                mode_decisions_differ=0, touch=0, clip=0, base_beyond_1e6=0, base_maxgap=0.0, maxgap_at=None, bounded=0)


def _report(family, S, ncases):
    share = S["left_out"] / max(1, S["pairs"])
    print(f"\n[{family}] cases {ncases} reads {S['reads']} usable {S['usable']} refused(I>63) {S['refused']} (lane,read) pairs {S['pairs']} left out {S['left_out']} ({100 * share:.2f} %) "
          f"lanes {S['lanes']} decisions {S['decisions']} core bases {S['bases']} floored {S['floored']} (tract {S['tract_floor']}) | full vs banded: max gap "
          f"{S['maxgap']:.2e} log2 at (case, J, I, lane) {S['maxgap_at']}, pairs beyond 1e-6 relative {S['disagree_1e6']}, lanes whose decision differs {S['mode_decisions_differ']} ({100 * S['mode_decisions_differ'] / max(1, S['lanes']):.3f} %) | "
          f"pairs with a scoring row on / off a joint-band limit {S['touch']} / {S['clip']} | reads whose banded fill differs from the full sum by more than 1e-6 relative "
          f"{S['base_beyond_1e6']} (max {S['base_maxgap']:.2e} log2)")
    assert share <= LEFT_OUT_CAP, (family, share)
    assert S["pairs"] > 0 and S["lanes"] > 0 and S["decisions"] > 0 and S["bases"] > 0
    # the band may lose mass pair by pair (printed above, DESIGN.md §2 "Banded link"), but on no lane of the lab does it move a decision: a band change that does turns this red
    assert S["mode_decisions_differ"] == 0, (family, S["mode_decisions_differ"])


def test_tables64_against_oracle_tables(built):
    for snr, model in [(SNR0, "default"), ((1.0, 30.0, 4.0, 20.0), "default"), ((4.0, 15.0, 9.5, 13.9), "perturbed")]:
        ME, INSm, DL = O.tables(_model(model), np.array(snr, np.float32)); t64 = A.tables64(_model(model), snr)
        assert np.abs(ME / 4 / t64[0] - 1).max() < 1e-6 and np.abs(INSm / 4 / t64[1] - 1).max() < 1e-6 and np.abs(DL / t64[2] - 1).max() < 1e-6
        assert np.allclose(t64[0].sum(1) + t64[1].sum(1) + t64[2], 1.0, atol=1e-6)      # (the model's emissions are float32 values)


def test_family_limits(built):
    S = _stats(); cases = lab("limits"); got = {}
    for c in cases:
        X, out = _check_case(c, S)
        got[c["name"]] = (X, out)
    X, out = got["J31_I63"]
    assert [len(r) for r in X["rr"][:6]] == [63, 63, 63, 62, 62, 62] and len(cases[0]["tpl"]) == 31 and X["use"][:3].sum() > 0, "no usable read with I = 63 in a J = 31 window"
    X, _ = got["J31_I5"]
    assert len(cases[1]["tpl"]) == 31 and len(X["rr"][0]) == 5 and len(X["rr"][1]) == 5          # (26 deleted columns: both sides must agree whether such a read is usable)
    assert not X["use"][:2].any()
    X, _ = got["J31_smallI"]
    small = sorted(len(r) for r, u in zip(X["rr"], X["use"]) if u)
    print("\n[limits] J31_smallI: lengths of the usable reads of a J = 31 window:", small, "of", sorted(len(r) for r in X["rr"]))
    assert len(got["J31_smallI"][0]["rr"]) == 15 and small and small[0] <= 10, "no usable read with I <= 10 in a J = 31 window"
    X, out = got["J5"]
    assert len(cases[3]["tpl"]) == 5 and X["use"].sum() > 0
    X, out = got["I0_I64"]
    assert X["refused"] == 1 and len(X["rr"][0]) == 0 and out["nvalid"] == int(X["use"].sum()) <= 6, "I = 64 must be refused"
    _report("limits", S, len(cases))


def test_family_skew(built):
    S = _stats(); cases = lab("skew"); dij = set(); touched = 0
    for c in cases:
        X, _ = _check_case(c, S)
        for r in np.flatnonzero(X["use"]):
            d = abs(len(X["rr"][r]) - len(c["tpl"]))
            if d >= 4:
                dij.add(d); touched += int(X["gb"]["touch"][r].any())
    print("\n[skew] |I - J| of usable reads:", sorted(dij))
    assert min(dij) <= 5 and max(dij) >= 30 and len(dij) >= 8 and any(18 <= d <= 23 for d in dij) and any(24 <= d <= 29 for d in dij), sorted(dij)
    assert touched > 0 and S["clip"] > 0, "no scoring band was clamped into a corner of its window"
    _report("skew", S, len(cases))


def test_family_reverse(built):
    S = _stats(); cases = lab("reverse")
    for c in cases:
        X, out = _check_case(c, S)
        if not c["name"].startswith("allrev"): continue
        # the same reads given as forward reads of rc(tpl): the gains must map lane for lane (by the explicit mutated template)
        t2, J = A.revcomp(c["tpl"]), len(c["tpl"])
        lf2, rf2 = (3 - c["rf"] if c["rf"] < 4 else 4), (3 - c["lf"] if c["lf"] < 4 else 4)
        out2 = O.polish_window(*X["t32"], t2, J - c["ce"], J - c["cs"], lf2, rf2, c["reads"], [0] * len(c["reads"]), qv_only=True)
        v1, ty1, c1, x1 = A.lanes(c["tpl"]); v2, ty2, c2, x2 = A.lanes(t2)
        image = {A.mutate(t2, ty2[m], c2[m], x2[m]).tobytes(): m for m in np.flatnonzero(v2)}
        nmap = 0
        for m in np.flatnonzero(v1):
            m2 = image[A.revcomp(A.mutate(c["tpl"], ty1[m], c1[m], x1[m])).tobytes()]
            same_site = c2[m2] == (J - c1[m] if ty1[m] == A.INS else J - 1 - c1[m])      # (a run admits its indel at its first base in EACH orientation: another column, the same template)
            if same_site: assert out["delta"][m] == out2["delta"][m2], (c["name"], int(m), int(m2))
            else: assert abs(out["delta"][m] - out2["delta"][m2]) <= 2 * len(c["reads"]) * PER_READ
            nmap += 1
        assert nmap == int(v1.sum()) == int(v2.sum())
    assert sum(all(c["strands"]) for c in cases) >= 3 and sum(0 < sum(c["strands"]) < len(c["strands"]) for c in cases) >= 3
    _report("reverse", S, len(cases))


def test_family_deep(built):
    S = _stats(); cases = lab("deep"); unfloored = {}; before = 0
    for c in cases:
        X, out = _check_case(c, S)
        assert out["nvalid"] >= len(c["reads"]) - 3
        if c["name"].startswith("split"): unfloored[len(c["reads"])] = S["bounded"] - before
        before = S["bounded"]
    assert sorted({len(c["reads"]) for c in cases}) == [33, 64, 96]
    print("\n[deep] core bases held to the propagated p_err bound (no floor binding), by read count:", unfloored)
    assert sorted(unfloored) == [33, 64, 96] and min(unfloored.values()) >= 1, "the propagated bound on p_err was not exercised at 33 / 64 / 96 reads (every base floored)"
    _report("deep", S, len(cases))


def test_family_snr(built):
    S = _stats(); cases = lab("snr")
    m0 = api.default_model()
    assert any(max(c["snr"]) < m0.snr_lo for c in cases) and any(min(c["snr"]) > m0.snr_hi for c in cases) and any(c["model"] == "perturbed" for c in cases)
    assert any(len(set(c["snr"])) == 4 for c in cases) and any(set(c["snr"]) == {float(m0.snr_lo), float(m0.snr_hi)} for c in cases)
    for c in cases: _check_case(c, S)
    _report("snr", S, len(cases))


def test_family_ends(built):
    S = _stats(); cases = lab("ends")
    assert sorted(c["lf"] for c in cases) == [0, 1, 2, 3, 4] and sorted(c["rf"] for c in cases) == [0, 1, 2, 3, 4]
    for c in cases:
        J = len(c["tpl"]); v = A.lanes(c["tpl"])[0]
        assert all(v[s * 32 + col] for s in range(3) for col in (0, 1, J - 2, J - 1)) and v[3 * 32 + 0] and any(v[s * 32 + J] for s in range(4, 8)) and any(v[s * 32] for s in range(4, 8))
        _check_case(c, S)
    _report("ends", S, len(cases))


def test_family_homopolymer(built):
    S = _stats(); cases = lab("homopolymer"); seen = set()
    for c in cases:
        X, out = _check_case(c, S)
        n = int(X["use"].sum())
        vis = ([c["lf"]] if c["lf"] < 4 else []) + list(c["tpl"]) + ([c["rf"]] if c["rf"] < 4 else [])
        fls = [A.tract_floor(vis, col + (c["lf"] < 4), n) for col in range(c["cs"], c["ce"])]
        top = max(fls)
        if c["name"].startswith("hp7"): assert top == 0.0
        else:
            L = {"hp9": 9, "hp12": 12, "di10": 10, "di14": 14}[c["name"].split("_")[0]]
            closed = "closed" in c["name"]
            assert abs(top - 0.2 / L * ((100.0 / (n * n)) if closed and n > 10 else 1.0)) < 1e-12, (c["name"], top, n)
            seen.add((c["name"].split("_")[0], closed, n > 10))
            k = int(np.argmax(fls))
            if top > A.p_min(c["max_qv"]) and c["max_qv"] == 93: assert abs(out["perr"][k] / top - 1) < 3e-7      # clean reads: the tract floor is what is reported
    assert len(seen) == 8 and S["tract_floor"] > 0
    _report("homopolymer", S, len(cases))


def test_zparams_closed_form_and_monte_carlo(built):
    """MU / VAR of the z-score gate: orc_zparams (float32, det_log2) against the float64 closed form, and the closed form against reads GENERATED by the model.
    Measured (python -m pytest tests/test_arrow_ref.py -q -s -k zparams): largest relative error of the oracle MU 1.33e-07, VAR 3.40e-07 over the SNR vectors and the
    two models below; asserted at 4x (float32 evaluation order and det_log2 are the only differences; 4x covers another libm / compiler)."""
    rng = np.random.default_rng(11)
    worst_mu = worst_var = 0.0
    for snr, model in [(SNR0, "default"), ((3.0, 30.0, 6.0, 11.0), "default"), ((4.0, 15.0, 9.5, 13.9), "perturbed")]:
        m = _model(model)
        MU, VAR = O.zparams(m, np.array(snr, np.float32)); mu64, var64 = A.zmoments(m, snr)
        worst_mu = max(worst_mu, float(np.abs(MU / mu64 - 1).max())); worst_var = max(worst_var, float(np.abs(VAR / var64 - 1).max()))
        for k in (0, 5, 10, 15, 6):
            x = A.sample_position_loglik(m, snr, k, 400000, rng)
            n = len(x); mean, var = x.mean(), x.var()
            se_mean = np.sqrt(var / n); se_var = np.sqrt((np.mean((x - mean) ** 4) - var * var) / n)
            assert abs(mean - mu64[k]) < 4 * se_mean, ("MU", snr, k, mean, mu64[k], se_mean)
            assert abs(var - var64[k]) < 4 * se_var, ("VAR", snr, k, var, var64[k], se_var)
    print(f"\n[zparams] largest relative error oracle vs float64 closed form: MU {worst_mu:.2e} VAR {worst_var:.2e}")
    assert worst_mu < 4 * 1.33e-7 and worst_var < 4 * 3.40e-7


def test_stage_entry_points_do_not_inherit_the_floor_of_an_earlier_zmw(built):
    """orc_polish_window used to report with the max_qv of whatever whole-ZMW call ran last on the thread"""
    rng = np.random.default_rng(3)
    t = rng.integers(0, 4, 24).astype(np.uint8)
    reads = [_read(rng, t, k & 1, p=0.0) for k in range(8)]; st = [k & 1 for k in range(8)]
    t32 = O.tables(api.default_model(), np.array(SNR0, np.float32))
    alone = O.polish_window(*t32, t, 2, 22, 4, 4, reads, st)
    assert abs(alone["perr"].min() - 1e-5) < 1e-12 and alone["qv"].max() == pytest.approx(50.0, abs=1e-3)
    o = api.default_opts(); o.max_qv = 30; o.min_rq = 0.0
    b = api.synth(2, 5, 300, seed=4)
    O.consensus_batch(api.default_model(), o, b, api.Results.allocate(b), nthreads=1)
    after = O.polish_window(*t32, t, 2, 22, 4, 4, reads, st)
    assert np.array_equal(after["perr"], alone["perr"]) and np.array_equal(after["qv"], alone["qv"])
    q93 = O.polish_window(*t32, t, 2, 22, 4, 4, reads, st, max_qv=93)
    assert q93["perr"].min() < 1e-6
    assert np.array_equal(O.polish_window(*t32, t, 2, 22, 4, 4, reads, st)["perr"], alone["perr"])

"""k_polish_t against the float64 restatement of tests/arrow_ref.py (banded mode), through the existing polish seam (ccsx_polish_batch, heuristics and z-score gate
off, the draft handed in).  A lab batch plants the shapes the kernel has limits for — I = 63 in a J = 30 window, segments of 64 and more bases (refused with
trimming off, trimmed at the default), |I - J| of 8 .. 33, 40 and 96 passes (two and three groups of 32 reads), a ZMW whose usable passes are all reverse, SNR below
and above the model's range, homopolymer and dinucleotide tracts — and every test ASSERTS from the engine's own stage outputs (tests/arrow_ref.py collect_stage) that
the run contained them.  A window of a QV_ONLY run has at most 30 columns (a core of at most 28 at the draft's end plus one overhang, DESIGN.md §2 "Windows"): J = 31
exists only after an insertion has been applied, i.e. in the full-polish test.  Nothing here reads anything outside the repository."""
import time

import numpy as np
import pytest

from ccs_amd import api
import arrow_ref as A
import oracle_lib as O

pytestmark = pytest.mark.gpu
SNR0 = (9.0, 16.0, 8.0, 13.0)


def _noisy(rng, t, p):
    r = []
    for b in t:
        while rng.random() < p: r.append(int(rng.integers(0, 4)))
        if rng.random() < p: continue
        r.append(int(b) if rng.random() > p / 2 else int(rng.integers(0, 4)))
    return np.array(r, np.uint8)


def _template(rng, lo, want_j30=False, inserts=()):
    """random template of about `lo` bases (with `inserts` = (position, bases) planted first) whose last window has 30 columns if asked; returns (tpl, window bounds)"""
    for L in range(lo, lo + 60):
        t = rng.integers(0, 4, L).astype(np.uint8)
        for at, b in inserts: t[at:at + len(b)] = b
        wb = O.windows(t)
        if not want_j30 or (L - int(wb[-2]) + 2 == 30): return t, wb
    raise AssertionError("no template with a 30-column last window")


def lab_batch(model, seed=5):
    """(batch, templates): six ZMWs, one planted shape each (see the comments below); planted on purpose, not the CPU lab's windows joined by spacers — the evidence
    assertions of the tests say what reached the kernel"""
    rng = np.random.default_rng(seed)
    lo_snr = (4.0,) * 4
    t64 = A.tables64(model, lo_snr)
    zs = []          # (template, snr, [(bases, pw, strand)])

    def passes(tpl, n, p, edits=None, pw_fixed=None, strands=None):
        out = []
        for k in range(n):
            t = list(tpl)
            for at, ins, cut in sorted((edits or {}).get(k, []), reverse=True):
                t = t[:at] + [int(tpl[at])] * ins + t[at + cut:]
            clean = k in (edits or {})
            b = np.array(t, np.uint8) if clean else _noisy(rng, t, p)
            st = (k & 1) if strands is None else strands[k]
            if st: b = A.revcomp(b)
            pw = np.full(len(b), pw_fixed, np.uint8) if (clean and pw_fixed) else rng.integers(1, 4, len(b)).astype(np.uint8)
            out.append((b, pw, st))
        return out

    mid = lambda wb, w: (int(wb[w]) + int(wb[w + 1])) // 2
    # z0 skew: inserted blocks of copies of the base that follows (branch events: anything else falls below TINY_P), low SNR; the last window has J = 30, + 33 = I 63
    t, wb = _template(rng, 176, want_j30=True); nw = len(wb) - 1
    # (33 branch events leave the segment about 4 bits above TINY_P only where they are cheapest: the site and the pulse-width bin are chosen by the reference itself)
    ws = int(wb[nw - 1]) - 2; best = (-np.inf, 0, 1)
    for at in range(int(wb[nw - 1]) + 2, len(t) - 3):
        for b in (1, 2, 3):
            seg = np.concatenate([t[ws:at], np.full(33, t[at]), t[at:]])
            best = max(best, (A.loglik(t64, t[ws:], int(t[ws - 1]), A.obs_codes(seg, np.full(len(seg), b)))[0] + 2 * len(seg), at, b))
    assert best[0] > A.LOG2_TINY + 2.0, best
    at63, pw_best = best[1], best[2]
    e = {1: [(mid(wb, 1), 8, 0), (mid(wb, 5), 26, 0)], 2: [(mid(wb, 3), 14, 0), (at63, 33, 0)], 3: [(at63, 33, 0)], 4: [(mid(wb, 5), 26, 0)], 5: [(mid(wb, 1), 8, 0)], 6: [(at63, 33, 0)]}
    zs.append((t, lo_snr, passes(t, 8, 0.02, e, pw_best)))
    # z1 limits: a block of 45 (segments of 64 and more bases) and a deleted stretch of 12
    t, wb = _template(rng, 150)
    e = {1: [(mid(wb, 2), 45, 0)], 2: [(mid(wb, 2), 45, 0), (mid(wb, 5) - 6, 0, 12)], 3: [(mid(wb, 5) - 6, 0, 12)]}
    zs.append((t, lo_snr, passes(t, 8, 0.02, e, pw_best)))
    # z2 / z3 deep: three and two groups of 32 reads; SNR above / below the model's range
    t, _ = _template(rng, 118); zs.append((t, (model.snr_hi + 5.0,) * 4, passes(t, 96, 0.03)))
    t, _ = _template(rng, 118); zs.append((t, (model.snr_lo - 2.0,) * 4, passes(t, 40, 0.03)))
    # z4 reverse: the forward pass is junk (it fails the alignment), every usable pass is reverse
    t, _ = _template(rng, 130)
    ps = passes(t, 8, 0.03, strands=[0] + [1] * 7)
    ps[0] = (rng.integers(0, 4, len(t)).astype(np.uint8), np.full(len(t), 2, np.uint8), 0)
    zs.append((t, SNR0, ps))
    # z5 tracts: a homopolymer of 9 and (CG)6 inside windows, 12 passes, four distinct channel values
    t, _ = _template(rng, 150, inserts=[(30, [3] * 9), (96, [1, 2] * 6)])
    zs.append((t, (5.5, 17.0, 7.3, 11.1), passes(t, 12, 0.02)))
    n = len(zs)
    reads = [r for _, _, ps in zs for r in ps]
    batch = api.Batch(np.arange(n, dtype=np.int32), np.array([s for _, s, _ in zs], np.float32), np.concatenate([[0], np.cumsum([len(ps) for _, _, ps in zs])]).astype(np.int32),
                      np.concatenate([[0], np.cumsum([len(r[0]) for r in reads])]).astype(np.int64), np.ascontiguousarray(np.concatenate([r[0] for r in reads])),
                      np.ascontiguousarray(np.concatenate([r[1] for r in reads])), np.full(sum(len(r[0]) for r in reads), 5, np.uint8), np.array([r[2] for r in reads], np.uint8))
    return batch, [t for t, _, _ in zs]


def reference_windows(model, batch, wins):
    """per window of collect_stage's output the banded float64 gains (the expensive part: shared by the max_qv settings of a run)"""
    out = {}
    for z, ws in wins.items():
        t64 = A.tables64(model, batch.snr[z]); out[z] = []
        for w in ws:
            rr = [r for r in w["reads"] if r is not None]; ss = [s for r, s in zip(w["reads"], w["strands"]) if r is not None]
            g = A.read_gains(t64, w["tpl"], w["lf"], w["rf"], rr, ss, banded=True)
            use = A.usable(g, rr)
            out[z].append(dict(rr=rr, ss=ss, g=g, use=use, n=int(use.sum()), d=A.deltas(t64, w["tpl"], w["lf"], w["rf"], rr, ss, gains=g)))
    return out


def check_raw_qvs(raw, wins, refs, max_qv, S):
    """every core base's raw QV inside the propagated bound of its banded float64 error probability (or ON the floor where a floor binds on both sides)"""
    pos = 0
    for w, R in zip(wins, refs):
        g, n, d, use = R["g"], R["n"], R["d"], R["use"]; bound = n * A.PER_READ
        scaled = g["mut"] + 2 * np.array([len(r) for r in R["rr"]], np.int64).reshape(-1, 1)
        valid, J = g["valid"], len(w["tpl"])
        clean = np.array([n > 0 and bool(np.all(scaled[use, m] > A.LOG2_TINY)) and bool(np.all(np.abs(g["d"][use, m]) < A.DQ_CLAMP - A.PER_READ)) for m in range(256)])
        _, _, _, fl = A.perr(d, valid, w["tpl"], w["lf"], w["rf"], w["cs"], w["ce"], n, max_qv)
        for k, col in enumerate(range(w["cs"], w["ce"])):
            q = float(raw[pos]); pos += 1
            lanes_c = A.base_lanes(valid, col, J)
            S["bases"] += 1
            if n and not all(clean[m] for m in lanes_c):
                S["left_out"] += 1; continue
            p_lo, p_hi = A.p_bounds(d, lanes_c, bound)
            p_lo, p_hi = max(p_lo, fl[k] * (1 - A.FLOOR_F32)), max(p_hi, fl[k] * (1 + A.FLOOR_F32))
            # raw QV = -3.01029996 log2 p with det_log2 (2e-5 absolute: tests/test_oracle_hmm.py::test_det_log2_exp2_accuracy), float32 rounding of a value <= 93
            slack = 3.0103 * 2e-5 + 1e-5
            q_hi = min(93.0, max(0.0, -10 * np.log10(p_lo))) + slack; q_lo = min(93.0, max(0.0, -10 * np.log10(p_hi))) - slack
            assert q_lo <= q <= q_hi, (w["ws"], col, q, q_lo, q_hi, n)
            S["unfloored"] += int(fl[k] < p_lo)
    assert pos == len(raw)


def evidence(wins, refs):
    """what the run contained, from the engine's stage outputs and the reference's usable sets"""
    E = dict(maxJ=0, I63_used=0, I64_dropped=0, trimmed=0, skew8_used=0, skew_max=0, over32=0, over64=0, all_reverse=0, first_noflank=0, last_noflank=0, small_I_used=0)
    for z in wins:
        for wi, (w, R) in enumerate(zip(wins[z], refs[z])):
            J = len(w["tpl"]); E["maxJ"] = max(E["maxJ"], J)
            E["I64_dropped"] += sum(1 for r, n in zip(w["reads"], w["n_raw"]) if r is None and n >= 64)
            E["trimmed"] += w["trimmed"]
            lens = [len(r) for r, u in zip(R["rr"], R["use"]) if u]
            E["I63_used"] += sum(1 for i in lens if i == 63)
            E["skew8_used"] += sum(1 for i in lens if abs(i - J) >= 8); E["skew_max"] = max([E["skew_max"]] + [abs(i - J) for i in lens])
            E["small_I_used"] += sum(1 for i in lens if J - i >= 8)
            E["over32"] += int(32 < R["n"] <= 64); E["over64"] += int(R["n"] > 64)
            st = [s for s, u in zip(R["ss"], R["use"]) if u]
            E["all_reverse"] += int(len(st) >= 3 and all(st))
            E["first_noflank"] += int(wi == 0 and w["lf"] == 4); E["last_noflank"] += int(wi == len(wins[z]) - 1 and w["rf"] == 4)
    E["z0_last"] = [(n, len(r) if r is not None else None) for r, n in zip(wins[0][-1]["reads"], wins[0][-1]["n_raw"])] if 0 in wins else None     # (segment cut, length scored)
    return E


@pytest.mark.parametrize("maxins", [-1, 0])
def test_lab_batch_qv_only(built, maxins):
    """The lab batch, templates handed in as drafts, CCSX_QV_ONLY, max_qv 50 and 93 on the SAME segments, max_insertion_size -1 (a segment of 64 and more bases is
    refused) and the default (it is trimmed): (a) bit-exact against the CPU restatement, (b) raw QVs against the banded float64 reference on the segments the engine
    cut, (c) the evidence.  CPU time of the float64 reference: printed (8 s for the 38 windows; python -m pytest tests/test_arrow_gpu.py -s -m gpu)."""
    model = api.default_model()
    batch, tpls = lab_batch(model)
    refs = None
    for max_qv in (50, 93):
        o = api.default_opts(); o.disable_heuristics = 1; o.min_rq = 0.0; o.min_zscore = 0.0; o.top_passes = 0; o.max_qv = max_qv; o.max_insertion_size = maxins
        h = api.Handle(0, model=model, opts=o)
        try:
            d = api.Drafts.allocate(batch)
            for z, t in enumerate(tpls): d.set_draft(z, t, backbone=0)
            res = h.polish(batch, d, flags=api.QV_ONLY)
            wins = A.collect_stage(h, batch, range(batch.n_zmw), max_insertion_size=maxins)
            for z, t in enumerate(tpls):
                assert np.array_equal(h.stage_windows(z), O.windows(t)), f"zmw {z}: the windows are not those the lab was built on"
            O.counts_reset()
            ref = O.polish_batch(model, o, batch, d, api.Results.allocate(batch), flags=api.QV_ONLY)
            cnt = O.counts()
        finally:
            h.close()
        if refs is None:
            t0 = time.time(); refs = reference_windows(model, batch, wins); t_ref = time.time() - t0
        S = dict(bases=0, left_out=0, unfloored=0)
        for z in range(batch.n_zmw):
            assert res.status[z] == ref.status[z] and res.np_[z] == ref.np_[z] and np.array_equal(res.sequence(z), tpls[z]) and np.array_equal(ref.sequence(z), tpls[z])
            assert np.array_equal(res.raw(z), ref.raw(z)), f"zmw {z}: raw QVs differ from the CPU restatement"
            check_raw_qvs(res.raw(z), wins[z], refs[z], max_qv, S)
            # the engine used the reads the reference calls usable: ec is its mean count of usable reads per window
            assert abs(float(res.ec[z]) - np.mean([R["n"] for R in refs[z]])) < 1e-3, (z, float(res.ec[z]), [R["n"] for R in refs[z]])
        E = evidence(wins, refs)
        print(f"\n[arrow gpu lab] max_qv {max_qv} max_insertion_size {maxins}: {S} evidence {E} oracle counts trim {cnt['trim']} zdrop {cnt['zdrop']} "
              f"float64 reference {t_ref:.1f} s")
        assert S["left_out"] <= 0.02 * S["bases"] and S["unfloored"] > 0
        assert E["maxJ"] == 30 and E["skew8_used"] > 0 and E["skew_max"] >= 26 and E["small_I_used"] > 0
        assert E["over32"] > 0 and E["over64"] > 0 and E["all_reverse"] > 0 and E["first_noflank"] == batch.n_zmw and E["last_noflank"] == batch.n_zmw
        # the oracle took the same paths: it trimmed exactly the segments the engine's stage outputs say were trimmed, and dropped nothing by z-score
        assert cnt["trim"] == E["trimmed"] and cnt["zdrop"] == 0
        cut63 = sum(1 for n, _ in E["z0_last"] if n == 63)
        if maxins < 0: assert E["I64_dropped"] > 0 and E["trimmed"] == 0 and E["I63_used"] > 0 and E["skew_max"] == 33
        else: assert E["trimmed"] > 0 and E["I64_dropped"] == 0 and cut63 > 0 and all(i == 30 for n, i in E["z0_last"] if n == 63)     # 63 > 30 + 30: the same segments, trimmed to J


def _with_errors(rng, t):
    """a draft: the template with a substitution, a deleted and an inserted base, each about 45 bases apart"""
    d = [int(b) for b in t]
    for k, at in enumerate(range(len(d) - 20, 20, -45)):
        if k % 3 == 0: d[at] = (d[at] + 1 + int(rng.integers(0, 3))) & 3
        elif k % 3 == 1: del d[at]
        else: d.insert(at, int(rng.integers(0, 4)))
    return np.array(d, np.uint8)


def test_lab_batch_full_polish(built):
    """The same batch through the full polish (heuristics off), drafts = the templates with planted errors: bit-exact against the CPU restatement, and window by window the
    core the engine reports equals the greedy result of the float64 reference (arrow_ref.polish_ref) wherever every decision of the reference lies outside the delta
    bound; the share of windows left out for sitting inside it is printed and capped at 5 %."""
    model = api.default_model()
    batch, tpls = lab_batch(model)
    rng = np.random.default_rng(17)
    drafts = [_with_errors(rng, t) for t in tpls]
    o = api.default_opts(); o.disable_heuristics = 1; o.min_rq = 0.0; o.min_zscore = 0.0; o.top_passes = 0; o.max_insertion_size = -1
    h = api.Handle(0, model=model, opts=o)
    try:
        d = api.Drafts.allocate(batch)
        for z, t in enumerate(drafts): d.set_draft(z, t, backbone=0)
        res = h.polish(batch, d)
        wins = A.collect_stage(h, batch, range(batch.n_zmw), max_insertion_size=-1)
        ref = O.polish_batch(model, o, batch, d, api.Results.allocate(batch))
    finally:
        h.close()
    nwin = amb = maxJ = 0; t0 = time.time()
    for z in range(batch.n_zmw):
        assert res.status[z] == ref.status[z] and np.array_equal(res.sequence(z), ref.sequence(z)) and np.array_equal(res.raw(z), ref.raw(z)), f"zmw {z}: differs from the CPU restatement"
        t64 = A.tables64(model, batch.snr[z]); t32 = O.tables(model, batch.snr[z])
        seq = res.sequence(z); pos = 0
        for w in wins[z]:
            rr = [r for r in w["reads"] if r is not None]; ss = [s for r, s in zip(w["reads"], w["strands"]) if r is not None]
            core, rounds, ambiguous = A.polish_ref(t64, w["tpl"], w["lf"], w["rf"], w["cs"], w["ce"], rr, ss)
            nwin += 1
            if ambiguous:
                # (only to find where the next window starts: the length of this window's core as the CPU restatement polishes it; the engine equals it bit for bit above)
                amb += 1; pos += len(O.polish_window(*t32, w["tpl"], w["cs"], w["ce"], w["lf"], w["rf"], w["reads"], w["strands"])["seq"]); continue
            assert np.array_equal(seq[pos:pos + len(core)], core), (z, w["ws"], rounds)
            pos += len(core); maxJ = max(maxJ, len(w["tpl"]) + (len(core) - (w["ce"] - w["cs"])))
        assert pos == len(seq), (z, pos, len(seq))
        assert O.edit_distance(seq, tpls[z]) <= O.edit_distance(drafts[z], tpls[z])
    print(f"\n[arrow gpu lab] full polish: {nwin} windows, {amb} left out as ambiguous ({100 * amb / nwin:.1f} %), largest polished window J {maxJ}, float64 reference {time.time() - t0:.1f} s")
    assert amb <= 0.05 * nwin
    assert maxJ == 31, "no window reached JMAX columns through an applied insertion"


def _opts(max_qv=50, maxins=0):
    o = api.default_opts(); o.disable_heuristics = 1; o.min_rq = 0.0; o.min_zscore = 0.0; o.top_passes = 0; o.max_qv = max_qv; o.max_insertion_size = maxins
    return o


def _qv_only_on_fused(model, o, batch, zs):
    """the engine's own consensus (its drafts, not handed-in ones) scored again with CCSX_QV_ONLY: every ZMW bit-exact against the CPU restatement, ZMWs `zs` per base
    against the banded float64 reference on every window.  Returns (counts, seconds the reference took, seconds the CPU restatement took)."""
    h = api.Handle(0, model=model, opts=o)
    try:
        fused = h.consensus(batch)
        d = api.Drafts.allocate(batch)
        for z in range(batch.n_zmw): d.set_draft(z, fused.sequence(z), backbone=0)
        res = h.polish(batch, d, flags=api.QV_ONLY)
        wins = A.collect_stage(h, batch, zs, max_insertion_size=o.max_insertion_size)
    finally:
        h.close()
    t0 = time.time()
    ref = O.polish_batch(model, o, batch, d, api.Results.allocate(batch), flags=api.QV_ONLY)
    t_orc = time.time() - t0
    for z in range(batch.n_zmw):
        assert res.status[z] == ref.status[z] and np.array_equal(res.sequence(z), ref.sequence(z)) and np.array_equal(res.sequence(z), fused.sequence(z))
        assert np.array_equal(res.raw(z), ref.raw(z)), f"zmw {z}: raw QVs differ from the CPU restatement"
    t0 = time.time(); refs = reference_windows(model, batch, wins); t_ref = time.time() - t0
    S = dict(bases=0, left_out=0, unfloored=0, windows=sum(len(w) for w in wins.values()))
    for z in zs:
        assert len(fused.sequence(z)) > 0
        check_raw_qvs(res.raw(z), wins[z], refs[z], o.max_qv, S)
        assert abs(float(res.ec[z]) - np.mean([R["n"] for R in refs[z]])) < 1e-3, (z, float(res.ec[z]))
    assert S["left_out"] <= 0.02 * S["bases"]
    return S, t_ref, t_orc


def test_second_model_and_snr_at_the_range_limits(built):
    """A perturbed parameter set (api.model_from_json; SNR range 5 .. 14) on the device: ZMWs whose SNR sits exactly at snr_lo, exactly at snr_hi, at both by channel, and
    inside the range with four distinct values, max_qv 93 so that few bases hide behind the floor."""
    model = api.model_from_json(A.perturbed_model_json(api.model_to_json(api.default_model())))
    lo, hi = float(model.snr_lo), float(model.snr_hi)
    assert (lo, hi) == (5.0, 14.0)
    batch = api.synth(4, 8, 400, seed=71)
    batch.snr[:] = np.array([(lo,) * 4, (hi,) * 4, (lo, hi, hi, lo), (6.1, 13.2, 8.4, 10.9)], np.float32)
    S, t_ref, _ = _qv_only_on_fused(model, _opts(max_qv=93), batch, range(4))
    print(f"\n[arrow gpu] second model: {S} float64 reference {t_ref:.1f} s")
    assert S["windows"] >= 60 and S["unfloored"] > 100


def test_c2_shape_qv_only_on_the_fused_consensus(built):
    """BASELINE c2 size (64 ZMWs, 10 passes x 10 kb, api.synth): CCSX_QV_ONLY on the engine's fused consensus, all 64 ZMWs bit-exact against the CPU restatement, raw QVs of
    EVERY window of one ZMW (about 450 windows, 10 000 bases) against the banded float64 reference.  Measured (python -m pytest tests/test_arrow_gpu.py -s -m gpu -k c2
    --durations=8, and -k headline_size of tests/test_gpu_parity.py, on a 16-CPU MI355X box): the float64 reference takes 76 s per 10 kb ZMW on one core (152 s for two ZMWs,
    0.17 s per window); the CPU restatement's QV_ONLY pass over all 64 ZMWs takes 5.2 s on one thread, and test_headline_size_matches_oracle as a whole 0.3 s of wall time
    with 16 threads.  The restatement is thus two orders of magnitude cheaper than the reference: NO whole ZMW fits below what the headline test spends in it, so the case is
    sized at the smallest meaningful number, one ZMW; the shorter cases of this file carry the breadth.  Both times are printed."""
    batch = api.synth(64, 10, 10000, seed=0xC2)
    S, t_ref, t_orc = _qv_only_on_fused(api.default_model(), _opts(), batch, [40])
    print(f"\n[arrow gpu] c2 shape: {S} float64 reference {t_ref:.1f} s for 1 ZMW, CPU restatement (QV_ONLY, 64 ZMWs, one thread) {t_orc:.1f} s")
    assert S["windows"] >= 400 and S["bases"] >= 9500

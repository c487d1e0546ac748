"""The candidate filter and the z-score gate of DESIGN.md §2: the float64 reference (tests/arrow_ref.py filter_margins, filtered_lanes, travel, zscore, polish_ref) against
itself, and the CPU restatement (oracle/ccs_oracle.c through oracle_lib.polish_batch, DEFAULT options: heuristics on, z-score gate on) against the reference on the filter
lab (tests/filter_lab.py), window by window: core sequence, raw QVs — a base the reference calls skipped must report its p_skip, every other base must lie inside the
propagated bound, a quiet base's sum starting at p_skip — usable counts, rounds.  No GPU.  The three left-out shares are printed (-s) and capped."""
import time

import numpy as np
import pytest

from ccs_amd import api
import arrow_ref as A
import filter_lab as F
import oracle_lib as O


def test_filter_margins_is_the_definition():
    """g, ev and p_skip against a literal second restatement (sets of positions, counts of clean and dirty passes) on random small inputs, the thresholds among them"""
    rng = np.random.default_rng(7)
    seen = set()
    for trial in range(300):
        J = int(rng.integers(1, 32)); R = int(rng.integers(0, 20))
        use = [bool(rng.random() < 0.8) for _ in range(R)]
        rows = [[int(rng.random() < (0.5 if rng.random() < 0.1 else 0.08)) for _ in range(J)] for _ in range(R)]
        for r in range(R):
            if rng.random() < 0.1: rows[r] = [1] * J                        # a split or partial pass
        max_qv = (50, 93, 0, 30)[trial % 4]
        g, ev, ps = A.filter_margins(rows, use, J, max_qv)
        for c in range(J):
            clean = sum(1 for r in range(R) if use[r] and not rows[r][c]); dirty = sum(1 for r in range(R) if use[r] and rows[r][c])
            assert g[c] == clean - dirty
            majority = {q for q in range(J) if sum(1 for r in range(R) if use[r] and rows[r][q]) * 2 > sum(use)}
            want = clean - dirty >= 6 and not any(abs(q - c) <= 3 for q in majority)
            assert ev[c] == want, (trial, c)
            if g[c] >= 0: assert ps[c] == max(8.0 / 8.0 ** min(g[c], 12), 10.0 ** (-(max_qv or 50) / 10.0))
            seen.add(("g", min(g[c], 13)))
            if want: seen.add("ev")
            if clean - dirty >= 6 and not want: seen.add("spread")
    assert {("g", 5), ("g", 6), ("g", 12), ("g", 13), "ev", "spread"} <= seen
    assert A.filter_margins([[0] * 4] * 5, [True] * 5, 4)[1] == [False] * 4 and A.filter_margins([[0] * 4] * 6, [True] * 6, 4)[1] == [True] * 4      # fewer than 6 passes: nothing
    g, ev, _ = A.filter_margins([[0, 0, 0, 0, 1, 0, 0, 0, 0]] * 4 + [[0] * 9] * 3, [True] * 7, 9)                                                  # 3 against 4 columns away
    assert g[4] == -1 and ev == [True] + [False] * 7 + [True]


def _noisy(rng, t, p):
    r = []
    for b in t:
        while rng.random() < p: r.append(int(rng.integers(0, 4)))
        if rng.random() < p: continue
        r.append(int(b) if rng.random() > p / 2 else int(rng.integers(0, 4)))
    return np.array(r, np.uint8)


def _frozen_polish(tabs, tpl, lf, rf, cs, ce, reads, strands):
    """the unfiltered polish loop as it stood before evidence and the z-score gate were added to arrow_ref.polish_ref: a frozen copy, kept to hold the rewrite to it"""
    t = np.asarray(tpl, np.uint8).copy(); amb = False; it = 0
    for it in range(8):
        g = A.read_gains(tabs, t, lf, rf, reads, strands, banded=True)
        n = int(A.usable(g, reads).sum()); bound = n * A.PER_READ
        d = A.deltas(tabs, t, lf, rf, reads, strands, gains=g)
        valid = g["valid"]
        amb = amb or bool(np.any(valid & (np.abs(d - A.MUT_EPS) <= bound)))
        cand = valid & (d > A.MUT_EPS)
        if not cand.any() or it == 7: break
        acc, Jn = [], len(t)
        while cand.any():
            bm = int(np.argmax(np.where(cand, d, -np.inf)))
            amb = amb or bool(np.any(cand & (np.abs(d - d[bm]) <= 2 * bound) & (np.arange(256) != bm)))
            cand[bm] = False
            slot, c = bm >> 5, bm & 31
            if slot >= 4 and Jn >= A.JMAX: continue
            if slot == 3 and Jn <= 5: continue
            Jn += 1 if slot >= 4 else (-1 if slot == 3 else 0)
            acc.append(bm)
            if it >= 2: break
            cand &= np.abs((np.arange(256) & 31) - c) >= 5
        if not acc: break
        for bm in sorted(acc, key=lambda m: -(m & 31)):
            _, ty, cc, xx = A.lanes(t)
            c = int(cc[bm])
            t = A.mutate(t, ty[bm], c, xx[bm])
            if ty[bm] == A.INS:
                if c < cs: cs, ce = cs + 1, ce + 1
                elif c < ce: ce += 1
            elif ty[bm] == A.DEL:
                if c < cs: cs, ce = cs - 1, ce - 1
                elif c < ce: ce -= 1
    return t[cs:ce].copy(), it + 1, amb


def test_polish_ref_without_evidence_is_the_unfiltered_polish():
    """polish_ref without arguments, and polish_ref_ev with ev all false (z-score gate off), equal the loop as it stood before the filter was added (_frozen_polish): same core,
    rounds and ambiguity on windows that need mutations"""
    rng = np.random.default_rng(3)
    t64 = A.tables64(api.default_model(), F.SNR0)
    applied = 0
    for trial in range(4):
        truth = rng.integers(0, 4, 18).astype(np.uint8)
        draft = truth.copy(); draft[7] = (draft[7] + 1) & 3
        if trial & 1: draft = np.delete(draft, 12)
        reads = [A.obs_codes(b, rng.integers(1, 4, len(b))) for b in [_noisy(rng, truth, 0.03) for _ in range(6)]]
        strands = [0] * 6
        plain = A.polish_ref(t64, draft, 4, 4, 2, len(draft) - 2, reads, strands)
        frozen = _frozen_polish(t64, draft, 4, 4, 2, len(draft) - 2, reads, strands)
        assert np.array_equal(plain[0], frozen[0]) and plain[1:] == frozen[1:]
        J = len(draft)
        core, rounds, amb, last = A.polish_ref_ev(t64, draft, 4, 4, 2, len(draft) - 2, reads, strands, ev=[False] * J, p_skip=[0.0] * J)
        assert np.array_equal(core, plain[0]) and (rounds, amb) == plain[1:]
        assert not any(last["skipped"]) and not any(last["quiet"]) and np.array_equal(last["valid"], A.lanes(last["tpl"])[0])
        applied += int(rounds > 1)
    assert applied >= 3


def test_evidence_travels_with_its_base():
    """travel() against "give every base an identity and look where it went": after a sequence of applied mutations the evidence of a surviving base is what it was
    unless some mutation was applied within 3 positions of where the base stood at that time; an inserted base has none"""
    rng = np.random.default_rng(5)
    for trial in range(200):
        J = int(rng.integers(8, 31))
        ev = [bool(rng.random() < 0.8) for _ in range(J)]; ps = [float(rng.random()) for _ in range(J)]
        ids = list(range(J)); alive_ev = {i: ev[i] for i in ids}; pskip_of = {i: ps[i] for i in ids}; nxt = J
        e, p = list(ev), list(ps)
        for step in range(int(rng.integers(1, 5))):
            ty = int(rng.integers(0, 3)); c = int(rng.integers(0, len(ids) + (1 if ty == A.INS else 0)))
            if ty == A.DEL and len(ids) <= 5: continue
            if ty == A.INS and len(ids) >= 31: continue
            e, p = A.travel(e, p, ty, c)
            if ty == A.INS: ids.insert(c, nxt); alive_ev[nxt] = False; pskip_of[nxt] = 0.0; nxt += 1
            elif ty == A.DEL: del ids[c]
            for pos, i in enumerate(ids):
                if abs(pos - c) <= 3: alive_ev[i] = False
        assert e == [alive_ev[i] for i in ids] and p == [pskip_of[i] for i in ids]
    e, p = A.travel([True] * 30, [0.5] * 30, A.INS, 10)                     # 30 columns and an insertion: the evidence of column 29 is at column 30 ("bit 31" of a 32-bit word is never reached)
    assert len(e) == 31 and e[30] and e[14] and not e[13] and not e[7] and e[6]


def test_zscore_bound_and_decision():
    """the float32 bound of z sqrt(V) is small against the threshold, and a decision inside it is undecided"""
    model = api.default_model(); rng = np.random.default_rng(2)
    t = rng.integers(0, 4, 26).astype(np.uint8); obs = A.obs_codes(t, rng.integers(1, 4, 26))
    d, V, bound = A.zscore(A.tables64(model, F.SNR0), model, F.SNR0, t, 4, 26, obs=obs)
    assert d > 0 and 5 < np.sqrt(V) < 20 and 0 < bound < 1e-3
    T = 3.4 * np.sqrt(V)
    assert A.z_decision(-T - 1.0, V, bound, -3.4) == (True, False) and A.z_decision(-T + 1.0, V, bound, -3.4) == (False, False)
    assert A.z_decision(-T - bound / 2, V, bound, -3.4)[1] and A.z_decision(-T + bound / 2, V, bound, -3.4)[1] and A.z_decision(-1e9, V, bound, 0.0) == (False, False)


@pytest.fixture(scope="module")
def cut_lab(built):
    return {z.name: F.cut_oracle(z) for z in F.lab()}


@pytest.mark.parametrize("qv_only,max_qv,min_zscore", F.RUNS)
def test_restatement_against_reference_on_the_lab(built, cut_lab, qv_only, max_qv, min_zscore):
    """oracle_lib.polish_batch with default heuristics on the lab, drafts handed in, against the reference on the windows and segments the restatement's own alignments cut.
    The first case pays for the float64 gains (about 25 s on one core, 8 s where numpy has 16 threads: 80 windows against the 20 s the lab was sized for, the
    windows of the 40- and 70-pass ZMWs being the dearest); the others share them."""
    model = api.default_model(); lab = F.lab(); batch = F.batch_of(lab); o = F.opts(max_qv, min_zscore)
    d = api.Drafts.allocate(batch)
    for zi, z in enumerate(lab): d.set_draft(zi, z.draft, backbone=0)
    res = O.polish_batch(model, o, batch, d, api.Results.allocate(batch), flags=api.QV_ONLY if qv_only else 0)
    t0 = time.time(); W_of = {}
    for z in lab:
        W = [dict(w) for w in cut_lab[z.name]]
        W_of[z.name] = F.reference(model, W, qv_only, max_qv, min_zscore, F.caches_for(z, W))
    tag = f"{'QV_ONLY' if qv_only else 'full polish'} max_qv {max_qv} min_zscore {min_zscore}"
    if not qv_only:
        for z in lab:
            if (max_qv, min_zscore) == (50, -3.4): F.run_checks(z, W_of[z.name], z.checks)
            F.run_checks(z, W_of[z.name], z.zchecks.get(min_zscore, []))
    S = F.compare_run(res, {z.name: zi for zi, z in enumerate(lab)}, W_of, qv_only, max_qv, tag)
    F.assert_caps(S, W_of, tag + f" (float64 reference {time.time() - t0:.1f} s)")


def test_a_run_indel_is_marked_at_the_run_start_and_stays_out_of_the_window_the_run_enters_from_the_left(built):
    """Two properties of the alignment that the lab's construction and DESIGN.md's argument about column 0 rest on, asserted instead of assumed.
    (1) A pass whose homopolymer (or dinucleotide tract) is one or two bases (one unit) longer or shorter than the draft's is dirty at the run's FIRST base and the
    position before it, nowhere else — for deletions and insertions, both alignment bands.
    (2) A run that enters a window from its left flank (t[0] = lf != t[1]): passes with the run longer or shorter have, in THAT window, segments equal to the template —
    the indel belongs to the window before — so the two lanes the quiet rule keeps at column 0 (deletion of t[0], insertion of t[0] before it) lose on every pass:
    whether column 0 counts as inside a homopolymer by its flank cannot change a result there."""
    for L in (3, 5, 8, 12):
        d = F.run_at(F.template(f"place{L}", 120), 50, L)
        for wide in (0, 1):
            for name, t, ok in (("del", F.delete(d, 52), {0}), ("ins", F.insert(d, 52, [d[52]]), {-1, 0}), ("del2", F.delete(d, 51, 2), {0, 1}), ("ins2", F.insert(d, 52, [d[52]] * 2), {-1, 0})):
                r = O.route(t, d, wide=wide)
                assert r[2] and set(int(x) - 50 for x in np.flatnonzero(r[4])) == ok, (L, name, wide, np.flatnonzero(r[4]) - 50)
    d = F.template("place2", 120); d[50:62] = [1, 2] * 6; d[49] = 0; d[62] = 3
    for t, ok in ((F.delete(d, 54, 2), {0, 1}), (F.insert(d, 54, [1, 2]), {-1, 0})):
        r = O.route(t, d); assert r[2] and set(int(x) - 50 for x in np.flatnonzero(r[4])) == ok
    # (2)
    for k in range(20):
        d = F.template(f"leftflank#{k}", 110); wb = O.windows(d); ws = int(wb[2]) - 2
        d = F.run_at(d, ws - 4, 5)
        if np.array_equal(O.windows(d), wb): break
    else: raise AssertionError("no draft whose windows survive the run")
    mods = {k: (lambda t: F.insert(t, ws - 2, [t[ws - 2]])) if k < 4 else (lambda t: F.delete(t, ws - 2)) for k in range(8)}
    z = F.Zmw("leftflank", "argument", d, F.make_passes("leftflank", d, 8, mods))
    W = F.cut_oracle(z); w = W[2]; t = w["tpl"]
    assert w["lf"] == t[0] != t[1] and all(w["seg"])
    for obs, st in zip(w["reads"], w["strands"]):
        assert np.array_equal(obs // 3, A.revcomp(t) if st else t), "a pass disagrees with the template inside the window the run enters"
    assert not any(any(row) for row in w["dirty"]), "a pass is dirty inside the window the run enters"
    valid, ty, cc, xx = A.lanes(t); only = np.zeros(256, bool); only[[3 * 32, (4 + int(t[0])) * 32]] = True
    assert valid[3 * 32] and valid[(4 + int(t[0])) * 32]
    dl = A.deltas(A.tables64(api.default_model(), F.SNR0), t, w["lf"], w["rf"], w["reads"], w["strands"], banded=True, gains=A.read_gains(A.tables64(api.default_model(), F.SNR0), t, w["lf"], w["rf"], w["reads"], w["strands"], banded=True, only=only))
    assert dl[3 * 32] < -8 and dl[(4 + int(t[0])) * 32] < -8, dl[[3 * 32, (4 + int(t[0])) * 32]]

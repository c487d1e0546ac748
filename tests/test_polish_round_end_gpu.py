"""k_polish_t ends a round behind ONE barrier: every wave loads all 256 gains and validity bytes (four per lane), converts them in registers, decides by its own
ballot whether a mutation is favourable and takes the round's exits by itself (E1); the QV terms go to the head of the gamma/beta area, unenumerated lanes as exact
zeros, with no barrier in front of them (E2); the ordered sum of a window's error probabilities is 32 straight-line steps and the z-score sums are 31 (E3).  Every
case below runs the whole engine and compares with the CPU restatement BIT FOR BIT — status, seq_len, iters, n_windows, np, sequence, raw QVs as uint32 — and asserts
on the restatement's results and counters alone that the path it is about was taken (the seeds were chosen on the CPU).  Small batches: a second or two each.

Which assertion pins which item:
  E1  `iters` in every case: a wave that misjudged `anyfav` or an exit would leave the loop alone and the window would hang or end a round early or late —
      test_one_round_and_many (windows of one round, of several, of more than MULTI_ROUNDS: the selection reads the gains from registers, the next round zeroes
      integer words), test_window_reaches_max_iter (the third exit, status NON_CONVERGENT), test_only_favourable_mutation_in_one_slice (the draft's one defect is repaired by a
      mutation in lanes 192 - 255, or 0 - 63, and one round later no lane is favourable: a wave that judged by one slice would end such a window a round early)
  E2  the raw QVs, bit for bit, in every case; test_qv_floors (max_qv 93 and 30: the terms' new home feeds every floor), test_more_than_32_passes (a group reload
      inside the round precedes its end: the gamma/beta area is still dead behind the round's last barrier)
  E3  wsum: a ZMW's predicted accuracy `rq` comes from the ordered sums of its windows and is compared bit for bit in every case; test_core_lengths has cores of
      28 and of 5 positions and windows without a left or a right flank (32 steps against ce - cs).  The z-score sums: test_zscore_gate (z-dropped reads at the
      default threshold, the sums not formed at 0.0, windows of J < 8 and of J = 30)
  E4  not built: the compiler already reads a row pair's two observation bytes from one address, and the second row's diagonal test needs its decrement
      (profiles/polish_round_end.txt)"""
import difflib

import numpy as np
import pytest

from ccs_amd import api
import oracle_lib as O

pytestmark = pytest.mark.gpu

MULTI_ROUNDS, MAX_ITER, NON_CONVERGENT = 2, api.MAX_ITER, 4


def _oracle(batch, o, model=None):
    ref = api.Results.allocate(batch)
    O.lib().orc_counts_sync(); O.counts_reset()
    O.consensus_batch(model if model is not None else api.default_model(), o, batch, ref, nthreads=8)
    O.lib().orc_counts_sync()
    ref.paths = O.counts()                                              # which SPEC paths the restatement took (the engine took the same: everything is bit-exact)
    return ref


def _bit_exact(res, ref, batch):
    assert np.array_equal(res.status, ref.status), (res.status, ref.status)
    assert np.array_equal(res.seq_len, ref.seq_len)
    assert np.array_equal(res.iters, ref.iters), (res.iters, ref.iters)
    assert np.array_equal(res.n_windows, ref.n_windows)
    assert np.array_equal(res.np_, ref.np_), (res.np_, ref.np_)
    assert np.array_equal(res.rq.view(np.uint32), ref.rq.view(np.uint32)), (res.rq, ref.rq)        # (the ordered sum of the windows' error probabilities)
    for z in range(batch.n_zmw):
        assert np.array_equal(res.sequence(z), ref.sequence(z)), f"zmw {z}: sequence differs"
        a, b = res.raw(z), ref.raw(z)
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"zmw {z}: raw QVs differ, max |d| = {np.abs(a - b).max() if a.shape == b.shape else 'shape'}"


def _check(case, paths):
    batch, o = case
    h = api.Handle(0, opts=o)
    try:
        res = h.consensus(batch)
        ref = _oracle(batch, o, h.model)
    finally:
        h.close()
    paths(ref, batch)
    _bit_exact(res, ref, batch)
    return res, ref


def _rewrite(batch, tpls, rng, sub=0.015, dele=0.03, dup=0.02, noisy=()):
    """the batch with every pass rewritten as a noisy copy of its ZMW's template tpls[z] (native orientation by the pass's flag)"""
    bases, pw, ipd, off = [], [], [], [0]
    for r in range(int(batch.read_off[-1])):
        z = int(np.searchsorted(batch.read_off, r, side="right") - 1)
        k = 6.0 if r - int(batch.read_off[z]) in noisy else 1.0       # (the passes listed in `noisy`: six times the error rates)
        t = tpls[z]
        t = t[rng.random(len(t)) > k * dele].copy()
        s = rng.random(len(t)) < k * sub
        t[s] = (t[s] + rng.integers(1, 4, int(s.sum()))) & 3
        t = np.repeat(t, 1 + (rng.random(len(t)) < k * dup))
        if batch.flags[r] & 1: t = (3 - t[::-1]).astype(np.uint8)
        bases.append(t.astype(np.uint8)); pw.append(rng.integers(1, 4, len(t)).astype(np.uint8)); ipd.append(np.full(len(t), 5, np.uint8)); off.append(off[-1] + len(t))
    return api.Batch(batch.zmw_id, batch.snr, batch.read_off, np.array(off, np.int64), np.concatenate(bases), np.concatenate(pw), np.concatenate(ipd),
                     batch.flags.copy(), batch.tpl_off, batch.tpl)


def _win_cols(d):
    """(columns J with the overhang, core length, has a left flank, has a right flank) of every window of draft d"""
    wb = O.windows(d)
    return [(min(len(d), int(wb[w + 1]) + 2) - max(0, int(wb[w]) - 2), int(wb[w + 1] - wb[w]), int(wb[w]) - 2 > 0, int(wb[w + 1]) + 2 < len(d)) for w in range(len(wb) - 1)]


# ---- the cases: (batch, opts) and what the restatement must have done on it (checked on `ref` alone, so the seeds can be fixed without a GPU)

ROUNDS_SEED = 929


def case_rounds():
    """single-window ZMWs (templates of 16 - 28 bases) of 3 - 5 passes: a ZMW's `iters` is its window's, and the draft's own errors give windows of many rounds"""
    o = api.default_opts(); o.min_rq = 0.0
    return api.synth(24, (3, 5), (16, 28), seed=ROUNDS_SEED), o


def paths_rounds(ref, batch):
    """windows that end after ONE round (the two-barrier exit), windows that go on (selection from registers, integer words zeroed by the next set-up), windows with
    a selection in a round from MULTI_ROUNDS on, where a single mutation is accepted (a fourth round exists only behind such a selection)"""
    one = (ref.seq_len > 0) & (ref.n_windows == 1)
    it = ref.iters[one]
    assert one.sum() >= 16 and (it == 1).sum() >= 3 and ((it == 2) | (it == 3)).sum() >= 3 and (it > MULTI_ROUNDS + 1).any() and (it < MAX_ITER).all(), (ref.status, ref.n_windows, ref.iters)
    assert ref.paths["nonconv_win"] == 0, ref.paths                     # (no window of this batch is cut off: that is the next case)


LOWCX_SEED = 2


def case_max_iter():
    """low-complexity templates (short tandem repeats with a few changed bases), 3 noisy passes each: some windows find a favourable mutation in every round"""
    rng = np.random.default_rng(870 + LOWCX_SEED)
    base = api.synth(8, 3, 300, seed=871)
    tpls = []
    for _ in range(base.n_zmw):
        unit = rng.integers(0, 4, int(rng.integers(1, 4)), dtype=np.uint8)
        t = np.tile(unit, 300 // len(unit) + 1)[:300].copy()
        s = rng.random(300) < 0.04
        t[s] = (t[s] + rng.integers(1, 4, int(s.sum()))) & 3
        tpls.append(t)
    o = api.default_opts(); o.min_rq = 0.0
    return _rewrite(base, tpls, rng, sub=0.03, dele=0.06, dup=0.05), o


def paths_max_iter(ref, batch):
    assert ref.paths["nonconv_win"] >= 1, ref.paths                     # a window ran CCSX_MAX_ITER rounds and still had a favourable mutation
    assert (ref.status == NON_CONVERGENT).any(), ref.status
    assert (ref.status == 0).any(), ref.status


def case_slice(high):
    """caller drafts = the templates with ONE defect in one window, through the whole engine's polish seam, every mutation lane valid (disable_heuristics).
    high: a base 2 or 3 is missing, so the repair is an insertion of base 2 / 3 = slot 6 / 7 = lanes 192 - 255; else a base is replaced by the one or two below it,
    so the repair is substitution slot 0 / 1 = lanes 0 - 63"""
    batch = api.synth(8, 10, 400, seed=881)
    rng = np.random.default_rng(882 + high)
    drafts, defects = [], []
    for z in range(batch.n_zmw):
        t = batch.tpl[batch.tpl_off[z]:batch.tpl_off[z + 1]].copy()
        ok = np.flatnonzero((t[1:-1] != t[:-2]) & (t[1:-1] != t[2:]) & ((t[1:-1] >= 2) if high else True)) + 1      # not inside a run: the repair has one place
        ok = ok[(ok > 40) & (ok < len(t) - 40)]
        p = int(ok[rng.integers(0, len(ok))])
        if high: d = np.delete(t, p)
        else: d = t.copy(); d[p] = (t[p] - 1 - int(rng.integers(0, 2))) & 3            # the repair (d + 1 + slot) & 3 = t: slot 0 or 1
        drafts.append(d); defects.append((p, int(t[p])))
    o = api.default_opts(); o.min_rq = 0.0; o.disable_heuristics = 1
    return batch, o, drafts, defects


def paths_slice(ref, batch, drafts, defects, high):
    """the restatement repaired exactly the defect and nothing else, in ONE extra round: the window of the defect found its favourable mutation in round 0 (in the
    slice the case is about), every other window of the ZMW found none in any slice"""
    n = 0
    for z in range(batch.n_zmw):
        if ref.status[z] != 0: continue
        t = batch.tpl[batch.tpl_off[z]:batch.tpl_off[z + 1]]
        ops = [op for op in difflib.SequenceMatcher(None, bytes(drafts[z].tolist()), bytes(ref.sequence(z).tolist()), autojunk=False).get_opcodes() if op[0] != "equal"]
        if not (np.array_equal(ref.sequence(z), t) and len(ops) == 1 and ref.iters[z] == ref.n_windows[z] + 1): continue
        tag, i1, i2, j1, j2 = ops[0]
        p, b = defects[z]
        if high: assert tag == "insert" and j2 - j1 == 1 and b >= 2 and t[j1] == b, (ops, defects[z])
        else: assert tag == "replace" and i2 - i1 == 1 and j2 - j1 == 1 and ((int(t[j1]) - int(drafts[z][i1]) - 1) & 3) <= 1, (ops, defects[z])
        n += 1
    assert n >= 5, (n, ref.status, ref.iters - ref.n_windows)


CORES_SEED = 0


def _tpl_24_5(rng):
    """29 bases with (ac)3 at 19 .. 24 and no a behind it: the boundaries 21 - 23 would break the repeat, 24 does not — cores of 24 and 5"""
    t = rng.integers(0, 4, 29, dtype=np.uint8)
    a = int(rng.integers(0, 4)); c = (a + 1 + int(rng.integers(0, 3))) & 3
    t[19:25] = [a, c, a, c, a, c]
    if t[25] == a: t[25] = (a + 1 + (c == ((a + 1) & 3))) & 3
    return t


def case_cores():
    """templates of 29 - 58 bases whose window rule gives last cores of 28 (the maximum) and, where a dinucleotide repeat pushes the first boundary to 24 of 29, of 5
    (the minimum met in practice: J = 7); single-window ZMWs have neither flank"""
    rng = np.random.default_rng(890 + CORES_SEED)
    base = api.synth(12, 10, 40, seed=891)
    tpls = []
    for z in range(base.n_zmw):
        if z % 3 == 0:                                                  # 29 bases, (AC)3 at 19 .. 24: boundaries 21 - 23 break a repeat, 24 does not -> cores 24 + 5
            t = _tpl_24_5(rng)
        elif z % 3 == 1: t = rng.integers(0, 4, 50, dtype=np.uint8)     # 22 + 28
        else: t = rng.integers(0, 4, int(rng.integers(16, 29)), dtype=np.uint8)      # one window, no flank on either side
        tpls.append(t)
    o = api.default_opts(); o.min_rq = 0.0
    return _rewrite(base, tpls, rng), o


def paths_cores(ref, batch):
    cols = []
    for z in np.flatnonzero(ref.seq_len > 0):
        assert ref.paths["fallback"] == 0, ref.paths                    # (the draft below is the one that was polished)
        cols += _win_cols(O.poa_draft(batch, int(z)))
    core = np.array([c[1] for c in cols]); J = np.array([c[0] for c in cols])
    assert (core == 28).any() and (core <= 5).any() and (J < 8).any() and (J >= 30).any(), (core, J)
    assert any(not c[2] and not c[3] for c in cols) and any(c[2] and not c[3] for c in cols) and any(c[3] and not c[2] for c in cols), cols


def case_zscore(min_z):
    """nine passes, two of them (4 and 5) six times as noisy; templates of case_cores' short kinds, so windows
    of J < 8 and of J = 30 form the sums, and of 400 bases"""
    rng = np.random.default_rng(897)
    base = api.synth(12, 9, 40, seed=898)
    tpls = []
    for z in range(base.n_zmw):
        if z % 3 == 0: t = _tpl_24_5(rng)
        elif z % 3 == 1: t = rng.integers(0, 4, 50, dtype=np.uint8)
        else: t = rng.integers(0, 4, 400, dtype=np.uint8)
        tpls.append(t)
    o = api.default_opts(); o.min_rq = 0.0
    if min_z is not None: o.min_zscore = min_z
    return _rewrite(base, tpls, rng, noisy=(4, 5)), o


def paths_zscore(ref, batch, on):
    if not on:
        assert ref.paths["zdrop"] == 0, ref.paths
        return
    assert ref.paths["zdrop"] >= 1, ref.paths                         # (read, window) pairs the gate dropped at the default threshold (it drops few: five here)
    J = np.array([c[0] for z in np.flatnonzero(ref.seq_len > 0) for c in _win_cols(O.poa_draft(batch, int(z)))])
    assert ref.paths["fallback"] == 0 and (J < 8).any() and J.max() >= 29, (ref.paths, np.bincount(J))


def case_reload():
    o = api.default_opts(); o.min_rq = 0.0
    return api.synth(6, 40, 400, seed=861), o


def paths_reload(ref, batch):
    done = ref.seq_len > 0
    assert done.sum() >= 5 and (ref.np_[done] == 40).all(), (ref.status, ref.np_)     # two groups of passes in every round: the reload precedes the round's end
    assert (ref.iters > ref.n_windows)[done].any() and (ref.iters < 2 * ref.n_windows)[done].any(), (ref.iters, ref.n_windows)


def case_qv(max_qv):
    o = api.default_opts(); o.min_rq = 0.0; o.max_qv = max_qv
    return api.synth(8, (5, 20), (400, 800), seed=895), o


def paths_qv(ref, batch, max_qv):
    done = ref.seq_len > 0
    assert done.sum() >= 6, ref.status
    top = max(float(ref.raw(int(z)).max()) for z in np.flatnonzero(done))
    assert max_qv - 0.01 <= top <= max_qv + 0.01, top                   # the floor of opts.max_qv is the best QV a base reports, and it is met
    assert any((ref.raw(int(z)) < max_qv - 1.0).any() for z in np.flatnonzero(done))      # and bases below it: sums of real terms


def test_one_round_and_many(built):
    _check(case_rounds(), paths_rounds)


def test_window_reaches_max_iter(built):
    _check(case_max_iter(), paths_max_iter)


@pytest.mark.parametrize("high", [1, 0])
def test_only_favourable_mutation_in_one_slice(built, high):
    batch, o, drafts, defects = case_slice(high)
    h = api.Handle(0, opts=o)
    try:
        d = api.Drafts.allocate(batch)
        for z, t in enumerate(drafts): d.set_draft(z, t, backbone=0)
        res = h.polish(batch, d)
        O.counts_reset()
        ref = O.polish_batch(h.model, o, batch, d, api.Results.allocate(batch))
    finally:
        h.close()
    paths_slice(ref, batch, drafts, defects, high)
    _bit_exact(res, ref, batch)


def test_core_lengths(built):
    _check(case_cores(), paths_cores)


def test_zscore_gate(built):
    res, ref = _check(case_zscore(None), lambda r, b: paths_zscore(r, b, True))
    res0, ref0 = _check(case_zscore(0.0), lambda r, b: paths_zscore(r, b, False))
    assert not np.array_equal(ref.ec, ref0.ec), (ref.ec, ref0.ec)


def test_more_than_32_passes(built):
    _check(case_reload(), paths_reload)


@pytest.mark.parametrize("max_qv", [93, 30])
def test_qv_floors(built, max_qv):
    _check(case_qv(max_qv), lambda ref, batch: paths_qv(ref, batch, max_qv))

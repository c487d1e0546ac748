"""k_polish_t sets a round up from registers: every lane loads its column's template base once and takes the neighbours, the reverse complement, both strands'
contexts, the skip mask and the validity of all eight mutation slots of its column from its own wave's lanes (no exchange between waves), and the fill's tables
from those contexts.  Every case below runs the whole engine and compares with the CPU restatement BIT FOR BIT — status, seq_len, iters, n_windows, np, sequence,
raw QVs — on the shapes at which that set-up can go wrong: all four 64-lane slices populated or nearly empty, J moving between rounds (the reverse-complement
index J-1-c and the tables follow it), windows without a flank, homopolymers under the quiet-position rule, the z-score sums on and off, a group reload inside a
round.  Every assertion that a path was taken is made on the restatement's results and counters.  Small batches: a second or two each."""
import difflib

import numpy as np
import pytest

from ccs_amd import api
import oracle_lib as O

pytestmark = pytest.mark.gpu


def _oracle(batch, o, model=None):
    ref = api.Results.allocate(batch)
    O.lib().orc_counts_sync(); O.counts_reset()
    O.consensus_batch(model if model is not None else api.default_model(), o, batch, ref, nthreads=8)
    O.lib().orc_counts_sync()
    ref.paths = O.counts()                                              # which SPEC paths the restatement took (the engine took the same: everything is bit-exact)
    return ref


def _run(batch, opts=None):
    o = opts if opts is not None else api.default_opts()
    h = api.Handle(0, opts=o)
    try:
        res = h.consensus(batch)
        ref = _oracle(batch, o, h.model)
    finally:
        h.close()
    return res, ref


def _bit_exact(res, ref, batch):
    assert np.array_equal(res.status, ref.status), (res.status, ref.status)
    assert np.array_equal(res.seq_len, ref.seq_len)
    assert np.array_equal(res.iters, ref.iters), (res.iters, ref.iters)
    assert np.array_equal(res.n_windows, ref.n_windows)
    assert np.array_equal(res.np_, ref.np_), (res.np_, ref.np_)
    for z in range(batch.n_zmw):
        assert np.array_equal(res.sequence(z), ref.sequence(z)), f"zmw {z}: sequence differs"
        a, b = res.raw(z), ref.raw(z)
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"zmw {z}: raw QVs differ, max |d| = {np.abs(a - b).max() if a.shape == b.shape else 'shape'}"


def _edit(batch, fn):
    """the batch with every read (bases, pw, ipd, flags) passed through fn(z, q, bases, pw, ipd, flag) -> (bases, pw, ipd, flag); q = the read's index in its ZMW"""
    bases, pw, ipd, off, flags = [], [], [], [0], batch.flags.copy()
    for r in range(int(batch.read_off[-1])):
        a, b = int(batch.base_off[r]), int(batch.base_off[r + 1])
        z = int(np.searchsorted(batch.read_off, r, side="right") - 1)
        bb, pp, ii, fl = fn(z, r - int(batch.read_off[z]), batch.bases[a:b], batch.pw[a:b], batch.ipd[a:b], int(flags[r]))
        bases.append(bb); pw.append(pp); ipd.append(ii); flags[r] = fl; off.append(off[-1] + len(bb))
    return api.Batch(batch.zmw_id, batch.snr, batch.read_off, np.array(off, np.int64), np.concatenate(bases).astype(np.uint8), np.concatenate(pw).astype(np.uint8),
                     np.concatenate(ipd).astype(np.uint8), flags, batch.tpl_off, batch.tpl)


# ---- the cases: (batch, opts) and what the restatement must have done on it (checked on `ref` alone, so the seeds can be fixed without a GPU)

def case_slices(noheur):
    o = api.default_opts(); o.min_rq = 0.0; o.disable_heuristics = 1 if noheur else 0
    return api.synth(8, 10, 600, seed=811), o


_SLICES_REF = {}                                                        # the restatement of both runs, each computed once


def _slices_ref(noheur):
    if noheur not in _SLICES_REF: _SLICES_REF[noheur] = _oracle(*case_slices(noheur))
    return _SLICES_REF[noheur]


def _enumerated(t):
    """mutation lanes the SPEC enumerates on template t: 3 substitutions and a deletion per column (no deletion inside a run), 4 insertions in front of every
    column and behind the last (not of the base before)"""
    J = len(t)
    return 7 * J + 4 - int((t[1:] == t[:-1]).sum())


def paths_slices(ref, batch, noheur):
    """what the restatement says about the lane lists of the two runs.  Unfiltered, every enumerated lane is valid: all eight slots of a column, so every 64-lane
    slice, by construction; the enumeration on the draft's windows says how long the compacted list gets.  The filter's effect shows in the number of
    (lane, read) scorings — cells_score counts each scored lane's band rows — and in results that differ"""
    assert (ref.status == 0).sum() >= 6, ref.status
    assert (ref.np_[ref.seq_len > 0] == 10).all(), ref.np_
    full, filt = (ref, _slices_ref(0)) if noheur else (_slices_ref(1), ref)
    n = []
    for z in np.flatnonzero(full.seq_len > 0):
        d = O.poa_draft(batch, int(z)); wb = O.windows(d)
        n += [_enumerated(d[max(0, int(wb[w]) - 2):min(len(d), int(wb[w + 1]) + 2)]) for w in range(len(wb) - 1)]
    n = np.array(n)
    assert (n > 128).all() and (n <= 256).all() and (n > 192).any(), n  # round 0's lists: three blocks of 64 lanes and more (waves 1 - 3 write behind other waves' lanes), one of four
    assert 2 * filt.paths["cells_score"] < full.paths["cells_score"], (filt.paths, full.paths)      # the filter leaves out more than half of the scorings
    assert not np.array_equal(full.iters, filt.iters) or any(not np.array_equal(full.raw(z).view(np.uint32), filt.raw(z).view(np.uint32)) for z in range(8))


MOVING_J_SEEDS = {3: 923, 4: 954, 5: 955}                               # (3 and 4 passes: seeds with a window that reaches CCSX_JMAX columns)


def case_moving_j(passes, untrimmed):
    o = api.default_opts(); o.min_rq = 0.0
    if untrimmed: o.max_insertion_size = -1
    return api.synth(8, passes, 800, seed=MOVING_J_SEEDS[passes]), o


def _window_moves(ref, batch):
    """per window of the restatement's draft: (columns J0 with the overhang, bases the consensus inserted there, bases it deleted), from an alignment of draft and consensus"""
    out = []
    for z in np.flatnonzero(ref.seq_len > 0):
        d, s = O.poa_draft(batch, int(z)), ref.sequence(int(z))
        wb = O.windows(d)
        ins, dl = np.zeros(len(d) + 1, int), np.zeros(len(d) + 1, int)
        for tag, i1, i2, j1, j2 in difflib.SequenceMatcher(None, bytes(d.tolist()), bytes(s.tolist()), autojunk=False).get_opcodes():
            n = (j2 - j1) - (i2 - i1)
            if tag != "equal" and n > 0: ins[i1] += n
            elif tag != "equal" and n < 0: dl[i1:i1 - n] += 1
        for w in range(len(wb) - 1):
            ws, we = max(0, int(wb[w]) - 2), min(len(d), int(wb[w + 1]) + 2)
            out.append((we - ws, ins[ws:we + 1].sum(), dl[ws:we].sum()))
    return np.array(out)


def paths_moving_j(ref, batch, passes):
    done = ref.seq_len > 0
    assert done.sum() >= 6, ref.status
    assert ref.paths["fallback"] == 0 and ref.paths["third_draft"] == 0, ref.paths                  # (the draft below is the one that was polished)
    assert (ref.iters > ref.n_windows)[done].sum() > done.sum() // 2, (ref.iters, ref.n_windows)    # second and third rounds in most ZMWs
    assert (ref.iters - ref.n_windows)[done].sum() >= 5 * done.sum()                              # many of them
    w = _window_moves(ref, batch)
    net = w[:, 1] - w[:, 2]
    assert (net > 0).sum() >= 20 and (net < 0).sum() >= 10, ((net > 0).sum(), (net < 0).sum())      # windows that grew, windows that shrank: J moved both ways
    if passes < 5:                                                                                  # a window of 29 or 30 columns that ended on CCSX_JMAX = 31
        assert ((w[:, 0] >= 29) & (w[:, 0] + net == 31)).any(), w[w[:, 0] >= 29]


def case_no_flank():
    o = api.default_opts(); o.min_rq = 0.0
    return api.synth(8, 10, (16, 50), seed=836), o


def paths_no_flank(ref, batch):
    done = ref.seq_len > 0
    assert done.sum() >= 6, ref.status
    assert set(ref.n_windows[done].tolist()) == {1, 2}, ref.n_windows     # windows whose first / last column has no flank on either strand


def _hp_template(rng, n):
    """a template of about n bases in which runs of 4 - 10 equal bases alternate with 3 - 8 random ones"""
    out, last = [], -1
    while sum(len(x) for x in out) < n:
        b = int(rng.integers(0, 4))
        if b == last: b = (b + 1) & 3
        out.append(np.full(int(rng.integers(4, 11)), b, np.uint8)); last = b
        out.append(rng.integers(0, 4, int(rng.integers(3, 9)), dtype=np.uint8))
    return np.concatenate(out)


def case_homopolymers(passes):
    """every ZMW's passes are rewritten as noisy copies of a homopolymer-rich template: 1.5 % substitutions, 3 % deleted and 2 % doubled bases (a doubled or deleted
    base inside a run changes the run's length — the draft gets some of them wrong, the polish moves run lengths)"""
    rng = np.random.default_rng(840 + passes)
    base = api.synth(8, passes, 500, seed=841)
    tpls = [_hp_template(rng, 500) for _ in range(base.n_zmw)]

    def fn(z, q, bb, pp, ii, fl):
        t = tpls[z]
        t = t[rng.random(len(t)) > 0.03].copy()
        sub = rng.random(len(t)) < 0.015
        t[sub] = (t[sub] + rng.integers(1, 4, int(sub.sum()))) & 3
        t = np.repeat(t, 1 + (rng.random(len(t)) < 0.02))
        if fl & 1: t = (3 - t[::-1]).astype(np.uint8)
        return t, rng.integers(1, 4, len(t)).astype(np.uint8), np.full(len(t), 5, np.uint8), fl

    o = api.default_opts(); o.min_rq = 0.0
    return _edit(base, fn), o


def paths_homopolymers(ref, batch):
    done = ref.seq_len > 0
    assert done.sum() >= 6, ref.status
    assert (ref.iters > ref.n_windows)[done].any(), (ref.iters, ref.n_windows)
    for z in np.flatnonzero(done):                                     # the consensus kept the runs
        s = ref.sequence(z)
        runs = np.diff(np.flatnonzero(np.concatenate([[True], s[1:] != s[:-1], [True]])))
        assert (runs >= 4).sum() >= 20, runs


def case_zscore(min_z):
    rng = np.random.default_rng(73)
    base = api.synth(8, 9, 1200, seed=852)

    def fn(z, q, bb, pp, ii, fl):
        if q in (4, 5):                                                # two neighbouring passes: one of each orientation
            keep = rng.random(len(bb)) > 0.08
            bb, pp, ii = bb[keep].copy(), pp[keep], ii[keep]
            sub = rng.random(len(bb)) < 0.10
            bb[sub] = (bb[sub] + rng.integers(1, 4, int(sub.sum()))) & 3
            ins = rng.random(len(bb)) < 0.06
            bb, pp, ii = np.repeat(bb, 1 + ins), np.repeat(pp, 1 + ins), np.repeat(ii, 1 + ins)
        return bb, pp, ii, fl

    batch = _edit(base, fn)
    o = api.default_opts(); o.min_rq = 0.0; o.min_zscore = min_z
    return batch, o


def paths_zscore_on(ref, batch):
    fl = batch.flags.reshape(batch.n_zmw, 9)
    assert ((fl[:, 4] ^ fl[:, 5]) & 1).all(), fl                       # the noisy passes: both orientations, so both strands' sums decide
    assert ref.paths["zdrop"] >= 100, ref.paths                       # (read, window) pairs the gate dropped
    assert (ref.ec[ref.seq_len > 0] < 9.0).all(), ref.ec
    assert (ref.iters - ref.n_windows).sum() >= 40                     # second rounds: the gate's bits are kept, the sums are not formed again


def paths_zscore_off(ref, batch):
    assert ref.paths["zdrop"] == 0, ref.paths


def case_reload():
    o = api.default_opts(); o.min_rq = 0.0
    return api.synth(8, 33, 600, seed=861), o


def paths_reload(ref, batch):
    done = ref.seq_len > 0
    assert done.sum() >= 6 and (ref.np_[done] == 33).all(), (ref.status, ref.np_)     # two groups of passes in every round: the set-up runs once, the plan twice
    assert (ref.iters > ref.n_windows)[done].any()


def _check(case, paths):
    batch, o = case
    res, ref = _run(batch, o)
    paths(ref, batch)
    _bit_exact(res, ref, batch)
    return res, ref


@pytest.mark.parametrize("noheur", [1, 0])
def test_lanes_across_the_four_slices(built, noheur):
    """10 passes x 600 bp.  disable_heuristics = 1: every enumerated lane is valid (all eight slots of a column, so all four 64-lane slices of the compaction, by
    construction), compacted lists of three blocks of 64 lanes, one of four; the default filter: under half of the scorings.  No counter of the restatement covers the
    skip mask or the quiet-position rule by itself: the bit-for-bit comparison is the check of both"""
    _check(case_slices(noheur), lambda ref, batch: paths_slices(ref, batch, noheur))


@pytest.mark.parametrize("untrimmed", [0, 1])
@pytest.mark.parametrize("passes", [3, 4, 5])
def test_j_moves_between_rounds(built, passes, untrimmed):
    """3, 4 and 5 passes x 800 bp: the draft's own errors give many second and third rounds, insertions and deletions change J (up to CCSX_JMAX at 3 and 4 passes);
    with max_insertion_size = -1 too"""
    _check(case_moving_j(passes, untrimmed), lambda ref, batch: paths_moving_j(ref, batch, passes))


def test_window_ends_without_a_flank(built):
    """templates of 16 - 50 bp: ZMWs of one and two windows (a template of 30 bp or more already has two), lf / rf = 4 in both strands' first and last columns"""
    _check(case_no_flank(), paths_no_flank)


@pytest.mark.parametrize("passes", [10, 20])
def test_quiet_homopolymer_rule_and_skip_mask(built, passes):
    """templates with runs of 4 - 10 equal bases: the homopolymer flag keeps quiet positions in the round, the rule keeps only their length-changing mutations.
    The restatement has no counter of either; what is asserted on it is that the consensus is made of such runs and that rounds were repeated, the comparison
    bit for bit is the check of the rule"""
    _check(case_homopolymers(passes), paths_homopolymers)


def test_zscore_sums_on_and_off(built):
    """two noisy passes of opposite orientation at min_zscore = -2: the gate needs all four sums of round 0; at min_zscore = 0 they are skipped"""
    res, ref = _check(case_zscore(-2.0), paths_zscore_on)
    res_off, ref_off = _check(case_zscore(0.0), paths_zscore_off)
    assert (ref_off.ec[ref_off.seq_len > 0] > ref.ec[ref_off.seq_len > 0]).all(), (ref.ec, ref_off.ec)


def test_group_reload_inside_a_round(built):
    """33 passes x 600 bp: two groups of 32 in every round"""
    _check(case_reload(), paths_reload)

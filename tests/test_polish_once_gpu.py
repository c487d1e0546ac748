"""k_polish_t plans the gamma/beta chunks of a group once per round (one wave; the other waves read the plan at the barrier that opens a chunk), and every wave
derives the reads' validity from alpha(I,J) / beta(0,0) after the fill.  Every case below runs the whole engine and compares with the CPU restatement BIT FOR BIT —
sequence, raw QVs, status, iters, n_windows, np — on the shapes at which that bookkeeping can go wrong: every chunk count from one to three full chunks, a group
reload inside a round (more than 32 passes), reads without a segment / long units / trimmed insertions in one window, and the two ways a read leaves a chunk (the
validity step: alpha(I,J) at or below TINY_P or not in agreement with beta(0,0); the z-score gate, decided in round 0 and kept).  Small batches: a second or two each."""
import numpy as np
import pytest

from ccs_amd import api
import oracle_lib as O
import test_oracle_draft as T

pytestmark = pytest.mark.gpu


def _run(batch, opts=None):
    o = opts if opts is not None else api.default_opts()
    h = api.Handle(0, opts=o)
    try:
        res = h.consensus(batch)
        ref = api.Results.allocate(batch)
        O.lib().orc_counts_sync(); O.counts_reset()
        O.consensus_batch(h.model, o, batch, ref, nthreads=8)
        O.lib().orc_counts_sync()
        ref.paths = O.counts()                                          # which SPEC paths the restatement took (the engine took the same: everything is bit-exact)
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


def _insert(rng, bb, pp, ii, at, size):
    blk = rng.integers(0, 4, size, dtype=np.uint8)
    return (np.concatenate([bb[:at], blk, bb[at:]]), np.concatenate([pp[:at], np.full(size, 2, np.uint8), pp[at:]]),
            np.concatenate([ii[:at], np.full(size, 5, np.uint8), ii[at:]]))


@pytest.mark.parametrize("passes", [3, 8, 9, 10, 11, 17, 24, 33, 40])
def test_chunk_counts_and_group_reload(built, passes):
    """600 bp; a chunk holds eight reads: 3 passes = one chunk, 8 = exactly one full chunk, 9 / 10 / 11 = 8 + 1 / 2 / 3, 17 = three chunks, 24 = three full chunks;
    33 and 40 passes = two groups of 32, i.e. a reload (and a new plan) inside every round.  The draft's own errors give windows a second round: iters > n_windows"""
    batch = api.synth(8, passes, 600, seed=500 + passes)
    res, ref = _run(batch)
    _bit_exact(res, ref, batch)
    ok = res.status == 0
    assert ok.sum() >= (0 if passes == 3 else 6), res.status          # (three passes: LOW_RQ is the rule)
    assert (res.np_[res.seq_len > 0] == passes).all(), res.np_         # every pass reached the polish
    assert (res.iters > res.n_windows).any(), (res.iters, res.n_windows)   # some window ran at least two rounds


def test_no_segment_long_units_and_trimmed_insertions(built):
    """partial passes (no segment in the windows they do not reach), inserted blocks of 4-5 bases (not trimmed at max_insertion_size = 5: |I - J| >= 4, segments of
    more than 31 bases — the long fill units) and of 6-12 bases (trimmed to the window's length) in the same ZMWs, often the same window"""
    rng = np.random.default_rng(71)
    base = T.partial_pass_batch(n=8, seed=58, nfull=9, length=(700, 1600))

    def fn(z, q, bb, pp, ii, fl):
        if q == 0 or len(bb) < 200: return bb, pp, ii, fl              # (the POA backbone stays clean)
        for k in range(int(rng.integers(1, 4))):
            at = int(rng.integers(40, len(bb) - 40))
            bb, pp, ii = _insert(rng, bb, pp, ii, at, int(rng.integers(4, 6)))
            bb, pp, ii = _insert(rng, bb, pp, ii, min(at + int(rng.integers(3, 25)), len(bb)), int(rng.integers(6, 13)))
        return bb, pp, ii, fl

    batch = _edit(base, fn)
    o = api.default_opts(); o.max_insertion_size = 5; o.min_rq = 0.0
    res, ref = _run(batch, o)
    _bit_exact(res, ref, batch)
    assert (res.status == 0).sum() >= 6, res.status
    assert ref.paths["trim"] >= 8 and ref.paths["partial_used"] >= 8, ref.paths
    o2 = api.default_opts(); o2.max_insertion_size = -1; o2.min_rq = 0.0
    h = api.Handle(0, opts=o2)
    try:
        untrimmed = h.consensus(batch)
    finally:
        h.close()
    both = (res.status == 0) & (untrimmed.status == 0)
    assert res.ec[both].sum() > untrimmed.ec[both].sum()             # trimming kept segments that leave the window untrimmed: the blocks reached the trim


def test_reads_that_fail_the_validity_step_are_dropped(built):
    """two passes per ZMW carry a stretch of 80 bases in which EVERY base is wrong ((b + 2) & 3): they align (the rest of the pass is the ZMW's), and in windows
    under the stretch alpha(I,J) / beta(0,0) fall to the underflow range — at or below TINY_P, or no longer in agreement.  With the
    z-score gate off nothing else can drop a read from a window: ec, the mean number of usable reads per window, falls below the pass count"""
    base = api.synth(8, 10, 1500, seed=601)

    def fn(z, q, bb, pp, ii, fl):
        if q in (2, 7) and len(bb) > 600:
            m = len(bb) // 2 + 40 * q
            bb = bb.copy(); bb[m:m + 80] = (bb[m:m + 80] + 2) & 3
        return bb, pp, ii, fl

    batch = _edit(base, fn)
    o = api.default_opts(); o.min_zscore = 0.0; o.min_rq = 0.0
    res, ref = _run(batch, o)
    _bit_exact(res, ref, batch)
    assert ref.paths["zdrop"] == 0 and ref.paths["split"] == 0 and ref.paths["trim"] == 0, ref.paths
    assert (res.status == 0).all() and (res.np_ == 10).all()
    assert (res.ec < 10.0).sum() >= 4, res.ec                         # reads left windows, in at least half of the ZMWs


def test_zscore_gate_drops_a_noisy_pass_and_keeps_it_dropped(built):
    """one pass per ZMW with 8 % deletions, 10 % substitutions and 6 % insertions: it aligns, and the z-score gate (min_zscore = -2) drops it from many windows in
    round 0; the windows among them that run a second round — about a third of all windows do — must not take it back (the gate's bits are decided on the draft
    window only; the restatement keeps them, and iters / QVs are compared bit for bit).  With the gate off the same pass is used everywhere"""
    rng = np.random.default_rng(73)
    base = api.synth(8, 9, 1200, seed=602)

    def fn(z, q, bb, pp, ii, fl):
        if q == 4:
            keep = rng.random(len(bb)) > 0.08
            bb, pp, ii = bb[keep].copy(), pp[keep], ii[keep]
            sub = rng.random(len(bb)) < 0.10
            bb[sub] = (bb[sub] + rng.integers(1, 4, int(sub.sum()))) & 3
            for at in sorted(rng.integers(1, len(bb) - 1, int(len(bb) * 0.06)).tolist(), reverse=True):
                bb, pp, ii = _insert(rng, bb, pp, ii, at, 1)
        return bb, pp, ii, fl

    batch = _edit(base, fn)
    o = api.default_opts(); o.min_rq = 0.0; o.min_zscore = -2.0
    res, ref = _run(batch, o)
    _bit_exact(res, ref, batch)
    assert ref.paths["zdrop"] >= 50, ref.paths                        # (read, window) pairs the gate dropped
    assert (res.iters - res.n_windows).sum() >= 80                     # second rounds
    off = api.default_opts(); off.min_rq = 0.0; off.min_zscore = 0.0
    res_off, ref_off = _run(batch, off)
    _bit_exact(res_off, ref_off, batch)
    assert ref_off.paths["zdrop"] == 0 and (res_off.ec == 9.0).all() and (res.ec < 9.0).all(), (res.ec, res_off.ec)

"""k_orient on an MI355X (DESIGN.md §2 "Pass orientation", §4): the seam's report against tests/orient_ref.py on the lab of tests/orient_lab.py, field for field;
the fused path's stage accessor; batches whose every pass is submitted strand-unknown with random bits give, byte for byte, the results of their true flags —
synchronous, ticketed, with kinetics, through the draft seam and through ccsx_hd_batch; tickets in flight keep to themselves; a batch without the bit launches
nothing."""
import os
import subprocess
import sys

import numpy as np
import pytest

from ccs_amd import api
import orient_lab as LAB
import orient_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES_FIELDS = ("status", "seq_len", "rq", "np_", "ec", "fn", "rn")
LOOSE = dict(min_votes=1, ratio=2)


@pytest.fixture(scope="module")
def lab(built):
    b, names = LAB.batch()
    return b, names, R.orient(b)


@pytest.fixture(scope="module")
def e2e(built):
    return LAB.end_to_end()


def _check_report(rep, want, names=None, batch=None):
    for k in R.FIELDS:
        bad = np.flatnonzero(np.asarray(getattr(rep, k)) != want[k])
        where = [names[int(np.searchsorted(batch.read_off, r, "right")) - 1] for r in bad[:4]] if names else bad[:4]
        assert len(bad) == 0, (k, where, np.asarray(getattr(rep, k))[bad[:4]], want[k][bad[:4]])


def _same_results(a, b, n, kinetics=False):
    for f in RES_FIELDS:
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f
    for z in range(n):
        assert np.array_equal(a.sequence(z), b.sequence(z)) and np.array_equal(a.quals(z), b.quals(z)), z
        if kinetics:
            assert np.array_equal(a.kinetics(z), b.kinetics(z)), z


def _opts(d):
    o = api.orient_opts_default()
    for k, v in d.items():
        setattr(o, k, v)
    return o


def test_seam_equals_the_reference_on_the_lab(lab):
    b, names, want = lab
    h = api.Handle(0)
    try:
        rep = h.orient(b)
        _check_report(rep, want, names, b)
        _check_report(h.stage_orient(), want, names, b)
        _check_report(h.orient(b, _opts(LOOSE)), R.orient(b, LOOSE), names, b)
        again = h.orient(b)                                             # two runs: identical reports (and the options of a call are its own)
        for k in R.FIELDS:
            assert np.array_equal(getattr(again, k), getattr(rep, k)), k
    finally:
        h.close()


def test_fused_consensus_reports_the_same(lab):
    b, names, want = lab
    h = api.Handle(0)
    try:
        h.consensus(b)
        _check_report(h.stage_orient(), want, names, b)
        h.set_orient_opts(_opts(LOOSE))                                 # from the next staged batch on
        h.consensus(b)
        _check_report(h.stage_orient(), R.orient(b, LOOSE), names, b)
        h.set_orient_opts(None)
        h.consensus(b)
        _check_report(h.stage_orient(), want, names, b)
    finally:
        h.close()


@pytest.mark.parametrize("kinetics", [False, True])
def test_unknown_strands_give_the_results_of_the_true_flags(e2e, kinetics):
    """fails without k_orient: bit 3 is ignored then, and the random bits put half of the passes on the wrong strand (measured on the commit before the
    feature: status, sequence or np of 63 of the 68 ZMWs differ from the run on the true flags, 27 end as TOO_MANY_UNUSABLE)"""
    true, unk = e2e
    o = api.default_opts()
    o.hifi_kinetics = int(kinetics)
    h = api.Handle(0, opts=o)
    try:
        want = h.consensus(true)
        assert (want.status == 0).sum() >= 60
        _same_results(h.consensus(unk), want, true.n_zmw, kinetics)
        rep = h.stage_orient()
        assert set(rep.call.tolist()) == {R.ANCHOR, R.SAME, R.OPPOSITE} and LAB.relative_strands_equal(true, true.flags, rep.strand).all()
        res = api.Results.allocate(unk, kinetics=kinetics, pinned=True)
        t = h.submit(unk.pinned(), res)
        _same_results(h.wait(t), want, true.n_zmw, kinetics)
        h.release(t)
    finally:
        h.close()


def test_draft_seam_and_hd_seam_honour_the_bit(e2e):
    """one place: every path that stages a batch"""
    true, unk = e2e
    true, unk = true.slice(0, 12), unk.slice(0, 12)
    assert not LAB.relative_strands_equal(true, true.flags, unk.flags).all()
    h = api.Handle(0)
    try:
        d = h.draft(true)
        du = h.draft(unk)
        assert d.status.tobytes() == du.status.tobytes() and d.len.tobytes() == du.len.tobytes() and (d.status == 0).all()
        for z in range(true.n_zmw):
            assert np.array_equal(d.draft(z), du.draft(z)), z
        want, got = h.hd(true, d), h.hd(unk, d)
        for k, _, _ in api.HdReport.PLANES:
            assert getattr(want, k).tobytes() == getattr(got, k).tobytes(), k
        rep = h.stage_orient()
        assert LAB.relative_strands_equal(true, true.flags, rep.strand).all() and (rep.call != R.GIVEN).all()
        _same_results(h.polish(unk, d), h.polish(true, d), true.n_zmw)
    finally:
        h.close()


def test_three_tickets_in_flight_the_middle_one_flagged(e2e):
    true, unk = e2e
    parts = [true.slice(0, 20), unk.slice(20, 44), true.slice(44, 68)]
    h = api.Handle(0)
    try:
        want = [h.consensus(p) for p in parts]
        res = [api.Results.allocate(p, pinned=True) for p in parts]
        pinned = [p.pinned() for p in parts]
        tickets = [h.submit(p, r) for p, r in zip(pinned, res)]
        for t, w, p in zip(tickets, want, parts):
            _same_results(h.wait(t), w, p.n_zmw)
            h.release(t)
        _same_results(want[1], h.consensus(true.slice(20, 44)), parts[1].n_zmw)
    finally:
        h.close()


_CHILD = """
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from ccs_amd import api
import orient_lab as LAB
true, unk = LAB.end_to_end()
h = api.Handle(0)
h.consensus((unk if sys.argv[2] == "unknown" else true).slice(0, 4))
h.close()
"""


def test_a_batch_without_the_bit_launches_nothing(e2e):
    true, unk = e2e
    h = api.Handle(0)
    try:
        before = h.consensus(true)
        rep = h.stage_orient()
        assert (rep.call == R.GIVEN).all() and np.array_equal(rep.strand, true.flags & 1) and not rep.votes_same.any() and not rep.votes_opp.any()
        h.consensus(unk)                                                # the handle's tables are reserved now
        _same_results(h.consensus(true), before, true.n_zmw)
        assert (h.stage_orient().call == R.GIVEN).all()
        rep = h.orient(true)                                            # the seam on such a batch: nothing to decide
        assert (rep.call == R.GIVEN).all() and np.array_equal(rep.strand, true.flags & 1)
    finally:
        h.close()
    env = dict(os.environ, CCSX_TRACE="1")
    log = {}
    for which in ("true", "unknown"):
        r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, which], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        log[which] = r.stderr
    assert "k_setup done" in log["true"] and "k_orient" not in log["true"] and "k_orient done: no error" in log["unknown"]

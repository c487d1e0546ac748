"""The alignment cascade on the device (k_align16, k_align16_tb, k_align, k_rescue) pinned at its limits: the alignment lab (tests/align_lab.py) through upload / run / sync,
every pass's (valid, score), entry rows at every window-edge column and dirty bits (ccsx_stage_align_ev) against the CPU restatement's result for that pass's route AND
against the plain unbanded reference (tests/align_ref.py: the score is the unbanded optimum, some optimal alignment enters each edge column at the reported row, a clean
position can be matched on an optimal alignment).  All integer, all exact.  The evidence test asserts that the run contained every planted shape; nothing here reads anything
outside the repository.  (python -m pytest tests/test_align_gpu.py -m gpu -s prints the evidence.)"""
import os
import subprocess
import sys

import numpy as np
import pytest

from ccs_amd import api
import align_lab as G
import oracle_lib as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(disable_heuristics=0):
    o = api.default_opts(); o.disable_heuristics = disable_heuristics
    h = api.Handle(0, opts=o)
    try:
        return G.stage_outputs(h, G.lab().batch())
    finally:
        h.close()


@pytest.fixture(scope="module")
def lab_run(built):
    return _run()


def _compare(out, drafts, wide):
    """the engine's stage outputs against the restatement's routes, pass by pass, then the independent properties on the engine's own numbers"""
    L, want = G.lab(), G.routes(wide)
    for z, (name, t, _) in enumerate(L.zmws):
        assert np.array_equal(drafts[z][0], t), f"zmw {z} ({name}): the draft is not the planted template"
        assert np.array_equal(drafts[z][1], O.windows(t)), f"zmw {z} ({name}): windows differ"
    got = {}
    for (z, k, b, t, pe), key in zip(L.passes(), want):
        route, rs_o, v_o, sc_o, dirty_o = want[key]
        rs, v, sc, dirty = out[key]
        tag = f"zmw {z} ({L.zmws[z][0]}) pass {k} [{route}]"
        assert v == v_o, f"{tag}: valid {v}, restatement {v_o}"
        if v or pe is None: assert sc == sc_o, f"{tag}: score {sc}, restatement {sc_o}"
        if v:
            I = len(b)
            for c in O.need_cols(t):                      # (an edge column the pass does not cover carries a row outside the pass on both sides: unusable, whatever its value)
                a, e = int(rs[c]), int(rs_o[c])
                assert a == e or not (0 <= a <= I or 0 <= e <= I), f"{tag}: column {int(c)}: entry row {a}, restatement {e}"
            bad = np.flatnonzero(dirty != dirty_o)
            assert not len(bad), f"{tag}: dirty bits differ at positions {bad.tolist()} (engine {dirty[bad].tolist()})"
        else:
            assert not dirty.any(), tag
        got[key] = (route, rs, v, sc, dirty)
    G.check_all(got, wide)
    return got


def test_lab_entries_scores_masks(lab_run):
    _compare(*lab_run, wide=0)


def test_lab_evidence(lab_run):
    """the run contained what the lab plants: every route, both saturation triggers (each alone: the 16-row attempt repeated with the other switched off), quads of 1 - 4
    passes, the tiny quad with its three exact neighbours, the Ld residues and both block-count parities, more than 128 edge columns, a narrow path past read row 2048,
    and the boundary pair of insertion runs (5 stays narrow, 6 does not).  A shape that did not occur fails this test, not the kernel.  Routes and triggers are
    restatement-side evidence: the engine's run enters through valid agreeing with the restatement for every pass (and score, entries and masks in the test above); the
    quad sizes follow from the pass counts, quads being consecutive passes of a ZMW on the host."""
    out, _ = lab_run
    want = G.routes(0)
    got = {key: (want[key][0],) + out[key] for key in want}
    for key in want: assert out[key][1] == want[key][2], key          # (the route names are the restatement's; they describe the engine's run iff valid agrees)
    E = G.evidence(got)
    print("\n[align gpu lab] evidence", E)
    G.assert_evidence(E)


def test_lab_disable_heuristics(built):
    """opts.disable_heuristics: every pass through align_pass in k_align (the forward-carried masks) against the restatement with wide = 1 and the same properties"""
    out, drafts = _run(disable_heuristics=1)
    got = _compare(out, drafts, wide=1)
    L = G.lab()
    for key, want in L.expect_dirty.items():
        assert set(np.flatnonzero(got[key][4]).tolist()) == want, key


_CHILD = """
import sys
sys.path[:0] = [%r, %r]
import numpy as np
from ccs_amd import api
import align_lab as G
assert api.lib().ccsx_runtime_switches() == b"CCSX_ALIGN16_MAX_SLOTS=8"
batch, z0 = G.lab_batch_after(int(sys.argv[2]))
h = api.Handle(0)
try:
    out, _ = G.stage_outputs(h, batch, z0)
finally:
    h.close()
np.savez(sys.argv[1], **G.packed(out))
"""


@pytest.mark.parametrize("prefix", [0, 40])
def test_lab_is_independent_of_launch_cuts(lab_run, tmp_path, prefix):
    """CCSX_ALIGN16_MAX_SLOTS=8 (a fresh child process: the hook is read once): the lab's 28 quads take four launches of k_align16 / k_align16_tb over both scratch regions,
    and behind 40 synthetic ZMWs, whose quads the length order interleaves with the lab's, several more — entries, masks, valid and score byte-identical to the uncut run"""
    if prefix:
        batch, z0 = G.lab_batch_after(prefix)
        h = api.Handle(0)
        try: whole, _ = G.stage_outputs(h, batch, z0)
        finally: h.close()
        for key, v in lab_run[0].items():                    # and the company of other ZMWs changes nothing either
            assert all(np.array_equal(a, b) for a, b in zip(v, whole[key])), key
    else:
        whole = lab_run[0]
    dst = str(tmp_path / "cut.npz")
    p = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, os.path.join(ROOT, "tests")), dst, str(prefix)], env=dict(os.environ, CCSX_ALIGN16_MAX_SLOTS="8"),
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    cut, ref = np.load(dst), G.packed(whole)
    for k in ("ent", "valid", "score", "dirty"):
        assert cut[k].tobytes() == ref[k].tobytes(), f"{k} differs between the cut and the uncut run"


def test_consensus_of_the_lab_batch(built):
    """the planted alignments as the polish sees them: the lab batch end to end against the restatement"""
    import test_gpu_parity as P
    batch = G.lab().batch()
    h = api.Handle(0)
    try:
        res = h.consensus(batch)
        ref = P._oracle(h, batch)
    finally:
        h.close()
    P._compare(res, ref, batch)
    assert int((res.status == 0).sum()) >= 12

"""k_segment on an MI355X (DESIGN.md §2 "Segment rule", §4): Handle.segment_reads against tests/segment_ref.py on the whole limit set, field for field, on a
poisoned report, in one call per case and again with the reads in reverse order; the fused path on the molecules of tests/segment_lab.py — results byte for
byte those of consensus_batch, the report equal to the restatement applied to the returned sequences; three tickets in flight with different sets and options;
the request beside the adapter and coverage screens; a run without the request after one with it; the combinations that are refused.

Which lab ZMWs reach a consensus, and what the rule makes of it, was looked at with the oracle on the CPU for segment_lab.SEED (tests/oracle_lib.py
consensus_batch on the same passes, segment_ref.segment_reads on its sequences): the ten ZMWs of eight passes end SUCCESS, the two of two passes end
TOO_FEW_PASSES without a consensus (untested); both forward and both reverse arrays are complete with four segments and no leftover, both partial arrays give
three forward segments and are not complete, both arrays without their middle adapter give two segments and one leftover piece of 949 and 1054 bases, and the
two molecules without adapters have no hit.  The test asserts the occurrence of each kind on what the GPU returns."""
import numpy as np
import pytest

from ccs_amd import api
import segment_lab as LAB
import segment_ref as R

pytestmark = pytest.mark.gpu
CASES = R.limit_cases()
RES_FIELDS = ("status", "seq_len", "rq", "np_", "ec", "iters", "n_windows", "fn", "rn")


@pytest.fixture(scope="module")
def handle(built):
    h = api.Handle(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def lab(built):
    return LAB.batch()


def _opts(**kw):
    o = api.segment_opts_default()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _poisoned(n):
    rep = api.SegmentReport.allocate(n)
    for k in R.FIELDS:
        getattr(rep, k).view(np.uint8)[...] = 0xA5
    return rep


def _same_results(a, b, n):
    for f in RES_FIELDS:
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f
    for z in range(n):
        assert np.array_equal(a.sequence(z), b.sequence(z)) and np.array_equal(a.quals(z), b.quals(z)), z
        assert np.array_equal(a.raw(z).view(np.uint32), b.raw(z).view(np.uint32)), z


def _reads_of(res, n):
    return [res.sequence(z) if res.seq_len[z] > 0 else np.zeros(0, np.uint8) for z in range(n)]


def _as_dict(rep):
    return {k: getattr(rep, k) for k in R.FIELDS}


def _check_against_own_sequences(res, rep, S, n, **opts):
    want = R.segment_reads(S, _reads_of(res, n), **{**R.DEFAULTS, **opts})
    assert R.diff(rep, want) == [], R.diff(rep, want)
    return want


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0] for c in CASES])
def test_reads_equal_the_restatement_on_the_limit_set(handle, i):
    name, S, o, reads = CASES[i]
    sset, want = api.SegmentSet.from_codes(S), R.expected(i)
    rep = handle.segment_reads(sset, list(reads), _opts(**o), _poisoned(len(reads)))
    assert R.diff(rep, want) == [], (name, R.diff(rep, want))
    rev = handle.segment_reads(sset, list(reads)[::-1], _opts(**o), _poisoned(len(reads)))
    assert R.diff(rev, R.reversed_order(want)) == [], (name, "reversed", R.diff(rev, R.reversed_order(want)))


def test_reads_leave_slot_0_and_tickets_alone(handle, lab):
    """the synchronous seam stages nothing: a ticket in flight completes with its own results, and slot 0 still downloads what it ran"""
    b, _, _ = lab
    plain = handle.consensus(b)
    res = api.Results.allocate(b, pinned=True)
    t = handle.submit(b.pinned(), res)
    name, S0, o, reads = CASES[0]
    rep = handle.segment_reads(api.SegmentSet.from_codes(S0), list(reads), _opts(**o))
    assert R.diff(rep, R.expected(0)) == []
    handle.wait(t)
    handle.release(t)
    _same_results(res, plain, b.n_zmw)
    handle.upload(b)
    handle.run()
    handle.sync()
    rep = handle.segment_reads(api.SegmentSet.from_codes(S0), list(reads), _opts(**o))
    assert R.diff(rep, R.expected(0)) == []
    _same_results(handle.download(), plain, b.n_zmw)


def test_fused_report_is_the_rule_on_the_returned_sequences(handle, lab):
    b, kinds, S = lab
    plain = handle.consensus(b)
    res, rep = handle.consensus_segments(b, api.SegmentSet.from_codes(S))
    _same_results(res, plain, b.n_zmw)                               # detection only: byte for byte the plain run
    want = _check_against_own_sequences(res, rep, S, b.n_zmw)        # every ZMW, none left out
    seen = set()
    for z, kind in enumerate(kinds):
        f = {k: int(want[k][z]) for k in R.PLANES}
        if kind == "fail":
            assert f["tested"] == 0 and res.seq_len[z] == 0 and f["orient"] == -1
        elif kind in ("forward", "reverse"):
            assert (f["complete"], f["n_segments"], f["orient"], f["leftover_bases"]) == (1, 4, int(kind == "reverse"), 0), (z, f)
            assert [s[2] for s in rep.segments(z)] == ([0, 1, 2, 3] if kind == "forward" else [3, 2, 1, 0])
        elif kind == "partial":
            assert (f["complete"], f["n_segments"], f["orient"]) == (0, 3, 0), (z, f)
        elif kind == "missing":
            assert (f["complete"], f["n_segments"], f["n_cuts"]) == (0, 2, 4) and f["leftover_bases"] >= 600 and [s[2] for s in rep.segments(z)] == [0, 3], (z, f)
        else:
            assert (f["tested"], f["n_hits"], f["orient"], f["leftover_bases"]) == (1, 0, -1, int(res.seq_len[z])), (z, f)
        seen.add(kind)
    assert seen == set(LAB.KINDS)
    # a run without the request after one with it: the plain results
    _same_results(handle.consensus(b), plain, b.n_zmw)


def test_three_tickets_with_their_own_sets_and_options(handle, lab):
    b, _, S = lab
    sets = [S, S[:3], [R.rc(a) for a in reversed(S)]]
    opts = [dict(), dict(min_len=400, max_dist_pct=0), dict(max_dist_pct=30, min_len=1)]
    sync = [handle.consensus_segments(b, api.SegmentSet.from_codes(s), _opts(**o)) for s, o in zip(sets, opts)]
    pb = b.pinned()
    out = []
    for s, o in zip(sets, opts):
        res, rep = api.Results.allocate(b, pinned=True), api.SegmentReport.allocate(b.n_zmw, pinned=True)
        out.append((handle.submit(pb, res, segments=rep, segment_set=api.SegmentSet.from_codes(s), segment_opts=_opts(**o)), res, rep))
    for (t, res, rep), (sres, srep), s, o in zip(out, sync, sets, opts):
        handle.wait(t)
        _same_results(res, sres, b.n_zmw)
        assert R.diff(rep, _as_dict(srep)) == []
        _check_against_own_sequences(res, rep, s, b.n_zmw, **o)
        handle.release(t)
    assert R.diff(out[0][2], _as_dict(out[1][2])) != [] and R.diff(out[0][2], _as_dict(out[2][2])) != []     # (the tickets did differ)


def test_beside_the_adapter_and_coverage_screens(handle, lab):
    b, _, S = lab
    n = b.n_zmw
    res0, vrep0, _, _, arep0, _, _ = handle.consensus_coverage(b, adapters=api.AdapterSet.default())
    arep, vrep = api.AdapterReport.allocate(n), api.CoverageReport.allocate(n)
    res, rep = handle.consensus_segments(b, api.SegmentSet.from_codes(S), adapters=arep, coverage=vrep)
    _same_results(res, res0, n)
    for k, _, _ in api.AdapterReport.PLANES:
        assert getattr(arep, k).tobytes() == getattr(arep0, k).tobytes(), k
    for k, _, _ in api.CoverageReport.PLANES:
        assert getattr(vrep, k).tobytes() == getattr(vrep0, k).tobytes(), k
    _check_against_own_sequences(res, rep, S, n)


def test_the_refused_combinations(handle, lab):
    """with the heteroduplex request, the hand-off, the barcode request and the represent request: refused before anything is enqueued, and the handle runs on"""
    b, _, S = lab
    n = b.n_zmw
    sset, rep, res = api.SegmentSet.from_codes(S), api.SegmentReport.allocate(n), api.Results.allocate(b)
    bset = api.BarcodeSet.from_codes([a[:16] for a in S])
    for kw in (dict(hd=api.HdReport.allocate(n)), dict(handoff=api.Handoff.allocate(b, 4)), dict(barcodes=api.BarcodeReport.allocate(n), barcode_set=bset),
               dict(represent=api.RepresentReport.allocate(n))):
        with pytest.raises(ValueError, match="segment request is not combined"):
            handle.submit(b, res, segments=rep, segment_set=sset, **kw)
    with pytest.raises(ValueError, match="segment_set is needed"):
        handle.submit(b, res, segments=rep)
    res1, rep1 = handle.consensus_segments(b, sset)
    _check_against_own_sequences(res1, rep1, S, n)

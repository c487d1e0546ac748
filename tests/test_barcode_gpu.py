"""k_barcode on an MI355X (DESIGN.md §2 "Barcode calls", §4): Handle.barcode_reads against tests/barcode_ref.py on the whole limit set, field for field, in one
call per case and again with the reads in reverse order; the fused path on the molecules of tests/barcode_lab.py — results byte for byte those of
consensus_batch, the report equal to the restatement applied to the returned sequences; three tickets in flight with different sets and windows; the request
beside the adapter and coverage screens; a run without the request after one with it.

Which lab ZMWs reach a consensus, and which calls the rule makes on it, was looked at with the oracle on the CPU for barcode_lab.SEED (tests/oracle_lib.py
consensus_batch on the same passes, barcode_ref.call_reads on its sequences): the 20 ZMWs of eight passes end SUCCESS, the four of two passes end without a
consensus, and the calls 3, 1, 2 and 0 occur eight, four, four and four times.  The test asserts the occurrence on what the GPU returns."""
import numpy as np
import pytest

from ccs_amd import api
import barcode_lab as LAB
import barcode_ref as R

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
    o = api.barcode_opts_default()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _same_results(a, b, n):
    for f in RES_FIELDS:
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f
    for z in range(n):
        assert np.array_equal(a.sequence(z), b.sequence(z)) and np.array_equal(a.quals(z), b.quals(z)), z
        assert np.array_equal(a.raw(z).view(np.uint32), b.raw(z).view(np.uint32)), z


def _reads_of(res, n):
    return [res.sequence(z) if res.seq_len[z] > 0 else np.zeros(0, np.uint8) for z in range(n)]


def _check_against_own_sequences(res, rep, S, n, **opts):
    want = R.call_reads(S, _reads_of(res, n), **{**R.DEFAULTS, **opts})
    assert R.diff(rep, want) == [], R.diff(rep, want)
    return want


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0] for c in CASES])
def test_reads_equal_the_restatement_on_the_limit_set(handle, i):
    name, S, o, reads = CASES[i]
    bset, want = api.BarcodeSet.from_codes(S), R.expected(i)
    rep = handle.barcode_reads(bset, list(reads), _opts(**o))
    assert R.diff(rep, want) == [], (name, R.diff(rep, want))
    rev = handle.barcode_reads(bset, list(reads)[::-1], _opts(**o))
    assert R.diff(rev, {k: v[::-1] for k, v in want.items()}) == [], (name, "reversed", R.diff(rev, {k: v[::-1] for k, v in want.items()}))


def test_reads_leave_slot_0_and_tickets_alone(handle, lab):
    """the synchronous seam stages nothing: a ticket in flight completes with its own results, and slot 0 still downloads what it ran"""
    b, _, _, S = lab
    plain = handle.consensus(b)
    res = api.Results.allocate(b, pinned=True)
    t = handle.submit(b.pinned(), res)
    name, S0, o, reads = CASES[0]
    rep = handle.barcode_reads(api.BarcodeSet.from_codes(S0), list(reads), _opts(**o))
    assert R.diff(rep, R.expected(0)) == []
    handle.wait(t)
    handle.release(t)
    _same_results(res, plain, b.n_zmw)
    handle.upload(b)
    handle.run()
    handle.sync()
    rep = handle.barcode_reads(api.BarcodeSet.from_codes(S0), list(reads), _opts(**o))
    assert R.diff(rep, R.expected(0)) == []
    _same_results(handle.download(), plain, b.n_zmw)


def test_fused_report_is_the_rule_on_the_returned_sequences(handle, lab):
    b, kinds, planted, S = lab
    plain = handle.consensus(b)
    res, rep = handle.consensus_barcodes(b, api.BarcodeSet.from_codes(S))
    _same_results(res, plain, b.n_zmw)                               # detection only: byte for byte the plain run
    want = _check_against_own_sequences(res, rep, S, b.n_zmw)        # every ZMW, none left out
    assert set(want["call"][want["tested"] == 1].tolist()) == {0, 1, 2, 3} and (want["tested"] == 0).any() and (want["tested"] == 1).sum() >= 16
    for z, (kind, (a, c)) in enumerate(zip(kinds, planted)):         # the planted barcodes are the ones that are called
        if rep.tested[z] and kind == "both":
            assert rep.call[z] == 3 and rep.idx[z].tolist() == [a, c], (z, rep.fields(z))
    # a run without the request after one with it: the plain results
    _same_results(handle.consensus(b), plain, b.n_zmw)


def test_three_tickets_with_their_own_sets_and_windows(handle, lab):
    b, _, _, S = lab
    sets = [S, S[:5], list(reversed(S))]
    opts = [dict(window=64), dict(window=24, min_margin=0), dict(window=300, max_dist_pct=30)]
    sync = [handle.consensus_barcodes(b, api.BarcodeSet.from_codes(s), _opts(**o)) for s, o in zip(sets, opts)]
    pb = b.pinned()
    out = []
    for s, o in zip(sets, opts):
        res, rep = api.Results.allocate(b, pinned=True), api.BarcodeReport.allocate(b.n_zmw, pinned=True)
        out.append((handle.submit(pb, res, barcodes=rep, barcode_set=api.BarcodeSet.from_codes(s), barcode_opts=_opts(**o)), res, rep))
    for (t, res, rep), (sres, srep), s, o in zip(out, sync, sets, opts):
        handle.wait(t)
        _same_results(res, sres, b.n_zmw)
        assert R.diff(rep, {k: getattr(srep, k) for k in R.FIELDS}) == []
        _check_against_own_sequences(res, rep, s, b.n_zmw, **o)
        handle.release(t)
    assert R.diff(out[0][2], {k: getattr(out[1][2], k) for k in R.FIELDS}) != []     # (the tickets did differ)


def test_beside_the_adapter_and_coverage_screens(handle, lab):
    b, _, _, S = lab
    n = b.n_zmw
    res0, vrep0, _, _, arep0, _, _ = handle.consensus_coverage(b, adapters=api.AdapterSet.default())
    arep, vrep = api.AdapterReport.allocate(n), api.CoverageReport.allocate(n)
    res, rep = handle.consensus_barcodes(b, api.BarcodeSet.from_codes(S), adapters=arep, coverage=vrep)
    _same_results(res, res0, n)
    for k, _, _ in api.AdapterReport.PLANES:
        assert getattr(arep, k).tobytes() == getattr(arep0, k).tobytes(), k
    for k, _, _ in api.CoverageReport.PLANES:
        assert getattr(vrep, k).tobytes() == getattr(vrep0, k).tobytes(), k
    _check_against_own_sequences(res, rep, S, n)
    with pytest.raises(ValueError):
        handle.submit(b, res, barcodes=rep, barcode_set=api.BarcodeSet.from_codes(S), hd=api.HdReport.allocate(n))

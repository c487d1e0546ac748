"""k_cdna on an MI355X (DESIGN.md §2 "cDNA rule", §4): Handle.cdna_reads against tests/cdna_ref.py on the whole limit set, field for field, on a poisoned
report, in one call per case and again with the reads in reverse order; the fused path on the molecules of tests/cdna_lab.py — results byte for byte those of
consensus_batch, the report equal to the restatement applied to the returned sequences; three tickets in flight with different sets and options; the request
beside the adapter and coverage screens; a run without the request after one with it; the combinations that are refused.

Which lab ZMWs reach a consensus, and what the rule makes of it, was looked at with the oracle on the CPU for cdna_lab.SEED (tests/oracle_lib.py
consensus_batch on the same passes, cdna_ref.cdna_reads on its sequences): the twelve ZMWs of eight passes end SUCCESS, the two of two passes end
TOO_FEW_PASSES without a consensus (untested).  Both sense and both antisense molecules are FULL_LENGTH with strand 0 / 1, both primers at distance 0 and clips
of 25; the consensus of the A x 30 tail is 30 or 31 bases long (a homopolymer: ZMW 8 gains a base), so the test allows 28 .. 32.  Both molecules without
a tail are NO_TAIL with polya_len 0, both concatemers CONCATEMER with two internal hits (rc(3p) and 5p at the junction), polya_len 30 and first_internal at
the first molecule's end; both molecules without the 3' primer are ONE_END (the tail's best primer stands at distance 10 and 11), both 5p - 5p molecules
SAME_ROLE with idx 0, 0, and the molecule without primers is NO_PRIMER.  The test asserts the occurrence of each kind on what the GPU returns."""
import numpy as np
import pytest

from ccs_amd import api
import cdna_lab as LAB
import cdna_ref as R

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
    o = api.cdna_opts_default()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _poisoned(n, pinned=False):
    rep = api.CdnaReport.allocate(n, pinned=pinned)
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


def _check_against_own_sequences(res, rep, S, roles, n, **opts):
    want = R.cdna_reads(S, roles, _reads_of(res, n), **opts)
    assert R.diff(rep, want) == [], R.diff(rep, want)
    return want


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0] for c in CASES])
def test_reads_equal_the_restatement_on_the_limit_set(handle, i):
    name, S, roles, o, reads = CASES[i]
    pset, want = api.CdnaPrimers.from_codes(S, roles), R.expected(i)
    rep = handle.cdna_reads(pset, list(reads), _opts(**o), _poisoned(len(reads)))
    assert R.diff(rep, want) == [], (name, R.diff(rep, want))
    rev = handle.cdna_reads(pset, list(reads)[::-1], _opts(**o), _poisoned(len(reads)))
    assert R.diff(rev, R.reversed_order(want)) == [], (name, "reversed", R.diff(rev, R.reversed_order(want)))


def test_reads_leave_slot_0_and_tickets_alone(handle, lab):
    """the synchronous seam stages nothing: a ticket in flight completes with its own results, and slot 0 still downloads what it ran"""
    b = lab[0]
    plain = handle.consensus(b)
    res = api.Results.allocate(b, pinned=True)
    t = handle.submit(b.pinned(), res)
    name, S0, roles0, o, reads = CASES[0]
    rep = handle.cdna_reads(api.CdnaPrimers.from_codes(S0, roles0), list(reads), _opts(**o))
    assert R.diff(rep, R.expected(0)) == []
    handle.wait(t)
    handle.release(t)
    _same_results(res, plain, b.n_zmw)
    handle.upload(b)
    handle.run()
    handle.sync()
    rep = handle.cdna_reads(api.CdnaPrimers.from_codes(S0, roles0), list(reads), _opts(**o))
    assert R.diff(rep, R.expected(0)) == []
    _same_results(handle.download(), plain, b.n_zmw)


def test_fused_report_is_the_rule_on_the_returned_sequences(handle, lab):
    b, kinds, S, roles = lab
    plain = handle.consensus(b)
    res, rep = handle.consensus_cdna(b, api.CdnaPrimers.from_codes(S, roles))
    _same_results(res, plain, b.n_zmw)                               # detection only: byte for byte the plain run
    want = _check_against_own_sequences(res, rep, S, roles, b.n_zmw)   # every ZMW, none left out
    seen = set()
    for z, kind in enumerate(kinds):
        f = {k: want[k][z].tolist() for k in R.FIELDS}
        L = int(res.seq_len[z])
        if kind == "fail":
            assert f["tested"] == 0 and L == 0 and f["strand"] == -1 and f["idx"] == [-1, -1]
        elif kind in ("sense", "antisense"):
            strand = int(kind == "antisense")
            assert (f["cls"], f["strand"], f["n_internal"], f["idx"]) == (R.FULL_LENGTH, strand, 0, [strand, 1 - strand]) and 28 <= f["polya_len"] <= 32, (z, f)
            assert (f["start"], f["end"]) == ((f["clip"][0] + f["polya_len"], L - f["clip"][1]) if strand else (f["clip"][0], L - f["clip"][1] - f["polya_len"]))
        elif kind == "notail":
            assert (f["cls"], f["strand"], f["polya_len"], f["start"], f["end"]) == (R.NO_TAIL, 0, 0, f["clip"][0], L - f["clip"][1]), (z, f)
        elif kind == "concatemer":
            assert (f["cls"], f["strand"], f["n_internal"]) == (R.CONCATEMER, 0, 2) and f["first_internal"] > 500 and f["end"] > f["start"] > 0, (z, f)
        elif kind == "oneprimer":
            assert (f["cls"], f["strand"], f["start"], f["end"], f["polya_len"], f["first_internal"]) == (R.ONE_END, -1, 0, 0, 0, -1) and f["dist"][0] == 0, (z, f)
        elif kind == "fivefive":
            assert (f["cls"], f["strand"], f["idx"], f["end"]) == (R.SAME_ROLE, -1, [0, 0], 0), (z, f)
        else:
            assert (f["tested"], f["cls"], f["strand"], f["n_internal"]) == (1, R.NO_PRIMER, -1, 0), (z, f)
        seen.add(kind)
    assert seen == set(LAB.KINDS) | {"fail"}
    # a run without the request after one with it: the plain results
    _same_results(handle.consensus(b), plain, b.n_zmw)


def test_three_tickets_with_their_own_sets_and_options(handle, lab):
    b, _, S, roles = lab
    sets = [(S, roles), (S[::-1], roles), (list(S) + [R.rc(S[0])], [0, 1, 1])]
    opts = [dict(), dict(min_polya=0, min_len=700, max_dist_pct=0), dict(max_dist_pct=30, window=40, polya_mismatch=1, polya_xdrop=0, min_len=1)]
    sync = [handle.consensus_cdna(b, api.CdnaPrimers.from_codes(*s), _opts(**o)) for s, o in zip(sets, opts)]
    pb = b.pinned()
    out = []
    for s, o in zip(sets, opts):
        res, rep = api.Results.allocate(b, pinned=True), _poisoned(b.n_zmw, pinned=True)
        out.append((handle.submit(pb, res, cdna=rep, cdna_primers=api.CdnaPrimers.from_codes(*s), cdna_opts=_opts(**o)), res, rep))
    for (t, res, rep), (sres, srep), s, o in zip(out, sync, sets, opts):
        handle.wait(t)
        _same_results(res, sres, b.n_zmw)
        assert R.diff(rep, _as_dict(srep)) == []
        _check_against_own_sequences(res, rep, s[0], s[1], b.n_zmw, **o)
        handle.release(t)
    assert R.diff(out[0][2], _as_dict(out[1][2])) != [] and R.diff(out[0][2], _as_dict(out[2][2])) != []     # (the tickets did differ)


def test_beside_the_adapter_and_coverage_screens(handle, lab):
    b, _, S, roles = lab
    n = b.n_zmw
    res0, vrep0, _, _, arep0, _, _ = handle.consensus_coverage(b, adapters=api.AdapterSet.default())
    arep, vrep = api.AdapterReport.allocate(n), api.CoverageReport.allocate(n)
    res, rep = handle.consensus_cdna(b, api.CdnaPrimers.from_codes(S, roles), adapters=arep, coverage=vrep)
    _same_results(res, res0, n)
    for k, _, _ in api.AdapterReport.PLANES:
        assert getattr(arep, k).tobytes() == getattr(arep0, k).tobytes(), k
    for k, _, _ in api.CoverageReport.PLANES:
        assert getattr(vrep, k).tobytes() == getattr(vrep0, k).tobytes(), k
    _check_against_own_sequences(res, rep, S, roles, n)


def test_the_refused_combinations(handle, lab):
    """with the heteroduplex request, the hand-off, the barcode, the represent and the segment request: refused before anything is enqueued, and the handle
    runs on"""
    b, _, S, roles = lab
    n = b.n_zmw
    pset, rep, res = api.CdnaPrimers.from_codes(S, roles), api.CdnaReport.allocate(n), api.Results.allocate(b)
    bset, sset = api.BarcodeSet.from_codes([a[:16] for a in S]), api.SegmentSet.from_codes(S)
    for kw in (dict(hd=api.HdReport.allocate(n)), dict(handoff=api.Handoff.allocate(b, 4)), dict(barcodes=api.BarcodeReport.allocate(n), barcode_set=bset),
               dict(represent=api.RepresentReport.allocate(n)), dict(segments=api.SegmentReport.allocate(n), segment_set=sset)):
        with pytest.raises(ValueError, match="cdna request is not combined"):
            handle.submit(b, res, cdna=rep, cdna_primers=pset, **kw)
    with pytest.raises(ValueError, match="cdna_primers is needed"):
        handle.submit(b, res, cdna=rep)
    res1, rep1 = handle.consensus_cdna(b, pset)
    _check_against_own_sequences(res1, rep1, S, roles, n)

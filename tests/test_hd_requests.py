"""The heteroduplex finder beside the other requests of the fused path (ccsx_consensus_hd_requests / ccsx_submit_hd_requests, include/ccsx.h): the entry
points' ABI and argument checks, and on an MI355X the call without requests against ccsx_consensus_hd, every report of a call that carries all requests against
the calls that carry one of them, the order in which the coverage gate and the split give a status, and api.consensus_hd_stream with requests passed through."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ccs_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["ccsx_consensus_hd_requests", "ccsx_submit_hd_requests"]


# ---------------------------------------------------------------- CPU: ABI and argument checks
def test_entry_points_match_the_header(built):
    """the two prototypes as include/ccsx.h declares them against the ctypes argument lists; the versions an additive change leaves alone"""
    text = open(os.path.join(ROOT, "include", "ccsx.h")).read()
    ctype = {"ccsx_handle": C.c_void_p, "const ccsx_batch *": C.POINTER(api.CBatch), "ccsx_results *": C.POINTER(api.CResults),
             "const ccsx_requests *": C.POINTER(api.CRequests), "const ccsx_hd_request *": C.POINTER(api.CHdRequest), "ccsx_ticket *": C.POINTER(C.c_int64)}
    L = api.lib()
    for entry in ENTRIES:
        m = re.search(r"^int\s+%s\(([^)]*)\);" % entry, text, re.M)
        assert m, entry
        args = [re.sub(r"\w+$", "", a.strip()).strip() for a in m.group(1).split(",")]
        assert [ctype[a] for a in args] == list(getattr(L, entry).argtypes), entry
        assert entry in api.EXPORTS
    assert len(L.ccsx_submit_hd_requests.argtypes) == len(L.ccsx_consensus_hd_requests.argtypes) + 1
    assert L.ccsx_abi_version() == 6 and L.ccsx_hd_rule_version() == 1 and L.ccsx_spec_version() == 8
    assert "#define CCSX_ABI_VERSION 6" in text and "#define CCSX_SPEC_VERSION 8" in text


def _request(rep, **kw):
    o = api.hd_opts_default()
    for k, v in kw.pop("opts", {}).items():
        setattr(o, k, v)
    cr = rep.c_struct()
    q = api.CHdRequest(C.pointer(o), C.pointer(cr), kw.pop("split", 0), kw.pop("reserved", 0))
    return q, (o, cr)


@pytest.mark.parametrize("entry", ENTRIES)
def test_entry_points_refuse_bad_requests(built, entry):
    """the list of test_hd_fused.py::test_entry_points_refuse_bad_requests with rq NULL and with an empty ccsx_requests, then a bad member of rq"""
    L = api.lib()
    import hd_synth
    b, _ = hd_synth.make(3, 3, 300, seed=2)
    res = api.Results.allocate(b)
    cb, cr = b.c_struct(), res.c_struct()
    t = C.c_int64(-7)

    def call(h, q, rq=None):
        args = [h, C.byref(cb), C.byref(cr), C.byref(rq) if rq is not None else None, q]
        rc = getattr(L, entry)(*(args + [C.byref(t)] if entry == "ccsx_submit_hd_requests" else args))
        assert rc == 0 or t.value == -7                             # a refused submit hands out no ticket
        return rc

    def empty():
        return api.CRequests(None, None, None, None, None, (C.c_void_p * 3)())

    rep = api.HdReport.allocate(b.n_zmw)
    bad = {
        "null request": None,
        "null request or report": C.byref(api.CHdRequest(None, None, 0, 0)),
        "reserved 0": _request(rep, reserved=1),
        "split must be 0 or 1": _request(rep, split=2),
        "options out of range": _request(rep, opts=dict(min_indel=22)),
        "sized for another batch": _request(api.HdReport.allocate(b.n_zmw + 1)),
    }
    for rq in (None, empty()):
        for msg, q in bad.items():
            if isinstance(q, tuple):
                q = C.byref(q[0])
            assert call(None, q, rq) < 0, msg
            assert msg.encode() in L.ccsx_last_error(), (msg, L.ccsx_last_error())
        q, keep = _request(rep, opts=dict(min_strand_passes=0))
        assert call(None, C.byref(q), rq) < 0 and b"options out of range" in L.ccsx_last_error()
        q, keep = _request(rep)                                       # a valid request: the handle is what is missing
        assert call(None, C.byref(q), rq) < 0 and b"null argument" in L.ccsx_last_error()
    # a bad member of rq beside a good heteroduplex request: refused by that member's own message
    q, keep = _request(rep)
    rq = empty()
    rq.reserved[1] = 8
    assert call(None, C.byref(q), rq) < 0 and b"ccsx_requests: reserved must be NULL" in L.ccsx_last_error()
    frep = api.FoldReport.allocate(b.n_zmw + 1).c_struct()
    fq = api.CFoldRequest(None, C.pointer(frep), (C.c_int32 * 2)(0, 0))
    rq = empty()
    rq.fold = C.pointer(fq)
    assert call(None, C.byref(q), rq) < 0 and b"sized for another batch" in L.ccsx_last_error()
    cq = api.CControlRequest(None, None, None, (C.c_int32 * 2)(0, 0))
    rq = empty()
    rq.control = C.pointer(cq)
    assert call(None, C.byref(q), rq) < 0 and b"null control request or report" in L.ccsx_last_error()
    vrep = api.CoverageReport.allocate(b.n_zmw).c_struct()
    vq = api.CCoverageRequest(None, C.pointer(vrep), 1, (C.c_int32 * 2)(0, 0))
    rq = empty()
    rq.coverage = C.pointer(vq)
    assert call(None, C.byref(q), rq) < 0 and b"gate has bits outside 2 .. 5" in L.ccsx_last_error()
    ex = api.CExtras(None, None, -1, 0)
    rq = empty()
    rq.ex = C.pointer(ex)
    assert call(None, C.byref(q), rq) < 0 and b"min_tandem_repeat_length must be >= 0" in L.ccsx_last_error()
    # a good coverage request with a gate beside a good heteroduplex request: accepted as far as the missing handle
    vq = api.CCoverageRequest(None, C.pointer(vrep), api.COVERAGE_GATE_ALL, (C.c_int32 * 2)(0, 0))
    rq = empty()
    rq.coverage = C.pointer(vq)
    assert call(None, C.byref(q), rq) < 0 and b"null argument" in L.ccsx_last_error()


def test_python_routes_the_request_beside_the_others(built):
    """_requests makes the CRequests without the finder's request and keeps it as a further argument; without hd_requests the combination stays refused"""
    hd, cov = api.HdReport.allocate(2), api.CoverageReport.allocate(2)
    ex, hq, fq, aq, cq, keep = api._requests(hd=hd, coverage=cov, hd_requests=True)
    assert hq is not None and isinstance(keep[-1], api.CRequests) and bool(keep[-1].coverage) and not keep[-1].fold
    ex, hq, fq, aq, cq, keep = api._requests(hd=hd, fold=api.FoldReport.allocate(2), hd_requests=True)
    assert hq is not None and isinstance(keep[-1], api.CRequests) and bool(keep[-1].fold)
    ex, hq, fq, aq, cq, keep = api._requests(hd=hd)                 # extras only: ccsx_*_hd as before
    assert hq is not None and not isinstance(keep[-1], api.CRequests)
    with pytest.raises(ValueError, match="heteroduplex"):
        api._requests(hd=hd, fold=api.FoldReport.allocate(2))


# ---------------------------------------------------------------- GPU
from test_hd_fused import _same_report, _same_zmw                   # noqa: E402  (the comparisons of the fused finder's tests)

_RUN = {}
COV_FIELDS = ("verdict", "np_aligned", "spans", "cov_max", "clean_min", "drop_window", "drop_windows", "reach_sum", "used_sum", "used_min")
PRE_POLISH = COV_FIELDS[:8]


@pytest.fixture(scope="module", autouse=True)
def _close_the_shared_handle():
    yield
    if _RUN:
        _RUN.pop("h").close()


def planted():
    """40 ZMWs of 1500 bases: 8 with three substitutions at 10 + 10 passes, 8 with a 30-bp insertion on one strand, 8 homoduplex controls, 8 of 2 .. 12 passes
    with partial passes (seed 86 draws two ZMWs of one pass per strand: below --min-passes, UNTESTED), 8 plain api.synth ZMWs"""
    import hd_synth
    return api.concat([hd_synth.make(8, 10, 1500, seed=81, k_sub=3)[0], hd_synth.make(8, 10, 1500, seed=82, indel=30)[0],
                       hd_synth.make(8, 10, 1500, seed=83, control=True)[0], hd_synth.make(8, (1, 6), 1500, seed=86, k_sub=2, partial=True)[0],
                       api.synth(8, 10, 1500, seed=85)])


def planted_yields(rep):
    """the condition every comparison rests on, from the library's own report: the planted set holds each kind"""
    het = rep.verdict == api.HD_HETERODUPLEX
    assert (het & (rep.n_sub_sites >= 2) & (rep.n_indel_sites == 0)).sum() >= 1, "no heteroduplex by substitution"
    assert (het & (rep.n_indel_sites >= 1)).sum() >= 1, "no heteroduplex by large indel"
    assert (rep.verdict == api.HD_DOUBLE_STRAND).sum() >= 1 and (rep.verdict == api.HD_UNTESTED).sum() >= 1


def _kin_handle():
    o = api.default_opts()
    o.hifi_kinetics = 1
    return api.Handle(0, opts=o)


def _cov_opts():
    """block 10: the passes that carry the planted 30-bp insertion count as carrying a block even where it straddles two windows, so the coverage screen and
    the finder claim the same ZMWs"""
    o = api.coverage_opts_default()
    o.block = 10
    return o


def _base():
    """one handle with kinetics and the runs every GPU test compares against, computed once and left unchanged"""
    if not _RUN:
        import control_synth as CS
        b = planted()
        h = _kin_handle()
        _RUN.update(h=h, b=b, control=api.ControlSeq.from_string(CS.TEST_CONTROL))
        for split in (False, True):
            _RUN["hd", split] = h.consensus_hd(b, split=split, tandem=True, pileup=True)
        planted_yields(_RUN["hd", False][1])
    return _RUN


def _same_cov(a, b, fields=COV_FIELDS, zs=None, what=""):
    for f in fields:
        x, y = getattr(a, f), getattr(b, f)
        assert np.array_equal(x if zs is None else x[zs], y if zs is None else y[zs]), (what, f)


def _same_planes(a, b, what=""):
    for name, dt, _ in type(a).PLANES:
        x, y = getattr(a, name), getattr(b, name)
        for f in (np.dtype(dt).names or (None,)):                     # (a struct's fields one by one: the bytes of its padding are not a result)
            u, v = (x, y) if f is None else (np.ascontiguousarray(x[f]), np.ascontiguousarray(y[f]))
            assert u.tobytes() == v.tobytes(), (what, name, f)


@pytest.mark.gpu
def test_without_requests_it_is_consensus_hd(built):
    R = _base()
    h, b = R["h"], R["b"]
    for split in (False, True):
        want, wrep, wt, wp = R["hd", split]
        for via in (True, False):                                     # an empty rq with only `ex`; and rq->ex alone through the old form
            got, rep, _, _, _, _, gt, gp = h.consensus_hd_requests(b, split=split, tandem=True, pileup=True, via_requests=via)
            _same_report(rep, wrep, (split, via))
            assert np.array_equal(gt, wt)
            for z in range(b.n_zmw):
                _same_zmw(want, got, z, wp, gp)
        # rq = NULL: the raw call
        res = api.Results.allocate(b, kinetics=True)
        rep = api.HdReport.allocate(b.n_zmw)
        o, cr = api.hd_opts_default(), rep.c_struct()
        q = api.CHdRequest(C.pointer(o), C.pointer(cr), int(split), 0)
        cb, crs = b.c_struct(), res.c_struct()
        assert api.lib().ccsx_consensus_hd_requests(h._h, C.byref(cb), C.byref(crs), None, C.byref(q)) == 0, api.lib().ccsx_last_error()
        plain, prep, _, _ = h.consensus_hd(b, split=split)
        _same_report(rep, prep, split)
        for z in range(b.n_zmw):
            _same_zmw(plain, res, z)


@pytest.mark.gpu
def test_every_request_in_one_call(built):
    """fold + adapters + control + coverage (gate 0) beside the finder: the finder's report is ccsx_consensus_hd's, every screen's report that of
    ccsx_consensus_requests without the finder, and without the split every result byte too"""
    R = _base()
    h, b, ctl = R["h"], R["b"], R["control"]
    kw = dict(control=ctl, fold=True, adapters=api.AdapterSet.default(), tandem=True, pileup=True)
    want, vrep, crep, frep, arep, wt, wp = h.consensus_coverage(b, _cov_opts(), gate=0, **kw)
    assert (vrep.verdict >= 2).sum() >= 1 and (vrep.used_sum > 0).sum() >= 20
    for split in (False, True):
        got, rep, gv, gc, gf, ga, gt, gp = h.consensus_hd_requests(b, split=split, coverage=_cov_opts(), gate=0, **kw)
        _same_report(rep, R["hd", split][1], split)
        _same_planes(gc, crep, "control"); _same_planes(gf, frep, "fold"); _same_planes(ga, arep, "adapters")
        assert np.array_equal(gt, wt)
        het = rep.verdict == api.HD_HETERODUPLEX
        if not split:
            _same_cov(gv, vrep)
            for z in range(b.n_zmw):
                _same_zmw(want, got, z, wp, gp)
            continue
        # the split: a HETERODUPLEX ZMW keeps its pre-polish planes and, not polished, has used nothing; every other ZMW is untouched
        _same_cov(gv, vrep, PRE_POLISH[1:])
        _same_cov(gv, vrep, COV_FIELDS, np.flatnonzero(~het))
        assert np.array_equal(gv.verdict[het], np.where(vrep.verdict[het] == 5, 1, vrep.verdict[het]))   # (verdict 5 is reached after the polish only: NONE before it)
        assert not gv.used_sum[het].any() and not gv.used_min[het].any() and het.sum() >= 2
        split_only = R["hd", True][0]
        for z in range(b.n_zmw):
            _same_zmw(split_only if het[z] else want, got, z, None if het[z] else wp, None if het[z] else gp)
            assert int(got.status[z]) == (api.HETERODUPLEX if het[z] else int(want.status[z]))


def expected_status(cov0, hd0, gated_only, gate):
    """DESIGN.md §2 "In the fused path": the coverage gate's pre-polish verdicts first, then the finder's split, then whatever the polish and the post-polish
    gate make of the rest (the statuses of the run with the gate alone)"""
    out = []
    for z in range(len(cov0.verdict)):
        v = int(cov0.verdict[z])
        if 2 <= v <= 4 and (gate >> v) & 1:
            out.append(9 + v)
        elif hd0.verdict[z] == api.HD_HETERODUPLEX:
            out.append(api.HETERODUPLEX)
        else:
            out.append(int(gated_only.status[z]))
    return np.array(out)


@pytest.mark.gpu
def test_the_coverage_gate_precedes_the_split(built):
    R = _base()
    h, b = R["h"], R["b"]
    hd0, split_only = R["hd", False][1], R["hd", True][0]
    plain = R["hd", False][0]
    _, cov0, *_ = h.consensus_coverage(b, _cov_opts(), gate=0)
    both = (cov0.verdict >= 2) & (cov0.verdict <= 4) & (hd0.verdict == api.HD_HETERODUPLEX)
    assert both.sum() >= 1, "no ZMW that the gate and the split both claim"
    for gate in (api.COVERAGE_GATE_ALL, 1 << 3):                      # every verdict gated; INSUFFICIENT_SPANS only: the split gets the ZMWs with drops
        gated_only, covg, *_ = h.consensus_coverage(b, _cov_opts(), gate=gate)
        got, rep, gv, *_ = h.consensus_hd_requests(b, split=True, coverage=_cov_opts(), gate=gate)
        want = expected_status(cov0, hd0, gated_only, gate)
        assert np.array_equal(got.status, want), (gate, got.status, want)
        by_gate = np.array([2 <= int(v) <= 4 and (gate >> int(v)) & 1 for v in cov0.verdict], bool)
        by_split = ~by_gate & (hd0.verdict == api.HD_HETERODUPLEX)
        assert by_split.sum() >= 1 and (by_gate.sum() >= 1 or gate != api.COVERAGE_GATE_ALL)
        if gate == api.COVERAGE_GATE_ALL:
            assert (by_gate & both).sum() >= 1
        else:
            assert (by_split & both).sum() >= 1
        # the finder: a gated ZMW is UNTESTED and carries its gate status, every other ZMW is as without the coverage request
        assert (rep.verdict[by_gate] == api.HD_UNTESTED).all() and np.array_equal(rep.status[by_gate], want[by_gate])
        assert not rep.n_sub_sites[by_gate].any() and not rep.n_indel_sites[by_gate].any() and not rep.n_listed[by_gate].any()
        free = np.flatnonzero(~by_gate)
        for k in ("verdict", "n_sub_sites", "n_indel_sites", "n_listed", "status"):
            assert np.array_equal(getattr(rep, k)[free], getattr(hd0, k)[free]), (gate, k)
        assert np.array_equal(rep.min_p[free].view(np.uint64), hd0.min_p[free].view(np.uint64))
        # the coverage report: the pre-polish planes of every ZMW do not depend on the finder; a split ZMW used nothing
        _same_cov(gv, covg, PRE_POLISH[1:])
        _same_cov(gv, covg, COV_FIELDS, np.flatnonzero(~by_split))
        assert not gv.used_sum[by_split].any() and not gv.used_min[by_split].any()
        for z in range(b.n_zmw):                                      # results: the gate's ZMWs as the gate alone leaves them, the split's as the split alone
            _same_zmw(split_only if by_split[z] else gated_only, got, z)
            if not by_gate[z] and not by_split[z] and gated_only.status[z] == plain.status[z]:
                _same_zmw(plain, got, z)                              # neither path touched it
        # the ticketed form
        bp = b
        res = api.Results.allocate(bp, kinetics=True, pinned=True)
        trep, tcov = api.HdReport.allocate(b.n_zmw, pinned=True), api.CoverageReport.allocate(b.n_zmw, pinned=True)
        t = h.submit(bp, res, hd=trep, hd_split=True, coverage=tcov, coverage_opts=_cov_opts(), coverage_gate=gate)
        h.wait(t)
        h.release(t)
        _same_report(trep, rep, gate)
        _same_cov(tcov, gv)
        for z in range(b.n_zmw):
            _same_zmw(got, res, z)


@pytest.mark.gpu
def test_stream_passes_the_requests_through(built):
    """requests that take no read away (fold, adapters, control, coverage without a gate, pileup, tandem detection): the records of the plain stream; the
    reports of an hd ticket equal the synchronous call's, a strand ticket carries the same requests and no finder"""
    import hd_synth
    R = _base()
    h, ctl = R["h"], R["control"]
    bs = [R["b"], hd_synth.make(6, 8, 1200, seed=91, k_sub=4)[0], api.synth(5, 8, 1000, seed=92)]
    plain = list(api.consensus_hd_stream(h, bs))
    tickets = []
    got = list(api.consensus_hd_stream(h, bs, tickets_out=tickets, fold=True, adapter_set=api.AdapterSet.default(), control_seq=ctl, coverage=_cov_opts(),
                                       pileup=True, tandem=True))
    assert len(got) == len(plain) == len(bs)
    n_ss = 0
    for (recs, rep), (want, wrep) in zip(got, plain):
        _same_report(rep, wrep)
        assert len(recs) == len(want)
        for x, y in zip(recs, want):
            assert (x.zmw, x.zmw_id, x.group, x.status, x.np_) == (y.zmw, y.zmw_id, y.group, y.status, y.np_)
            assert np.array_equal(x.seq, y.seq) and np.array_equal(x.qual, y.qual) and np.float32(x.rq).tobytes() == np.float32(y.rq).tobytes()
            n_ss += x.group != "DS"
    assert n_ss >= 4
    kinds = [(i, kind) for i, kind, *_ in tickets]
    assert [k for k in kinds if k[1] == "hd"] == [(i, "hd") for i in range(len(bs))] and (0, "strand") in kinds and (1, "strand") in kinds
    for i, kind, tb, tres, kw in tickets:
        assert {"fold", "adapters", "control", "coverage", "pileup", "tandem"} <= set(kw) and "hd" not in kw
        if kind == "strand":                                           # an ordinary ticket with the run's requests: the synchronous call without a finder
            want, vrep, crep, frep, arep, wt, wp = h.consensus_coverage(tb, _cov_opts(), control=ctl, fold=True, adapters=api.AdapterSet.default(), tandem=True,
                                                                        pileup=True)
            _same_cov(kw["coverage"], vrep)
        else:
            want, _, vrep, crep, frep, arep, wt, wp = h.consensus_hd_requests(tb, split=True, coverage=_cov_opts(), control=ctl, fold=True,
                                                                             adapters=api.AdapterSet.default(), tandem=True, pileup=True)
            _same_cov(kw["coverage"], vrep)
        _same_planes(kw["control"], crep); _same_planes(kw["fold"], frep); _same_planes(kw["adapters"], arep)
        assert np.array_equal(kw["tandem"][: tb.n_zmw], wt)
        for z in range(tb.n_zmw):
            _same_zmw(want, tres, z, wp, kw["pileup"])

"""The three draft screens at their kernels' limits, on an MI355X (DESIGN.md §2 "Adapter palindromes", "Adapter screen", "Control screen").  The limit sets
of tests/screen_lab.py are handed to k_fold, k_adapter and k_control as exact bytes: every ZMW has three identical passes on alternating strands, so the POA
draft is the template itself (tests/test_screen_limits.py holds that for the oracle; here it is asserted of the engine's draft for every ZMW).  Per screen one
handle; per batch of the set every request of the batch runs over every draft of the batch, and every field of every ZMW must equal fold_ref / adapter_ref /
control_ref.  Nothing is left out: every ZMW's draft stage ends with status 0 and every report says tested.  Each request runs a second time with the ZMWs in
reverse order (the screens take the ZMWs longest first through zmw_perm), through a ticket whose report arrays the caller poisoned with 0xA5."""
import numpy as np
import pytest

from ccs_amd import api
import adapter_ref as AR
import control_ref as CR
import screen_lab as LAB
import sdust_lab
import test_adapters as TA
import test_control as TC
import test_fold as TF
from test_screen_limits import unique_drafts


def _set(o, d):
    for k, v in d.items():
        setattr(o, k, v)
    return o


def _fold_opts(d):
    return _set(api.fold_opts_default(), d)


def _adapter_opts(d):
    return _set(api.adapter_opts_default(), d)


def _control_opts(d):
    return _set(api.control_opts_default(), d)


def _poisoned(cls, n):
    """a pinned report of the caller's, every byte 0xA5"""
    rep = cls.allocate(n, pinned=True)
    for k, _, _ in cls.PLANES:
        getattr(rep, k).view(np.uint8)[...] = 0xA5
    return rep


def _planes(rep) -> bytes:
    return b"".join(np.ascontiguousarray(getattr(rep, k)).tobytes() for k, _, _ in rep.PLANES)


def _reversed_planes(rep) -> bytes:
    return b"".join(np.ascontiguousarray(getattr(rep, k)[::-1]).tobytes() for k, _, _ in rep.PLANES)


def _exact_batch(h, cases):
    """(drafts, batch, reversed batch, draft seam): every ZMW's draft stage succeeds and hands the planted draft back, byte for byte"""
    drafts = [d for d, _ in unique_drafts(cases)]
    names = [n for _, n in unique_drafts(cases)]
    b = sdust_lab.batch_from_drafts(drafts)
    d = h.draft(b)
    for z, want in enumerate(drafts):
        assert d.status[z] == 0, (names[z], int(d.status[z]))
        assert np.array_equal(d.draft(z), want), names[z]
    return drafts, names, b, sdust_lab.batch_from_drafts(drafts[::-1], seed=1), d


def _handed_back(h, drafts, names):
    """after a consensus call: the draft the screens were given is the planted one"""
    for z, want in enumerate(drafts):
        assert np.array_equal(h.stage_draft(z), want), names[z]


def _ticket(h, b, **requests):
    res = api.Results.allocate(b, pinned=True)
    h.wait(h.submit(b, res, **requests))
    return res


@pytest.mark.gpu
def test_fold_limit_set(built):
    S = LAB.fold_cases()
    h = api.Handle(0)
    for bname, keys in S.batch_requests.items():
        drafts, names, b, b_rev, d = _exact_batch(h, S.batch(bname))
        n = len(drafts)
        for key in keys:
            o = S.requests[key]
            res, rep = h.consensus_fold(b, _fold_opts(o))
            if key == keys[0]:
                _handed_back(h, drafts, names)
            assert TF._check_report(d, rep, o) == n, (bname, key)
            assert (rep.verdict != api.FOLD_UNTESTED).all()
            for c in S.batch(bname):                                 # the named case under its own request, by name
                if c.request == key:
                    z = next(z for z, x in enumerate(drafts) if x is c.draft or np.array_equal(x, c.draft))
                    got = (int(rep.verdict[z]), int(rep.fold[z]), int(rep.hits[z]), int(rep.span[z]))
                    assert got == LAB.FR.fold(c.draft, opts=o), (c.name, got)
            back = _poisoned(api.FoldReport, n)
            _ticket(h, b_rev, fold=back, fold_opts=_fold_opts(o))
            assert _reversed_planes(back) == _planes(rep), (bname, key)
    h.close()


@pytest.mark.gpu
def test_adapter_limit_set(built):
    S = LAB.adapter_cases()
    h = api.Handle(0)
    for bname, keys in S.batch_requests.items():
        drafts, names, b, b_rev, d = _exact_batch(h, S.batch(bname))
        n = len(drafts)
        for key in keys:
            rq = S.requests[key]
            aset = api.AdapterSet.from_strings(rq["adapters"])
            res, _, rep, _, _ = h.consensus_screen(b, adapters=aset, opts=_adapter_opts(rq["opts"]))
            if key == keys[0]:
                _handed_back(h, drafts, names)
            assert len(TA._check_report(d, rep, rq["adapters"], rq["opts"])) == n, (bname, key)
            assert (rep.tested == 1).all()
            back = _poisoned(api.AdapterReport, n)
            _ticket(h, b_rev, adapters=back, adapter_set=aset, adapter_opts=_adapter_opts(rq["opts"]))
            assert _reversed_planes(back) == _planes(rep), (bname, key)
    c = S.case("list/1025_hits_16th_end_shared")                     # (the overflow pass ran: more hits than the buffer holds, and still the first 16)
    assert AR.screen(c.draft, S.requests[c.request]["adapters"], S.requests[c.request]["opts"])["n_hits"] == LAB.BUF + 1
    h.close()


@pytest.mark.gpu
def test_control_limit_set(built):
    S = LAB.control_cases()
    h = api.Handle(0)
    for bname, keys in S.batch_requests.items():
        drafts, names, b, b_rev, d = _exact_batch(h, S.batch(bname))
        n = len(drafts)
        for key in keys:
            rq = S.requests[key]
            seq = api.ControlSeq.from_codes(rq["control"])
            res, rep, _, _, _, _ = h.consensus_control(b, seq, _control_opts(rq["opts"]))
            if key == keys[0]:
                _handed_back(h, drafts, names)
            assert len(TC._check_report(d, rep, rq["control"], rq["opts"])) == n, (bname, key)
            L14 = [z for z, x in enumerate(drafts) if len(x) < LAB.K]
            assert (rep.verdict != CR.UNTESTED).all() and all(rep.verdict[z] == CR.NONE for z in L14)
            back = _poisoned(api.ControlReport, n)
            _ticket(h, b_rev, control=back, control_seq=seq, control_opts=_control_opts(rq["opts"]))
            assert _reversed_planes(back) == _planes(rep), (bname, key)
    h.close()


@pytest.mark.gpu
def test_three_screens_in_one_call_equal_the_separate_calls(built):
    """the union of the three sets (the 25 kb draft left to its own test: it alone would double this one's time) through one consensus_control call that carries
    all three requests, against one call per screen on the same batch: every report byte for byte"""
    F, A, C = LAB.fold_cases(), LAB.adapter_cases(), LAB.control_cases()
    cases = [c for S in (F, A, C) for c in S.cases if c.batch != "cap3072"]
    h = api.Handle(0)
    drafts, names, b, _, d = _exact_batch(h, cases)
    fo = _fold_opts(LAB.ONE)
    arq, crq = A.requests["eight/pct20"], C.requests["c100"]
    aset, ao = api.AdapterSet.from_strings(arq["adapters"]), _adapter_opts(arq["opts"])
    seq, co = api.ControlSeq.from_codes(crq["control"]), _control_opts(crq["opts"])
    _, crep, frep, arep, _, _ = h.consensus_control(b, seq, co, fold=fo, adapters=aset, adapter_opts=ao)
    _handed_back(h, drafts, names)
    _, f1 = h.consensus_fold(b, fo)
    _, _, a1, _, _ = h.consensus_screen(b, adapters=aset, opts=ao)
    _, c1, _, _, _, _ = h.consensus_control(b, seq, co)
    assert _planes(frep) == _planes(f1) and _planes(arep) == _planes(a1) and _planes(crep) == _planes(c1)
    assert (frep.verdict != api.FOLD_UNTESTED).all() and (arep.tested == 1).all() and (crep.verdict != CR.UNTESTED).all()
    assert TF._check_report(d, frep, LAB.ONE) == len(drafts)
    h.close()

"""The representative rule on the CPU (DESIGN.md §2 "Representative rule"): ccsx_represent_host against tests/represent_ref.py on the limit set — class, pass and
every byte of every plane, on poisoned planes, so that a byte written where the rule writes none shows —, the restatement's median against the rank count it
stands in for, the structs against the header, and every argument error of the host call."""
import ctypes as C

import numpy as np
import pytest

from ccs_amd import api
import oracle_lib
import represent_lab as LAB
import represent_ref as R

CASES = R.limit_cases()


def _opts(top_passes=0, hifi_kinetics=0):
    o = api.default_opts()
    o.top_passes, o.hifi_kinetics = top_passes, hifi_kinetics
    return o


def _run(case, fallback, kinetics, raw=True, high_bits=False):
    name, zmws, top, status, drafts = case
    b = R.make_batch(zmws, seed=5, high_bits=high_bits)
    start = R.poisoned_results(b, kinetics=bool(kinetics), raw=raw)
    want, got = R.clone(start), R.clone(start)
    wcls, wpass = R.apply(b, top, status, drafts, want, fallback, kinetics)
    rep = api.represent_host(b, _opts(top, int(kinetics)), status, drafts, got, fallback, kinetics)
    return b, start, want, got, wcls, wpass, rep


@pytest.mark.parametrize("kinetics", (0, 1))
@pytest.mark.parametrize("fallback", (0, 1))
@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0] for c in CASES])
def test_host_equals_the_restatement_on_the_limit_set(built, i, fallback, kinetics):
    b, start, want, got, wcls, wpass, rep = _run(CASES[i], fallback, kinetics, high_bits=bool(i & 1))
    assert rep.cls.tolist() == wcls.tolist() and rep.pass_.tolist() == wpass.tolist()
    assert R.diff(got, want) == []
    for z in range(b.n_zmw):                                         # nothing of a POLISHED or NONE ZMW is touched, status and counts of no ZMW
        if wcls[z] in (R.POLISHED, R.NONE):
            assert R.diff_zmw(got, start, z) == [], z
        else:
            assert set(R.diff_zmw(got, start, z)) <= {"seq_len", "rq", "ec", "seq", "qual", "raw_qv", "kin"}, z
            assert got.rq[z] == -1.0 and got.ec[z] == 0.0 and (got.quals(z) == 10).all() and (got.raw(z) == 10.0).all() and (got.sequence(z) <= 3).all()
            o, L = int(got.seq_off[z]), int(got.seq_len[z])
            if kinetics:
                assert (got.kin[2:, o:o + L] == R.POISON).all()      # ri / rp are not written
                assert (got.kin[:2, o:o + L] == R.POISON).all() == (wcls[z] == R.DRAFT) or L == 0


def test_the_limit_set_holds_what_it_is_for(built):
    seen_cls, seen_len, by_name = set(), set(), {}
    for fb in (0, 1):
        for case in CASES:
            b, start, want, got, wcls, wpass, rep = _run(case, fb, 0)
            by_name[(case[0], fb)] = (b, want, wcls, wpass)
            seen_cls |= set(wcls.tolist())
            seen_len |= {int(want.seq_len[z]) for z in range(b.n_zmw) if wcls[z] >= R.DRAFT}
    assert seen_cls == {0, 1, 2, 3} and set(R.LENGTHS) <= seen_len
    b, want, cls, pas = by_name[("statuses", 0)]
    assert cls.tolist() == [0, 3, 2, 2, 2, 1, 1, 0, 2, 2, 2] + [0, 3, 3, 3, 3, 1, 1, 0, 3, 3, 3]
    assert by_name[("statuses", 1)][2].tolist() == [0, 3, 3, 3, 3, 1, 1, 0, 3, 3, 3] * 2
    b, want, cls, pas = by_name[("nall", 0)]
    assert cls.tolist() == [R.NONE] + [R.SUBREAD] * 5 and pas[:3].tolist() == [-1, 0, 0]   # (of lengths 30, 29: rank 1 is the longer)
    assert pas[4] == pas[3] and pas[4] < 255 and pas[5] == 254      # the cut: passes 255 .. 259 do not count, the only full-length pass is the set
    assert by_name[("top_passes_2", 0)][3].tolist() == [0, 0]       # of (50, 40 | 30, 20, 10): rank 1 of the first two; of two partial passes: rank 1
    assert by_name[("ties", 0)][3].tolist() == [1, 1, 2, 2, 2, 2, 1]
    assert by_name[("draft_beyond_slot", 0)][2].tolist() == [R.NONE, R.DRAFT] and by_name[("draft_beyond_slot", 1)][2].tolist() == [R.SUBREAD] * 2
    b, want, cls, pas = by_name[("ties", 0)]
    assert b.flags[b.read_off[1] + pas[1]] & 1 and b.flags[b.read_off[3] + pas[3]] & 1   # a representative on the reverse strand: native orientation
    z = 1
    o = int(b.base_off[b.read_off[z] + pas[z]])
    assert np.array_equal(want.sequence(z), b.bases[o:o + want.seq_len[z]] & 3)


@pytest.mark.parametrize("seed", range(3))
def test_median_is_the_rank_count(seed):
    """the sort of tuples picks the pass that exactly |C| // 2 members precede in (length, index) order — k_poa_init's definition"""
    rng = np.random.default_rng(seed)
    for _ in range(200):
        k = int(rng.integers(1, 12))
        lens = rng.integers(1, 5, k).tolist()
        flags = (rng.integers(0, 2, k) * 2 | rng.integers(0, 2, k)).tolist()
        nfull = sum(1 for f in flags if not f & 2)
        C_ = [q for q in range(k) if nfull == 0 or not flags[q] & 2]
        ranks = {i: sum(1 for q in C_ if lens[q] < lens[i] or (lens[q] == lens[i] and q < i)) for i in C_}
        assert ranks[R.median_pass(lens, flags)] == len(C_) // 2


def test_without_a_raw_plane_and_with_none_asked_for(built):
    b, start, want, got, wcls, wpass, rep = _run(CASES[0], 0, 0, raw=False)
    assert got.raw_qv is None and R.diff(got, want) == []


def test_structs_and_version(built):
    assert api.lib().ccsx_represent_rule_version() == 1
    assert C.sizeof(api.CRepresentRequest) == 24 and api.CRepresentRequest.report.offset == 8 and api.CRepresentRequest.reserved.offset == 16
    assert C.sizeof(api.CRepresentReport) == 24 and api.CRepresentReport.cls.offset == 8
    assert (api.REPRESENT_POLISHED, api.REPRESENT_NONE, api.REPRESENT_DRAFT, api.REPRESENT_SUBREAD) == (0, 1, 2, 3)
    assert api.lib().ccsx_abi_version() == 6                          # the pinned versions stay


def _call(b, opts, status, drafts, res, req, ipd=True):
    n = b.n_zmw
    st = np.ascontiguousarray(status, np.int32)
    dlen = np.array([len(d) for d in drafts], np.int32).reshape(n)
    doff = np.concatenate([[0], np.cumsum(dlen[:-1])]).astype(np.int64)
    dseq = np.concatenate(list(drafts) + [np.zeros(1, np.uint8)]).astype(np.uint8)
    cb, cr = b.c_struct(), res.c_struct()
    if not ipd:
        cb.ipd = None
    p = api._ptr
    rc = api.lib().ccsx_represent_host(C.byref(cb), C.byref(opts), p(st, C.c_int32), p(dseq, C.c_uint8), p(doff, C.c_int64), p(dlen, C.c_int32),
                                       C.byref(req) if req is not None else None, C.byref(cr))
    return rc, api.lib().ccsx_last_error().decode()


def test_argument_errors_leave_everything_alone(built):
    name, zmws, top, status, drafts = CASES[0]
    b = R.make_batch(zmws, seed=5)
    start = R.poisoned_results(b, kinetics=True)
    n = b.n_zmw

    def refused(words, opts=None, req=None, report=None, null_req=False, **fields):
        res, rep = R.clone(start), report if report is not None else api.RepresentReport.allocate(n)
        rep.cls[...] = -7; rep.pass_[...] = -7
        crep = rep.c_struct()
        for k, v in fields.pop("crep", {}).items():
            setattr(crep, k, v)
        q = api.CRepresentRequest(0, 0, C.pointer(crep), (C.c_int32 * 2)(0, 0))
        for k, v in fields.items():
            setattr(q, k, v)
        rc, err = _call(b, opts or _opts(0, 1), status, drafts, res, None if null_req else q)
        assert rc == -1 and words in err, (rc, err)
        assert R.diff(res, start) == [] and (rep.cls == -7).all() and (rep.pass_ == -7).all()
    refused("null represent request", null_req=True)
    q = api.CRepresentRequest(0, 0, None, (C.c_int32 * 2)(0, 0))
    rc, err = _call(b, _opts(0, 1), status, drafts, R.clone(start), q)
    assert rc == -1 and "null represent report" in err
    refused("sized for another batch", report=api.RepresentReport.allocate(n + 1))
    refused("sized for another batch", crep={"cls": None})
    refused("reserved must be 0", reserved=(C.c_int32 * 2)(0, 1))
    refused("reserved must be 0", reserved=(C.c_int32 * 2)(5, 0))
    refused("must be 0 or 1", subread_fallback=2)
    refused("must be 0 or 1", kinetics=-1)
    refused("needs opts.hifi_kinetics", opts=_opts(0, 0), kinetics=1)
    res = R.clone(start)
    rep = api.RepresentReport.allocate(n)
    crep = rep.c_struct()
    q = api.CRepresentRequest(0, 1, C.pointer(crep), (C.c_int32 * 2)(0, 0))
    rc, err = _call(b, _opts(0, 1), status, drafts, res, q, ipd=False)
    assert rc == -1 and "needs batch.ipd" in err and R.diff(res, start) == []
    # a results struct that is not on the batch's capacity layout
    other = R.poisoned_results(R.make_batch(zmws[:-1] + [[(np.zeros(99, np.uint8), 0)]], seed=5))
    rep = api.RepresentReport.allocate(n)
    crep = rep.c_struct()
    q = api.CRepresentRequest(0, 0, C.pointer(crep), (C.c_int32 * 2)(0, 0))
    rc, err = _call(b, _opts(0, 0), status, drafts, other, q)
    assert rc == -1 and "capacity layout" in err


def test_the_lab_reaches_its_statuses_on_the_oracle(built):
    """what tests/test_represent_gpu.py builds on, on the CPU restatement of the whole path at min_passes 2: the unrelated passes end TOO_MANY_UNUSABLE after the
    cascade, the ZMWs of fewer than two full-length passes TOO_FEW_PASSES, the neighbours with a consensus"""
    b, kinds = LAB.batch()
    o = api.default_opts()
    o.min_passes = 2
    ref = api.Results.allocate(b)
    oracle_lib.consensus_batch(api.default_model(), o, b, ref)
    assert b.n_zmw == len(kinds) == 21
    for z, kind in enumerate(kinds):
        want = {"polished": (R.SUCCESS, R.LOW_RQ), "few": (R.TOO_FEW_PASSES,), "unrelated": (R.TOO_MANY_UNUSABLE,)}[kind]
        assert int(ref.status[z]) in want, (z, kind, int(ref.status[z]))
    assert kinds.count("unrelated") == 4 and kinds.count("few") == 10

"""Control screen (DESIGN.md §2 "Control screen"; docs/faq/fail-reads.md fail class 0x2): the restatement against a brute-force reading of the rule, exact
fields by hand, verdicts on planted templates, the request's ABI and argument checks, and on an MI355X exact parity of k_control with the restatement on the
engine's own drafts, no effect on any result, and tickets that carry different controls against the synchronous call."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from ccs_amd import api
import control_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
K = R.K
LOOSE = dict(max_occ=1, min_matched=1, min_ctl_tenths=0, min_draft_tenths=0)
NONDEFAULT = dict(max_occ=2, min_matched=10, min_ctl_tenths=3, min_draft_tenths=6)


def _edge_cases(rng):
    """(name, draft, control, the options to try): drafts of 0-600 bases against controls of 64-200 bases"""
    import control_synth as S
    rnd = lambda m: rng.integers(0, 4, int(m)).astype(np.uint8)
    nz = lambda t: S.noisy(rng, t, 0.03, 0.02)
    c = rnd(rng.integers(64, 201))
    c64 = rnd(64)
    unit = np.tile(rnd(20), 10)
    acgt = np.tile(np.array([0, 1, 2, 3], np.uint8), 16)
    one_deleted = np.concatenate([rnd(15), c64[:30], c64[31:]])      # d = 64 before the deletion, 63 after it
    usual = (None, LOOSE, NONDEFAULT)
    caps = tuple(dict(LOOSE, max_occ=m) for m in (1, 4, 64))
    return [("L = 0", np.zeros(0, np.uint8), c, usual), ("L = K - 1", c[:K - 1].copy(), c, usual), ("L = K", c[5:5 + K].copy(), c, usual),
            ("draft == control", c.copy(), c, usual), ("draft == rc(control)", R.revcomp(c), c, usual),
            ("M = 64", np.concatenate([rnd(40), nz(c64), rnd(30)]), c64, usual),
            ("repeated unit", np.concatenate([rnd(30), nz(unit[7:150]), rnd(20)]), unit, caps),
            ("homopolymer", np.zeros(120, np.uint8), np.zeros(100, np.uint8), caps),
            ("ACGT tandem", np.concatenate([rnd(20), acgt[:40], rnd(20)]), acgt, caps),
            ("two copies", np.concatenate([c, rnd(rng.integers(0, 100)), nz(c)]), c, usual),
            ("bin boundary", one_deleted, c64, usual),
            ("orientations tie", np.concatenate([c[:100], R.revcomp(c[:100])]), c[:100].copy(), usual),
            ("noisy rc inside", np.concatenate([rnd(rng.integers(0, 200)), nz(R.revcomp(c)), rnd(rng.integers(0, 200))]), c, usual),
            ("random", rnd(rng.integers(100, 600)), c, usual)]


# ---------------------------------------------------------------- CPU: the restatement
@pytest.mark.parametrize("seed", range(5))
def test_restatement_equals_the_bruteforce(seed):
    rng = np.random.default_rng(seed)
    got = {}
    for name, d, c, opts in _edge_cases(rng):
        for o in opts:
            want = R.screen_bruteforce(d, c, o)
            assert R.screen(d, c, o) == want, (name, o, want)
            got.setdefault(name, []).append(want)
    none = dict(zip(R.FIELDS, (R.NONE, -1, 0, 0, 0, 0, 0, 0)))
    assert got["L = 0"][0] == got["L = K - 1"][0] == got["homopolymer"][2] == none
    assert got["L = K"][1]["hits"] == 1 and got["L = K"][1]["verdict"] == R.FOUND and got["L = K"][0]["verdict"] == R.NONE
    assert [r["hits"] for r in got["repeated unit"]][0] == 0 and got["repeated unit"][2]["hits"] > got["repeated unit"][2]["matched"] > 0
    t = got["ACGT tandem"][2]                                       # every k-mer of the tandem is the reverse complement of another: both orientations hit
    assert t["hits"] > 0 and t["strand"] >= 0
    two = got["two copies"][1]
    assert two["hits"] >= two["matched"] >= 64 - K + 1
    b = got["bin boundary"][1]
    assert b["hits"] == b["matched"] >= 64 - K + 1 - K and b["hits"] < 64 - K + 1 and (b["ctl_start"], b["ctl_end"], b["draft_start"], b["draft_end"]) == (0, 64, 15, 78)
    tie = got["orientations tie"][1]
    assert tie["strand"] == 0 and tie["hits"] == 100 - K + 1 and (tie["draft_start"], tie["draft_end"]) == (0, 100)
    assert R.screen(np.zeros(50, np.uint8), np.zeros(64, np.uint8), tested=False) == R.screen_bruteforce(np.zeros(50, np.uint8), np.zeros(64, np.uint8), tested=False) \
        == dict(zip(R.FIELDS, (R.UNTESTED, -1, 0, 0, 0, 0, 0, 0)))


def test_two_copies_count_distinct_control_positions():
    rng = np.random.default_rng(3)
    c = rng.integers(0, 4, 150).astype(np.uint8)
    d = np.concatenate([c, rng.integers(0, 4, 10).astype(np.uint8), c])     # diagonals 160 apart: three bins, so one copy wins
    r = R.screen(d, c, LOOSE)
    assert r == R.screen_bruteforce(d, c, LOOSE) and r["hits"] == r["matched"] == 136
    c = c[:64].copy()
    d = np.concatenate([c, c])                                              # diagonals 49 and 113: both copies in the winning pair of bins
    r = R.screen(d, c, LOOSE)
    assert r == R.screen_bruteforce(d, c, LOOSE) and r["matched"] == 50 and r["hits"] == 100 and (r["draft_start"], r["draft_end"]) == (0, 128)


def test_fields_by_hand():
    import control_synth as S
    c = S.encode(S.TEST_CONTROL)
    assert len(c) == 2000 and len(np.unique(R.codes(c)[0])) == 1986 and S.TEST_CONTROL != S.TEST_CONTROL_B and len(S.TEST_CONTROL_B) == 2000
    assert R.screen(c, c) == dict(verdict=R.FOUND, strand=0, hits=1986, matched=1986, ctl_start=0, ctl_end=2000, draft_start=0, draft_end=2000)
    rng = np.random.default_rng(9)
    d = np.concatenate([rng.integers(0, 4, 100).astype(np.uint8), R.revcomp(c), rng.integers(0, 4, 100).astype(np.uint8)])
    assert R.screen(d, c) == dict(verdict=R.FOUND, strand=1, hits=1986, matched=1986, ctl_start=0, ctl_end=2000, draft_start=100, draft_end=2100)
    assert R.screen(d, S.encode(S.TEST_CONTROL_B))["verdict"] == R.NONE
    assert R.screen(d, c, dict(min_draft_tenths=10))["verdict"] == R.NONE           # 2000 of 2200 bases


def test_planted_templates():
    """templates with 2 % substitutions + 1 % indels under the default options"""
    import control_synth as S
    rng = np.random.default_rng(21)
    c = S.encode(S.TEST_CONTROL)
    for _ in range(8):
        for kind, strand in (("control", 0), ("control_rc", 1)):
            r = R.screen(S.noisy(rng, S.template(rng, kind, 0, c)), c)
            assert r["verdict"] == R.FOUND and r["strand"] == strand and r["matched"] > 500, (kind, r)
        t = S.noisy(rng, S.template(rng, "concat", 0, c))
        r = R.screen(t, c)
        assert r["matched"] > 500 and 10 * (r["draft_end"] - r["draft_start"]) < 8 * len(t) and r["verdict"] == R.NONE, r    # one copy wins: half of the draft
        r = R.screen(S.noisy(rng, S.template(rng, "partial", int(rng.integers(300, 12001)), c)), c)
        assert r["verdict"] == R.NONE and 0 < r["ctl_end"] - r["ctl_start"] < 1000, r
        for kind in ("random", "lowcx"):
            r = R.screen(S.template(rng, kind, int(rng.integers(300, 12001)), c), c)
            assert r["verdict"] == R.NONE and r["matched"] < 3, (kind, r)


# ---------------------------------------------------------------- CPU: ABI and argument checks
def test_structs_match_the_header(built, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ccsx.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d %d %d %d\\n", '
                   'sizeof(ccsx_control_opts), offsetof(ccsx_control_opts, min_draft_tenths), sizeof(ccsx_control_seq), offsetof(ccsx_control_seq, seq), '
                   'sizeof(ccsx_control_report), offsetof(ccsx_control_report, verdict), offsetof(ccsx_control_report, draft_end), '
                   'sizeof(ccsx_control_request), offsetof(ccsx_control_request, opts), offsetof(ccsx_control_request, report), '
                   'offsetof(ccsx_control_request, reserved), sizeof(ccsx_extras), sizeof(ccsx_adapter_request), CCSX_CONTROL_MIN_LEN, CCSX_CONTROL_MAX_LEN, '
                   'CCSX_CONTROL_UNTESTED, CCSX_CONTROL_NONE, CCSX_CONTROL_FOUND, CCSX_ABI_VERSION, CCSX_SPEC_VERSION);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    O, S, Rp, Q = api.ControlOpts, api.ControlSeq, api.CControlReport, api.CControlRequest
    assert got == [C.sizeof(O), O.min_draft_tenths.offset, C.sizeof(S), S.seq.offset, C.sizeof(Rp), Rp.verdict.offset, Rp.draft_end.offset, C.sizeof(Q),
                   Q.opts.offset, Q.report.offset, Q.reserved.offset, 24, C.sizeof(api.CAdapterRequest), api.CONTROL_MIN_LEN, api.CONTROL_MAX_LEN,
                   api.CONTROL_UNTESTED, api.CONTROL_NONE, api.CONTROL_FOUND, 6, 8]
    assert got[0] == 16 and got[2] == 16 and got[4] == 72 and got[7] == 32 and (R.MIN_LEN, R.MAX_LEN) == (64, 4096)
    assert (R.UNTESTED, R.NONE, R.FOUND) == (api.CONTROL_UNTESTED, api.CONTROL_NONE, api.CONTROL_FOUND) and R.FIELDS == api.ControlReport.FIELDS
    L = api.lib()
    assert L.ccsx_control_rule_version() == 1 and L.ccsx_abi_version() == 6 and L.ccsx_spec_version() == 8
    o = api.control_opts_default()
    assert {k: getattr(o, k) for k in R.DEFAULTS} == R.DEFAULTS
    assert api.ControlSeq.from_string("acgtACGT").codes().tolist() == [0, 1, 2, 3, 0, 1, 2, 3] == api.ControlSeq.from_codes([0, 1, 2, 3, 0, 1, 2, 3]).codes().tolist()


def _request(rep, seq=None, reserved=(0, 0), opts=True, **kw):
    o = api.control_opts_default()
    for k, v in kw.items():
        setattr(o, k, v)
    s = seq if seq is not None else api.ControlSeq.from_codes(np.arange(100) % 4)
    cr = rep.c_struct() if rep is not None else None
    q = api.CControlRequest(C.pointer(s), C.pointer(o) if opts else None, C.pointer(cr) if cr is not None else None, (C.c_int32 * 2)(*reserved))
    return q, (o, s, cr)


def _call(entry, h, b, res, q, fold=None, adapters=None):
    cb, cr = b.c_struct(), res.c_struct()
    t = C.c_int64(-7)
    args = [h, C.byref(cb), C.byref(cr), None, fold, adapters, q]
    rc = getattr(api.lib(), entry)(*(args + [C.byref(t)] if entry == "ccsx_submit_control" else args))
    assert rc == 0 or t.value == -7                                 # a refused submit hands out no ticket
    return rc


def _seq(n, poke=None, reserved=0):
    a = (np.arange(n) % 4).astype(np.uint8)
    if poke:
        a[poke[0]] = poke[1]
    s = api.ControlSeq.from_codes(a)
    s.reserved = reserved
    return s


@pytest.mark.parametrize("entry", ["ccsx_consensus_control", "ccsx_submit_control"])
def test_entry_points_refuse_bad_requests(built, entry):
    L = api.lib()
    b = api.synth(3, 4, 300, seed=2)
    res = api.Results.allocate(b)
    rep = api.ControlReport.allocate(b.n_zmw)
    bad = [("null control request or report", _request(None)),
           ("reserved must be 0", _request(rep, reserved=(0, 1))),
           ("reserved must be 0", _request(rep, reserved=(7, 0))),
           ("control sequence: reserved must be 0", _request(rep, _seq(100, reserved=1))),
           ("sized for another batch", _request(api.ControlReport.allocate(b.n_zmw + 1))),
           ("control length outside 64 .. 4096", _request(rep, _seq(63))),
           ("control length outside 64 .. 4096", _request(rep, _seq(4097))),
           ("control length outside 64 .. 4096", _request(rep, _seq(0))),
           ("control: code above 3", _request(rep, _seq(64, poke=(63, 4)))),
           ("control: code above 3", _request(rep, _seq(4096, poke=(0, 255))))]
    for kw in (dict(max_occ=0), dict(max_occ=65), dict(min_matched=0), dict(min_ctl_tenths=-1), dict(min_ctl_tenths=11), dict(min_draft_tenths=-1),
               dict(min_draft_tenths=11)):
        bad.append(("control options out of range", _request(rep, **kw)))
    for msg, (q, keep) in bad:
        assert _call(entry, None, b, res, C.byref(q)) < 0 and msg.encode() in L.ccsx_last_error(), (msg, L.ccsx_last_error())
    q, keep = _request(rep)
    q.control = None
    assert _call(entry, None, b, res, C.byref(q)) < 0 and b"null control sequence" in L.ccsx_last_error()
    nul = api.ControlSeq(100, 0, None)
    q, keep = _request(rep, nul)
    assert _call(entry, None, b, res, C.byref(q)) < 0 and b"null control sequence" in L.ccsx_last_error()
    # a bad fold or adapter request beside a good control request is refused by its own check's message
    frep = api.FoldReport.allocate(b.n_zmw + 1).c_struct()
    fq = api.CFoldRequest(None, C.pointer(frep), (C.c_int32 * 2)(0, 0))
    q, keep = _request(rep)
    assert _call(entry, None, b, res, C.byref(q), fold=C.byref(fq)) < 0 and b"sized for another batch" in L.ccsx_last_error()
    aq = api.CAdapterRequest(None, None, None, (C.c_int32 * 2)(0, 0))
    assert _call(entry, None, b, res, C.byref(q), adapters=C.byref(aq)) < 0 and b"null adapter request or report" in L.ccsx_last_error()
    # valid requests (the limits of every range; NULL options = the defaults): the handle is what is missing
    for q, keep in (_request(rep), _request(rep, opts=False), _request(rep, _seq(64), max_occ=1, min_matched=1, min_ctl_tenths=0, min_draft_tenths=0),
                    _request(rep, _seq(4096), max_occ=64, min_ctl_tenths=10, min_draft_tenths=10)):
        assert _call(entry, None, b, res, C.byref(q)) < 0 and b"null argument" in L.ccsx_last_error(), L.ccsx_last_error()
    assert _call(entry, None, b, res, None) < 0 and b"null argument" in L.ccsx_last_error()


# ---------------------------------------------------------------- GPU
RES_FIELDS = ("status", "seq_len", "rq", "np_", "ec", "iters", "n_windows", "fn", "rn")
MIX_SEED = 61


def _same(a, b, z):
    for f in RES_FIELDS:
        assert getattr(a, f)[z].tobytes() == getattr(b, f)[z].tobytes(), (z, f)
    assert np.array_equal(a.sequence(z), b.sequence(z)) and np.array_equal(a.quals(z), b.quals(z)), z
    assert np.array_equal(a.raw(z).view(np.uint32), b.raw(z).view(np.uint32)), z


def _mix(seed=MIX_SEED):
    """(batch, kind name per ZMW): 96 ZMWs of every control_synth kind around TEST_CONTROL, 3-10 passes, random parts of 300-12000 bases, and one random
    template of 42 kb at 3 passes, and the short random drafts of scan_edges"""
    import control_synth as S
    import scan_edges
    rng = np.random.default_rng(seed)
    b1, k1 = S.make(96, (3, 10), (300, 12000), seed)
    long = S.from_templates([S.template(rng, "random", 42000, S.encode(S.TEST_CONTROL))], [3], rng)
    short = scan_edges.batch()
    return api.concat([b1, long, short]), [S.KINDS[k] for k in k1] + ["long"] + ["short"] * short.n_zmw


def _check_report(d, rep, control, o=None):
    """the report against control_ref on the draft seam's drafts (the drafts k_polish is given), every field of every ZMW; returns the tested ZMWs"""
    tested = []
    for z in range(len(rep.verdict)):
        want = R.screen(d.draft(z), control, o, tested=d.status[z] == 0)
        got = {f: int(getattr(rep, f)[z]) for f in R.FIELDS}
        assert got == want, (z, got, want, int(d.status[z]), len(d.draft(z)))
        if want["verdict"] != R.UNTESTED:
            tested.append(z)
    return tested


def _opts(d):
    o = api.control_opts_default()
    for k, v in d.items():
        setattr(o, k, v)
    return o


@pytest.mark.gpu
def test_report_equals_the_restatement_and_results_do_not_change(built):
    """The oracle on the CPU for MIX_SEED (a final status that is not a draft-stage failure = tested): 97 of 97 ZMWs, 16 of 16 of every kind and the 42 kb
    one (70 SUCCESS, 27 LOW_RQ); the 8 short ZMWs of scan_edges besides"""
    import control_synth as S
    import scan_edges
    b, kinds = _mix()
    c = S.encode(S.TEST_CONTROL)
    seq = api.ControlSeq.from_string(S.TEST_CONTROL)
    h = api.Handle(0)
    d = h.draft(b)
    one = api.AdapterSet.default()
    ref, frep_ref, arep_ref, tl_ref, pile_ref = h.consensus_screen(b, fold=True, adapters=one, tandem=True, pileup=True)
    res, rep, frep, arep, tl, pile = h.consensus_control(b, seq, fold=True, adapters=one, tandem=True, pileup=True)
    tested = _check_report(d, rep, c)
    assert np.array_equal(rep.verdict == R.UNTESTED, d.status != 0)
    # the only ZMWs the comparison leaves out are the untested ones: three quarters of the batch and half of every kind are tested
    assert len(tested) >= 0.75 * b.n_zmw, (len(tested), b.n_zmw)
    for kind in set(kinds):
        zs = [z for z in range(b.n_zmw) if kinds[z] == kind]
        assert 2 * sum(z in tested for z in zs) >= len(zs), (kind, [int(d.status[z]) for z in zs])
    assert max(len(d.draft(z)) for z in tested) > 40000
    scan_edges.assert_every_class(len(d.draft(z)) for z in tested)
    # detection only: every result byte, the fold and adapter reports, the pileup planes and tandem_len equal the call without the control request
    for z in range(b.n_zmw):
        _same(res, ref, z)
    for f in ("verdict", "fold", "hits", "span"):
        assert np.array_equal(getattr(frep, f), getattr(frep_ref, f)), f
    for f in api.AdapterReport.INT_FIELDS:
        assert np.array_equal(getattr(arep, f), getattr(arep_ref, f)), f
    assert arep.hits.tobytes() == arep_ref.hits.tobytes()
    assert np.array_equal(tl, tl_ref)
    for f in ("coverage", "matches", "mismatches"):
        assert np.array_equal(getattr(pile, f), getattr(pile_ref, f)), f
    # the planted controls are found on the engine's drafts in their orientation (a draft has the orientation of its backbone pass), nothing else is
    for z in tested:
        if kinds[z] in ("control", "control_rc"):
            assert rep.verdict[z] == R.FOUND and rep.strand[z] == ((kinds[z] == "control_rc") ^ bool(d.backbone[z] & 1)), (z, kinds[z])
        else:
            assert rep.verdict[z] == R.NONE, (z, kinds[z])
    # alone, it reports the same
    res1, rep1, _, _, _, _ = h.consensus_control(b, seq)
    for f in R.FIELDS:
        assert np.array_equal(getattr(rep1, f), getattr(rep, f)), f
    for z in range(b.n_zmw):
        _same(res1, ref, z)
    # a bad request with a handle: an error of the call, and the handle still works
    q, keep = _request(api.ControlReport.allocate(b.n_zmw + 1), seq)
    assert _call("ccsx_submit_control", h._h, b, api.Results.allocate(b), C.byref(q)) < 0
    q, keep = _request(api.ControlReport.allocate(b.n_zmw), _seq(63))
    assert _call("ccsx_consensus_control", h._h, b, api.Results.allocate(b), C.byref(q)) < 0
    _, rep3, _, _, _, _ = h.consensus_control(b, seq)
    for f in R.FIELDS:
        assert np.array_equal(getattr(rep3, f), getattr(rep, f)), f
    h.close()


@pytest.mark.gpu
def test_shortest_and_longest_control_with_other_options(built):
    """a 64-base and a 4096-base control, each planted in a few templates, under non-default options"""
    import control_synth as S
    rng = np.random.default_rng(33)
    rnd = lambda m: rng.integers(0, 4, int(m)).astype(np.uint8)
    c64, c4096 = rnd(64), rnd(4096)
    tpls = [S.template(rng, k, 1500, c4096) for k in ("control", "control_rc", "partial", "concat", "random")]
    tpls += [np.concatenate([rnd(40), c64, rnd(30)]), np.concatenate([rnd(30), S.rc(c64), rnd(40)]), np.concatenate([rnd(700), c64, rnd(500)]), c4096[:3000].copy()]
    b = S.from_templates(tpls, [6] * len(tpls), rng)
    h = api.Handle(0)
    d = h.draft(b)
    ref = h.consensus(b)
    for c, o in ((c64, NONDEFAULT), (c4096, NONDEFAULT), (c4096, dict(max_occ=64, min_matched=4000, min_ctl_tenths=10, min_draft_tenths=10)), (c64, LOOSE)):
        res, rep, _, _, _, _ = h.consensus_control(b, api.ControlSeq.from_codes(c), _opts(o))
        tested = _check_report(d, rep, c, o)
        assert len(tested) >= 7 and (rep.hits[tested] > 0).sum() >= 3, (rep.verdict, rep.hits)
        for z in range(b.n_zmw):
            _same(res, ref, z)
        if (o is NONDEFAULT and len(c) == 4096) or o is LOOSE:     # (the 64-base control inside 134 bases spans less than 6 tenths of the draft)
            assert (rep.verdict == R.FOUND).sum() >= 2, rep.verdict
    h.close()


@pytest.mark.gpu
def test_hits_at_the_cap(built):
    """four drafts of 20 copies of a 300-base unit, max_occ = 64: against the unit as the control (20 diagonals), and against a control of 13 copies of it
    (13 hits per look-up, 78000 LDS atomics per draft)"""
    import control_synth as S
    rng = np.random.default_rng(35)
    unit = rng.integers(0, 4, 300).astype(np.uint8)
    b = S.from_templates([np.tile(unit, 20) for _ in range(4)], [8] * 4, rng)
    h = api.Handle(0)
    d = h.draft(b)
    o = dict(max_occ=64)
    for c in (unit, np.tile(unit, 13)):
        _, rep, _, _, _, _ = h.consensus_control(b, api.ControlSeq.from_codes(c), _opts(o))
        tested = _check_report(d, rep, c, o)
        assert len(tested) >= 3, d.status
        # one copy's diagonal wins (the copies are 300 apart, a pair of bins is 128 wide): at most 286 hits of the unit, 13 x 286 of the 13 copies; at least half
        assert min(int(rep.hits[z]) for z in tested) > (143 if len(c) == 300 else 13 * 143), rep.hits
    _, rep, _, _, _, _ = h.consensus_control(b, api.ControlSeq.from_codes(np.tile(unit, 13)), _opts(dict(max_occ=12)))
    assert (rep.hits[tested] < 200).all()                           # (the repeated codes are dropped: what is left are the noise-free k-mers of nothing)
    _check_report(d, rep, np.tile(unit, 13), dict(max_occ=12))
    h.close()


@pytest.mark.gpu
def test_two_stream_batch(built):
    """4608 ZMWs: the draft stage's POA runs as two half-batches on two streams"""
    import control_synth as S
    c = S.encode(S.TEST_CONTROL)[:1000]
    b, kk = S.make(4608, 5, (600, 1500), seed=71, control=c)
    h = api.Handle(0)
    d = h.draft(b)
    res, rep, _, _, _, _ = h.consensus_control(b, api.ControlSeq.from_codes(c))
    tested = _check_report(d, rep, c)
    assert len(tested) > 3500 and (rep.verdict == R.FOUND).sum() > 1000
    ref = h.consensus(b)
    for k in ("status", "seq_len", "rq", "np_", "iters", "fn", "rn"):
        assert getattr(res, k).tobytes() == getattr(ref, k).tobytes(), k
    assert np.array_equal(res.seq, ref.seq) and np.array_equal(res.qual, ref.qual)
    h.close()


@pytest.mark.gpu
def test_tickets_carry_their_own_control(built):
    """five tickets on three slots, alternating two controls: a per-handle index that a later submit overwrites would be read by the earlier ticket"""
    import control_synth as S
    ctl = [S.TEST_CONTROL, S.TEST_CONTROL_B]
    seqs = [api.ControlSeq.from_string(s) for s in ctl]
    batches = [S.make(24, (5, 8), (800, 4000), seed=90 + k, control=ctl[k & 1])[0] for k in range(5)]
    h = api.Handle(0)
    one = api.AdapterSet.default()
    want = [h.consensus_control(b, seqs[k & 1], fold=True, adapters=one, tandem=True) for k, b in enumerate(batches)]
    other = [h.consensus_control(b, seqs[1 - (k & 1)])[1] for k, b in enumerate(batches)]
    tickets, outs = [], []
    for k, b in enumerate(batches):                                # five tickets on three slots: three in flight
        res = api.Results.allocate(b, pinned=True)
        rep = api.ControlReport.allocate(b.n_zmw, pinned=True)
        frep = api.FoldReport.allocate(b.n_zmw, pinned=True) if k in (0, 2, 3) else None
        arep = api.AdapterReport.allocate(b.n_zmw, pinned=True) if k in (2, 4) else None
        tl = api.tandem_buffer(b.n_zmw, pinned=True) if k in (2, 3) else None          # (ticket 1 carries the control request alone)
        tickets.append(h.submit(b, res, fold=frep, tandem=tl, adapters=arep, adapter_set=one, control=rep, control_seq=seqs[k & 1]))
        outs.append((res, rep, frep, arep, tl))
    for t in (tickets[3], tickets[2], tickets[4]):                 # out of order (0 and 1 were retired by the submits that reused their slots)
        h.wait(t)
    for k, ((res, rep, frep, arep, tl), (wres, wrep, wfrep, warep, wtl, _), b) in enumerate(zip(outs, want, batches)):
        for f in R.FIELDS:
            assert np.array_equal(getattr(rep, f), getattr(wrep, f)), (k, f)
        assert (rep.verdict == R.FOUND).sum() >= 4 and not (other[k].verdict == R.FOUND).any(), (k, rep.verdict, other[k].verdict)
        if frep is not None:
            for f in ("verdict", "fold", "hits", "span"):
                assert np.array_equal(getattr(frep, f), getattr(wfrep, f)), (k, f)
        if arep is not None:
            for f in api.AdapterReport.INT_FIELDS:
                assert np.array_equal(getattr(arep, f), getattr(warep, f)), (k, f)
            assert arep.hits.tobytes() == warep.hits.tobytes()
        if tl is not None:
            assert np.array_equal(tl, wtl), k
        for z in range(b.n_zmw):
            _same(res, wres, z)
    # a slot that carried the request runs without it afterwards: a plain submit, nothing of the screen left behind
    res = api.Results.allocate(batches[0], pinned=True)
    h.wait(h.submit(batches[0], res))
    for z in range(batches[0].n_zmw):
        _same(res, want[0][0], z)
    h.close()

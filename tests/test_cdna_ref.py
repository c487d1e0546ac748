"""The cDNA rule on the CPU (DESIGN.md §2 "cDNA rule"): the poly(A) scan of tests/cdna_ref.py against the O(K^2) brute force from the definition,
ccsx_cdna_reads_host against cdna_ref on the limit set (on poisoned planes, and again with the reads in reverse order), the structs against the header, and
every argument error of the four entry points."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from ccs_amd import api
import cdna_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = R.limit_cases()
NAMES = [c[0] for c in CASES]


def _opts(d):
    o = api.CdnaOpts()
    for k in R.DEFAULTS:
        setattr(o, k, d[k])
    return o


def poisoned(n):
    """a report whose every byte is 0xA5: what the rule does not write shows"""
    rep = api.CdnaReport.allocate(n)
    for k in R.FIELDS:
        getattr(rep, k).view(np.uint8)[...] = 0xA5
    return rep


def test_the_scan_equals_the_bruteforce_on_random_inputs():
    """A-rich and mixed inputs of 0 .. 200 positions under options from every corner of their ranges"""
    rng = np.random.default_rng(7)
    for _ in range(600):
        K = int(rng.integers(0, 200))
        x = (rng.random(K) < rng.choice([0.5, 0.8, 0.95])).astype(int).tolist()
        mm, xd = int(rng.integers(1, 9)), int(rng.choice([0, 1, 2, 3, 4, 6, 64]))
        assert R.polya_scan(x, mm, xd) == R.polya_brute(x, mm, xd), (x, mm, xd)
    assert R.polya_scan([1] * 10 + [0] + [1, 1] + [0] * 9, 2, 6) == 10 == R.polya_scan([1] * 10 + [0] + [1, 1] + [0] * 9, 2, 3)   # the tie goes to the smallest k
    assert R.polya_scan([], 2, 6) == 0 and R.polya_scan([0] * 5, 2, 6) == 0 and R.polya_scan([1], 2, 6) == 1


SCAN_CASES = [i for i, n in enumerate(NAMES) if n.startswith(("tails", "scan", "polya_max", "classes"))]


@pytest.mark.parametrize("i", SCAN_CASES, ids=[NAMES[i] for i in SCAN_CASES])
def test_the_restatement_equals_the_bruteforce_scan_on_the_limit_set(i):
    name, S, roles, o, reads = CASES[i]
    brute = R.cdna_reads(S, roles, reads, polya=R.polya_brute, **o)
    assert R.diff(brute, R.expected(i)) == [], name


def test_the_limit_set_holds_what_it_is_for():
    """the cases are there, and the values the issue names occur in what the restatement says about them"""
    E = {name: R.expected(i) for i, name in enumerate(NAMES)}
    for P in (2, 3, 63, 64):
        for which in ("last", "first"):
            w = E[f"n{P}_{which}"]
            assert w["cls"][:2].tolist() == [R.FULL_LENGTH] * 2 and w["strand"][:2].tolist() == [0, 1] and w["polya_len"][:2].tolist() == [30, 30]
            assert w["idx"][0].tolist() == [0, P - 1] and w["idx"][1].tolist() == [P - 1, 0]
            assert w["cls"][2:4].tolist() == [R.NO_TAIL] * 2 and w["strand"][2:4].tolist() == [1, 0] and w["tested"][4] == 0 and w["cls"][5] == R.NO_PRIMER
    for name in ("m8", "m25", "m63", "m64", "mixed"):
        assert len(CASES[NAMES.index(name)][4][-1]) == 3001 and E[name]["cls"][-1] in (R.FULL_LENGTH, R.CONCATEMER) and E[name]["tested"][0] == 0
    for m in (25, 63, 64):
        w = E[f"m{m}"]                                              # m - 1 and m bases: one end each way, same primer: same role; 2 m - 1: SHORT from step 3
        assert w["cls"][3] == R.SHORT and w["strand"][3] == 0 and w["clip"][3].sum() >= 2 * m - 1 and w["polya_len"][3] == 0
    assert E["overlap"]["cls"].tolist() == [R.SHORT] * 4 + [R.NO_TAIL] * 2 and E["overlap"]["end"][4] - E["overlap"]["start"][4] == 1   # ins_len 0, -5, 1
    for W in (8, 64, 1024):
        w = E[f"window{W}"]
        assert w["strand"][6] == 0 and w["strand"][7] == 1 and w["cls"][6] == R.FULL_LENGTH        # both primers end at the windows' last base
        assert w["cls"][8] == R.ONE_END and w["cls"][10] == R.ONE_END                                 # one base further out, at the head / at the tail
    for kind in ("sub", "ins", "del"):
        w = E[f"edits_{kind}"]                                      # per read pair: 0, k, k + 1 edits in the head's primer, then in the tail's
        assert w["cls"][[0, 2, 4, 6]].tolist() == [R.FULL_LENGTH] * 4 and w["cls"][[8, 10]].tolist() == [R.ONE_END] * 2, kind
        assert w["dist"][4, 0] == R.K25 and w["dist"][6, 1] == R.K25 and w["dist"][5, 1] == R.K25
    assert (E["edits_p30"]["cls"] == R.FULL_LENGTH).all() and (E["edits_p0"]["cls"] == R.FULL_LENGTH).sum() == 4
    w0, w1 = E["ties_m0"], E["ties_m1"]                             # identical primers of opposite roles
    assert w0["idx"][0, 0] == 0 and w0["second"][0, 0] == 0 and w0["strand"][0] == 0 and w0["cls"][0] == R.FULL_LENGTH
    assert w1["cls"][0] == R.ONE_END and w1["cls"][1] == R.ONE_END and w1["strand"][0] == -1
    assert E["ties_swapped_m0"]["strand"][0] == 1 and E["ties_swapped_m0"]["idx"][0, 0] == 0
    assert w1["cls"][2] == R.FULL_LENGTH and w0["cls"][4] == R.CONCATEMER and w0["n_internal"][4] == 2      # the palindrome: both of its searches hit
    assert (E["ties_m64"]["cls"] == R.NO_PRIMER).all()
    w = E["classes"]
    assert w["cls"].tolist() == [R.NO_PRIMER] * 2 + [R.ONE_END] * 4 + [R.SAME_ROLE] * 4 + [R.SHORT] * 2 + [R.CONCATEMER] * 2 + [R.NO_TAIL] * 2
    assert w["strand"][10:].tolist() == [0, 1] * 3 and w["n_internal"][12] == 2 and w["polya_len"][14:].tolist() == [5, 5]
    w = E["classes_full"]
    assert w["cls"].tolist() == [R.FULL_LENGTH] * 4 + [R.SHORT] * 2 and w["strand"].tolist() == [0, 1] * 3
    assert (w["start"][0], w["end"][0]) == (25, 175) and (w["start"][1], w["end"][1]) == (55, 205) and w["end"][4] == 0
    w = E["classes_min_len"]
    assert w["cls"].tolist() == [R.NO_TAIL] * 2 + [R.FULL_LENGTH] * 2 + [R.SHORT] * 2 and w["polya_len"][4:].tolist() == [40, 40]
    tails = [0, 1, 19, 20, 63, 64, 65, 127, 128, 129]
    for name in ("tails_sense", "tails_anti"):
        w = E[name]
        assert w["polya_len"].tolist() == tails and w["cls"].tolist() == [R.NO_TAIL] * 3 + [R.FULL_LENGTH] * 7
        assert (E[name + "_nomin"]["cls"] == R.FULL_LENGTH).all()
    for pm in (16, 512):
        assert E[f"polya_max{pm}"]["polya_len"].tolist() == [pm - 1] * 2 + [pm] * 4 + [40 if pm > 40 else pm] * 2
    assert all(len(r) == 3001 for r in CASES[NAMES.index("polya_max4096")][4])
    assert E["polya_max4096"]["polya_len"].tolist() == [2000, 2000, 2403, 2403, 2500, 2500] and E["polya_max2048"]["polya_len"].tolist() == [2000, 2000, 2048, 2048, 2048, 2048]
    w = E["scan"]["polya_len"].tolist()
    assert w[0::2] == w[1::2] and w[0::2] == [104, 105, 51, 62, 63, 10, 0, 5]
    assert E["scan_x2"]["polya_len"].tolist()[0::2] == [63, 64, 30, 62, 63, 10, 0, 5] == E["scan_x0"]["polya_len"].tolist()[0::2]
    assert E["scan_mm1"]["polya_len"].tolist()[0::2] == [104, 105, 51, 85, 86, 13, 0, 21]
    assert E["scan_mm2"]["polya_len"].tolist()[0::2] == [104, 105, 51, 62, 63, 10, 0, 5]          # (read 5: the tie, s = 10, 8, 9, 10)
    w = E["internal_edges"]
    own = [0, 1, 4, 5, 8, 9, 10, 11]                               # (reads 2, 3 and 6, 7 are the two sets' below: the copy lacks its last / first base here)
    assert w["n_internal"][own].tolist() == [1] * 8 and w["cls"][own].tolist() == [R.CONCATEMER] * 8 and (w["strand"] >= 0).all()
    assert w["first_internal"][0] == 25 + 120 and w["first_internal"][4] == 25 and w["first_internal"][8] == 25 + 120 + 15
    for name in ("internal_edges_Qe", "internal_edges_Qs"):                     # one base past L - clip_1, one base before clip_0: not internal
        assert E[name]["n_internal"].tolist() == [1, 1, 0, 0] and (E[name]["strand"] >= 0).all() and (E[name]["clip"] == 25).all()
    ends = (R.CHUNK - 1, R.CHUNK, R.CHUNK + 1, R.CHUNK + 4, R.CHUNK + 12, 2 * R.CHUNK - 1, 2 * R.CHUNK, 2 * R.CHUNK + 1)
    assert E["internal_chunks"]["first_internal"].tolist() == [e - 25 for e in ends] and (E["internal_chunks_rc"]["n_internal"] == 1).all()
    w = E["internal_edits"]
    assert w["n_internal"].tolist() == [1, 1, 0] * 3 + [2, 3, 2] and w["first_internal"][9:].tolist() == [25 + 700, 25 + 300, 25 + 30 + 60]


@pytest.mark.parametrize("i", range(len(CASES)), ids=NAMES)
def test_the_host_rule_equals_the_restatement(built, i):
    name, S, roles, o, reads = CASES[i]
    pset = api.CdnaPrimers.from_codes(S, roles)
    rep = api.cdna_reads_host(pset, list(reads), _opts(o), poisoned(len(reads)))
    assert R.diff(rep, R.expected(i)) == [], (name, R.diff(rep, R.expected(i)))
    rep = api.cdna_reads_host(pset, list(reads)[::-1], _opts(o), poisoned(len(reads)))
    assert R.diff(rep, R.reversed_order(R.expected(i))) == [], (name, "reversed", R.diff(rep, R.reversed_order(R.expected(i))))


def test_structs_match_the_header(built, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ccsx.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu '
                   '%d %d %d %d %d %zu\\n", '
                   'sizeof(ccsx_cdna_opts), offsetof(ccsx_cdna_opts, polya_mismatch), offsetof(ccsx_cdna_opts, min_len), sizeof(ccsx_cdna_set), '
                   'offsetof(ccsx_cdna_set, len), offsetof(ccsx_cdna_set, role), offsetof(ccsx_cdna_set, seq), sizeof(ccsx_cdna_report), '
                   'offsetof(ccsx_cdna_report, tested), offsetof(ccsx_cdna_report, end), offsetof(ccsx_cdna_report, first_internal), '
                   'offsetof(ccsx_cdna_report, clip), sizeof(ccsx_cdna_request), offsetof(ccsx_cdna_request, set), offsetof(ccsx_cdna_request, report), '
                   'offsetof(ccsx_cdna_request, reserved), CCSX_CDNA_MAX_PRIMERS, CCSX_CDNA_MIN_LEN, CCSX_CDNA_MAX_LEN, CCSX_CDNA_FULL_LENGTH, CCSX_ABI_VERSION, '
                   'sizeof(ccsx_requests));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    O, S, Rp, Q = api.CdnaOpts, api.CdnaPrimers, api.CCdnaReport, api.CCdnaRequest
    assert got == [C.sizeof(O), O.polya_mismatch.offset, O.min_len.offset, C.sizeof(S), S.len.offset, S.role.offset, S.seq.offset, C.sizeof(Rp), Rp.tested.offset,
                   Rp.end.offset, Rp.first_internal.offset, Rp.clip.offset, C.sizeof(Q), Q.set.offset, Q.report.offset, Q.reserved.offset,
                   api.CDNA_MAX_PRIMERS, api.CDNA_MIN_LEN, api.CDNA_MAX_LEN, api.CDNA_FULL_LENGTH, 6, C.sizeof(api.CRequests)]
    assert got[0] == 32 and got[3] == 4 + 64 * 4 + 64 + 64 * 64 and got[7] == 8 + 12 * 8 and got[12] == 32 and got[-1] == 64
    assert R.READ_PLANES == api.CDNA_READ_PLANES and R.END_PLANES == api.CDNA_END_PLANES and len(api.CDNA_NAMES) == 7
    L = api.lib()
    assert L.ccsx_cdna_rule_version() == 1 and L.ccsx_abi_version() == 6 and L.ccsx_spec_version() == 8
    o = api.cdna_opts_default()
    assert {k: getattr(o, k) for k in R.DEFAULTS} == R.DEFAULTS
    p = api.CdnaPrimers.from_codes(["acgtACGT", [3, 2, 1, 0, 0, 1, 2, 3, 3]], [1, 0])
    assert [c.tolist() for c in p.codes()] == [[0, 1, 2, 3] * 2, [3, 2, 1, 0, 0, 1, 2, 3, 3]] and p.roles() == [1, 0]


# ---------------------------------------------------------------- argument errors: refused before anything is enqueued (no handle is ever needed to be refused)
def _set(lens, roles=None, poke=None, n=None):
    s = api.CdnaPrimers.from_codes([("ACGT" * 16)[:m] for m in lens], roles if roles is not None else [k & 1 for k in range(len(lens))])
    if poke:
        s.seq[poke[0]][poke[1]] = poke[2]
    if n is not None:
        s.n_primers = n
    return s


def _bad_sets_and_opts():
    """(message, set, opts kwargs)"""
    long2 = _set([8, 64, 64])
    long2.len[2] = 65
    bad = [("n_primers outside 2 .. 64", _set([16], [0], n=1), {}), ("n_primers outside 2 .. 64", _set([16] * 64, n=65), {}),
           ("n_primers outside 2 .. 64", _set([16, 16], n=0), {}),
           ("primer 1: role above 1", _set([16, 16, 16], [0, 2, 1]), {}), ("primer 0: role above 1", _set([16, 16], [255, 1]), {}),
           ("needs a primer of role 0 (5') and one of role 1 (3')", _set([16, 16, 16], [0, 0, 0]), {}),
           ("needs a primer of role 0 (5') and one of role 1 (3')", _set([16, 16], [1, 1]), {}),
           ("primer 1: length outside 8 .. 64", _set([16, 7, 30]), {}), ("primer 0: length outside 8 .. 64", _set([0, 16]), {}),
           ("primer 2: length outside 8 .. 64", long2, {}), ("primer 2: code above 3", _set([64, 16, 40], poke=(2, 39, 4)), {})]
    for kw in (dict(window=7), dict(window=1025), dict(max_dist_pct=-1), dict(max_dist_pct=31), dict(min_margin=-1), dict(min_margin=65), dict(polya_mismatch=0),
               dict(polya_mismatch=9), dict(polya_xdrop=-1), dict(polya_xdrop=65), dict(polya_max=15), dict(polya_max=4097), dict(min_polya=-1), dict(min_polya=256),
               dict(min_len=0), dict(min_len=65536)):
        bad.append(("cdna options out of range", _set([16, 16]), kw))
    return bad


def _mk_opts(kw):
    o = api.cdna_opts_default()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


LIMITS = (dict(window=8, max_dist_pct=0, min_margin=0, polya_mismatch=1, polya_xdrop=0, polya_max=16, min_polya=0, min_len=1),
          dict(window=1024, max_dist_pct=30, min_margin=64, polya_mismatch=8, polya_xdrop=64, polya_max=4096, min_polya=255, min_len=65535))


@pytest.mark.parametrize("entry", ["ccsx_cdna_reads_host", "ccsx_cdna_reads"])
def test_the_read_forms_refuse_bad_arguments(built, entry):
    L = api.lib()
    reads = [np.zeros(30, np.uint8), np.zeros(0, np.uint8)]

    def call(pset, opts, rep, poke=None, null=()):
        args, _, keep = api._reads_args(api.CdnaReport, pset if pset is not None else _set([16, 16]), opts, reads, rep)
        args = list(args)
        if pset is None:
            args[0] = None
        for k in null:
            args[k] = None
        if poke:
            poke(keep)
        return getattr(L, entry)(*(([None] if entry == "ccsx_cdna_reads" else []) + args))

    for msg, s, kw in _bad_sets_and_opts():
        assert call(s, _mk_opts(kw), None) < 0 and msg.encode() in L.ccsx_last_error() and entry.encode() in L.ccsx_last_error(), (msg, L.ccsx_last_error())
    assert call(None, None, None) < 0 and b"null cdna set" in L.ccsx_last_error()
    assert call(_set([16, 16]), None, None, null=(6,)) < 0 and b"null cdna report" in L.ccsx_last_error()
    assert call(_set([16, 16]), None, api.CdnaReport.allocate(3)) < 0 and b"sized for another batch" in L.ccsx_last_error()
    for k in (2, 3, 4):
        assert call(_set([16, 16]), None, None, null=(k,)) < 0 and b"null argument" in L.ccsx_last_error(), k

    def neg(keep):
        keep[3][0] = -1
    assert call(_set([16, 16]), None, None, poke=neg) < 0 and b"read 0: negative seq_off" in L.ccsx_last_error()
    for kw in LIMITS:                                            # valid arguments at the limits of every range: only the handle is missing, where one is needed
        rc = call(_set([8, 64] * 32), _mk_opts(kw), None)
        if entry == "ccsx_cdna_reads":
            assert rc < 0 and b"null argument" in L.ccsx_last_error(), L.ccsx_last_error()
        else:
            assert rc == 0, L.ccsx_last_error()


@pytest.mark.parametrize("entry", ["ccsx_consensus_cdna", "ccsx_submit_cdna"])
def test_the_fused_forms_refuse_bad_requests(built, entry):
    L = api.lib()
    b = api.synth(3, 4, 300, seed=2)
    res = api.Results.allocate(b)
    rep = api.CdnaReport.allocate(b.n_zmw)

    def call(q, rq=None, batch=b):
        cb, cr = batch.c_struct() if batch is not None else None, res.c_struct()
        t = C.c_int64()
        args = [None, C.byref(cb) if cb is not None else None, C.byref(cr), rq, q]
        return getattr(L, entry)(*(args + [C.byref(t)] if entry == "ccsx_submit_cdna" else args))

    def request(pset, opts=None, report=rep, reserved=(0, 0)):
        cr = report.c_struct() if report is not None else None
        q = api.CCdnaRequest(C.pointer(opts) if opts is not None else None, C.pointer(pset) if pset is not None else None,
                             C.pointer(cr) if cr is not None else None, (C.c_int32 * 2)(*reserved))
        return q, (pset, opts, cr)

    for msg, s, kw in _bad_sets_and_opts():
        q, keep = request(s, _mk_opts(kw))
        assert call(C.byref(q)) < 0 and msg.encode() in L.ccsx_last_error(), (msg, L.ccsx_last_error())
    for msg, (q, keep) in (("null cdna set", request(None)), ("null cdna report", request(_set([16, 16]), report=None)),
                           ("cdna request: reserved must be 0", request(_set([16, 16]), reserved=(0, 1))),
                           ("cdna request: reserved must be 0", request(_set([16, 16]), reserved=(5, 0))),
                           ("sized for another batch", request(_set([16, 16]), report=api.CdnaReport.allocate(b.n_zmw + 1)))):
        assert call(C.byref(q)) < 0 and msg.encode() in L.ccsx_last_error(), (msg, L.ccsx_last_error())
    assert call(None) < 0 and b"null cdna request" in L.ccsx_last_error()
    q, keep = request(_set([16, 16]))
    assert call(C.byref(q), batch=None) < 0 and b"null argument" in L.ccsx_last_error()
    # a bad member of the ccsx_requests beside a good cdna request is refused by that member's message; nonzero reserved pointers of the struct too
    frep = api.FoldReport.allocate(b.n_zmw + 1).c_struct()
    fq = api.CFoldRequest(None, C.pointer(frep), (C.c_int32 * 2)(0, 0))
    rq = api.CRequests(None, C.pointer(fq), None, None, None, (C.c_void_p * 3)())
    assert call(C.byref(q), C.byref(rq)) < 0 and b"sized for another batch" in L.ccsx_last_error()
    rq = api.CRequests(None, None, None, None, None, (C.c_void_p * 3)(0, 1, 0))
    assert call(C.byref(q), C.byref(rq)) < 0 and b"reserved must be NULL" in L.ccsx_last_error()
    # valid requests (NULL options = the defaults, the limits of every range): the handle is what is missing
    for q, keep in (request(_set([16, 16])), request(_set([8, 64] * 32), _mk_opts(LIMITS[1])), request(_set([8, 8]), _mk_opts(LIMITS[0]))):
        assert call(C.byref(q)) < 0 and b"null argument" in L.ccsx_last_error(), L.ccsx_last_error()


def test_the_mirror_refuses_the_combinations_no_entry_point_takes(built):
    """the cdna request goes beside the members of ccsx_requests only: hd, hand-off, barcode, represent and segment requests have entry points of their own,
    and none takes two.  Handle.submit says so before it looks at anything else (no handle state is touched: the check comes first)"""
    b = api.synth(2, 4, 300, seed=2)
    res, rep = api.Results.allocate(b), api.CdnaReport.allocate(b.n_zmw)
    pset = _set([16, 16])
    others = (dict(hd=api.HdReport.allocate(b.n_zmw)), dict(handoff=object()), dict(barcodes=api.BarcodeReport.allocate(b.n_zmw), barcode_set=object()),
              dict(represent=api.RepresentReport.allocate(b.n_zmw)), dict(segments=api.SegmentReport.allocate(b.n_zmw), segment_set=object()))
    for kw in others:
        with pytest.raises(ValueError, match="cdna request is not combined"):
            api.Handle.submit(None, b, res, cdna=rep, cdna_primers=pset, **kw)

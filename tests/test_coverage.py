"""Coverage screen (DESIGN.md §2 "Coverage rule"; docs/faq/reports-aux-files.md "Coverage drops", "Insufficient draft cov", "Draft too different", "Reads failed
polishing"): the rule's reference by hand, the reference on the CPU restatement's alignments of planted layouts, the request's ABI and argument checks, and on an
MI355X exact parity of k_coverage with the reference on the engine's own windows and alignments, the post-polish planes against the effective coverage, no
effect on any result without a gate, the gate, tickets that carry their own options, and the old entry points against ccsx_*_requests."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from ccs_amd import api
import coverage_ref as R
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


# ---------------------------------------------------------------- CPU: the reference by hand
def _pass(Ld, bounds, rows, valid=True, L=None, partial=False):
    """a pass whose entry rows at the edge columns are `rows` (one per column of coverage_ref.edge_cols)"""
    cols = R.edge_cols(bounds, Ld)
    assert len(rows) == len(cols)
    rs = np.full(Ld + 1, -1, np.int32)
    rs[cols] = rows
    return rs, int(valid), int(L if L is not None else max(rows)), partial


def test_reference_by_hand():
    # three windows of a 70-base draft: bounds 0 22 44 70, edge columns 0 20 24 42 46 70; J = 24, 26, 28
    Ld, wb = 70, [0, 22, 44, 70]
    assert R.edge_cols(wb, Ld) == [0, 20, 24, 42, 46, 70]
    clean = _pass(Ld, wb, [0, 20, 24, 42, 46, 70])
    # segments of window 0: rows[2] - rows[0], window 1: rows[4] - rows[1], window 2: rows[5] - rows[3]
    blk1 = _pass(Ld, wb, [0, 20, 24, 42 + 57, 46 + 57, 70 + 57])          # window 1 holds 26 + 57 = 83 > 26 + 30 bases; window 2 is clean again
    at_limit = _pass(Ld, wb, [0, 20, 24, 42 + 30, 46 + 30, 70 + 30])      # exactly J + block: not a block
    r = R.screen(Ld, wb, [clean] * 4 + [blk1] * 4)
    assert r == dict(verdict=R.COVERAGE_DROPS, np_aligned=8, spans=8, cov_max=8, clean_min=4, drop_window=1, drop_windows=1, reach_sum=24, used_sum=0, used_min=0)
    assert R.screen(Ld, wb, [clean] * 4 + [at_limit] * 4)["verdict"] == R.NONE
    # the <= at exactly drop_percent: 4 clean of cov_max 8 drops at 50, 5 of 8 does not, and drop_percent 62 / 63 brackets 5 of 8 (500 <= 62 * 8 = 496 is false)
    r5 = R.screen(Ld, wb, [clean] * 5 + [blk1] * 3)
    assert (r5["verdict"], r5["clean_min"], r5["drop_windows"]) == (R.NONE, 5, 0)
    assert R.screen(Ld, wb, [clean] * 5 + [blk1] * 3, dict(drop_percent=62))["drop_windows"] == 0
    assert R.screen(Ld, wb, [clean] * 5 + [blk1] * 3, dict(drop_percent=63))["drop_windows"] == 1
    assert R.screen(Ld, wb, [clean] * 8, dict(drop_percent=100))["drop_windows"] == 3 and R.screen(Ld, wb, [clean] * 8, dict(drop_percent=99))["drop_windows"] == 0
    assert R.screen(Ld, wb, [clean] * 8, dict(drop_percent=0))["verdict"] == R.NONE
    # ties in drop_window: blocks in windows 0 and 2 of different passes, equally many -> the first
    blk0 = _pass(Ld, wb, [0, 20 + 60, 24 + 60, 42 + 60, 46 + 60, 70 + 60])
    blk2 = _pass(Ld, wb, [0, 20, 24, 42, 46, 70 + 60])
    r = R.screen(Ld, wb, [clean] * 4 + [blk2] * 2 + [blk0] * 2)
    assert (r["clean_min"], r["drop_window"], r["drop_windows"], r["verdict"]) == (6, 0, 0, R.NONE)
    r = R.screen(Ld, wb, [clean] * 2 + [blk2] * 3 + [blk0] * 3)
    assert (r["clean_min"], r["drop_window"], r["drop_windows"], r["verdict"]) == (5, 0, 0, R.NONE)
    r = R.screen(Ld, wb, [blk2] * 4 + [blk0] * 4)
    assert (r["clean_min"], r["drop_window"], r["drop_windows"], r["verdict"]) == (4, 0, 2, R.COVERAGE_DROPS)
    # block: the option moves the limit
    assert R.screen(Ld, wb, [clean] * 4 + [blk1] * 4, dict(block=57))["verdict"] == R.NONE
    assert R.screen(Ld, wb, [clean] * 4 + [blk1] * 4, dict(block=56))["verdict"] == R.COVERAGE_DROPS
    # passes that do not reach: not valid; a negative segment (uncovered edge columns of a partial or double-split pass); a segment longer than the pass
    head = _pass(Ld, wb, [0, 20, 24, -(1 << 20) - 192, -(1 << 20) - 256, -(1 << 20) - 320], L=30, partial=True)   # reaches window 0 only
    r = R.screen(Ld, wb, [clean] * 3 + [head])
    assert (r["np_aligned"], r["spans"], r["cov_max"], r["clean_min"], r["drop_window"], r["reach_sum"], r["verdict"]) == (3, 3, 4, 3, 1, 10, R.NONE)
    # a double split: window 0 ends on an uncovered column (negative), window 2 starts on one (longer than the pass), window 1 lies between two covered
    # columns and holds everything in between (a block)
    dsplit = _pass(Ld, wb, [0, 20, -(1 << 20) - 128, -(1 << 20) - 192, 300, 324], L=324)
    r = R.screen(Ld, wb, [clean] * 3 + [dsplit])
    assert (r["np_aligned"], r["spans"], r["cov_max"], r["clean_min"], r["reach_sum"], r["verdict"]) == (4, 3, 4, 3, 10, R.NONE)
    r = R.screen(Ld, wb, [clean] * 2 + [dsplit] * 2)
    assert (r["np_aligned"], r["spans"], r["verdict"]) == (4, 2, R.INSUFFICIENT_SPANS)
    dead = _pass(Ld, wb, [0, 20, 24, 42, 46, 70], valid=False)
    r = R.screen(Ld, wb, [clean] * 2 + [dead] * 2)
    assert (r["np_aligned"], r["spans"], r["cov_max"], r["verdict"]) == (2, 2, 2, R.DRAFT_TOO_DIFFERENT)
    # min_spans: 0 = min_passes; the verdicts in their order
    assert R.screen(Ld, wb, [clean] * 2 + [dsplit] * 2, dict(min_spans=2))["verdict"] == R.COVERAGE_DROPS      # clean 2 2 2 of cov_max 4
    assert R.screen(Ld, wb, [clean] * 2 + [dsplit] * 2, dict(drop_percent=49), min_passes=2)["verdict"] == R.NONE
    assert R.screen(Ld, wb, [clean] * 2 + [dsplit] * 2, min_passes=5)["verdict"] == R.DRAFT_TOO_DIFFERENT
    assert R.screen(Ld, wb, [clean] * 4 + [blk1] * 4, dict(min_spans=9))["verdict"] == R.INSUFFICIENT_SPANS
    # a single window: edge columns 0 and Ld
    r = R.screen(20, [0, 20], [_pass(20, [0, 20], [0, 21])] * 3 + [_pass(20, [0, 20], [0, 51])] * 3)
    assert r == dict(verdict=R.COVERAGE_DROPS, np_aligned=6, spans=6, cov_max=6, clean_min=3, drop_window=0, drop_windows=1, reach_sum=6, used_sum=0, used_min=0)
    assert R.screen(20, [0, 20], [_pass(20, [0, 20], [0, 21])] * 3 + [_pass(20, [0, 20], [0, 50])] * 3)["verdict"] == R.NONE
    # untested
    assert R.screen(Ld, wb, [clean] * 8, tested=False) == dict.fromkeys(R.FIELDS, 0)
    # the post-polish planes: 24 reaching segments, the polish used 12 / 11 of them
    used = [4, 4, 4]
    r = R.screen(Ld, wb, [clean] * 8, used=used)
    assert (r["verdict"], r["reach_sum"], r["used_sum"], r["used_min"]) == (R.NONE, 24, 12, 4)                      # (24 - 12) * 100 > 50 * 24 is false
    r = R.screen(Ld, wb, [clean] * 8, used=[4, 4, 3])
    assert (r["verdict"], r["used_sum"], r["used_min"]) == (R.READS_FAILED_POLISHING, 11, 3)
    assert R.screen(Ld, wb, [clean] * 8, used=[4, 4, 3], final_status=4)["verdict"] == R.NONE                       # NON_CONVERGENT: not decided
    assert R.screen(Ld, wb, [clean] * 8, used=[4, 4, 3], final_status=R.LOW_RQ)["verdict"] == R.READS_FAILED_POLISHING
    assert R.screen(Ld, wb, [clean] * 8, dict(max_lost_percent=0), used=[8, 8, 8])["verdict"] == R.NONE
    assert R.screen(Ld, wb, [clean] * 8, dict(max_lost_percent=0), used=[8, 8, 7])["verdict"] == R.READS_FAILED_POLISHING
    r = R.screen(Ld, wb, [clean] * 4 + [blk1] * 4, used=[1, 1, 1])                                                 # the earlier verdict stays
    assert (r["verdict"], r["used_sum"]) == (R.COVERAGE_DROPS, 3)
    r = R.screen(Ld, wb, [clean] * 4 + [blk1] * 4, used=[1, 1, 1], gate=1 << R.COVERAGE_DROPS)                      # gated before the polish: not polished
    assert (r["verdict"], r["used_sum"], r["used_min"], r["reach_sum"]) == (R.COVERAGE_DROPS, 0, 0, 24)


# ---------------------------------------------------------------- CPU: the reference on the CPU restatement's alignments
def _oracle_report(b, z, opts=None, min_passes=3):
    """the reference on what the CPU restatement makes of ZMW z: pass-0 POA draft, its windows, every pass through the alignment cascade.
    Returns (report, route names, draft, bounds)"""
    draft = O.poa_draft(b, z)
    wb = O.windows(draft)
    r0, r1 = int(b.read_off[z]), int(b.read_off[z + 1])
    f0 = int(b.flags[r0]) & 1
    passes, names = [], []
    for r in range(r0, r1):
        bases = b.bases[int(b.base_off[r]):int(b.base_off[r + 1])]
        fl = int(b.flags[r])
        rev = (fl & 1) != f0
        partial = None if not fl & 2 else ((fl >> 2) & 1) ^ int(rev)
        name, rs, v, _, _ = O.route(O.orient(bases, rev), draft, partial)
        passes.append((rs, v, len(bases), bool(fl & 2)))
        names.append(name)
    return R.screen(len(draft), wb, passes, opts, min_passes), names, draft, wb


def _block_column(t, at, draft):
    """the draft column the template's position `at` falls on: the draft prefix closest to the template's"""
    ks = list(range(max(at - 20, 0), min(at + 21, len(draft) + 1)))
    return ks[int(np.argmin([O.edit_distance(t[:at], draft[:k]) for k in ks]))]


@pytest.mark.parametrize("seed", [20, 43])
def test_planted_layouts_on_the_oracle(built, seed):
    """600-base templates, 8 forward passes through the 11 % channel, the default options.  The seeds are chosen so that every outcome below holds on the
    oracle (of the seeds 0 .. 59 these two).  What varies with the seed is the 35-base block: its four passes go through the 16-row band, the 64-row retry or
    the split alignment as the noise around the block decides (of the seeds 0 .. 59: COVERAGE_DROPS with clean_min 4 for 25, NONE with clean_min 5 .. 8 for
    35, clean_min 7 for three): 35 bases sit at the margin of block = 30."""
    import coverage_synth as S
    rng = np.random.default_rng(seed)
    t, at, lay = S.layouts(rng)
    got = {}
    for name, passes in lay.items():
        b = S.batch([passes], rng)
        got[name] = _oracle_report(b, 0)
    rep = {k: v[0] for k, v in got.items()}
    r = rep["clean"]
    assert (r["verdict"], r["spans"], r["clean_min"], r["np_aligned"], r["cov_max"], r["drop_windows"]) == (R.NONE, 8, 8, 8, 8, 0)
    r = rep["block300_2of8"]
    assert (r["verdict"], r["clean_min"], r["spans"]) == (R.NONE, 6, 8) and got["block300_2of8"][1].count("split") == 2
    for k in ("block300_last4", "block300_alternating"):
        r, names, draft, wb = got[k]
        assert (r["verdict"], r["clean_min"], r["spans"], r["np_aligned"]) == (R.COVERAGE_DROPS, 4, 8, 8) and names.count("split") == 4, (k, r, names)
        assert abs(len(draft) - len(t)) < 20                                   # the draft did not take the block
        w, col = r["drop_window"], _block_column(t, at, draft)
        assert max(int(wb[w]) - 2, 0) <= col < min(int(wb[w + 1]) + 2, len(draft)), (k, w, col, wb[w], wb[w + 1])
    assert rep["block60_4of8"]["verdict"] == R.COVERAGE_DROPS
    r = rep["block35_4of8"]
    assert (r["verdict"], r["clean_min"]) == (R.NONE, 7), (r, got["block35_4of8"][1])
    r, names, draft, _ = got["block300_first5"]
    assert (r["verdict"], r["np_aligned"], r["spans"]) == (R.NONE, 5, 5) and names.count("lost") == 3 and len(draft) > len(t) + 250   # the draft took it
    r, names, _, _ = got["partials"]
    assert (r["verdict"], r["cov_max"], r["np_aligned"], r["spans"]) == (R.NONE, 8, 6, 6) and names.count("partial") == 2


# ---------------------------------------------------------------- CPU: ABI and argument checks
def test_structs_match_the_header(built, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ccsx.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu '
                   '%d %d %d %d %d %d %d %d %d %d %d %d\\n", '
                   'sizeof(ccsx_coverage_opts), offsetof(ccsx_coverage_opts, max_lost_percent), sizeof(ccsx_coverage_report), offsetof(ccsx_coverage_report, verdict), '
                   'offsetof(ccsx_coverage_report, used_min), sizeof(ccsx_coverage_request), offsetof(ccsx_coverage_request, report), '
                   'offsetof(ccsx_coverage_request, gate), offsetof(ccsx_coverage_request, reserved), sizeof(ccsx_requests), offsetof(ccsx_requests, fold), '
                   'offsetof(ccsx_requests, control), offsetof(ccsx_requests, coverage), offsetof(ccsx_requests, reserved), '
                   'CCSX_COVERAGE_UNTESTED, CCSX_COVERAGE_NONE, CCSX_COVERAGE_DRAFT_TOO_DIFFERENT, CCSX_COVERAGE_INSUFFICIENT_SPANS, CCSX_COVERAGE_COVERAGE_DROPS, '
                   'CCSX_COVERAGE_READS_FAILED_POLISHING, CCSX_DRAFT_TOO_DIFFERENT, CCSX_INSUFFICIENT_SPANS, CCSX_COVERAGE_DROPS, CCSX_READS_FAILED_POLISHING, '
                   'CCSX_ABI_VERSION, CCSX_SPEC_VERSION);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    Op, Rp, Q, Rq = api.CoverageOpts, api.CCoverageReport, api.CCoverageRequest, api.CRequests
    assert got == [C.sizeof(Op), Op.max_lost_percent.offset, C.sizeof(Rp), Rp.verdict.offset, Rp.used_min.offset, C.sizeof(Q), Q.report.offset, Q.gate.offset,
                   Q.reserved.offset, C.sizeof(Rq), Rq.fold.offset, Rq.control.offset, Rq.coverage.offset, Rq.reserved.offset,
                   api.COVERAGE_UNTESTED, api.COVERAGE_NONE, api.COVERAGE_DRAFT_TOO_DIFFERENT, api.COVERAGE_INSUFFICIENT_SPANS, api.COVERAGE_COVERAGE_DROPS,
                   api.COVERAGE_READS_FAILED_POLISHING, api.DRAFT_TOO_DIFFERENT, api.INSUFFICIENT_SPANS, api.COVERAGE_DROPS, api.READS_FAILED_POLISHING, 6, 8]
    assert got[0] == 16 and got[2] == 88 and got[5] == 32 and got[9] == 64 and got[20:24] == [11, 12, 13, 14]
    assert (R.UNTESTED, R.NONE, R.DRAFT_TOO_DIFFERENT, R.INSUFFICIENT_SPANS, R.COVERAGE_DROPS, R.READS_FAILED_POLISHING) == tuple(range(6))
    assert R.FIELDS == api.CoverageReport.FIELDS and R.PRE == api.CoverageReport.PRE and R.POST == api.CoverageReport.POST
    assert {v: api.STATUS_NAMES[s] for v, s in R.GATE_STATUS.items()} == {2: "DRAFT_TOO_DIFFERENT", 3: "INSUFFICIENT_SPANS", 4: "COVERAGE_DROPS", 5: "READS_FAILED_POLISHING"}
    L = api.lib()
    assert L.ccsx_coverage_rule_version() == 1 and L.ccsx_abi_version() == 6 and L.ccsx_spec_version() == 8
    o = api.coverage_opts_default()
    assert {k: getattr(o, k) for k in R.DEFAULTS} == R.DEFAULTS
    assert api.COVERAGE_GATE_ALL == sum(1 << v for v in R.GATE_STATUS)


def _request(rep, gate=0, reserved=(0, 0), opts=True, **kw):
    o = api.coverage_opts_default()
    for k, v in kw.items():
        setattr(o, k, v)
    cr = rep.c_struct() if rep is not None else None
    q = api.CCoverageRequest(C.pointer(o) if opts else None, C.pointer(cr) if cr is not None else None, gate, (C.c_int32 * 2)(*reserved))
    return q, (o, cr)


def _call(entry, h, b, res, q, fold=None, control=None, reserved=None):
    cb, cr = b.c_struct(), res.c_struct()
    t = C.c_int64(-7)
    rq = api.CRequests(None, fold, None, control, C.pointer(q) if q is not None else None, (C.c_void_p * 3)(*(reserved or (None, None, None))))
    args = [h, C.byref(cb), C.byref(cr), C.byref(rq)]
    rc = getattr(api.lib(), entry)(*(args + [C.byref(t)] if entry == "ccsx_submit_requests" else args))
    assert rc == 0 or t.value == -7                                 # a refused submit hands out no ticket
    return rc


def _bad_requests(b):
    rep = api.CoverageReport.allocate(b.n_zmw)
    bad = [("null coverage request or report", _request(None)),
           ("coverage request: reserved must be 0", _request(rep, reserved=(0, 1))),
           ("coverage request: reserved must be 0", _request(rep, reserved=(7, 0))),
           ("sized for another batch", _request(api.CoverageReport.allocate(b.n_zmw + 1))),
           ("gate has bits outside 2 .. 5", _request(rep, gate=1)), ("gate has bits outside 2 .. 5", _request(rep, gate=2)),
           ("gate has bits outside 2 .. 5", _request(rep, gate=0x40)), ("gate has bits outside 2 .. 5", _request(rep, gate=0x8000003c))]
    for kw in (dict(drop_percent=-1), dict(drop_percent=101), dict(max_lost_percent=-1), dict(max_lost_percent=101), dict(block=0), dict(block=4097),
               dict(min_spans=-1), dict(min_spans=256)):
        bad.append(("coverage options out of range", _request(rep, **kw)))
    good = [_request(rep), _request(rep, opts=False), _request(rep, gate=api.COVERAGE_GATE_ALL, drop_percent=0, max_lost_percent=0, block=1, min_spans=0),
            _request(rep, gate=4, drop_percent=100, max_lost_percent=100, block=4096, min_spans=255)]
    return rep, bad, good


@pytest.mark.parametrize("entry", ["ccsx_consensus_requests", "ccsx_submit_requests"])
def test_entry_points_refuse_bad_requests(built, entry):
    L = api.lib()
    b = api.synth(3, 4, 300, seed=2)
    res = api.Results.allocate(b)
    rep, bad, good = _bad_requests(b)
    for msg, (q, keep) in bad:
        assert _call(entry, None, b, res, q) < 0 and msg.encode() in L.ccsx_last_error(), (msg, L.ccsx_last_error())
    q, keep = _request(rep)
    q.report.contents.used_min = None
    assert _call(entry, None, b, res, q) < 0 and b"coverage report arrays missing" in L.ccsx_last_error()
    q, keep = _request(rep)
    assert _call(entry, None, b, res, q, reserved=(None, 8, None)) < 0 and b"ccsx_requests: reserved must be NULL" in L.ccsx_last_error()
    # a bad fold or control request beside a good coverage request is refused by its own check's message
    frep = api.FoldReport.allocate(b.n_zmw + 1).c_struct()
    fq = api.CFoldRequest(None, C.pointer(frep), (C.c_int32 * 2)(0, 0))
    assert _call(entry, None, b, res, q, fold=C.pointer(fq)) < 0 and b"sized for another batch" in L.ccsx_last_error()
    cq = api.CControlRequest(None, None, None, (C.c_int32 * 2)(0, 0))
    assert _call(entry, None, b, res, q, control=C.pointer(cq)) < 0 and b"null control request or report" in L.ccsx_last_error()
    # valid requests (the limits of every range; NULL options = the defaults), no request, NULL ccsx_requests: the handle is what is missing
    for q, keep in good:
        assert _call(entry, None, b, res, q) < 0 and b"null argument" in L.ccsx_last_error(), L.ccsx_last_error()
    assert _call(entry, None, b, res, None) < 0 and b"null argument" in L.ccsx_last_error()
    cb, cr, t = b.c_struct(), res.c_struct(), C.c_int64(-7)
    tail = [C.byref(t)] if entry == "ccsx_submit_requests" else []
    assert getattr(L, entry)(None, C.byref(cb), C.byref(cr), None, *tail) < 0 and b"null argument" in L.ccsx_last_error() and t.value == -7


def test_python_refuses_the_heteroduplex_request_beside_it(built):
    b = api.synth(2, 4, 300, seed=2)
    with pytest.raises(ValueError, match="heteroduplex"):
        api._requests(hd=api.HdReport.allocate(2), coverage=api.CoverageReport.allocate(2))


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module", autouse=True)
def _close_the_shared_handle():
    yield
    if _RUN:
        _RUN.pop("h").close()


RES_FIELDS = ("status", "seq_len", "rq", "np_", "ec", "iters", "n_windows", "fn", "rn")
MIX_SEED = 20


def _same(a, b, z):
    for f in RES_FIELDS:
        assert getattr(a, f)[z].tobytes() == getattr(b, f)[z].tobytes(), (z, f)
    assert np.array_equal(a.sequence(z), b.sequence(z)) and np.array_equal(a.quals(z), b.quals(z)), z
    assert np.array_equal(a.raw(z).view(np.uint32), b.raw(z).view(np.uint32)), z


_MIX = {}


def _mix():
    """(batch, name per ZMW): 23 ZMWs (not a multiple of 4).  The planted layouts on both strands; random templates of 200-600 bases at 3-8 passes; 1500 bases
    (more than 64 windows: the lane stride wraps); 40 passes of 200 bases (more than one polish group of 32); partial passes on both strands; two blocks of 90
    and 250 bases in two of eight passes; three blocks of 250 bases in two of eight passes (the double split: uncovered edge columns, segments longer than
    the pass); the shortest drafts (one and two windows); two ZMWs that fail the
    cascade (two passes; passes of unrelated molecules)"""
    if not _MIX:
        import coverage_synth as S
        rng = np.random.default_rng(MIX_SEED)
        t, at, lay = S.layouts(rng, both=True)
        zmws, names = list(lay.values()), list(lay)
        for k in range(5):
            zmws.append(S.clean(S.rnd(rng, rng.integers(200, 601)), int(rng.integers(3, 9)), both=True)); names.append("random")
        zmws.append(S.clean(S.rnd(rng, 1500), 5, both=True)); names.append("long")
        zmws.append(S.clean(S.rnd(rng, 200), 40, both=True)); names.append("deep")
        zmws.append(S.with_partials(S.rnd(rng, 450), 5, (0.7, 0.4, 0.55), both=True)); names.append("partials_both")
        t2 = S.rnd(rng, 600)
        two = S.with_block(S.with_block(t2, S.rnd(rng, 250), 420), S.rnd(rng, 90), 180)
        zmws.append([S.Pass(two if q in (5, 6) else t2, bool(q & 1)) for q in range(8)]); names.append("two_blocks")
        zmws.append(S.clean(S.rnd(rng, 16), 6, both=True)); names.append("one_window")
        zmws.append(S.clean(S.rnd(rng, 40), 6, both=True)); names.append("two_windows")
        zmws.append(S.clean(S.rnd(rng, 300), 2, both=True)); names.append("two_passes")
        zmws.append([S.Pass(S.rnd(rng, 300), bool(q & 1)) for q in range(6)]); names.append("unrelated")
        zmws.append(S.blocked(t, S.rnd(rng, 120), 200, {1, 3, 5, 7}, 8, both=True)); names.append("block120_one_strand")
        t3 = S.rnd(rng, 900)
        three = t3
        for at3 in (720, 450, 180):
            three = S.with_block(three, S.rnd(rng, 250), at3)
        zmws.append([S.Pass(three if q in (4, 7) else t3, bool(q & 1)) for q in range(8)]); names.append("three_blocks")
        _MIX["b"] = (S.batch(zmws, rng), names)
        assert len(zmws) == 23
    return _MIX["b"]


def _reference(h, b, d, opts=None, gate=0):
    """coverage_ref on the stage accessors of the handle's last synchronous run, for every ZMW: the pre-polish planes and reach_sum"""
    out = []
    for z in range(b.n_zmw):
        tested = d.status[z] == 0
        if not tested:
            out.append(R.screen(0, [0], [], tested=False)); continue
        Ld = len(h.stage_draft(z))
        wb = h.stage_windows(z)
        passes = []
        for r in range(int(b.read_off[z]), int(b.read_off[z + 1])):
            rs, v, _ = h.stage_align(r, Ld)
            passes.append((rs, v, int(b.base_off[r + 1] - b.base_off[r]), bool(b.flags[r] & 2)))
        out.append(R.screen(Ld, wb, passes, opts, h.opts.min_passes, gate=gate))
    return out


def _opts(**kw):
    o = api.coverage_opts_default()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _report_dicts(rep):
    return [{f: int(getattr(rep, f)[z]) for f in R.FIELDS} for z in range(len(rep.verdict))]


_RUN = {}


def _base_run():
    """one handle, the draft seam's statuses, the plain results, the gate-0 run with the default options and its reference: shared by the GPU tests"""
    if not _RUN:
        b, names = _mix()
        h = api.Handle(0)
        d = h.draft(b)
        plain = h.consensus(b)
        res, rep, *_ = h.consensus_coverage(b)
        want = _reference(h, b, d)
        _RUN.update(h=h, b=b, names=names, d=d, plain=plain, res=res, rep=rep, want=want)
    return _RUN


@pytest.mark.gpu
def test_report_equals_the_reference(built):
    run = _base_run()
    b, names, d, rep, want, res = run["b"], run["names"], run["d"], run["rep"], run["want"], run["res"]
    got = _report_dicts(rep)
    for z in range(b.n_zmw):
        for f in R.PRE + ("reach_sum",):
            assert got[z][f] == want[z][f], (z, names[z], f, got[z], want[z])
    assert np.array_equal(rep.verdict == R.UNTESTED, d.status != 0)
    by = dict(zip(names, range(b.n_zmw)))                                      # (the last ZMW of each name)
    v = lambda name: int(rep.verdict[by[name]])
    # the batch holds what it is meant to hold
    assert v("two_passes") == R.UNTESTED and v("unrelated") == R.UNTESTED
    assert v("clean") == R.NONE and v("block300_2of8") == R.NONE and v("partials") == R.NONE and v("long") == R.NONE and v("deep") == R.NONE
    assert v("block300_last4") == v("block300_alternating") == v("block60_4of8") == v("block120_one_strand") == R.COVERAGE_DROPS
    assert rep.clean_min[by["block300_last4"]] == 4 and rep.spans[by["block300_last4"]] == 8
    assert rep.np_aligned[by["block300_first5"]] == rep.spans[by["block300_first5"]] == 5
    assert rep.cov_max[by["partials"]] == 8 and rep.np_aligned[by["partials"]] == 6 and rep.cov_max[by["partials_both"]] > rep.np_aligned[by["partials_both"]]
    assert res.n_windows[by["long"]] > 64 and rep.np_aligned[by["deep"]] == 40 == rep.cov_max[by["deep"]]
    assert rep.spans[by["three_blocks"]] < rep.np_aligned[by["three_blocks"]] == 8   # the double-split passes align and do not span
    assert v("one_window") != R.UNTESTED and res.n_windows[by["one_window"]] == 1 and v("two_windows") != R.UNTESTED and res.n_windows[by["two_windows"]] == 2
    assert b.n_zmw % 4 != 0


@pytest.mark.gpu
def test_post_polish_planes(built):
    run = _base_run()
    b, names, rep, res, h = run["b"], run["names"], run["rep"], run["res"], run["h"]
    ref = api.Results.allocate(b)
    O.consensus_batch(h.model, h.opts, b, ref)
    some = 0
    for z in range(b.n_zmw):
        if res.seq_len[z] > 0:
            some += 1
            nw = int(res.n_windows[z])
            assert ref.n_windows[z] == nw and rep.used_sum[z] == int(np.rint(float(ref.ec[z]) * nw)), (z, names[z], rep.used_sum[z], ref.ec[z], nw)
            assert rep.used_min[z] * nw <= rep.used_sum[z] and rep.reach_sum[z] >= rep.used_sum[z] > 0, (z, names[z])
        elif rep.verdict[z] == R.UNTESTED:
            assert rep.used_sum[z] == rep.used_min[z] == rep.reach_sum[z] == 0
    assert some >= 18
    z2 = names.index("two_blocks")
    assert res.seq_len[z2] > 0 and rep.reach_sum[z2] > rep.used_sum[z2]
    # max_lost_percent = 0: exactly the ZMWs that lost a segment, of those the earlier verdicts left NONE and the polish left SUCCESS or LOW_RQ
    res0, rep0, *_ = h.consensus_coverage(b, _opts(max_lost_percent=0))
    lost = (rep.reach_sum > rep.used_sum) & (rep.verdict == R.NONE) & np.isin(res.status, (R.SUCCESS, R.LOW_RQ))
    assert lost.any() and (~lost & (rep.verdict == R.NONE)).any()
    assert np.array_equal(rep0.verdict == R.READS_FAILED_POLISHING, lost)
    assert np.array_equal(rep0.verdict[~lost], rep.verdict[~lost])
    for f in R.FIELDS[1:]:
        assert np.array_equal(getattr(rep0, f), getattr(rep, f)), f
    for z in range(b.n_zmw):
        _same(res0, run["plain"], z)


@pytest.mark.gpu
def test_detection_only_changes_nothing(built):
    import control_synth as CS
    run = _base_run()
    b, h, rep = run["b"], run["h"], run["rep"]
    for z in range(b.n_zmw):
        _same(run["res"], run["plain"], z)
    seq = api.ControlSeq.from_string(CS.TEST_CONTROL)
    one = api.AdapterSet.default()
    ref, crep_ref, frep_ref, arep_ref, tl_ref, pile_ref = h.consensus_control(b, seq, fold=True, adapters=one, tandem=True, pileup=True)
    res, vrep, crep, frep, arep, tl, pile = h.consensus_coverage(b, control=seq, fold=True, adapters=one, tandem=True, pileup=True)
    for z in range(b.n_zmw):
        _same(res, ref, z)
        _same(res, run["plain"], z)
    for f in api.ControlReport.FIELDS:
        assert np.array_equal(getattr(crep, f), getattr(crep_ref, f)), f
    for f in ("verdict", "fold", "hits", "span"):
        assert np.array_equal(getattr(frep, f), getattr(frep_ref, f)), f
    for f in api.AdapterReport.INT_FIELDS:
        assert np.array_equal(getattr(arep, f), getattr(arep_ref, f)), f
    assert arep.hits.tobytes() == arep_ref.hits.tobytes() and np.array_equal(tl, tl_ref)
    for f in ("coverage", "matches", "mismatches"):
        assert np.array_equal(getattr(pile, f), getattr(pile_ref, f)), f
    for f in R.FIELDS:
        assert np.array_equal(getattr(vrep, f), getattr(rep, f)), f


@pytest.mark.gpu
def test_the_old_entry_points_equal_the_requests_form(built):
    import control_synth as CS
    run = _base_run()
    b, h = run["b"], run["h"]
    seq = api.ControlSeq.from_string(CS.TEST_CONTROL)
    one = api.AdapterSet.default()

    def go(form, via):
        res = api.Results.allocate(b, pinned=form == "submit")
        reps = (api.ControlReport.allocate(b.n_zmw, True), api.FoldReport.allocate(b.n_zmw, True), api.AdapterReport.allocate(b.n_zmw, True))
        tl = api.tandem_buffer(b.n_zmw, pinned=True)
        rq = api._requests(None, tl, 0, fold=reps[1], adapters=reps[2], adapter_set=one, control=reps[0], control_seq=seq, via_requests=via)
        assert isinstance(rq[-1][-1], api.CRequests) == via
        if form == "submit":
            t = C.c_int64()
            keep = h._fused("submit", b, res, rq, t)
            h._check(h._L.ccsx_wait(h._h, t.value), "ccsx_wait")
        else:
            keep = h._fused("consensus", b, res, rq)
        return res, reps, tl, keep, rq

    for form in ("consensus", "submit"):
        old, new = go(form, False), go(form, True)
        for z in range(b.n_zmw):
            _same(old[0], new[0], z)
        for ro, rn in zip(old[1], new[1]):
            for k, _, _ in ro.PLANES:
                assert getattr(ro, k).tobytes() == getattr(rn, k).tobytes(), (form, k)
        assert np.array_equal(old[2], new[2])
    # no member at all: ccsx_consensus_batch
    res = api.Results.allocate(b)
    h._fused("consensus", b, res, api._requests(via_requests=True))
    for z in range(b.n_zmw):
        _same(res, run["plain"], z)


def _check_gated(b, res, rep, plain, rep0, gate, names):
    """res / rep of a run with `gate` against the plain results and the gate-0 report rep0 of the same options"""
    n_gated = 0
    for z in range(b.n_zmw):
        v = int(rep0.verdict[z])
        if v >= 2 and (gate >> v) & 1:
            n_gated += 1
            assert res.status[z] == R.GATE_STATUS[v] and res.seq_len[z] == 0, (z, names[z], v, res.status[z])
            pre = v < R.READS_FAILED_POLISHING
            if pre:
                assert res.n_windows[z] == res.iters[z] == 0 and res.rq[z] == res.ec[z] == 0 and res.np_[z] == rep0.np_aligned[z] == res.fn[z] + res.rn[z]
            for f in R.FIELDS:
                want = 0 if pre and f in ("used_sum", "used_min") else int(getattr(rep0, f)[z])
                assert getattr(rep, f)[z] == want, (z, names[z], f)
        else:
            _same(res, plain, z)
            for f in R.FIELDS:
                assert getattr(rep, f)[z] == getattr(rep0, f)[z], (z, names[z], f)
    return n_gated


@pytest.mark.gpu
def test_gate(built):
    run = _base_run()
    b, h, names, plain, rep0 = run["b"], run["h"], run["names"], run["plain"], run["rep"]
    res, rep, *_ = h.consensus_coverage(b, gate=api.COVERAGE_GATE_ALL)
    assert _check_gated(b, res, rep, plain, rep0, api.COVERAGE_GATE_ALL, names) == int((rep0.verdict >= 2).sum()) >= 4
    # one bit only: COVERAGE_DROPS is reported and not gated when its bit is clear
    only = 1 << R.INSUFFICIENT_SPANS
    res, rep, *_ = h.consensus_coverage(b, gate=only)
    assert _check_gated(b, res, rep, plain, rep0, only, names) == int((rep0.verdict == R.INSUFFICIENT_SPANS).sum())
    # every verdict once: min_spans 8 and max_lost_percent 0 beside the defaults' coverage drops; a handle with min_passes 7 for DRAFT_TOO_DIFFERENT
    o = _opts(min_spans=8, max_lost_percent=0)
    _, repo, *_ = h.consensus_coverage(b, o)
    res, rep, *_ = h.consensus_coverage(b, o, gate=api.COVERAGE_GATE_ALL)
    assert {R.INSUFFICIENT_SPANS, R.COVERAGE_DROPS, R.READS_FAILED_POLISHING, R.NONE, R.UNTESTED} <= set(repo.verdict.tolist())
    _check_gated(b, res, rep, plain, repo, api.COVERAGE_GATE_ALL, names)
    post = 1 << R.READS_FAILED_POLISHING
    res, rep, *_ = h.consensus_coverage(b, o, gate=post)
    assert _check_gated(b, res, rep, plain, repo, post, names) == int((repo.verdict == R.READS_FAILED_POLISHING).sum()) >= 1
    # the gated run with the screens and the optional outputs beside it: the same statuses
    import control_synth as CS
    res2, rep2, *_ = h.consensus_coverage(b, o, gate=api.COVERAGE_GATE_ALL, control=api.ControlSeq.from_string(CS.TEST_CONTROL), fold=True, tandem=True, pileup=True)
    res1, rep1, *_ = h.consensus_coverage(b, o, gate=api.COVERAGE_GATE_ALL)
    for z in range(b.n_zmw):
        _same(res2, res1, z)
    for f in R.FIELDS:
        assert np.array_equal(getattr(rep2, f), getattr(rep1, f)), f
    # a bad request with a handle: an error of the call, and the handle still works
    for entry in ("ccsx_consensus_requests", "ccsx_submit_requests"):
        q, keep = _request(api.CoverageReport.allocate(b.n_zmw + 1))
        assert _call(entry, h._h, b, api.Results.allocate(b), q) < 0 and b"sized for another batch" in api.lib().ccsx_last_error()
        q, keep = _request(api.CoverageReport.allocate(b.n_zmw), gate=3)
        assert _call(entry, h._h, b, api.Results.allocate(b), q) < 0
    _, rep3, *_ = h.consensus_coverage(b)
    for f in R.FIELDS:
        assert np.array_equal(getattr(rep3, f), getattr(rep0, f)), f


@pytest.mark.gpu
def test_draft_too_different(built):
    """a handle whose min_passes is above what aligns: the first verdict of the order"""
    run = _base_run()
    b, names = run["b"], run["names"]
    o = api.default_opts()
    o.min_passes = 7
    h = api.Handle(0, opts=o)
    d = h.draft(b)
    plain = h.consensus(b)
    res0, rep0, *_ = h.consensus_coverage(b)
    want = _reference(h, b, d)
    got = _report_dicts(rep0)
    for z in range(b.n_zmw):
        for f in R.PRE + ("reach_sum",):
            assert got[z][f] == want[z][f], (z, names[z], f, got[z], want[z])
        _same(res0, plain, z)
    zs = np.flatnonzero(rep0.verdict == R.DRAFT_TOO_DIFFERENT)
    assert len(zs) >= 1 and (rep0.np_aligned[zs] < 7).all() and names.index("block300_first5") in zs
    assert rep0.verdict[names.index("partials")] == R.UNTESTED                 # (six full-length passes: TOO_FEW_PASSES before any draft)
    res, rep, *_ = h.consensus_coverage(b, gate=1 << R.DRAFT_TOO_DIFFERENT)
    assert _check_gated(b, res, rep, plain, rep0, 1 << R.DRAFT_TOO_DIFFERENT, names) == len(zs)
    h.close()


@pytest.mark.gpu
def test_tickets_carry_their_own_options(built):
    """four tickets on three slots with different options and gates, waited for out of order; each equals its own synchronous call"""
    run = _base_run()
    b, h = run["b"], run["h"]
    bp = b.pinned()
    cfg = [(dict(), 0), (dict(drop_percent=80, block=20), api.COVERAGE_GATE_ALL), (dict(drop_percent=10, max_lost_percent=0), 1 << R.READS_FAILED_POLISHING),
           (dict(min_spans=8), 1 << R.INSUFFICIENT_SPANS)]
    want = [h.consensus_coverage(b, _opts(**kw), gate=g)[:2] for kw, g in cfg]
    assert len({w[1].verdict.tobytes() for w in want}) == len(cfg)             # the options matter on this batch
    tickets, outs = [], []
    for kw, g in cfg:
        res = api.Results.allocate(b, pinned=True)
        rep = api.CoverageReport.allocate(b.n_zmw, pinned=True)
        tickets.append(h.submit(bp, res, coverage=rep, coverage_opts=_opts(**kw), coverage_gate=g))
        outs.append((res, rep))
    for t in (tickets[2], tickets[1], tickets[3]):
        h.wait(t)
    for k, ((res, rep), (wres, wrep)) in enumerate(zip(outs, want)):
        for f in R.FIELDS:
            assert np.array_equal(getattr(rep, f), getattr(wrep, f)), (k, f)
        for z in range(b.n_zmw):
            _same(res, wres, z)
    # a slot that carried a gating request runs without it afterwards: a plain submit, nothing of the screen left behind
    res = api.Results.allocate(b, pinned=True)
    h.wait(h.submit(bp, res))
    for z in range(b.n_zmw):
        _same(res, run["plain"], z)

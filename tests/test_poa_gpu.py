"""The POA kernels (k_poa_init / k_poa_dp / k_poa_thread / k_poa_finish) on the planted lab of tests/poa_lab.py, held pass by pass to the plain reference
(tests/poa_ref.py) and to the CPU restatement through the engine's POA log (ccsx_poa_log / ccsx_stage_poa): I, end score, end position, threaded, vertices of every
pass of every generator, the drafts, and the unbanded optimum for every pass that is not excused by name.  Then the same ZMWs in other company: the lab reversed,
the 2100-base ZMW between short ones, partly filled waves — every draft and every record must come out the same."""
from functools import lru_cache

import numpy as np
import pytest

from ccs_amd import api
import oracle_lib as O
import poa_lab as L
import poa_ref as R

pytestmark = pytest.mark.gpu
FIELDS = ("pass", "I", "end score", "end position", "threaded", "vertices")


def opts(no_fallback=0):
    o = api.default_opts()
    o.max_poa_cov = L.COV
    o.no_fallback_draft = no_fallback
    return o


def rows(recs):
    return np.array([(q.rr,) + q.log() for q in recs], np.int32).reshape(-1, 6)


DRAFT_STAGE = (1, 2, 3, 5, 6)      # TOO_FEW_PASSES, DRAFT_FAILURE, TOO_MANY_UNUSABLE, TOO_SHORT, TOO_LONG: the statuses the draft stage decides;
                                   # every other status of the fused path (LOW_RQ, NON_CONVERGENT, ...) is the polish stage's, the draft seam reports SUCCESS


def oracle_run(z, no_fallback):
    """the CPU restatement's whole path on one ZMW: (status, consensus, fallback generator taken, last resort taken)"""
    b1 = L.batch_of([z])
    ref = api.Results.allocate(b1)
    O.lib().orc_counts_sync(); O.counts_reset()
    O.consensus_batch(api.default_model(), opts(no_fallback), b1, ref)
    O.lib().orc_counts_sync(); c = O.counts()
    return int(ref.status[0]), ref.sequence(0).copy(), bool(c["fallback"]), bool(c["third_draft"])


@lru_cache(maxsize=None)
def reference():
    """per lab ZMW: the reference's first generator (draft, log rows, the unbanded optimum of every pass), its second one, and for both modes (no_fallback_draft
    1 / 0) what the draft seam must hand out — `seam[nf]` = (status, backbone, draft or None, fallback generator runs) — from the CPU restatement's whole path
    under the same options: its status where the draft stage decides it, SUCCESS otherwise; the generator it ended with; that generator's draft by the reference"""
    out = []
    for z in L.lab():
        d, recs = R.poa_spec(z.reads, z.flags, L.COV, 0, snapshots=True)
        optima = [R.opt_unbanded(q.dag, R.orient(z.reads[q.read], (z.flags[q.read] & 1) != (z.flags[0] & 1))).opt for q in recs]
        fb = R.fallback_backbone(z.reads, z.flags)
        d2, recs2 = R.poa_spec(z.reads, z.flags, 2 * L.COV, fb)
        lens = [len(r) for r, f in zip(z.reads, z.flags) if not f & 2]
        bb3 = R.closest_to_median(lens, excluded=(0, fb) if len(lens) > 2 else (fb,) if len(lens) > 1 else ())
        seam = {}
        for nf in (1, 0):
            st, seq, took_fb, third = oracle_run(z, nf)
            assert not (nf and (took_fb or third))
            want = (bb3, R.orient(z.reads[bb3], 0)) if third else (fb, d2) if took_fb else (0, d)
            seam[nf] = (st if st in DRAFT_STAGE else 0, want[0], want[1], took_fb)
            if nf == 0: status, cons = st, seq
        out.append(dict(rows=rows(recs), opt=optima, rows2=rows(recs2), seam=seam, status=status, seq=cons))
    return out


def run_drafts(h, zmws):
    """the draft seam over `zmws` with the log on: (Drafts, [(generator 0 rows, generator 1 rows) per ZMW])"""
    b = L.batch_of(zmws)
    d = h.draft(b)
    return d, [h.stage_poa(k) for k in range(len(zmws))]


def assert_rows(z, what, got, want):
    assert len(got) == len(want), f"{z.name} ({z.cls}) {what}: {len(got)} passes in the engine's log, {len(want)} expected\n{got.tolist()}\n{want.tolist()}"
    for a, b in zip(got, want):
        for f in range(6):
            assert a[f] == b[f], f"{z.name} ({z.cls}) {what} pass {b[0]} {FIELDS[f]}: engine {a[f]}, expected {b[f]}"


def check_run(zmws, idx, d, logs, cascade):
    """every ZMW of a draft-seam run against the reference and the oracle; idx[k] = the lab index of zmws[k]"""
    ref = reference()
    for k, z in enumerate(zmws):
        E = ref[idx[k]]
        g0, g1 = logs[k]
        assert_rows(z, "generator 0", g0, E["rows"])
        for (what, fn) in z.log_checks: assert fn(g0), f"{z.name} ({z.cls}): the class is not in the engine's log — {what}: {g0.tolist()}"
        for row, opt in zip(g0, E["opt"]):
            if int(row[0]) in z.excused: assert row[2] < opt, f"{z.name} pass {row[0]}: excused, but the engine reaches the optimum {opt}"
            else: assert row[2] == opt, f"{z.name} ({z.cls}) pass {row[0]} end score: engine {row[2]}, unbanded optimum {opt}"
        want_st, want_bb, want_d, took_fb = E["seam"][0 if cascade else 1]
        assert_rows(z, "generator 1", g1, E["rows2"] if took_fb else np.zeros((0, 6), np.int32))
        if z.fallback is not None and cascade: assert took_fb, f"{z.name}: the fallback generator was expected to run"
        # status, backbone and draft of the seam, for every ZMW whatever the engine says about it: the generator the oracle's cascade ends with, its draft
        where = f"{z.name} ({z.cls}, {'cascade' if cascade else 'single attempt'})"
        assert int(d.status[k]) == want_st, f"{where}: status {api.STATUS_NAMES[int(d.status[k])]}, expected {api.STATUS_NAMES[want_st]}"
        if z.fails and not cascade: assert want_st == 2 and want_d is None, f"{where}: the lab expects DRAFT_FAILURE of the first generator"
        assert int(d.backbone[k]) == want_bb, f"{where}: backbone {int(d.backbone[k])}, expected {want_bb}"
        got = d.draft(k)
        if want_d is None: assert len(got) == 0, f"{where}: a draft of {len(got)} bases where the generator fails"
        else: assert np.array_equal(got, want_d), f"{where}: the draft ({len(got)} bases) differs from the reference's ({len(want_d)} bases, backbone {want_bb})"
        if z.planted is not None and (z.fallback is None or took_fb) and want_st in (0, 5):
            assert np.array_equal(got, z.planted), f"{where}: the planted draft was not found"
        if want_st == 0: assert np.array_equal(d.windows(k), O.windows(got)), f"{where}: window bounds of a draft of {len(got)} bases"
        else: assert int(d.n_windows[k]) == 0, f"{where}: {int(d.n_windows[k])} windows with status {api.STATUS_NAMES[want_st]}"


@pytest.fixture(scope="module")
def whole(built):
    """the whole lab through the draft seam with the log on: without the fallback, then with the cascade"""
    out = {}
    for nf in (1, 0):
        h = api.Handle(0, opts=opts(nf))
        h.poa_log(True)
        out[nf] = run_drafts(h, L.lab())
        h.close()
    return out


def test_lab_single_attempt(whole):
    d, logs = whole[1]
    check_run(L.lab(), list(range(len(L.lab()))), d, logs, cascade=False)
    assert sum(int(s) == 2 for s in d.status) >= 1                         # the overflow ZMW at least ends in DRAFT_FAILURE


def test_lab_cascade(whole):
    d, logs = whole[0]
    Z = L.lab()
    check_run(Z, list(range(len(Z))), d, logs, cascade=True)
    by = {z.name: k for k, z in enumerate(Z)}
    assert {int(d.backbone[by[n]]) for n in ("fallback_middle", "fallback_last")} == {2, 4}
    assert int(d.status[by["overflow_sibling"]]) == 0 and len(logs[by["overflow"]][1]) > 0


def same_as_whole(whole, nf, zmws, idx, d, logs):
    D, LG = whole[nf]
    for k, z in enumerate(zmws):
        j = idx[k]
        for gen in (0, 1): assert_rows(z, f"generator {gen} in other company", logs[k][gen], LG[j][gen])
        assert int(d.status[k]) == int(D.status[j]) and int(d.backbone[k]) == int(D.backbone[j]) and np.array_equal(d.draft(k), D.draft(j)), \
            f"{z.name} ({z.cls}): draft, status or backbone depend on the batch it is in"


def test_composition_invariance(whole):
    Z = L.lab()
    by = {z.name: k for k, z in enumerate(Z)}
    order = [k for k in reversed(range(len(Z))) if Z[k].name != "chunk_reload"]
    at = order.index(by["short_2"])
    order.insert(at, by["chunk_reload"])                                       # the 2100-base ZMW between short ones
    picks = [by[n] for n in ("ring_del_9", "chunk_reload", "overflow", "ring_bubble_9", "ring_bubble_20", "overflow_sibling", "ring_del_8", "ring_del_20")]
    groups = [order, picks[:1], picks[1:3], picks[3:6], picks[1:2] + picks[4:8]]   # the lab reversed, then partly filled waves of 1, 2, 3 and 5 graphs
    assert [len(g) for g in groups[1:]] == [1, 2, 3, 5]
    for nf in (1, 0):
        h = api.Handle(0, opts=opts(nf))
        h.poa_log(True)
        for g in groups:
            zm = [Z[k] for k in g]
            d, logs = run_drafts(h, zm)
            same_as_whole(whole, nf, zm, g, d, logs)
        h.close()


def test_log_off_changes_nothing(whole):
    """drafts and the full fused results with the log off, byte for byte those with it on; the fused results are the oracle's"""
    b = L.batch_of(L.lab())
    h = api.Handle(0, opts=opts(0))
    d_off = h.draft(b)
    r_off = h.consensus(b)
    with pytest.raises(RuntimeError): h.stage_poa(0)
    h.poa_log(True)
    d_on = h.draft(b)
    r_on = h.consensus(b)
    assert len(h.stage_poa(0)[0]) > 0
    h.close()
    D = whole[0][0]
    for x in (d_off, d_on):
        for f in ("status", "len", "backbone", "n_windows"): assert np.array_equal(getattr(x, f), getattr(D, f)), f"drafts differ in {f}"
        for k, z in enumerate(L.lab()):              # (the bytes behind a draft's end are nobody's)
            assert x.draft(k).tobytes() == D.draft(k).tobytes(), f"{z.name}: the draft differs with the log off / on"
            # (a ZMW without windows — a draft below opts.min_length — has no bounds: k_poa_finish writes none, the words are whatever the allocation held)
            if x.n_windows[k] > 0: assert x.windows(k).tobytes() == D.windows(k).tobytes(), f"{z.name}: the window bounds differ with the log off / on"
    for f in ("status", "seq_len", "rq", "np_", "ec", "iters", "n_windows", "fn", "rn"):
        assert getattr(r_off, f).tobytes() == getattr(r_on, f).tobytes(), f"the fused results differ in {f} with the log on"
    for k, z in enumerate(L.lab()):                  # (the bytes behind a consensus' end are nobody's either)
        for f in ("sequence", "quals", "raw"):
            assert getattr(r_off, f)(k).tobytes() == getattr(r_on, f)(k).tobytes(), f"{z.name}: the fused results differ in {f} with the log on"
    ref = reference()
    for k, z in enumerate(L.lab()):
        assert int(r_on.status[k]) == ref[k]["status"], f"{z.name}: status {api.STATUS_NAMES[int(r_on.status[k])]}, the oracle's {api.STATUS_NAMES[ref[k]['status']]}"
        assert np.array_equal(r_on.sequence(k), ref[k]["seq"]), f"{z.name}: the consensus differs from the oracle's"


@pytest.mark.parametrize("cov", [1, 2, 5])
def test_coverage_option(built, cov):
    """max_poa_cov below the passes: min(full passes, cov) - 1 records, never a partial pass among them"""
    Z = [z for z in L.lab() if z.cls in ("coverage option", "ties", "strands", "in-edge count")]
    o = opts(1); o.max_poa_cov = cov
    h = api.Handle(0, opts=o)
    h.poa_log(True)
    d, logs = run_drafts(h, Z)
    h.close()
    for k, z in enumerate(Z):
        want_d, recs = R.poa_spec(z.reads, z.flags, cov, 0)
        assert_rows(z, f"max_poa_cov {cov}", logs[k][0], rows(recs))
        assert len(logs[k][0]) == min(sum(1 for f in z.flags if not f & 2), cov) - 1
        if int(d.status[k]) == 0: assert np.array_equal(d.draft(k), want_d), f"{z.name}: draft at max_poa_cov {cov}"


def test_stage_poa_takes_a_zmw_of_many_passes(built):
    """the log's stride is the most passes of a ZMW in the batch: Handle.stage_poa asks again with the size ccsx_stage_poa names"""
    t = L.template("many", 60)
    z = L.Zmw("many_passes", "coverage option", [t] * 70, [0] * 70)
    h = api.Handle(0, opts=opts(1))
    h.poa_log(True)
    d, logs = run_drafts(h, [z, L.lab()[0]])
    h.close()
    assert [tuple(r) for r in logs[0][0]] == [(rr, 60, 180, 59, 1, 60) for rr in range(1, L.COV)] and len(logs[0][1]) == 0
    assert int(d.status[0]) == 0 and np.array_equal(d.draft(0), t)
    assert_rows(L.lab()[0], "beside it", logs[1][0], reference()[0]["rows"])

"""Adapter screen (DESIGN.md §2 "Adapter screen"; docs/faq/fail-reads.md fail classes 0x10 and 0x40): the restatement against a brute-force reading of the rule,
verdicts on planted templates and controls, the request's ABI and argument checks, and on an MI355X exact parity of k_adapter with the restatement on the
engine's own drafts, no effect on any result, and tickets against the synchronous call."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from ccs_amd import api
import adapter_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
HAIRPIN = R.encode(R.SMRTBELL)
NONDEFAULT = dict(max_dist_pct=30, min_copies=3, max_insert=40, end_slack=60)


def _short_drafts(rng):
    """(draft, adapters) of 0-400 bases: the edge cases of the rule"""
    import adapter_synth
    a = rng.integers(0, 4, int(rng.integers(16, 25))).astype(np.uint8)          # short patterns keep the brute force quick
    b = rng.integers(0, 4, int(rng.integers(16, 25))).astype(np.uint8)
    rnd = lambda m: rng.integers(0, 4, int(m)).astype(np.uint8)
    nz = lambda t: adapter_synth.noisy(rng, t, 0.04, 0.03)
    out = [(np.zeros(0, np.uint8), [a]), (a[:len(a) - 3].copy(), [a]), (rnd(rng.integers(1, 16)), [a, b]),
           (np.concatenate([a, rnd(rng.integers(30, 300))]), [a]),              # flush at position 0
           (np.concatenate([rnd(rng.integers(30, 300)), R.revcomp(a)]), [a]),   # flush at L
           (np.concatenate([rnd(40), a, a, rnd(60)]), [a]),                     # two copies 0 bases apart
           (np.concatenate([rnd(25), a[:len(a) - 5], b[4:], rnd(30), nz(a), rnd(20)]), [a, b]),
           (np.concatenate([rnd(30), a, rnd(50)]), [a, np.concatenate([a[6:], rnd(6)])]),   # overlapping hits of two different patterns
           (np.tile(np.array([0, 1], np.uint8), 200), [np.tile(np.array([0, 1], np.uint8), 10)]),          # one long run of E <= k
           (np.zeros(150, np.uint8), [np.zeros(18, np.uint8), np.concatenate([np.zeros(17, np.uint8), [1]]).astype(np.uint8)]),
           (np.concatenate([nz(np.concatenate([a, rnd(rng.integers(0, 20)), R.revcomp(a), rnd(rng.integers(0, 20)), a])), rnd(80)]), [a]),
           (rnd(rng.integers(100, 400)), [a, b])]
    return out


# ---------------------------------------------------------------- CPU: the restatement
@pytest.mark.parametrize("seed", range(6))
def test_restatement_equals_the_bruteforce(seed):
    rng = np.random.default_rng(seed)
    seen = 0
    for d, ads in _short_drafts(rng):
        for o in (None, NONDEFAULT, dict(max_dist_pct=0, min_copies=1, max_insert=0, end_slack=0)):
            want = R.screen_bruteforce(d, ads, o)
            assert R.screen(d, ads, o) == want, (len(d), o)
            seen += want["n_hits"]
    assert seen > 20
    assert R.screen(np.zeros(50, np.uint8), [HAIRPIN], tested=False) == R.screen_bruteforce(np.zeros(50, np.uint8), [HAIRPIN], tested=False)


def test_edge_cases_by_hand():
    a = HAIRPIN
    rnd = np.random.default_rng(5).integers(0, 4, 3000).astype(np.uint8)
    assert R.screen(np.zeros(0, np.uint8), [a]) == dict(tested=1, verdict=0, n_hits=0, n_listed=0, covered=0, max_gap=0, first_start=-1, last_end=-1, min_dist=255, hits=[])
    r = R.screen(np.concatenate([a, rnd]), [a])
    assert r["hits"] == [(0, 45, 0, 0)] and r["verdict"] == R.NEAR_END and r["max_gap"] == 3000 and r["covered"] == 45
    r = R.screen(np.concatenate([rnd, R.revcomp(a)]), [a])
    assert r["hits"] == [(3000, 3045, 1, 0)] and r["verdict"] == R.NEAR_END
    r = R.screen(np.concatenate([rnd[:90], a, a, rnd[:100]]), [a])
    assert r["hits"] == [(90, 135, 0, 0), (135, 180, 0, 0)] and r["verdict"] == R.CONCAT | R.NEAR_END and r["max_gap"] == 100
    r = R.screen(np.concatenate([rnd[:300], a, rnd[300:601], R.revcomp(a), rnd[:300]]), [a])
    assert r["n_hits"] == 2 and r["verdict"] == 0 and r["max_gap"] == 301          # an insert of 301 bases, both hits more than 200 from the ends


@pytest.mark.parametrize("adapter", [R.SMRTBELL, None])
def test_planted_templates_and_controls(adapter):
    """templates with 2 % substitutions + 1 % indels: dimers, short-arm near-end, interior adapters, controls"""
    import adapter_synth
    rng = np.random.default_rng(11 if adapter else 12)
    A = R.encode(adapter or adapter_synth.TEST_ADAPTER)
    for _ in range(12):
        t = adapter_synth.noisy(rng, adapter_synth.template(rng, "dimer", 0, A))
        r = R.screen(t, [A])
        assert r["verdict"] == R.CONCAT | R.NEAR_END and r["n_hits"] >= 4, r
        t = adapter_synth.noisy(rng, adapter_synth.template(rng, "near_end", int(rng.integers(500, 10001)), A))
        r = R.screen(t, [A])
        assert r["verdict"] == R.NEAR_END and r["n_hits"] == 1, r
        t = adapter_synth.noisy(rng, adapter_synth.template(rng, "interior", int(rng.integers(1000, 10001)), A))
        r = R.screen(t, [A])
        assert r["verdict"] == 0 and r["n_hits"] == 1 and r["min_dist"] <= 9, r
        t = adapter_synth.noisy(rng, adapter_synth.template(rng, "palindrome", int(rng.integers(1000, 10001)), A))
        r = R.screen(t, [A])
        assert r["verdict"] == 0 and r["n_hits"] == 1, r
    for kind in ("random", "lowcx"):
        for _ in range(6):
            t = adapter_synth.template(rng, kind, int(rng.integers(2000, 10001)), A)
            assert R.screen(t, [A])["n_hits"] == 0
            if adapter:
                assert R.smallest_distance(t, [A]) >= 12, kind


def test_more_hits_than_the_list_holds():
    rng = np.random.default_rng(13)
    parts = []
    for _ in range(40):
        parts += [HAIRPIN if rng.random() < 0.5 else R.revcomp(HAIRPIN), rng.integers(0, 4, int(rng.integers(0, 30))).astype(np.uint8)]
    d = np.concatenate(parts)
    r = R.screen(d, [HAIRPIN])
    every = sorted(sum((R.search_hits(p, d, 9, s)[0] for s, p in enumerate(R.searches([HAIRPIN]))), []), key=lambda h: (h[1], h[2]))
    assert r["n_hits"] == len(every) >= 40 and r["n_listed"] == 16 and r["hits"] == every[:16]
    assert r["last_end"] == max(h[1] for h in every) and r["covered"] >= 40 * 45 and r["verdict"] == R.CONCAT | R.NEAR_END


# ---------------------------------------------------------------- CPU: ABI and argument checks
def test_structs_match_the_header(built, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ccsx.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d %d %d\\n", '
                   'sizeof(ccsx_adapter_opts), offsetof(ccsx_adapter_opts, end_slack), sizeof(ccsx_adapter_set), offsetof(ccsx_adapter_set, len), '
                   'offsetof(ccsx_adapter_set, seq), sizeof(ccsx_adapter_hit), offsetof(ccsx_adapter_hit, search), offsetof(ccsx_adapter_hit, dist), '
                   'sizeof(ccsx_adapter_report), offsetof(ccsx_adapter_report, tested), offsetof(ccsx_adapter_report, min_dist), offsetof(ccsx_adapter_report, hits), '
                   'sizeof(ccsx_adapter_request), offsetof(ccsx_adapter_request, opts), offsetof(ccsx_adapter_request, report), offsetof(ccsx_adapter_request, reserved), '
                   'sizeof(ccsx_fold_request), sizeof(ccsx_extras), CCSX_ADAPTER_MAX_PATTERNS, CCSX_ADAPTER_MAX_LEN, CCSX_ADAPTER_MAX_HITS, CCSX_ADAPTER_CONCAT, '
                   'CCSX_ADAPTER_NEAR_END, CCSX_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    O, S, Rp, Q = api.AdapterOpts, api.AdapterSet, api.CAdapterReport, api.CAdapterRequest
    assert got == [C.sizeof(O), O.end_slack.offset, C.sizeof(S), S.len.offset, S.seq.offset, api.ADAPTER_HIT.itemsize, api.ADAPTER_HIT.fields["search"][1],
                   api.ADAPTER_HIT.fields["dist"][1], C.sizeof(Rp), Rp.tested.offset, Rp.min_dist.offset, Rp.hits.offset, C.sizeof(Q), Q.opts.offset,
                   Q.report.offset, Q.reserved.offset, C.sizeof(api.CFoldRequest), 24, api.ADAPTER_MAX_PATTERNS, api.ADAPTER_MAX_LEN, api.ADAPTER_MAX_HITS,
                   api.ADAPTER_CONCAT, api.ADAPTER_NEAR_END, 6]
    assert got[0] == 16 and got[2] == 4 + 32 + 512 and got[5] == 12 and got[8] == 88 and got[12] == 32 and got[16] == 24
    L = api.lib()
    assert L.ccsx_adapter_rule_version() == 1 and L.ccsx_abi_version() == 6 and L.ccsx_spec_version() == 8
    o = api.adapter_opts_default()
    assert dict(max_dist_pct=o.max_dist_pct, min_copies=o.min_copies, max_insert=o.max_insert, end_slack=o.end_slack) == R.DEFAULTS
    assert api.AdapterSet.default().strings() == [R.SMRTBELL] == ["ATCTCTCTCTTTTCCTCCTCCTCCGTTGTTGTTGTTGAGAGAGAT"]
    assert L.ccsx_adapter_set_default(None) < 0
    assert api.AdapterSet.from_strings(["acgtACGTacgtACGTa"]).strings() == ["ACGTACGTACGTACGTA"]


def _request(rep, aset=None, reserved=(0, 0), opts=True, **kw):
    o = api.adapter_opts_default()
    for k, v in kw.items():
        setattr(o, k, v)
    a = aset if aset is not None else api.AdapterSet.default()
    cr = rep.c_struct() if rep is not None else None
    q = api.CAdapterRequest(C.pointer(a), C.pointer(o) if opts else None, C.pointer(cr) if cr is not None else None, (C.c_int32 * 2)(*reserved))
    return q, (o, a, cr)


def _call(entry, h, b, res, q, fold=None):
    cb, cr = b.c_struct(), res.c_struct()
    t = C.c_int64()
    args = [h, C.byref(cb), C.byref(cr), None, fold, q]
    return getattr(api.lib(), entry)(*(args + [C.byref(t)] if entry == "ccsx_submit_screen" else args))


def _set(lens, poke=None):
    s = api.AdapterSet.from_strings([("ACGT" * 16)[:n] for n in lens])
    if poke:
        s.seq[poke[0]][poke[1]] = poke[2]
    return s


@pytest.mark.parametrize("entry", ["ccsx_consensus_screen", "ccsx_submit_screen"])
def test_entry_points_refuse_bad_requests(built, entry):
    L = api.lib()
    b = api.synth(3, 4, 300, seed=2)
    res = api.Results.allocate(b)
    rep = api.AdapterReport.allocate(b.n_zmw)
    nine = _set([20] * 8)
    nine.n_adapters = 9
    none = _set([20])
    none.n_adapters = 0
    bad = [("null adapter request or report", _request(None)),
           ("reserved must be 0", _request(rep, reserved=(0, 1))),
           ("reserved must be 0", _request(rep, reserved=(7, 0))),
           ("sized for another batch", _request(api.AdapterReport.allocate(b.n_zmw + 1))),
           ("n_adapters outside 1 .. 8", _request(rep, nine)),
           ("n_adapters outside 1 .. 8", _request(rep, none)),
           ("adapter 1: length outside 16 .. 64", _request(rep, _set([16, 15, 30]))),
           ("adapter 0: length outside 16 .. 64", _request(rep, _set([0]))),
           ("adapter 2: code above 3", _request(rep, _set([64, 16, 40], poke=(2, 39, 4))))]
    for kw in (dict(max_dist_pct=-1), dict(max_dist_pct=31), dict(min_copies=0), dict(max_insert=-1), dict(end_slack=-1)):
        bad.append(("adapter options out of range", _request(rep, **kw)))
    for msg, (q, keep) in bad:
        assert _call(entry, None, b, res, C.byref(q)) < 0 and msg.encode() in L.ccsx_last_error(), (msg, L.ccsx_last_error())
    q, keep = _request(rep)
    q.adapters = None
    assert _call(entry, None, b, res, C.byref(q)) < 0 and b"null adapter set" in L.ccsx_last_error()
    # a bad fold request beside a good adapter request is refused by the fold check's message
    frep = api.FoldReport.allocate(b.n_zmw + 1).c_struct()
    fq = api.CFoldRequest(None, C.pointer(frep), (C.c_int32 * 2)(0, 0))
    q, keep = _request(rep)
    assert _call(entry, None, b, res, C.byref(q), C.byref(fq)) < 0 and b"sized for another batch" in L.ccsx_last_error()
    # valid requests (the limits of every range; NULL options = the defaults): the handle is what is missing
    for q, keep in (_request(rep), _request(rep, opts=False), _request(rep, _set([16, 64] * 4), max_dist_pct=30, min_copies=1, max_insert=0, end_slack=0),
                    _request(rep, max_dist_pct=0)):
        assert _call(entry, None, b, res, C.byref(q)) < 0 and b"null argument" in L.ccsx_last_error(), L.ccsx_last_error()
    assert _call(entry, None, b, res, None) < 0 and b"null argument" in L.ccsx_last_error()


# ---------------------------------------------------------------- GPU
FIELDS = ("status", "seq_len", "rq", "np_", "ec", "iters", "n_windows", "fn", "rn")
MIX_SEED = 41
EIGHT = [R.SMRTBELL, None, "ACGTTGCAAGGCTTAACCGGTTAGC", "TTTTTTTTTTTTTTTTTTTT", "CACACACACACACACACA", "GATTACAGATTACAGATTACAGATTACAGATTACAGATTACAGATTACAGATTACAGATTACAG",
         "AGGCTTAGCTAGGATC", "CCGTTGTTGTTGTTGAGAGAGATATCTCTCTC"]


def _same(a, b, z):
    for f in FIELDS:
        assert getattr(a, f)[z].tobytes() == getattr(b, f)[z].tobytes(), (z, f)
    assert np.array_equal(a.sequence(z), b.sequence(z)) and np.array_equal(a.quals(z), b.quals(z)), z
    assert np.array_equal(a.raw(z).view(np.uint32), b.raw(z).view(np.uint32)), z


def _mix(seed=MIX_SEED):
    """(batch, kind name per ZMW): 54 ZMWs of every adapter_synth kind around the built-in adapter, 48 around the test adapter, 3-10 passes, templates of
    300-12000 bases, and one interior-adapter template of 42 kb at 3 passes"""
    import adapter_synth as S
    rng = np.random.default_rng(seed)
    b1, k1 = S.make(54, (3, 10), (300, 12000), seed, adapter=S.SMRTBELL)
    b2, k2 = S.make(48, (3, 10), (300, 12000), seed + 1, adapter=S.TEST_ADAPTER)
    long = S.from_templates([S.template(rng, "interior", 42000, R.encode(S.TEST_ADAPTER))], [3], rng)
    kinds = [S.KINDS[k] for k in k1] + [S.KINDS[k] for k in k2] + ["long"]
    return api.concat([b1, b2, long]), kinds


def _eight():
    import adapter_synth as S
    return [R.encode(s or S.TEST_ADAPTER) for s in EIGHT]


def _check_report(d, rep, adapters, o=None):
    """the report against adapter_ref on the draft seam's drafts (the drafts k_polish is given), every field of every ZMW; returns the tested ZMWs"""
    tested = []
    for z in range(len(rep.verdict)):
        want = R.screen(d.draft(z), adapters, o, tested=d.status[z] == 0)
        got = {f: int(getattr(rep, f)[z]) for f in R.FIELDS}
        got["hits"] = rep.listed(z)
        assert got == want, (z, got, want, int(d.status[z]), len(d.draft(z)))
        assert not rep.hits[z, int(rep.n_listed[z]):].view(np.uint8).any(), z
        if want["tested"]:
            tested.append(z)
    return tested


@pytest.mark.gpu
def test_report_equals_the_restatement_and_results_do_not_change(built):
    """The oracle on the CPU for MIX_SEED (a final status that is not a draft-stage failure = tested): 103 of 103 ZMWs, 17 of 17 of every kind and the 42 kb
    one (68 SUCCESS, 35 LOW_RQ)"""
    import adapter_synth as S
    b, kinds = _mix()
    h = api.Handle(0)
    d = h.draft(b)
    ref, tl_ref, pile_ref = h.consensus_extras(b, tandem=True, pileup=True)
    _, frep_ref = h.consensus_fold(b)
    one = api.AdapterSet.default()
    res, frep, rep, tl, pile = h.consensus_screen(b, fold=True, adapters=one, tandem=True, pileup=True)
    tested = _check_report(d, rep, [HAIRPIN])
    assert np.array_equal(rep.tested, (d.status == 0).astype(np.int32))
    # the only ZMWs the comparison leaves out are the untested ones: three quarters of the batch and half of every kind are tested
    assert len(tested) >= 0.75 * b.n_zmw, (len(tested), b.n_zmw)
    for kind in set(kinds):
        zs = [z for z in range(b.n_zmw) if kinds[z] == kind]
        assert 2 * sum(z in tested for z in zs) >= len(zs), (kind, [int(d.status[z]) for z in zs])
    assert max(len(d.draft(z)) for z in tested) > 40000
    # detection only: every result byte, the fold report, the pileup planes and tandem_len equal the calls without the adapter request
    for z in range(b.n_zmw):
        _same(res, ref, z)
    for f in ("verdict", "fold", "hits", "span"):
        assert np.array_equal(getattr(frep, f), getattr(frep_ref, f)), f
    assert np.array_equal(tl, tl_ref)
    for f in ("coverage", "matches", "mismatches"):
        assert np.array_equal(getattr(pile, f), getattr(pile_ref, f)), f
    # eight adapters, non-default options
    o = api.adapter_opts_default()
    for k, v in NONDEFAULT.items():
        setattr(o, k, v)
    eight = _eight()
    res8, _, rep8, _, _ = h.consensus_screen(b, adapters=api.AdapterSet.from_strings(eight), opts=o)
    _check_report(d, rep8, eight, NONDEFAULT)
    for z in range(b.n_zmw):
        _same(res8, ref, z)
    assert (rep8.n_hits > 16).any() and (rep.n_hits > 16).any()           # lists that are capped
    # planted adapters are found on the engine's drafts, controls and templates around another adapter give no hit (first 54: the built-in adapter)
    for z in tested:
        if z < 54 and kinds[z] in ("dimer", "near_end", "interior", "palindrome"):
            assert rep.n_hits[z] >= 1, (z, kinds[z])
        else:
            assert rep.n_hits[z] == 0, (z, kinds[z])
    # a bad request with a handle: an error of the call, and the handle still works
    q, keep = _request(api.AdapterReport.allocate(b.n_zmw + 1))
    assert _call("ccsx_submit_screen", h._h, b, api.Results.allocate(b), C.byref(q)) < 0
    _, _, rep3, _, _ = h.consensus_screen(b, adapters=one)
    for f in R.FIELDS:
        assert np.array_equal(getattr(rep3, f), getattr(rep, f)), f
    assert rep3.hits.tobytes() == rep.hits.tobytes()
    h.close()


def _made_of_adapters():
    """(batch, adapters): three templates of 200 copies of a random 80-base unit, the adapters eight 16-base windows of the unit (about 1600 hits each at one
    edit), and one of 150 hairpin adapters head to tail"""
    import adapter_synth as S
    rng = np.random.default_rng(17)
    U = rng.integers(0, 4, 80).astype(np.uint8)
    tpls = [np.tile(U, 200) for _ in range(3)] + [np.concatenate([HAIRPIN if q & 1 else R.revcomp(HAIRPIN) for q in range(150)])]
    return S.from_templates(tpls, [8] * len(tpls), rng), [np.tile(U, 2)[10 * q:10 * q + 16] for q in range(7)] + [HAIRPIN]


@pytest.mark.gpu
def test_a_draft_made_of_adapters(built):
    """more hits than k_adapter's LDS buffer holds (1024): the aggregates are over all of them and the list is the first 16 in (end, search) order.
    The oracle on the CPU gives status SUCCESS for the three tandem templates (the hairpin concatenation may fail its draft; it is compared when tested)"""
    b, ads = _made_of_adapters()
    h = api.Handle(0)
    d = h.draft(b)
    o = api.adapter_opts_default()
    o.max_dist_pct = 10
    _, _, rep, _, _ = h.consensus_screen(b, adapters=api.AdapterSet.from_strings(ads), opts=o)
    tested = _check_report(d, rep, ads, dict(max_dist_pct=10))
    assert len(tested) >= 3 and min(int(rep.n_hits[z]) for z in range(3)) > 1024, rep.n_hits
    assert (rep.n_listed[:3] == 16).all()
    h.close()


@pytest.mark.gpu
def test_two_stream_batch(built):
    """4608 ZMWs: the draft stage's POA runs as two half-batches on two streams"""
    import adapter_synth as S
    b, kk = S.make(4608, 5, (600, 1500), seed=71)
    h = api.Handle(0)
    d = h.draft(b)
    res, frep, rep, _, _ = h.consensus_screen(b, fold=True, adapters=api.AdapterSet.default())
    tested = _check_report(d, rep, [HAIRPIN])
    assert len(tested) > 3500
    ref = h.consensus(b)
    for k in ("status", "seq_len", "rq", "np_", "iters", "fn", "rn"):
        assert getattr(res, k).tobytes() == getattr(ref, k).tobytes(), k
    assert np.array_equal(res.seq, ref.seq) and np.array_equal(res.qual, ref.qual)
    _, frep_ref = h.consensus_fold(b)
    assert np.array_equal(frep.verdict, frep_ref.verdict) and np.array_equal(frep.span, frep_ref.span)
    h.close()


@pytest.mark.gpu
def test_submit_screen_equals_the_synchronous_call(built):
    import adapter_synth as S
    batches = [S.make(24, (5, 8), (800, 4000), seed=80 + k)[0] for k in range(5)]
    h = api.Handle(0)
    one = api.AdapterSet.default()
    want = [h.consensus_screen(b, fold=True, adapters=one) for b in batches]
    tickets, outs = [], []
    for k, b in enumerate(batches):                                # five tickets on three slots: three in flight
        res = api.Results.allocate(b, pinned=True)
        rep = api.AdapterReport.allocate(b.n_zmw, pinned=True)
        frep = api.FoldReport.allocate(b.n_zmw, pinned=True) if k != 1 else None
        tl = api.tandem_buffer(b.n_zmw, pinned=True) if k == 2 else None
        tickets.append(h.submit(b, res, fold=frep, tandem=tl, adapters=rep, adapter_set=one)); outs.append((res, rep, frep, tl))
    for t in tickets[2:]:
        h.wait(t)
    assert sum(int((w[2].verdict != 0).sum()) for w in want) > 10
    for (res, rep, frep, tl), (wres, wfrep, wrep, _, _), b in zip(outs, want, batches):
        for f in R.FIELDS:
            assert np.array_equal(getattr(rep, f), getattr(wrep, f)), f
        assert rep.hits.tobytes() == wrep.hits.tobytes()
        if frep is not None:
            for f in ("verdict", "fold", "hits", "span"):
                assert np.array_equal(getattr(frep, f), getattr(wfrep, f)), f
        for z in range(b.n_zmw):
            _same(res, wres, z)
    _, tl_want, _ = h.consensus_extras(batches[2], tandem=True)
    assert np.array_equal(outs[2][3], tl_want)
    # a slot that carried the request runs without it afterwards: plain submits, nothing of the screen left behind
    res = api.Results.allocate(batches[0], pinned=True)
    h.wait(h.submit(batches[0], res))
    for z in range(batches[0].n_zmw):
        _same(res, want[0][0], z)
    h.close()

"""Adapter palindromes (DESIGN.md §2 "Adapter palindromes"; docs/faq/fail-reads.md fail class 0x20): the restatement against a brute-force reading of the
rule, verdicts on planted palindromes and controls, the request's ABI and argument checks, and on an MI355X exact parity of k_fold with the restatement on
the engine's own drafts, no effect on any result, and tickets against the synchronous call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from ccs_amd import api
import fold_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(min_hits=2, min_arm=30, min_span_tenths=5, end_slack=40)


def _sampled_kmer(rng):
    """a random 15-mer whose canonical code is sampled"""
    while True:
        y = rng.integers(0, 4, R.K).astype(np.uint8)
        F, Rc = R.codes(y)
        if (R.fmix32(min(int(F[0]), int(Rc[0])))[0] & 7) == 0:
            return y


def _drafts(rng):
    """drafts of up to 3000 bases: edge lengths, random, planted folds with substitutions, asymmetric arms, low complexity, repeated sampled k-mers"""
    import fold_synth
    out = [rng.integers(0, 4, int(rng.integers(0, 40))).astype(np.uint8), rng.integers(0, 4, int(rng.integers(200, 3000))).astype(np.uint8)]
    for kind in ("palindrome", "asymmetric", "inverted", "tandem"):
        t, _ = fold_synth.template(rng, kind, int(rng.integers(300, 3000)))
        err = rng.random(len(t)) < 0.02
        t[err] = rng.integers(0, 4, int(err.sum()))
        out.append(t)
    y, t = _sampled_kmer(rng), rng.integers(0, 4, 2500).astype(np.uint8)
    for p in rng.choice(np.arange(0, 2400, 40), int(rng.integers(2, 14)), replace=False):
        t[p:p + R.K] = y if rng.random() < 0.5 else R.revcomp(y)
    out.append(t)
    out.append(np.concatenate([np.zeros(600, np.uint8), rng.integers(0, 4, 400).astype(np.uint8), np.tile(np.array([0, 3], np.uint8), 300)]))
    return out


# ---------------------------------------------------------------- CPU: the restatement
@pytest.mark.parametrize("seed", range(5))
def test_restatement_equals_the_bruteforce(seed):
    rng = np.random.default_rng(seed)
    for d in _drafts(rng):
        for o in (None, SMALL, dict(SMALL, max_occ=1), dict(SMALL, max_occ=3, end_slack=0)):
            assert R.fold(d, opts=o) == R.fold_bruteforce(d, opts=o), (len(d), o)


def test_ns_max_truncation(monkeypatch):
    """only the first NS_MAX sampled positions enter: with a small cap the restatement and the brute force agree, and the cap has bite"""
    import fold_synth
    rng = np.random.default_rng(3)
    t, _ = fold_synth.template(rng, "palindrome", 1500)
    full = R.fold(t, opts=SMALL)
    assert full[0] == R.PALINDROME
    for cap in (0, 1, 40, 100, 150, 400):
        monkeypatch.setattr(R, "NS_MAX", cap)
        assert R.fold(t, opts=SMALL) == R.fold_bruteforce(t, opts=SMALL), cap
    monkeypatch.setattr(R, "NS_MAX", 40)
    assert R.fold(t, opts=SMALL) == (R.NONE, -1, 0, 0)          # all 40 lie on the first arm: no hit


def test_occurrence_cap():
    """a code sampled c + 1 times (c copies of y, one rc(y)) gives c hits at max_occ = c + 1 and none at max_occ = c"""
    rng = np.random.default_rng(4)
    for c in (1, 3, 7):
        y = _sampled_kmer(rng)
        t = rng.integers(0, 4, 2000).astype(np.uint8)
        for q in range(c):
            t[100 + 60 * q:100 + 60 * q + R.K] = y
        t[1800:1800 + R.K] = R.revcomp(y)
        i, j = R.hits(t, c + 1)
        assert ((j == 1800) & np.isin(i, 100 + 60 * np.arange(c))).sum() == c
        i, j = R.hits(t, c)
        assert not (j == 1800).any()
        for mo in (c, c + 1):
            assert R.fold(t, opts=dict(SMALL, max_occ=mo)) == R.fold_bruteforce(t, opts=dict(SMALL, max_occ=mo))


@pytest.mark.parametrize("arm", [500, 1000, 2500, 5000, 10000])
def test_planted_palindromes_are_flagged(arm):
    import fold_synth
    rng = np.random.default_rng(arm)
    for err in ((0.0, 0.01) if arm >= 1000 else (0.0,)):          # (1 % substitutions can cost a 500-bp arm a fifth of its span: below 8 tenths)
        t, c = fold_synth.template(rng, "palindrome", 2 * arm + fold_synth.LOOP)
        e = rng.random(len(t)) < err
        t[e] = (t[e] + 1) & 3
        v, f, h, s = R.fold(t)
        assert v == R.PALINDROME and abs(f - c) <= 64 and h >= 12 and s >= 0.8 * arm, (arm, err, f, c, h, s)
        assert R.fold(R.revcomp(t))[0] == R.PALINDROME


def test_asymmetric_arms_are_flagged():
    import fold_synth
    rng = np.random.default_rng(7)
    for L in (1500, 3000, 6000, 12000):
        for _ in range(3):
            t, c = fold_synth.template(rng, "asymmetric", L)
            v, f, h, s = R.fold(t)
            assert v == R.PALINDROME and abs(f - c) <= 64, (L, f, c, h, s)


def test_controls_are_not_flagged():
    import fold_synth
    rng = np.random.default_rng(8)
    for kind in ("random", "inverted", "tandem"):
        for L in (2000, 5000, 10000):
            for _ in range(3):
                t, _ = fold_synth.template(rng, kind, L)
                assert R.fold(t)[0] == R.NONE, (kind, L, R.fold(t))
    assert R.fold(np.zeros(9000, np.uint8)) == (R.NONE, -1, 0, 0)   # a homopolymer: every position sampled, one code, dropped by the cap


# ---------------------------------------------------------------- CPU: ABI and argument checks
def test_structs_match_the_header(built, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ccsx.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d\\n", '
                   'sizeof(ccsx_fold_opts), offsetof(ccsx_fold_opts, min_hits), offsetof(ccsx_fold_opts, min_arm), offsetof(ccsx_fold_opts, min_span_tenths), '
                   'offsetof(ccsx_fold_opts, end_slack), sizeof(ccsx_fold_report), offsetof(ccsx_fold_report, verdict), offsetof(ccsx_fold_report, fold), '
                   'offsetof(ccsx_fold_report, hits), offsetof(ccsx_fold_report, span), sizeof(ccsx_fold_request), offsetof(ccsx_fold_request, report), '
                   'offsetof(ccsx_fold_request, reserved), sizeof(ccsx_extras), sizeof(ccsx_hd_request), CCSX_FOLD_PALINDROME, CCSX_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    O, Rp, Q = api.FoldOpts, api.CFoldReport, api.CFoldRequest
    assert got == [C.sizeof(O), O.min_hits.offset, O.min_arm.offset, O.min_span_tenths.offset, O.end_slack.offset, C.sizeof(Rp), Rp.verdict.offset,
                   Rp.fold.offset, Rp.hits.offset, Rp.span.offset, C.sizeof(Q), Q.report.offset, Q.reserved.offset, 24, 24, api.FOLD_PALINDROME, 6]
    assert got[0] == 20 and got[5] == 40 and got[10] == 24
    L = api.lib()
    assert L.ccsx_fold_rule_version() == 1 and L.ccsx_abi_version() == 6 and L.ccsx_spec_version() == 8
    o = api.fold_opts_default()
    assert dict(max_occ=o.max_occ, min_hits=o.min_hits, min_arm=o.min_arm, min_span_tenths=o.min_span_tenths, end_slack=o.end_slack) == R.DEFAULTS


def _request(rep, reserved=(0, 0), **kw):
    o = api.fold_opts_default()
    for k, v in kw.items():
        setattr(o, k, v)
    cr = rep.c_struct()
    return api.CFoldRequest(C.pointer(o), C.pointer(cr), (C.c_int32 * 2)(*reserved)), (o, cr)


def _call(entry, h, b, res, q):
    cb, cr = b.c_struct(), res.c_struct()
    t = C.c_int64()
    args = [h, C.byref(cb), C.byref(cr), None, q]
    return getattr(api.lib(), entry)(*(args + [C.byref(t)] if entry == "ccsx_submit_fold" else args))


BAD = {
    "null request or report": lambda rep, n: None,
    "reserved must be 0": lambda rep, n: _request(rep, reserved=(0, 1)),
    "options out of range": lambda rep, n: _request(rep, max_occ=65),
    "sized for another batch": lambda rep, n: _request(api.FoldReport.allocate(n + 1)),
}


@pytest.mark.parametrize("entry", ["ccsx_consensus_fold", "ccsx_submit_fold"])
def test_entry_points_refuse_bad_requests(built, entry):
    L = api.lib()
    b = api.synth(3, 4, 300, seed=2)
    res = api.Results.allocate(b)
    rep = api.FoldReport.allocate(b.n_zmw)
    for msg, make in BAD.items():
        q = make(rep, b.n_zmw)
        qq = C.byref(q[0]) if isinstance(q, tuple) else None
        assert _call(entry, None, b, res, qq) < 0 and msg.encode() in L.ccsx_last_error(), (msg, L.ccsx_last_error())
    assert _call(entry, None, b, res, C.byref(api.CFoldRequest(None, None, (C.c_int32 * 2)(0, 0)))) < 0
    assert b"null request or report" in L.ccsx_last_error()
    for kw in (dict(max_occ=0), dict(min_hits=0), dict(min_arm=0), dict(min_span_tenths=11), dict(min_span_tenths=-1), dict(end_slack=-1)):
        q, keep = _request(rep, **kw)
        assert _call(entry, None, b, res, C.byref(q)) < 0 and b"options out of range" in L.ccsx_last_error(), kw
    q, keep = _request(rep)                                        # a valid request: the handle is what is missing
    assert _call(entry, None, b, res, C.byref(q)) < 0 and b"null argument" in L.ccsx_last_error()


# ---------------------------------------------------------------- GPU
FIELDS = ("status", "seq_len", "rq", "np_", "ec", "iters", "n_windows", "fn", "rn")


def _same(a, b, z):
    for f in FIELDS:
        assert getattr(a, f)[z].tobytes() == getattr(b, f)[z].tobytes(), (z, f)
    assert np.array_equal(a.sequence(z), b.sequence(z)) and np.array_equal(a.quals(z), b.quals(z)), z
    assert np.array_equal(a.raw(z).view(np.uint32), b.raw(z).view(np.uint32)), z


def _mix(seed=61):
    """every fold_synth class, drafts long enough for two table passes (15 kb), homopolymer drafts with more than NS_MAX sampled positions, the two cap
    templates (the last two ZMWs), and before them the short drafts of scan_edges"""
    import fold_synth
    import scan_edges
    rng = np.random.default_rng(seed)
    poly = [np.concatenate([rng.integers(0, 4, 500).astype(np.uint8), np.zeros(9500, np.uint8), rng.integers(0, 4, 500).astype(np.uint8)]) for _ in range(4)]
    return api.concat([fold_synth.make(40, (5, 9), (1500, 6000), seed=seed)[0], fold_synth.make(10, 5, (14000, 16000), seed=seed + 1)[0],
                       _from_templates(poly, 6, seed), scan_edges.batch(), _from_templates(_cap_templates(), 8, seed + 2)])


CAP_Y = None


def _cap_templates():
    """a sampled 15-mer y planted c times plus rc(y) once: its code at exactly max_occ (c = 7, kept) and max_occ + 1 (c = 8, dropped) positions"""
    global CAP_Y
    rng = np.random.default_rng(5)
    CAP_Y = _sampled_kmer(rng)
    out = []
    for c in (7, 8):
        t = rng.integers(0, 4, 3000).astype(np.uint8)
        for q in range(c):
            t[200 + 80 * q:200 + 80 * q + R.K] = CAP_Y
        t[2600:2600 + R.K] = R.revcomp(CAP_Y)
        out.append(t)
    return out


def _code_count(d, y):
    s, F, Rc = R.sampled_positions(d)
    Fy, Ry = R.codes(y)
    return int((np.minimum(F, Rc) == min(int(Fy[0]), int(Ry[0]))).sum())


def _from_templates(tpls, passes, seed):
    import lowcx
    rng = np.random.default_rng(seed)
    zmw_id, snr, read_off, base_off, flags, bases, pws = [], [], [0], [0], [], [], []
    for z, t in enumerate(tpls):
        zmw_id.append(z); snr.append([9.0, 16.0, 8.0, 13.0])
        for q in range(passes):
            b, p = lowcx.sequence_read(rng, t)
            if q & 1:
                b, p = R.revcomp(b), p[::-1]
            bases.append(b); pws.append(p); flags.append(q & 1); base_off.append(base_off[-1] + len(b))
        read_off.append(read_off[-1] + passes)
    nb = base_off[-1]
    return api.Batch(np.array(zmw_id, np.int32), np.array(snr, np.float32), np.array(read_off, np.int32), np.array(base_off, np.int64),
                     np.concatenate(bases).astype(np.uint8), np.concatenate(pws).astype(np.uint8), rng.integers(1, 61, nb).astype(np.uint8),
                     np.array(flags, np.uint8), tpl_off=np.concatenate([[0], np.cumsum([len(t) for t in tpls])]).astype(np.int64),
                     tpl=np.concatenate(tpls).astype(np.uint8))


def _check_report(d, rep, o=None):
    """the report against fold_ref on the draft seam's drafts (the drafts k_polish is given), field for field; returns the tested ZMWs"""
    tested = 0
    for z in range(len(rep.verdict)):
        want = R.fold(d.draft(z), tested=d.status[z] == 0, opts=o)
        got = (int(rep.verdict[z]), int(rep.fold[z]), int(rep.hits[z]), int(rep.span[z]))
        assert got == want, (z, got, want, int(d.status[z]), len(d.draft(z)))
        tested += d.status[z] == 0
    return tested


@pytest.mark.gpu
def test_report_equals_the_restatement_and_results_do_not_change(built):
    import fold_synth
    import scan_edges
    b = _mix()
    h = api.Handle(0)
    d = h.draft(b)
    ref = h.consensus(b)
    res, rep = h.consensus_fold(b)
    assert _check_report(d, rep) > 40
    scan_edges.assert_every_class(len(d.draft(z)) for z in range(b.n_zmw) if d.status[z] == 0)
    assert max(len(R.sampled_positions(d.draft(z))[0]) for z in range(b.n_zmw) if d.status[z] == 0) == R.NS_MAX   # the cap was reached
    assert max(len(R.sampled_positions(d.draft(z))[0]) for z in range(40, 50) if d.status[z] == 0) > 1536            # several table passes
    for z in range(b.n_zmw):
        _same(res, ref, z)
    o = dict(max_occ=2, min_hits=3, min_arm=50, min_span_tenths=3, end_slack=0)
    fo = api.fold_opts_default()
    for k, v in o.items():
        setattr(fo, k, v)
    res2, rep2 = h.consensus_fold(b, fo)
    _check_report(d, rep2, o)
    # every planted palindrome is flagged, no control is
    kinds = np.concatenate([fold_synth.make(40, (5, 9), (1500, 6000), seed=61)[1], fold_synth.make(10, 5, (14000, 16000), seed=62)[1]])
    planted = np.isin(np.array(fold_synth.CLASSES)[kinds], fold_synth.PLANTED)
    assert (rep.verdict[:50][planted] == api.FOLD_PALINDROME).all(), rep.verdict[:50][planted]
    assert (rep.verdict[:50][~planted] != api.FOLD_PALINDROME).all()
    assert (rep.verdict[50:] != api.FOLD_PALINDROME).all()                  # the homopolymer drafts
    # the occurrence cap on the GPU: the planted code's sampled positions in each of the two drafts (n; a draft error can remove a copy), and runs at
    # max_occ = n (its hits kept) and n - 1 (dropped), the report equal to fold_ref in both
    cy = min(int(R.codes(CAP_Y)[0][0]), int(R.codes(CAP_Y)[1][0]))
    for z in (b.n_zmw - 2, b.n_zmw - 1):
        assert d.status[z] == 0
        n = _code_count(d.draft(z), CAP_Y)
        assert 6 <= n <= 9, n
        F, Rc = R.codes(d.draft(z))
        for mo in (n - 1, n):
            o9 = dict(max_occ=mo, min_hits=3, min_arm=50)
            assert bool((np.minimum(F, Rc)[R.hits(d.draft(z), mo)[1]] == cy).any()) == (mo == n), (z, mo)
            fo9 = api.fold_opts_default()
            fo9.max_occ, fo9.min_hits, fo9.min_arm = mo, 3, 50
            _, rep9 = h.consensus_fold(b, fo9)
            _check_report(d, rep9, o9)
    # a bad request with a handle: an error of the call, and the handle still works
    crep = api.FoldReport.allocate(b.n_zmw + 1).c_struct()
    q = api.CFoldRequest(None, C.pointer(crep), (C.c_int32 * 2)(0, 0))
    assert _call("ccsx_submit_fold", h._h, b, api.Results.allocate(b), C.byref(q)) < 0
    res3, rep3 = h.consensus_fold(b)
    assert np.array_equal(rep3.verdict, rep.verdict) and np.array_equal(rep3.span, rep.span)
    h.close()


@pytest.mark.gpu
def test_two_stream_batch(built):
    """4608 ZMWs: the draft stage's POA runs as two half-batches on two streams"""
    import fold_synth
    b, kinds, _ = fold_synth.make(4608, 5, (800, 1600), seed=71)
    h = api.Handle(0)
    d = h.draft(b)
    res, rep = h.consensus_fold(b)
    assert _check_report(d, rep) > 4000
    ref = h.consensus(b)
    for k in ("status", "seq_len", "rq", "np_", "iters", "fn", "rn"):
        assert getattr(res, k).tobytes() == getattr(ref, k).tobytes(), k
    assert np.array_equal(res.seq, ref.seq) and np.array_equal(res.qual, ref.qual)
    planted = np.isin(np.array(fold_synth.CLASSES)[kinds], fold_synth.PLANTED)
    assert (rep.verdict[~planted] != api.FOLD_PALINDROME).all()
    # the planted ZMWs whose true template the rule flags (short asymmetric arms fall below min_arm) and that are tested
    sure = np.array([planted[z] and d.status[z] == 0 and R.fold(b.tpl[b.tpl_off[z]:b.tpl_off[z + 1]])[0] == R.PALINDROME for z in range(b.n_zmw)])
    assert sure.sum() > 1500 and (rep.verdict[sure] == api.FOLD_PALINDROME).mean() > 0.95   # (0.964: draft errors cost a few short arms their span)
    h.close()


@pytest.mark.gpu
def test_submit_fold_equals_the_synchronous_call(built):
    import fold_synth
    batches = [fold_synth.make(20, (5, 8), (1500, 4000), seed=80 + k)[0] for k in range(5)]
    h = api.Handle(0)
    want = [h.consensus_fold(b) for b in batches]
    tickets, outs = [], []
    for k, b in enumerate(batches):                                # five tickets on three slots: three in flight
        res = api.Results.allocate(b, pinned=True)
        rep = api.FoldReport.allocate(b.n_zmw, pinned=True)
        tl = api.tandem_buffer(b.n_zmw, pinned=True) if k == 2 else None
        tickets.append(h.submit(b, res, fold=rep, tandem=tl)); outs.append((res, rep, tl))
    for t in tickets[2:]:
        h.wait(t)
    assert sum(int((w[1].verdict == api.FOLD_PALINDROME).sum()) for w in want) > 10
    for (res, rep, tl), (wres, wrep), b in zip(outs, want, batches):
        for f in ("verdict", "fold", "hits", "span"):
            assert np.array_equal(getattr(rep, f), getattr(wrep, f)), f
        for z in range(b.n_zmw):
            _same(res, wres, z)
    _, tl_want, _ = h.consensus_extras(batches[2], tandem=True)
    assert np.array_equal(outs[2][2], tl_want)
    h.close()

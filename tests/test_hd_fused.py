"""The heteroduplex finder in the fused, ticketed path (ccsx_consensus_hd / ccsx_submit_hd, include/ccsx.h): the request's ABI and argument checks, and on
an MI355X parity of its report with the third seam (ccsx_hd_batch on the draft seam's drafts), no effect on any result without the split, the split itself,
tickets against the synchronous call, the pipelined heteroduplex mode against api.consensus_hd, and a batch at scale."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from ccs_amd import api
import hd_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- CPU: ABI and argument checks
def test_request_struct_matches_the_header(built, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ccsx.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %d %d\\n", '
                   'sizeof(ccsx_hd_request), offsetof(ccsx_hd_request, opts), offsetof(ccsx_hd_request, report), offsetof(ccsx_hd_request, split), '
                   'offsetof(ccsx_hd_request, reserved), sizeof(ccsx_extras), CCSX_HETERODUPLEX, CCSX_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    R = api.CHdRequest
    assert got == [C.sizeof(R), R.opts.offset, R.report.offset, R.split.offset, R.reserved.offset, C.sizeof(api.CExtras), api.HETERODUPLEX, 6]
    assert got[5] == 24 and api.STATUS_NAMES[10] == "HETERODUPLEX"
    assert api.lib().ccsx_abi_version() == 6 and api.lib().ccsx_hd_rule_version() == 1


def _request(rep, **kw):
    o = api.hd_opts_default()
    for k, v in kw.pop("opts", {}).items():
        setattr(o, k, v)
    cr = rep.c_struct()
    q = api.CHdRequest(C.pointer(o), C.pointer(cr), kw.pop("split", 0), kw.pop("reserved", 0))
    return q, (o, cr)


@pytest.mark.parametrize("entry", ["ccsx_consensus_hd", "ccsx_submit_hd"])
def test_entry_points_refuse_bad_requests(built, entry):
    L = api.lib()
    import hd_synth
    b, _ = hd_synth.make(3, 3, 300, seed=2)
    res = api.Results.allocate(b)
    cb, cr = b.c_struct(), res.c_struct()
    t = C.c_int64()

    def call(h, q):
        args = [h, C.byref(cb), C.byref(cr), None, q]
        return getattr(L, entry)(*(args + [C.byref(t)] if entry == "ccsx_submit_hd" else args))

    rep = api.HdReport.allocate(b.n_zmw)
    bad = {
        "null request": None,
        "null request or report": C.byref(api.CHdRequest(None, None, 0, 0)),
        "reserved 0": _request(rep, reserved=1),
        "split must be 0 or 1": _request(rep, split=2),
        "options out of range": _request(rep, opts=dict(min_indel=22)),
        "sized for another batch": _request(api.HdReport.allocate(b.n_zmw + 1)),
    }
    for msg, q in bad.items():
        if isinstance(q, tuple):
            q = C.byref(q[0])
        assert call(None, q) < 0, msg
        assert msg.encode() in L.ccsx_last_error(), (msg, L.ccsx_last_error())
    q, keep = _request(rep, opts=dict(min_strand_passes=0))
    assert call(None, C.byref(q)) < 0 and b"options out of range" in L.ccsx_last_error()
    q, keep = _request(rep)                                           # a valid request: the handle is what is missing
    assert call(None, C.byref(q)) < 0 and b"null argument" in L.ccsx_last_error()
    if api.device_count() == 0:
        with pytest.raises(RuntimeError, match="no HIP device"):
            api.Handle(0)


# ---------------------------------------------------------------- GPU
def _mix():
    """an hd_synth mix (substitutions, a 30-bp insertion, controls, partial passes) + api.synth ZMWs"""
    import hd_synth
    return api.concat([hd_synth.make(24, 10, 1500, seed=51, k_sub=3)[0], hd_synth.make(16, 10, 1500, seed=52, indel=30)[0],
                       hd_synth.make(16, 6, 1500, seed=53, control=True)[0], hd_synth.make(16, (2, 12), (500, 2500), seed=54, k_sub=2, partial=True)[0],
                       api.synth(32, 10, 2000, seed=55)])


def _damaged():
    """damaged passes (foreign blocks, junk, truncations): ZMWs whose first draft fails and take the fallback or last-resort draft"""
    import corruption_fuzz
    return api.concat([corruption_fuzz.make_batch(k, 4242)[0] for k in range(8)])


def _same_report(a, b, what=""):
    assert np.array_equal(a.verdict, b.verdict), what
    for k in ("n_sub_sites", "n_indel_sites", "n_listed", "status"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), (what, k)
    assert np.array_equal(a.min_p.view(np.uint64), b.min_p.view(np.uint64)), what
    _same_sites(a.sites, b.sites, what)


def _same_sites(x, y, what=""):
    """every field of every site record, p bitwise (the four bytes of alignment padding before p are not a field: the kernels leave them undefined)"""
    for f in api.HD_SITE_DTYPE.names:
        u, v = np.ascontiguousarray(x[f]), np.ascontiguousarray(y[f])
        assert u.tobytes() == v.tobytes(), (what, f)


PER_ZMW = ("status", "seq_len", "rq", "np_", "ec", "iters", "n_windows", "fn", "rn")


def _same_zmw(a, b, z, pa=None, pb=None):
    """ZMW z of two Results (and pileups) byte for byte: every per-ZMW field and every per-base array up to seq_len (bytes beyond it are not results)"""
    for k in PER_ZMW:
        assert getattr(a, k)[z].tobytes() == getattr(b, k)[z].tobytes(), (z, k)
    assert np.array_equal(a.sequence(z), b.sequence(z)) and np.array_equal(a.quals(z), b.quals(z)), z
    assert np.array_equal(a.raw(z).view(np.uint32), b.raw(z).view(np.uint32)), z
    if a.kin is not None or b.kin is not None:
        assert np.array_equal(a.kinetics(z), b.kinetics(z)), z
    if pa is not None or pb is not None:
        for f in ("cov", "sm", "sx"):
            assert np.array_equal(getattr(pa, f)(z), getattr(pb, f)(z)), (z, f)


def _kin_handle():
    o = api.default_opts()
    o.hifi_kinetics = 1
    return api.Handle(0, opts=o)


@pytest.mark.gpu
def test_fused_report_equals_the_seam(built):
    h = api.Handle(0)
    for name, b in (("mix", _mix()), ("synth", api.synth(2048, 10, 3000, seed=56)), ("damaged", _damaged())):
        want = h.hd(b, h.draft(b))
        for split in (False, True):
            res, rep, _, _ = h.consensus_hd(b, split=split)
            _same_report(rep, want, (name, split))
        if name == "damaged":                                     # ZMWs whose final draft is a fallback / last-resort one: usable only with the cascade
            o = api.default_opts()
            o.no_fallback_draft = 1
            f = api.Handle(0, opts=o)
            d = f.draft(b)                                        # (kept: its arrays live in page-locked blocks the object owns)
            n_fallback = int(((want.status == 0) & (d.status != 0)).sum())
            f.close()
            assert n_fallback > 0
        elif name == "mix":
            assert (rep.verdict == api.HD_HETERODUPLEX).sum() >= 20
    h.close()


@pytest.mark.gpu
def test_detection_only_changes_nothing(built):
    import lowcx
    b = api.concat([_mix(), lowcx.make(24, 8, 1500, seed=57, tpl="lowcx")])
    h = _kin_handle()
    for thr in (0, 40):
        want, wt, wp = h.consensus_extras(b, tandem=True, min_tandem_repeat_length=thr, pileup=True)
        got, rep, gt, gp = h.consensus_hd(b, split=False, tandem=True, min_tandem_repeat_length=thr, pileup=True)
        assert np.array_equal(wt, gt), thr
        for z in range(b.n_zmw):
            _same_zmw(want, got, z, wp, gp)
        assert (rep.verdict == api.HD_HETERODUPLEX).sum() >= 20
    plain = h.consensus(b)
    got, rep, _, _ = h.consensus_hd(b)
    for z in range(b.n_zmw):
        _same_zmw(plain, got, z)
    h.close()


def _check_split(b, keep, split, rep):
    flagged = rep.verdict == api.HD_HETERODUPLEX
    for z in range(b.n_zmw):
        if not flagged[z]:
            continue
        assert int(split.status[z]) == api.HETERODUPLEX and split.seq_len[z] == 0 and split.n_windows[z] == 0 and split.iters[z] == 0, z
        assert split.fn[z] == keep.fn[z] and split.rn[z] == keep.rn[z] and split.np_[z] == keep.fn[z] + keep.rn[z], z
        assert split.rq[z] == 0 and split.ec[z] == 0, z
    return flagged


@pytest.mark.gpu
def test_split_keeps_heteroduplexes_out_of_the_polish_stage(built):
    b = _mix()
    h = _kin_handle()
    keep, rk, tk, pk = h.consensus_hd(b, split=False, tandem=True, pileup=True)
    split, rs, ts, ps = h.consensus_hd(b, split=True, tandem=True, pileup=True)
    _same_report(rk, rs)
    assert np.array_equal(tk, ts)
    flagged = _check_split(b, keep, split, rs)
    assert flagged.sum() >= 20 and (~flagged).sum() >= 40
    for z in np.flatnonzero(~flagged):
        _same_zmw(keep, split, z, pk, ps)
    assert (split.n_windows.sum() < keep.n_windows.sum())
    h.close()


@pytest.mark.gpu
def test_split_saves_the_polish_stage(built):
    """nearly every ZMW a heteroduplex (20 passes per strand, 4 substitutions): the split ticket's polish stage takes less than half the time"""
    import hd_synth
    b = hd_synth.make(512, 20, 2000, seed=58, k_sub=4)[0]
    h = api.Handle(0)
    ms = {}
    for run in range(2):                                          # (the first round warms up)
        for split in (False, True):
            res = api.Results.allocate(b, pinned=True)
            rep = api.HdReport.allocate(b.n_zmw, pinned=True)
            t = h.submit(b, res, hd=rep, hd_split=split) if split else h.submit(b, res)
            h.wait(t)
            ms[split] = h.ticket_timings(t).polish_ms
            h.release(t)
            if split:
                assert (rep.verdict == api.HD_HETERODUPLEX).mean() > 0.9 and (res.status == api.HETERODUPLEX).mean() > 0.9
    assert ms[True] < 0.5 * ms[False], ms
    h.close()


@pytest.mark.gpu
def test_split_with_several_polish_and_align16_launches(built, tmp_path):
    """the split does not depend on how the window slots or the quads are cut into launches (test hooks of the library)"""
    b = _mix()
    h = api.Handle(0)
    res, rep, _, _ = h.consensus_hd(b, split=True)
    h.close()
    out = tmp_path / "s.npz"
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r); import numpy as np; from ccs_amd import api\n"
            "import test_hd_fused as T; b = T._mix(); h = api.Handle(0); r, p, _, _ = h.consensus_hd(b, split=True)\n"
            "np.savez(%r, seq=r.seq, qual=r.qual, raw=r.raw_qv, status=r.status, seq_len=r.seq_len, rq=r.rq, np_=r.np_, ec=r.ec, iters=r.iters,\n"
            "         n_windows=r.n_windows, fn=r.fn, rn=r.rn, verdict=p.verdict, sites=p.sites.reshape(-1).view(np.uint8)); h.close()\n") % (
        ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools"), str(out))
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, CCSX_POLISH_MAX_BLOCKS="40", CCSX_ALIGN16_MAX_SLOTS="64"),
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    got = np.load(out)
    assert np.array_equal(got["verdict"], rep.verdict)
    _same_sites(got["sites"].view(api.HD_SITE_DTYPE).reshape(rep.sites.shape), rep.sites)
    for k in PER_ZMW:
        assert got[k].tobytes() == getattr(res, k).tobytes(), k
    for z in range(b.n_zmw):
        o, n = int(res.seq_off[z]), int(res.seq_len[z])
        for k, want in (("seq", res.seq), ("qual", res.qual), ("raw", res.raw_qv)):
            assert got[k][o:o + n].tobytes() == want[o:o + n].tobytes(), (z, k)


@pytest.mark.gpu
def test_tickets_equal_the_synchronous_calls(built):
    """HD, plain and extras tickets interleaved on one handle over more than three slots (a slot that ran an HD ticket is reused by a plain one), each
    against a fresh handle's synchronous call; ccsx_hd_batch still agrees afterwards"""
    import hd_synth
    import lowcx
    bs = [_mix(), hd_synth.make(24, 8, 1200, seed=61, k_sub=3)[0], lowcx.make(24, 8, 1200, seed=62, tpl="lowcx"),
          api.synth(40, 8, 1500, seed=63), hd_synth.make(24, 8, 1500, seed=64, indel=30)[0], _damaged(), api.synth(24, 6, 1000, seed=65)]
    jobs = [("hd", 0, dict(split=True)), ("hd", 1, dict(split=False, tandem=True, pileup=True)), ("extras", 2, dict(tandem=True, pileup=True)),
            ("plain", 3, {}), ("plain", 4, {}), ("hd", 5, dict(split=True, tandem=True)), ("hd", 4, dict(split=True, pileup=True)), ("plain", 6, {})]
    h = _kin_handle()
    tickets = []
    for kind, i, kw in jobs:
        b = bs[i]
        res = api.Results.allocate(b, kinetics=True, pinned=True)
        pile = api.Pileup.allocate(res, pinned=True) if kw.get("pileup") else None
        tl = api.tandem_buffer(b.n_zmw, pinned=True) if kw.get("tandem") else None
        rep = api.HdReport.allocate(b.n_zmw, pinned=True) if kind == "hd" else None
        t = h.submit(b, res, pileup=pile, tandem=tl, hd=rep, hd_split=kw.get("split", False))
        tickets.append((t, res, pile, tl, rep))
    for t, *_ in tickets[-3:]:                                    # (the earlier tickets were retired by the submits that reused their slots)
        h.wait(t)
    for (kind, i, kw), (t, res, pile, tl, rep) in zip(jobs, tickets):
        b = bs[i]
        f = _kin_handle()
        if kind == "hd":
            want, wrep, wt, wp = f.consensus_hd(b, split=kw["split"], tandem=kw.get("tandem", False), pileup=kw.get("pileup", False))
            _same_report(rep, wrep, (kind, i))
        elif kind == "extras":
            want, wt, wp = f.consensus_extras(b, tandem=True, pileup=True)
        else:
            want, wt, wp = f.consensus(b), None, None
        if tl is not None:
            assert np.array_equal(tl, wt), (kind, i)
        for z in range(b.n_zmw):
            _same_zmw(want, res, z, wp, pile)
        f.close()
    seam = h.hd(bs[0], h.draft(bs[0]))
    _same_report(seam, tickets[0][4])
    h.close()


@pytest.mark.gpu
def test_stream_equals_consensus_hd(built):
    import hd_synth
    bs = [_mix(), hd_synth.make(20, 10, 1500, seed=71, k_sub=4)[0], api.synth(48, 8, 1500, seed=72),
          hd_synth.make(20, 10, 1500, seed=73, indel=-30)[0], hd_synth.make(12, 6, 1000, seed=74, control=True)[0]]
    h = api.Handle(0)
    got = list(api.consensus_hd_stream(h, bs))
    assert len(got) == len(bs)
    n_het = 0
    for b, (recs, rep) in zip(bs, got):
        want, wrep = api.consensus_hd(h, b)
        _same_report(rep, wrep)
        n_het += int((rep.verdict == api.HD_HETERODUPLEX).sum())
        assert len(recs) == len(want)
        for x, y in zip(recs, want):
            assert (x.zmw, x.zmw_id, x.group, x.status, x.np_) == (y.zmw, y.zmw_id, y.group, y.status, y.np_)
            assert np.array_equal(x.seq, y.seq) and np.array_equal(x.qual, y.qual) and np.float32(x.rq).tobytes() == np.float32(y.rq).tobytes()
    assert n_het >= 40
    h.close()


@pytest.mark.gpu
def test_fused_hd_at_scale(built):
    b = api.synth(16384, 10, 10000, seed=41)
    h = api.Handle(0)
    d = h.draft(b)
    res, rep, _, _ = h.consensus_hd(b)
    assert (rep.verdict == api.HD_DOUBLE_STRAND).mean() > 0.95
    ref = hd_ref.hd_zmws(hd_ref.collect_stage(h, b, rep.status, d.backbone, range(512)))
    assert [int(v) for v in rep.verdict[:512]] == [r["verdict"] for r in ref]
    assert [int(v) for v in rep.n_sub_sites[:512]] == [r["n_sub"] for r in ref]
    h.close()

"""k_train (ccsx_train_batch) against the host statement of the same rule (ccsx_train_pair_host, train_core.h) — integer EQUALITY on the pairs the engine's own stage
outputs report (arrow_ref.collect_stage) — and against the float64 restatement of tests/train_ref.py within the bound of tests/test_train_ref.py, summed over a
ZMW's pairs.  The lab batch of tests/test_arrow_gpu.py plants the shapes the kernel has limits for; what the run counted is ASSERTED from the stage outputs.

Trimming and n_pairs.  With the default max_insertion_size a segment of n > J + 30 bases is left out.  With -1 nothing is trimmed, but a segment of more than 63 bases
is not eligible either way, and an eligible one may still fail the gate.  So the counted-plus-gated pairs fall by exactly the trimmed segments of at most 63 bases,
and n_pairs by exactly those of them the host rule counts: that is what test_default_trimming_leaves_segments_out asserts (the lab has trimmed segments of 64 and more bases, which no setting
counts)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from ccs_amd import api
import arrow_ref as A
import train_ref as T
import test_arrow_gpu as G

pytestmark = pytest.mark.gpu
FRAC, STEP = 2.0 ** 32, 2.0 ** -33
PLANES = [k for k, _, _ in api.TrainCounts.PLANES]


def _opts(maxins=0, min_zscore=0.0):
    o = api.default_opts(); o.disable_heuristics = 1; o.min_rq = 0.0; o.min_zscore = min_zscore; o.top_passes = 0; o.max_insertion_size = maxins
    return o


def _same(a, b, zs_a=None, zs_b=None, planes=PLANES):
    zs_a = range(a.n_zmw) if zs_a is None else zs_a; zs_b = zs_a if zs_b is None else zs_b
    for k in planes:
        assert np.array_equal(getattr(a, k)[list(zs_a)], getattr(b, k)[list(zs_b)]), k


def host_counts(model, o, batch, wins, zs):
    """The host rule on the pairs collect_stage reports.  Returns (TrainCounts with the rows of `zs` filled, info): info[z] = the counted pairs as
    (pair for train_ref, window columns ce - cs, n, J, strand), plus the eligible pairs that were trimmed away at this setting (n <= 63) as `trimmed63`."""
    tc = api.TrainCounts.allocate(batch)
    maxins = 30 if o.max_insertion_size == 0 else o.max_insertion_size
    info = {}
    for z in zs:
        counted, trimmed63 = [], 0
        for w in wins[z]:
            J = len(w["tpl"])
            for r, n, rev in zip(w["reads"], w["n_raw"], w["strands"]):
                if n < 0 or n > A.IMAX: continue
                if maxins > 0 and n > J + maxins: trimmed63 += 1; continue
                assert r is not None and len(r) == n
                to, lfo, cs, ce = T.oriented(w["tpl"], w["lf"], w["rf"], w["cs"], w["ce"], rev)
                rc = api.train_pair_host(model, batch.snr[z], to, lfo, cs, ce, r, min_zscore=float(o.min_zscore),
                                         out=(tc.match[z], tc.stay[z], tc.del_[z], tc.loglik[z:z + 1]))[0]
                assert rc >= 0
                if rc == 1:
                    tc.n_pairs[z] += 1; tc.n_bases[z] += n
                    counted.append((T.make_pair(to, lfo, cs, ce, r, z), ce - cs, n, J, rev))
                else: tc.n_gated[z] += 1
        info[z] = dict(counted=counted, trimmed63=trimmed63)
    return tc, info


def check_float64(model, batch, tc, info, zs):
    """a ZMW's tables inside the float64 bound, summed over its counted pairs; sum match + sum del = the core columns of those pairs"""
    pairs = [c[0] for z in zs for c in info[z]["counted"]]
    if not pairs: return
    tabs = [A.tables64(model, batch.snr[z]) for z in range(batch.n_zmw)]
    ref = T.e_step(tabs, pairs)
    zi = np.array([p["z"] for p in pairs])
    for z in zs:
        q = zi == z
        if not q.any(): continue
        for h, r, c in ((tc.match[z], ref["match"][q].sum(0), ref["cells_m"][q].sum(0)), (tc.stay[z], ref["stay"][q].sum(0), ref["cells_s"][q].sum(0)),
                        (tc.del_[z], ref["dele"][q].sum(0), ref["cells_d"][q].sum(0))):
            err = np.abs(h / FRAC - r); bound = 3 * A.LIK_TOL * r + c * STEP
            assert np.all(err <= bound), (z, float(err.max()))
        cols = sum(c[1] for c in info[z]["counted"])
        cells = int(ref["cells_m"][q].sum() + ref["cells_d"][q].sum())
        tot = (int(tc.match[z].sum()) + int(tc.del_[z].sum())) / FRAC
        assert abs(tot - cols) <= 3 * A.LIK_TOL * cols + cells * STEP, (z, tot, cols)


@pytest.fixture(scope="module")
def lab(built):
    """the lab batch counted at max_insertion_size -1 and at the default, each with the host rule on the engine's own pairs"""
    model = api.default_model()
    batch, tpls = G.lab_batch(model)
    out = dict(model=model, batch=batch, tpls=tpls)
    for maxins in (-1, 0):
        o = _opts(maxins)
        h = api.Handle(0, model=model, opts=o)
        try:
            d = api.Drafts.allocate(batch)
            for z, t in enumerate(tpls): d.set_draft(z, t, backbone=0)
            tc = h.train_counts(batch, d)
            again = h.train_counts(batch, d)                  # the same batch twice on one handle
            wins = A.collect_stage(h, batch, range(batch.n_zmw), max_insertion_size=maxins)
        finally:
            h.close()
        host, info = host_counts(model, o, batch, wins, range(batch.n_zmw))
        out[maxins] = dict(o=o, d=d, tc=tc, again=again, wins=wins, host=host, info=info)
    return out


@pytest.mark.parametrize("maxins", [-1, 0])
def test_lab_parity(lab, maxins):
    R, batch, model = lab[maxins], lab["batch"], lab["model"]
    tc, host, info = R["tc"], R["host"], R["info"]
    assert np.all(tc.status == 0)
    print(f"\n[train gpu lab] max_insertion_size {maxins}: pairs {tc.n_pairs.tolist()} gated {tc.n_gated.tolist()} bases {tc.n_bases.tolist()}")
    _same(tc, host, planes=PLANES[:-1])                      # integer equality: every table, loglik, n_pairs, n_gated, n_bases
    _same(tc, R["again"])
    check_float64(model, batch, tc, info, range(batch.n_zmw))
    # what the run counted
    cnt = [c for z in info for c in info[z]["counted"]]
    assert max(c[3] for c in cnt) == 30
    assert any(abs(c[2] - c[3]) >= 8 for c in cnt) and any(c[3] - c[2] >= 8 for c in cnt)
    if maxins < 0:
        assert any(c[2] == 63 and c[3] == 30 for c in cnt), "no counted pair with n = 63 in a 30-column window"
        assert any(abs(c[2] - c[3]) >= 26 for c in cnt), "no counted pair with |n - J| >= 26"
    npz = np.diff(batch.read_off)
    assert any(npz[z] > 64 and tc.n_pairs[z] > 64 * len(R["wins"][z]) for z in info), "no ZMW of more than 64 counted passes"
    assert any(len(info[z]["counted"]) >= 3 and all(c[4] for c in info[z]["counted"]) for z in info), "no ZMW whose counted passes are all reverse"
    out_of_range = [z for z in info if batch.snr[z].max() < model.snr_lo or batch.snr[z].min() > model.snr_hi]
    assert len(out_of_range) >= 2 and all(tc.n_pairs[z] > 0 for z in out_of_range)
    assert all(w["lf"] == 4 for z in R["wins"] for w in R["wins"][z][:1])


def test_default_trimming_leaves_segments_out(lab):
    off, on = lab[-1], lab[0]
    trimmed = sum(w["trimmed"] for z in on["wins"] for w in on["wins"][z])
    trimmed63 = sum(on["info"][z]["trimmed63"] for z in on["info"])
    over63 = sum(1 for z in on["wins"] for w in on["wins"][z] for n in w["n_raw"] if n > A.IMAX)
    assert trimmed > 0 and trimmed63 > 0 and trimmed == trimmed63 + over63         # (every segment of 64 and more bases of the lab is beyond J + 30)
    assert sum(w["trimmed"] for z in off["wins"] for w in off["wins"][z]) == 0
    elig = lambda R: int(R["tc"].n_pairs.sum() + R["tc"].n_gated.sum())
    assert elig(off) - elig(on) == trimmed63
    # of the trimmed segments of at most 63 bases, the ones the rule counts at -1: exactly the fall of n_pairs
    lost = 0
    for z in off["info"]:
        for c in off["info"][z]["counted"]:
            lost += c[2] > c[3] + 30
    assert lost > 0 and int(off["tc"].n_pairs.sum() - on["tc"].n_pairs.sum()) == lost


def _cat(parts):
    """the ZMWs of several batches as one batch, in order (batches without truth templates: api.concat wants those)"""
    ro, bo = [np.zeros(1, np.int32)], [np.zeros(1, np.int64)]
    for b in parts:
        ro.append(b.read_off[1:] + ro[-1][-1]); bo.append(b.base_off[1:] + bo[-1][-1])
    cat = lambda k: np.ascontiguousarray(np.concatenate([getattr(b, k) for b in parts]))
    n = sum(b.n_zmw for b in parts)
    return api.Batch(np.arange(n, dtype=np.int32), cat("snr"), np.concatenate(ro).astype(np.int32), np.concatenate(bo).astype(np.int64),
                     cat("bases"), cat("pw"), cat("ipd"), cat("flags"))


def _embed(tc, z0, n):
    full = api.TrainCounts.allocate(n)
    for k in PLANES: getattr(full, k)[z0:z0 + tc.n_zmw] = getattr(tc, k)
    return full


def test_invariance_order_and_slices(lab):
    batch, tpls, model = lab["batch"], lab["tpls"], lab["model"]
    n = batch.n_zmw
    h = api.Handle(0, model=model, opts=_opts(-1))
    try:
        def run(b, ts):
            d = api.Drafts.allocate(b)
            for z, t in enumerate(ts): d.set_draft(z, t, backbone=0)
            return h.train_counts(b, d)
        rev = run(_cat([batch.slice(z, z + 1) for z in range(n - 1, -1, -1)]), tpls[::-1])
        _same(lab[-1]["tc"], rev, range(n), range(n - 1, -1, -1))
        a, b = run(batch.slice(0, 2), tpls[:2]), run(batch.slice(2, n), tpls[2:])
        both = _embed(a, 0, n).add(_embed(b, 2, n))
        _same(lab[-1]["tc"], both, planes=PLANES[:-1])
        assert np.array_equal(both.status[2:], b.status)
    finally:
        h.close()


@pytest.fixture(scope="module")
def engine(built):
    """api.synth(32, 10, 2000) counted on the fused consensus as drafts (the backbone of the draft call), default options"""
    batch = api.synth(32, 10, 2000, seed=12)
    h = api.Handle(0)
    try:
        d0 = h.draft(batch)
        res = h.consensus(batch)
        d = api.Drafts.allocate(batch)
        for z in range(batch.n_zmw):
            if res.status[z] == 0: d.set_draft(z, res.sequence(z), backbone=int(d0.backbone[z]))
        d.len[5] = 0                                          # one ZMW is handed no draft
        tc = h.train_counts(batch, d)
        zs = [z for z in range(batch.n_zmw) if tc.status[z] == 0][:4]
        wins = A.collect_stage(h, batch, zs, max_insertion_size=h.opts.max_insertion_size)
        for z in zs: assert np.array_equal(h.stage_draft(z), d.draft(z))
        model, o = h.model, h.opts
    finally:
        h.close()
    return dict(batch=batch, d=d, tc=tc, zs=zs, wins=wins, model=model, o=o, res=res)


def test_engine_drafts(engine):
    E = engine
    tc, batch = E["tc"], E["batch"]
    assert E["o"].min_zscore != 0.0                          # the default options: the z-score gate is on
    host, info = host_counts(E["model"], E["o"], batch, E["wins"], E["zs"])
    _same(tc, host, E["zs"], planes=PLANES[:-1])            # bit-exact against the host rule, z-score gate included
    check_float64(E["model"], batch, tc, info, E["zs"][:2])
    ok = tc.status == 0
    assert ok.sum() >= 28 and np.all(tc.n_pairs[ok] > 600) and np.all(tc.n_bases[ok] > 15000)
    ll = tc.loglik[ok].sum() / 65536.0 / tc.n_bases[ok].sum()
    assert -4.0 < ll < -1.0, ll
    # a ZMW handed an empty draft: a status, and zeros
    assert tc.status[5] != 0
    for k in PLANES[:-1]: assert not getattr(tc, k)[5].any(), k
    for z in np.flatnonzero(~ok):
        for k in PLANES[:-1]: assert not getattr(tc, k)[z].any(), (z, k)


_CHILD = """
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
from ccs_amd import api
d = np.load(sys.argv[2])
batch = api.synth(32, 10, 2000, seed=12)
dr = api.Drafts.allocate(batch)
dr.seq[...] = d["seq"]; dr.len[...] = d["len"]; dr.backbone[...] = d["backbone"]
h = api.Handle(0)
tc = h.train_counts(batch, dr)
h.close()
assert "CCSX_POLISH_MAX_BLOCKS=16" in api.lib().ccsx_runtime_switches().decode()
np.savez(sys.argv[3], **{k: getattr(tc, k) for k, _, _ in api.TrainCounts.PLANES})
"""


def test_launch_pieces_do_not_change_a_bit(engine, tmp_path):
    """k_train is launched in the polish stage's pieces: a child process with CCSX_POLISH_MAX_BLOCKS=16 (16 workgroups = 128 windows per launch; the batch has about
    3000) returns the same bytes"""
    d = engine["d"]
    src, dst = str(tmp_path / "drafts.npz"), str(tmp_path / "counts.npz")
    np.savez(src, seq=d.seq, len=d.len, backbone=d.backbone)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CCSX_POLISH_MAX_BLOCKS="16")
    r = subprocess.run([sys.executable, "-c", _CHILD, root, src, dst], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(dst)
    assert sum(len(engine["wins"][z]) for z in engine["zs"]) > 0 and int(engine["tc"].n_pairs.sum()) > 128 * 10
    for k in PLANES: assert np.array_equal(got[k], getattr(engine["tc"], k)), k


def test_zscore_gate(lab):
    """the z-score gate of the polish (opts.min_zscore) gates training pairs too: on the lab batch, whose passes are not samples of the model, it turns counted pairs
    into gated ones, eligible pairs stay what they were, and the device still equals the host rule"""
    batch, tpls, model = lab["batch"], lab["tpls"], lab["model"]
    o = _opts(-1, min_zscore=-3.4)
    h = api.Handle(0, model=model, opts=o)
    try:
        d = api.Drafts.allocate(batch)
        for z, t in enumerate(tpls): d.set_draft(z, t, backbone=0)
        tc = h.train_counts(batch, d)
    finally:
        h.close()
    host, _ = host_counts(model, o, batch, lab[-1]["wins"], range(batch.n_zmw))
    _same(tc, host, planes=PLANES[:-1])
    off = lab[-1]["tc"]
    assert np.array_equal(tc.n_pairs + tc.n_gated, off.n_pairs + off.n_gated)
    assert np.all(tc.n_gated >= off.n_gated) and tc.n_gated.sum() > off.n_gated.sum()


def test_slot_hygiene(built):
    b = api.synth(8, 6, 1200, seed=31)
    h, fresh = api.Handle(0), api.Handle(0)
    try:
        before = h.consensus(b)
        d = h.draft(b)
        tc = h.train_counts(b, d)
        h._keep = b                                          # (Handle.download sizes its buffers from the last uploaded batch)
        for call in (h.run, h.download):
            with pytest.raises(RuntimeError, match="ccsx_upload"):
                call()
        assert len(h.stage_windows(0)) >= 2 and np.array_equal(h.stage_draft(0), d.draft(0))
        after, ref = h.consensus(b), fresh.consensus(b)
        for r in (after, ref):
            for k in ("status", "seq_len", "rq", "np_", "ec", "fn", "rn"):
                assert np.array_equal(getattr(before, k), getattr(r, k)), k
            for z in range(b.n_zmw):
                assert np.array_equal(before.sequence(z), r.sequence(z)) and np.array_equal(before.quals(z), r.quals(z)), z
                assert np.array_equal(before.raw(z).view(np.uint32), r.raw(z).view(np.uint32)), z
        assert (tc.status == 0).sum() >= 6 and tc.n_pairs.sum() > 0
        h.upload(b); h.run(); h.sync()
        assert np.array_equal(h.download().status, before.status)
        # errors of the call: nothing is enqueued, the handle stays usable
        cb, cd = b.c_struct(), d.c_struct()
        bad = api.TrainCounts.allocate(b).c_struct(); bad.reserved = 1
        small = api.TrainCounts.allocate(b.n_zmw - 1).c_struct()
        import ctypes as C
        L = api.lib()
        assert L.ccsx_train_batch(h._h, C.byref(cb), C.byref(cd), C.byref(bad)) < 0 and b"reserved" in L.ccsx_last_error()
        assert L.ccsx_train_batch(h._h, C.byref(cb), C.byref(cd), C.byref(small)) < 0
        assert L.ccsx_train_batch(h._h, C.byref(cb), None, C.byref(small)) < 0 and L.ccsx_train_batch(h._h, C.byref(cb), C.byref(cd), None) < 0
        _same(h.train_counts(b, d), tc)
    finally:
        h.close(); fresh.close()

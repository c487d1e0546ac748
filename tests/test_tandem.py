"""Tandem-repeat detection (sDUST) and the per-ZMW heuristics switch (DESIGN.md §2 "Tandem repeats"; docs/faq/low-complexity.md:8-18):
the restatement against the written definition, the ccsx_extras ABI, and on an MI355X exact parity of k_sdust with the restatement and the
per-ZMW invariant: a flagged ZMW gets exactly what opts.disable_heuristics gives it, every other ZMW exactly the default."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from ccs_amd import api
import sdust_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def enc(s):
    return np.array(["ACGT".index(c) for c in s], np.uint8)


# ---------------------------------------------------------------- CPU: the restatement
@pytest.mark.parametrize("seed", range(8))
def test_incremental_equals_the_definition(seed):
    """every window and every sub-interval of it, from the written definition, against the incremental form (and its 64-lane split)"""
    rng = np.random.default_rng(seed)
    L = int(rng.integers(120, 300))
    x = rng.integers(0, 4, L).astype(np.uint8)
    for _ in range(int(rng.integers(0, 4))):                     # plant short low-complexity stretches, some with errors
        u = rng.integers(0, 4, int(rng.integers(1, 7))).astype(np.uint8)
        n = int(rng.integers(8, 90))
        p = int(rng.integers(0, L - 8))
        rep = np.tile(u, n // len(u) + 1)[:min(n, L - p)]
        err = rng.random(len(rep)) < 0.05
        rep[err] = rng.integers(0, 4, int(err.sum()))
        x[p:p + len(rep)] = rep
    want = R.masked_bruteforce(x)
    assert np.array_equal(R.masked_incremental(x), want)
    assert np.array_equal(R.masked_lanes(x), want)
    assert np.array_equal(R.masked_lanes(x, lanes=7), want)


def test_short_and_edge_lengths():
    for L in range(0, 70):
        x = np.zeros(L, np.uint8)                                # homopolymer: masked as soon as an interval scores > 2
        assert np.array_equal(R.masked_incremental(x), R.masked_bruteforce(x)), L
        assert R.tandem_len(x) == (L if L >= 7 else 0), L      # 5 triplets: 10 pairs over 4 > 2; 4 triplets: 6 / 3 = 2 is not
    assert R.tandem_len(np.zeros(2, np.uint8)) == 0 and R.tandem_len(np.zeros(0, np.uint8)) == 0


def test_low_complexity_runs_are_masked():
    assert R.tandem_len(enc("A" * 200)) == 200
    assert R.tandem_len(enc("AC" * 100)) == 200
    assert R.tandem_len(enc("AGGGGT" * 50)) == 300
    assert R.tandem_len(enc("ACGTTG" * 40)) == 240


def test_random_sequence_is_not():
    rng = np.random.default_rng(5)
    for _ in range(4):
        x = rng.integers(0, 4, 3000).astype(np.uint8)
        assert R.tandem_len(x) < 40


def test_exact_interval_in_random_flanks():
    left = enc("GATCCTAGTCAGGTACCGTATGCAAC")
    right = enc("TGACCATGGTCAATCGGAGCTTAC")
    x = np.concatenate([left, enc("AGGGGT" * 20), right])
    m = R.masked_incremental(x)
    assert np.array_equal(m, R.masked_bruteforce(x))
    idx = np.flatnonzero(m)
    # exactly the tract: the flanks share no triplet with the unit's six rotations near the edges
    assert idx.min() == len(left) and idx.max() == len(left) + 120 - 1 and len(idx) == 120
    assert R.tandem_len(x) == 120


def test_reverse_complement_gives_the_same_answer():
    rng = np.random.default_rng(9)
    for k in range(6):
        x = rng.integers(0, 4, 800).astype(np.uint8)
        p = int(rng.integers(0, 500))
        u = rng.integers(0, 4, 2 + k % 3).astype(np.uint8)
        x[p:p + 250] = np.tile(u, 250)[:250]
        m, mr = R.masked_incremental(x), R.masked_incremental(R.revcomp(x))
        assert np.array_equal(m, mr[::-1])
        assert R.tandem_len(x) == R.tandem_len(R.revcomp(x)) >= 250


def test_extras_struct_and_versions(built, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ccsx.h"\nint main(void){printf("%zu %zu %zu %zu\\n", sizeof(ccsx_extras), '
                   'offsetof(ccsx_extras, tandem_len), offsetof(ccsx_extras, min_tandem_repeat_length), offsetof(ccsx_extras, reserved));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(api.CExtras), api.CExtras.tandem_len.offset, api.CExtras.min_tandem_repeat_length.offset, api.CExtras.reserved.offset]
    L = api.lib()
    assert L.ccsx_tandem_rule_version() == 1 and L.ccsx_spec_version() == 8 and L.ccsx_abi_version() == 6


def test_extras_entry_points_fail_loudly_without_a_handle(built):
    L = api.lib()
    b = api.synth(2, 4, 300, seed=1)
    res = api.Results.allocate(b)
    tl = np.zeros(2, np.int32)
    cb, cr = b.c_struct(), res.c_struct()
    ex = api._extras(None, tl, 100)
    assert L.ccsx_consensus_extras(None, C.byref(cb), C.byref(cr), C.byref(ex)) < 0 and b"null argument" in L.ccsx_last_error()
    t = C.c_int64()
    assert L.ccsx_submit_extras(None, C.byref(cb), C.byref(cr), C.byref(ex), C.byref(t)) < 0 and b"null argument" in L.ccsx_last_error()
    if api.device_count() == 0:
        with pytest.raises(RuntimeError):
            api.Handle(0)


# ---------------------------------------------------------------- GPU
FIELDS = ("status", "seq_len", "rq", "np_", "ec", "iters", "n_windows", "fn", "rn")


def _same(a, b, z, batch_kin=False):
    for f in FIELDS:
        assert getattr(a, f)[z] == getattr(b, f)[z], (z, f)
    assert np.array_equal(a.sequence(z), b.sequence(z)), z
    assert np.array_equal(a.quals(z), b.quals(z)), z
    assert np.array_equal(a.raw(z).view(np.uint32), b.raw(z).view(np.uint32)), z
    if batch_kin:
        assert np.array_equal(a.kinetics(z), b.kinetics(z)), z


def _opts(**kw):
    o = api.default_opts()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _expected_len(draft, o):
    return R.tandem_len(draft) if o.min_length <= len(draft) <= o.max_length and len(draft) > 0 else 0


@pytest.mark.gpu
def test_tandem_len_matches_the_restatement(built):
    import lowcx
    import tandem_synth
    o = _opts(no_fallback_draft=1)
    h = api.Handle(0, opts=o)
    sets = {
        "random": api.synth(24, 6, 1200, seed=3),
        "lowcx": lowcx.make(24, 8, 1500, seed=64, tpl="lowcx"),
        "tract": tandem_synth.make(24, 8, (1500, 3000), seed=11, frac=0.7, tract=(300, 1500))[0],
        "short": lowcx.make(16, 8, (12, 62), seed=5, tpl="lowcx"),         # drafts shorter than the window
        "empty": api.synth(12, (1, 2), 300, seed=8),                        # too few passes: no draft
    }
    seen_flag = 0
    for name, b in sets.items():
        res, tl, _ = h.consensus_extras(b, tandem=True)
        for z in range(b.n_zmw):
            d = h.stage_draft(z)
            assert tl[z] == _expected_len(d, o), (name, z, len(d), tl[z])
            seen_flag += tl[z] >= 100
    assert seen_flag > 10
    h.close()


def _invariant(b, thr, kin=False, **kw):
    hd = api.Handle(0, opts=_opts(hifi_kinetics=int(kin), **kw))
    hx = api.Handle(0, opts=_opts(hifi_kinetics=int(kin), disable_heuristics=1, **kw))
    ref_d, ref_x = hd.consensus(b), hx.consensus(b)
    res, tl, _ = hd.consensus_extras(b, tandem=True, min_tandem_repeat_length=thr)
    flagged = tl >= thr
    for z in range(b.n_zmw):
        _same(res, ref_x if flagged[z] else ref_d, z, kin)
    hd.close(); hx.close()
    return res, tl, flagged, ref_d, ref_x


@pytest.mark.gpu
def test_flagged_zmws_equal_disable_heuristics_the_others_the_default(built):
    import tandem_synth
    b, tracts = tandem_synth.make(48, (6, 12), (2500, 5000), seed=21, frac=0.5, tract=(400, 2000))
    res, tl, flagged, ref_d, ref_x = _invariant(b, 600, kin=True)
    assert 0 < flagged.sum() < b.n_zmw
    assert (flagged <= (tracts > 0)).all()                       # no control is flagged
    differ = sum(not np.array_equal(ref_d.sequence(z), ref_x.sequence(z)) or ref_d.status[z] != ref_x.status[z] for z in range(b.n_zmw))
    assert differ > 0                                            # (the two handles do differ on this data: the test can tell them apart)


@pytest.mark.gpu
def test_detection_alone_and_no_extras_change_nothing(built):
    import tandem_synth
    b, _ = tandem_synth.make(32, 8, (2000, 4000), seed=23, frac=0.5, tract=(500, 1500))
    h = api.Handle(0)
    ref = h.consensus(b)
    res, tl, _ = h.consensus_extras(b, tandem=True, min_tandem_repeat_length=0)   # report only
    assert (tl >= 500).sum() > 0
    for z in range(b.n_zmw):
        _same(res, ref, z)
    res2 = api.Results.allocate(b)
    cb, cr = b.c_struct(), res2.c_struct()
    assert api.lib().ccsx_consensus_extras(h._h, C.byref(cb), C.byref(cr), None) == 0                # NULL extras = ccsx_consensus_batch
    empty = api._extras(None, None, 0)
    res3 = api.Results.allocate(b)
    cr3 = res3.c_struct()
    assert api.lib().ccsx_consensus_extras(h._h, C.byref(cb), C.byref(cr3), C.byref(empty)) == 0     # everything off: the same
    r4 = api.Results.allocate(b, pinned=True)
    h.wait(h.submit(b, r4))
    for z in range(b.n_zmw):
        _same(res2, ref, z); _same(res3, ref, z); _same(r4, ref, z)
    bad = api._extras(None, None, -1)
    assert api.lib().ccsx_consensus_extras(h._h, C.byref(cb), C.byref(cr3), C.byref(bad)) < 0
    h.close()


@pytest.mark.gpu
def test_submit_extras_equals_the_synchronous_call(built):
    import tandem_synth
    batches = [tandem_synth.make(16, 6 + k, (1500, 3000), seed=40 + k, frac=0.5, tract=(300, 1200))[0] for k in range(5)]
    h = api.Handle(0)
    want = [h.consensus_extras(b, tandem=True, min_tandem_repeat_length=400, pileup=(k == 3)) for k, b in enumerate(batches)]
    tickets, outs = [], []
    for k, b in enumerate(batches):                                # five tickets on three slots: tickets 0 and 1 are retired by slot reuse
        res = api.Results.allocate(b, pinned=True)
        tl = api.tandem_buffer(b.n_zmw, pinned=True)
        pl = api.Pileup.allocate(res, pinned=True) if k == 3 else None
        tickets.append(h.submit(b, res, pileup=pl, tandem=tl, min_tandem_repeat_length=400)); outs.append((res, tl, pl))
    for t in tickets[2:]:
        h.wait(t)
    assert sum(int((w[1] >= 400).sum()) for w in want) > 0
    for (res, tl, pl), (wres, wtl, wpl), b in zip(outs, want, batches):
        assert np.array_equal(tl, wtl)
        for z in range(b.n_zmw):
            _same(res, wres, z)
            if pl is not None:
                assert np.array_equal(pl.cov(z), wpl.cov(z)) and np.array_equal(pl.sm(z), wpl.sm(z))
    # detection only, with the threshold off, through a ticket
    res = api.Results.allocate(batches[0], pinned=True)
    tl = api.tandem_buffer(batches[0].n_zmw, pinned=True)
    h.wait(h.submit(batches[0], res, tandem=tl))
    assert np.array_equal(tl, want[0][1])
    h.close()


@pytest.mark.gpu
def test_tandem_at_scale_flags_nothing_on_random_data(built):
    b = api.synth(16384, 10, 10000, seed=41)
    h = api.Handle(0)
    ref = h.consensus(b)
    res, tl, _ = h.consensus_extras(b, tandem=True, min_tandem_repeat_length=1000)
    assert (tl < 1000).all() and tl.max() > 0
    assert np.array_equal(res.status, ref.status) and np.array_equal(res.seq_len, ref.seq_len)
    assert np.array_equal(res.seq, ref.seq) and np.array_equal(res.qual, ref.qual) and np.array_equal(res.rq, ref.rq)
    assert np.array_equal(res.np_, ref.np_) and np.array_equal(res.iters, ref.iters)
    h.close()

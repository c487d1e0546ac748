"""Pass orientation (DESIGN.md §2 "Pass orientation") on the CPU: the restatement of tests/orient_ref.py against its brute-force reading on the lab and on random
small batches, the lab's ZMWs against what their names promise, anchors by hand, the ABI against the header, the argument errors ccsx_orient_batch finds
without a device, and the end-to-end inputs of tests/test_orient_gpu.py: the reference alone orients every one of their flagged passes correctly."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from ccs_amd import api
import orient_lab as LAB
import orient_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, U = R.K, R.UNKNOWN
KEYS = R.FIELDS + ("flags", "anchor")


def _equal(a, b, what):
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), (what, k, np.flatnonzero(np.asarray(a[k]) != np.asarray(b[k]))[:8])


@pytest.fixture(scope="module")
def lab(built):
    b, names = LAB.batch()
    return b, names, R.orient(b)


def test_lab_restatement_equals_the_bruteforce(lab):
    b, names, rep = lab
    _equal(rep, R.orient_bruteforce(b), "lab")
    loose = dict(min_votes=1, ratio=2)
    _equal(R.orient(b, loose), R.orient_bruteforce(b, loose), "lab, loose")


def test_lab_zmws_sit_on_their_limits(lab):
    b, names, rep = lab
    mv, ra = R.DEFAULTS["min_votes"], R.DEFAULTS["ratio"]
    NT = LAB.kernel_constants()["THREADS"]
    assert len(names) == b.n_zmw == len(set(names))

    def rows(name):
        z = names.index(name)
        r0, r1 = int(b.read_off[z]), int(b.read_off[z + 1])
        return [tuple(int(rep[k][r]) for k in R.FIELDS) + (int(rep["flags"][r]),) for r in range(r0, r1)], int(rep["anchor"][z]), b.flags[r0:r1]

    assert not (rep["flags"] & U).any() and np.array_equal(rep["flags"] & 1, rep["strand"]) and np.array_equal(rep["flags"] & 6, b.flags & 6)
    rw, a, fl = rows("12 / 13 / 14 bases, anchor of 13")
    assert a == 0 and [x[:4] for x in rw] == [(0, R.ANCHOR, 0, 0), (0, R.UNDETERMINED, 0, 0), (1, R.UNDETERMINED, 1, 0), (0, R.UNDETERMINED, 0, 1)]
    rw, a, fl = rows("N - K + 1 = threads - 1, threads, threads + 1")
    assert a == 0 and [x[:4] for x in rw[1:]] == [(1, R.OPPOSITE, 0, NT + d) for d in (-1, 0, 1)] + [(0, R.SAME, NT + d, 0) for d in (-1, 0, 1)]
    assert [x[4] for x in rw[1:]] == [3, 3, 3, 6, 6, 6]                  # bits 1 and 2 stay
    assert rows("one pass")[0] == [(1, R.ANCHOR, 0, 0, 1)]
    rw, a, fl = rows("255 passes of 64 bases")
    assert len(rw) == 255 and {x[1] for x in rw} == {R.ANCHOR, R.SAME, R.OPPOSITE} and all(x[2] + x[3] == 52 for x in rw if x[1] != R.ANCHOR)
    rw, a, fl = rows("only partial passes")
    assert a == -1 and [x[:4] for x in rw] == [(0, R.NO_ANCHOR, 0, 0), (1, R.NO_ANCHOR, 0, 0)] and [x[4] for x in rw] == [2, 7]
    rw, a, fl = rows("partial passes behind full ones")
    assert a == 0 and [x[:2] for x in rw] == [(1, R.GIVEN), (0, R.OPPOSITE), (1, R.SAME), (0, R.OPPOSITE), (1, R.SAME)] and [x[4] for x in rw] == [1, 0, 1, 2, 7]
    rw, a, fl = rows("median tie")
    assert a == 1 and [x[:2] for x in rw] == [(1, R.SAME), (1, R.ANCHOR), (0, R.OPPOSITE), (0, R.OPPOSITE)]
    rw, a, fl = rows("homopolymer anchor")
    assert a == 0 and [x[:4] for x in rw] == [(0, R.ANCHOR, 0, 0), (1, R.OPPOSITE, 0, 2988), (0, R.SAME, 2978, 0), (0, R.UNDETERMINED, 0, 0)]
    rw, a, fl = rows("v_same = min_votes, min_votes - 1")
    assert a == 0 and [x[:4] for x in rw[2:]] == [(1, R.SAME, mv, 0), (0, R.UNDETERMINED, mv - 1, 0), (0, R.OPPOSITE, 0, mv), (1, R.UNDETERMINED, 0, mv - 1)]
    rw, a, fl = rows("v_same = ratio x v_opp, one less")
    x = max(2, (mv + ra - 1) // ra)
    assert a == 0 and [x_[:4] for x_ in rw[2:]] == [(0, R.SAME, ra * x, x), (1, R.UNDETERMINED, ra * x - 1, x), (1, R.OPPOSITE, x, ra * x), (0, R.UNDETERMINED, x, ra * x - 1)]
    for name in ("(AT)n", "(ACGT)n", "X rc(X)", "junk anchor"):
        rw, a, fl = rows(name)
        assert all(x[1] == R.UNDETERMINED and x[0] == int(f) & 1 for q, (x, f) in enumerate(zip(rw, fl)) if q != a and int(f) & U), name
        assert {int(f) & 1 for q, f in enumerate(fl) if q != a and int(f) & U} == {0, 1}, name       # both values of the caller's bit
        assert name == "junk anchor" or all(x[2] >= mv and x[3] >= mv for q, x in enumerate(rw) if q != a and x[1] != R.GIVEN), name
    rw, a, fl = rows("base bytes with high bits")
    assert [x[:2] for x in rw] == [(1, R.ANCHOR), (0, R.OPPOSITE), (1, R.SAME), (0, R.OPPOSITE)]
    rw, a, fl = rows("GIVEN and unknown passes mixed")
    assert a == 0 and [x[:2] for x in rw] == [(1, R.GIVEN), (1, R.SAME), (1, R.GIVEN), (0, R.OPPOSITE), (0, R.GIVEN), (0, R.OPPOSITE)]
    rw, a, fl = rows("prefilter and first-probe collision")
    assert a == 0 and [x[2:4] for x in rw] == [(0, 0), (0, 0), (0, 0), (1, 0), (0, 1)]
    c = LAB.kernel_constants()
    h = LAB.fmix32(np.array(LAB.colliding_codes()))
    assert h[0] != h[1] and h[0] >> np.uint64(c["FILTER_SHIFT"]) == h[1] >> np.uint64(c["FILTER_SHIFT"]) and (h[0] ^ h[1]) & np.uint64(c["MIN_SLOTS"] - 1) == 0
    rw, a, fl = rows("two passes of 65535 bases")
    assert a == 0 and rw[1][1] == R.OPPOSITE and rw[1][3] > 40000 and rw[1][2] < 200    # (chance hits: 65523 positions x 65523 codes / 4^13 = 64 expected)


def _random_batch(rng):
    Z = []
    for _ in range(int(rng.integers(1, 5))):
        t = rng.integers(0, 4, int(rng.integers(10, 90))).astype(np.uint8)
        if rng.random() < 0.2:
            t = np.tile(t[:int(rng.integers(1, 5))], 30)[:len(t)]        # a tandem repeat: votes both ways
        nfull, npart = int(rng.integers(0, 6)), int(rng.integers(0, 3))
        passes = []
        for q in range(nfull + npart):
            s = t.copy()
            for _ in range(int(rng.integers(0, 3))):
                s[int(rng.integers(0, len(s)))] = rng.integers(0, 4)
            s = s[int(rng.integers(0, 4)):len(s) - int(rng.integers(0, 4))]
            if rng.random() < 0.5:
                s = R.revcomp(s)
            f = int(rng.integers(0, 2)) | (U if rng.random() < 0.7 else 0) | (2 | (4 if rng.random() < 0.5 else 0) if q >= nfull else 0)
            passes.append(((s | np.uint8(rng.integers(0, 64) << 2)).astype(np.uint8), f))
        if passes:
            Z.append(passes)
    return LAB.make_batch(Z) if Z else None


def test_random_small_batches(built):
    rng = np.random.default_rng(123)
    calls = set()
    done = 0
    while done < 200:
        b = _random_batch(rng)
        if b is None:
            continue
        o = dict(min_votes=int(rng.integers(1, 8)), ratio=int(rng.integers(2, 5)))
        got = R.orient(b, o)
        _equal(got, R.orient_bruteforce(b, o), done)
        calls |= set(got["call"].tolist())
        done += 1
    assert calls == set(range(6))


def test_anchor_median_and_ties():
    A = R.anchor
    assert A([10], [0]) == 0 and A([], []) == -1 and A([10, 20], [2, 2]) == -1
    assert A([10, 30], [0, 0]) == 1                                      # n = 2: element 1 of the sorted lengths
    assert A([30, 10], [0, 0]) == 0
    assert A([10, 20, 30, 40], [0, 0, 0, 0]) == 2                        # n = 4: element 2
    assert A([40, 30, 20, 10, 50], [8, 8, 8, 8, 8]) == 1                 # n = 5: element 2 = 30
    assert A([300, 310, 300, 310], [0] * 4) == 1 and A([310, 300, 310, 300], [0] * 4) == 0      # equal lengths: the first
    assert A([100, 500, 110, 90], [0, 0, 2, 2]) == 1                     # partial passes do not count: n = 2
    assert A([100, 90, 95], [0, 0, 0]) == 2 and A([100, 90, 95, 1000], [0, 0, 0, 6]) == 2


def test_structs_match_the_header(built, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ccsx.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d %d %d %d %d %d\\n", '
                   'sizeof(ccsx_orient_opts), offsetof(ccsx_orient_opts, ratio), sizeof(ccsx_orient_report), offsetof(ccsx_orient_report, strand), '
                   'offsetof(ccsx_orient_report, call), offsetof(ccsx_orient_report, votes_same), offsetof(ccsx_orient_report, votes_opp), sizeof(ccsx_requests), '
                   'CCSX_PASS_STRAND_UNKNOWN, CCSX_ORIENT_GIVEN, CCSX_ORIENT_ANCHOR, CCSX_ORIENT_SAME, CCSX_ORIENT_OPPOSITE, CCSX_ORIENT_UNDETERMINED, '
                   'CCSX_ORIENT_NO_ANCHOR, CCSX_ABI_VERSION, CCSX_SPEC_VERSION);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    O, Rp = api.OrientOpts, api.COrientReport
    assert got == [C.sizeof(O), O.ratio.offset, C.sizeof(Rp), Rp.strand.offset, Rp.call.offset, Rp.votes_same.offset, Rp.votes_opp.offset, C.sizeof(api.CRequests),
                   api.PASS_STRAND_UNKNOWN, api.ORIENT_GIVEN, api.ORIENT_ANCHOR, api.ORIENT_SAME, api.ORIENT_OPPOSITE, api.ORIENT_UNDETERMINED, api.ORIENT_NO_ANCHOR, 6, 8]
    assert got[:3] == [8, 4, 40] and got[7] == 64 and got[8] == 8 == R.UNKNOWN
    assert (R.GIVEN, R.ANCHOR, R.SAME, R.OPPOSITE, R.UNDETERMINED, R.NO_ANCHOR) == tuple(got[9:15]) and R.FIELDS == api.OrientReport.FIELDS
    L = api.lib()
    assert L.ccsx_orient_rule_version() == 1 and L.ccsx_abi_version() == 6 and L.ccsx_spec_version() == 8
    o = api.orient_opts_default()
    assert {k: getattr(o, k) for k in R.DEFAULTS} == R.DEFAULTS
    c = LAB.kernel_constants()
    assert c["K"] == R.K == 13 and c["THREADS"] == 256 and c["MIN_SLOTS"] & (c["MIN_SLOTS"] - 1) == 0


def test_with_unknown_strands(built):
    b = api.synth(3, 4, 200, seed=4)
    u = b.with_unknown_strands()
    assert np.array_equal(u.flags, b.flags | 8) and u.bases is b.bases and not (b.flags & 8).any()
    g = np.arange(len(b.flags)) % 2
    u = b.with_unknown_strands(g)
    assert np.array_equal(u.flags & 1, g) and np.array_equal(u.flags & 0xfe, (b.flags & 0xfe) | 8)


def test_orient_batch_refuses_bad_arguments(built):
    L = api.lib()
    b = api.synth(3, 4, 300, seed=2)
    cb = b.c_struct()
    R_ = int(b.read_off[-1])

    def call(rep, opts=None, batch=cb):
        cr = rep.c_struct() if rep is not None else None
        return L.ccsx_orient_batch(None, C.byref(batch) if batch is not None else None, C.byref(opts) if opts is not None else None, C.byref(cr) if cr is not None else None)

    good = api.OrientReport.allocate(R_)
    assert call(None) < 0 and b"null report" in L.ccsx_last_error()
    assert call(api.OrientReport.allocate(R_ + 1)) < 0 and b"sized for another batch" in L.ccsx_last_error()
    cr = good.c_struct()
    cr.votes_opp = None
    assert L.ccsx_orient_batch(None, C.byref(cb), None, C.byref(cr)) < 0 and b"report arrays missing" in L.ccsx_last_error()
    for kw in (dict(min_votes=0), dict(min_votes=-3), dict(ratio=1), dict(ratio=17), dict(ratio=0)):
        o = api.orient_opts_default()
        for k, v in kw.items():
            setattr(o, k, v)
        assert call(good, o) < 0 and b"orient options out of range" in L.ccsx_last_error(), kw
    for o in (None, api.OrientOpts(1, 2), api.OrientOpts(1 << 20, 16)):          # valid: the handle is what is missing
        assert call(good, o) < 0 and b"null argument" in L.ccsx_last_error()
    assert L.ccsx_set_orient_opts(None, None) < 0 and b"null handle" in L.ccsx_last_error()
    assert L.ccsx_stage_orient(None, None) < 0 and b"null report" in L.ccsx_last_error()
    cr = good.c_struct()
    assert L.ccsx_stage_orient(None, C.byref(cr)) < 0 and b"no batch uploaded" in L.ccsx_last_error()


def test_reference_orients_the_end_to_end_inputs(built):
    """what tests/test_orient_gpu.py feeds the engine: every flagged pass but the anchors is SAME or OPPOSITE, and the resolved bits give every pair of passes of a
    ZMW the relative orientation of the true flags (the anchor's own bit is the caller's random one: the ZMW's frame, which reaches no result)"""
    true, unk = LAB.end_to_end()
    assert not LAB.relative_strands_equal(true, true.flags, unk.flags).all()                # the random bits are wrong somewhere
    rep = R.orient(unk)
    assert set(rep["call"].tolist()) == {R.ANCHOR, R.SAME, R.OPPOSITE} and (rep["call"] == R.ANCHOR).sum() == true.n_zmw
    assert LAB.relative_strands_equal(true, true.flags, rep["flags"]).all() and not (rep["flags"] & U).any()

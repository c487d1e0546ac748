"""The HiFi-kinetics planes (k_kinetics_t<1, 1> and <1, 0>; DESIGN.md §2 "HiFi kinetics") and the record's scalars (k_stitch, k_post; "QVs (A6), stitch")
against tests/kinetics_ref.py on the engine's own stages: every plane byte for byte, every scalar exactly, on the planted batches of tests/kinetics_lab.py.
Every test asserts, from the reference's census of the stage outputs, that the limit it is about occurred, and prints that census.

rq is the one inexact comparison.  The reference rebuilds p from the float32 raw_qv in float64; measured on the CPU over the oracle's results for these batches
(tests/test_kinetics_ref.py::test_rq_deviation_on_the_gpu_batches) 1 - rq deviates by at most 1.358e-3 of itself, so |rq - rq_ref| <= 4 x 1.36e-3 x (1 - rq_ref)
+ one float32 ulp of rq (kinetics_lab.rq_bound).  A ZMW whose rq_ref lies within that bound of min_rq is left out of the LOW_RQ / SUCCESS check alone; the LOW_RQ
test asserts that it leaves none out.

Not reached: CAPACITY and EMPTY_WINDOW (no honest input makes the polished consensus outgrow 1.25 x the longest pass + 64, or empties every core), and the
bytes beyond seq_len (the whole device planes are copied into the caller's arrays, so nothing of a caller's sentinel stays)."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import kinetics_lab as Lab
import kinetics_ref as K
from ccs_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu
FAILED_BEFORE = (1, 2, 3, 5, 6)          # TOO_FEW_PASSES, DRAFT_FAILURE, TOO_MANY_UNUSABLE, TOO_SHORT, TOO_LONG: the statuses a ZMW has before the polish


class Run:
    """one synchronous ccsx_consensus_pileup run with its stages, the reference's alignment of them and its census"""

    def __init__(self, h, b):
        self.h, self.b = h, b
        self.res, self.pile = h.consensus_pileup(b)
        self.zmws, self.wmeta, self.backbone = K.collect(h, b)
        self.segs = K.aligned_segments(self.zmws)
        self.census = K.census(self.zmws, self.segs)
        self.sums = K.kinetics_sums(self.zmws, self.segs)
        self.kin = K.codes_of(self.zmws, self.sums)

    def compare(self):
        """every plane and every scalar of every ZMW; returns the ZMWs left out of the LOW_RQ / SUCCESS check"""
        res, b, left_out = self.res, self.b, []
        self.ref = {}
        for z, zm in enumerate(self.zmws):
            o, cap = int(res.seq_off[z]), int(res.seq_off[z + 1] - res.seq_off[z])
            if not zm.tpls:                                              # failed before the polish
                got = (int(res.seq_len[z]), int(res.n_windows[z]), int(res.iters[z]), float(res.rq[z]), float(res.ec[z]))
                assert got == (0, 0, 0, 0.0, 0.0) and int(res.status[z]) in FAILED_BEFORE and res.kinetics(z).shape == (4, 0), (z, got, int(res.status[z]))
                continue
            r = self.ref[z] = K.stitch_zmw(zm.tpls, zm.cores, self.wmeta[z], res.raw_qv[o:o + cap], self.h.opts)
            assert int(res.seq_len[z]) == r["seq_len"] and np.array_equal(res.sequence(z), r["seq"]) and np.array_equal(res.quals(z), r["qual"]), z
            got = (int(res.n_windows[z]), int(res.iters[z]), int(res.np_[z]), (int(res.fn[z]), int(res.rn[z])))
            assert got == (r["n_windows"], r["iters"], r["np"], K.strand_counts(zm)), (z, got, r)
            assert res.ec.dtype == np.float32 and res.ec[z] == r["ec"], (z, res.ec[z], r["ec"])
            bound = Lab.rq_bound(r["rq_ref"])
            print(f"zmw {z}: rq {float(res.rq[z]):.9f} rq_ref {r['rq_ref']:.9f} bound {bound:.3e}")
            assert abs(float(res.rq[z]) - r["rq_ref"]) <= bound, (z, float(res.rq[z]), r["rq_ref"], bound)
            if r["status"] in (K.LOW_RQ, K.SUCCESS) and abs(r["rq_ref"] - float(self.h.opts.min_rq)) <= bound:
                left_out.append(z)
                assert int(res.status[z]) in (K.LOW_RQ, K.SUCCESS), z
            else:
                assert int(res.status[z]) == r["status"], (z, int(res.status[z]), r["status"])
            assert np.array_equal(res.kinetics(z), self.kin[z]), (z, np.argwhere(res.kinetics(z) != self.kin[z])[:5].tolist())
        return left_out

    def plain_run_is_identical(self):
        """ccsx_consensus_batch on the same handle runs k_kinetics_t<1, 0>: the same bytes"""
        assert Lab.result_bytes(self.h.consensus(self.b)) == Lab.result_bytes(self.res)


_handles, _runs = {}, {}


def handle(**kw):
    key = tuple(sorted(kw.items()))
    if key not in _handles:
        _handles[key] = api.Handle(0, opts=Lab.kin_opts(**kw))
    return _handles[key]


def run(name) -> Run:
    """the named batch under its options, run and compared once per session"""
    if name not in _runs:
        b = Lab.many_windows()[0] if name == "many_windows" else Lab.BATCHES[name]()
        r = Run(handle(**Lab.OPTS.get(name, {})), b)
        print(name, "census", dict(r.census))
        r.left_out = r.compare()
        _runs[name] = r
    return _runs[name]


@pytest.fixture(scope="module", autouse=True)
def _close(built):
    yield
    for h in _handles.values():
        h.close()
    _handles.clear(); _runs.clear()


# ---------------------------------------------------------------- segment lengths
@gpu
def test_segment_length_limits():
    r = run("segment_limits")
    c = r.census
    assert (r.res.status == 0).all() and c["zmws"] == 8
    assert min(c["n=0"], c["n=31"], c["n=32"], c["n=63"]) >= 1, c                       # usable: the empty segment, the last paired, the first unpaired, the last row
    assert c["n=64"] >= 1 and c["n>64"] >= 1, c                                           # unusable
    assert c["lone_half_wave"] >= 1 and c["paired_and_unpaired"] >= 1, c                  # an odd number of short segments; a group with both kinds of task
    r.plain_run_is_identical()


# ---------------------------------------------------------------- groups of 32 passes
@gpu
def test_passes_beyond_the_second_group_count():
    r = run("groups70")
    z = r.zmws[0]
    assert r.res.status[0] == 0 and len(z.reads) == 70 and r.census["passes_above_64"] == 6 and r.census["opposite_segments"] > 100, r.census
    for k in (32, 64):                                                                    # the planes of the first k passes alone are other planes
        part = K.codes_of(r.zmws, K.kinetics_sums(r.zmws, r.segs, keep=lambda zi, p, k=k: p < k))[0]
        assert not np.array_equal(part, r.kin[0]) and (part != r.kin[0]).mean() > 0.05, k
    r.plain_run_is_identical()


@gpu
def test_255_passes_of_code_255_do_not_wrap():
    r = run("groups255")
    s = np.concatenate([sw[:, :, cs:ce] for sw, (cs, ce) in zip(r.sums[0], r.zmws[0].cores)], axis=2)
    assert r.res.status[0] == 0 and len(r.zmws[0].reads) == 255 and r.census["opposite_segments"] == 0
    full = np.flatnonzero(s[0, 2] == 255)
    print("columns of 255 agreeing passes:", len(full), "of", s.shape[2])
    assert len(full) >= 1 and (s[0, 0, full] == 255 * 952).all() and (s[0, 1, full] == 255 * 952).all()
    fi, fp, ri, rp = r.res.kinetics(0)
    assert (fi[s[0, 2] > 0] == 255).all() and (fp[s[0, 2] > 0] == 255).all() and not ri.any() and not rp.any()


# ---------------------------------------------------------------- the strand reference
@gpu
def test_strand_reference_and_partial_passes():
    r = run("strand_reference")
    b, res = r.b, r.res
    assert [int(s) for s in res.status] == [0, 0, 0, 0, 3, 0, 0] and not r.left_out
    assert r.backbone[0] == 0 and r.zmws[0].ref_strand == 1                               # pass 0 on the reverse strand
    assert r.backbone[1] != 0 and r.backbone[2] != 0 and r.zmws[1].ref_strand == 1        # the fallback draft's backbone: a reverse pass while pass 0 is forward
    assert int(b.flags[int(b.read_off[1])]) & 1 == 0
    # ZMW 3: the partial passes feed the planes and ec, not np / fn / rn
    z3 = r.zmws[3]
    partial = [p for p, rd in enumerate(z3.reads) if rd[1] & 2]
    assert partial == [8, 9] and all(z3.reads[p][2] for p in partial) and r.census["partial_cells"] > 100
    without = K.codes_of([z3], K.kinetics_sums([z3], [s._replace(zi=0) for s in r.segs if s.zi == 3], keep=lambda zi, p: p < 8))[0]
    assert not np.array_equal(without, r.kin[3])
    assert res.np_[3] == 8 == res.fn[3] + res.rn[3] and res.ec[3] > 8.5
    # ZMW 6: fn + rn counts the aligned passes, np the passes most windows used
    assert res.np_[6] < res.fn[6] + res.rn[6] == 10, (res.np_[6], res.fn[6], res.rn[6])
    r.plain_run_is_identical()


@gpu
def test_base_coded_kinetics_follow_the_strand():
    """ipd = 10 + 10 base, pw = 1 + 2 (base & 1): only agreeing bases are averaged, so the forward planes carry the code of SEQ's base and the reverse planes
    that of its complement, whatever the backbone (no reference needed: a swap of planes or strands shows at once)"""
    seen = 0
    for name in ("strand_reference", "segment_limits"):
        b = Lab.BATCHES[name]()
        b.ipd = (10 + 10 * b.bases).astype(np.uint8)
        b.pw = (1 + (b.bases & 1) * 2).astype(np.uint8)
        for res in (handle().consensus_pileup(b)[0], handle().consensus(b)):
            for z in range(b.n_zmw):
                if res.seq_len[z] == 0:
                    continue
                s, (fi, fp, ri, rp) = res.sequence(z).astype(int), res.kinetics(z).astype(int)
                f, v = fi > 0, ri > 0
                assert (fi[f] == 10 + 10 * s[f]).all() and (fp[f] == 1 + (s[f] & 1) * 2).all(), (name, z)
                assert (ri[v] == 10 + 10 * (3 - s[v])).all() and (rp[v] == 1 + ((3 - s[v]) & 1) * 2).all(), (name, z)
                assert not fp[~f].any() and not rp[~v].any() and f.mean() > 0.9, (name, z)
                seen += int(v.mean() > 0.9)
    assert seen >= 20                                                                     # ZMWs with both planes filled, over the two kinds of run


# ---------------------------------------------------------------- core edges
@gpu
def test_core_edges():
    c = run("segment_limits").census + run("strand_reference").census
    print("census", dict(c))
    assert c["diag_on_overhang"] > 1000 and c["core_mismatch"] > 20, c                  # cells that do not count: outside the core, bases that differ
    assert min(c["seam_insertion"], c["del_first_core_col"], c["del_last_core_col"]) >= 3, c
    nominal = sum(1 for name in ("segment_limits", "strand_reference") for z in run(name).zmws for cs, ce in z.cores if ce - cs == 22)
    assert c["core_not_19"] >= 1 and 0 < nominal < c["windows"], (c, nominal)           # cores of the window rule's 22 bases and others (moved bounds, last windows)


# ---------------------------------------------------------------- launch pieces
@gpu
def test_launch_pieces():
    """CCSX_POLISH_MAX_BLOCKS (read once per process) cuts the window slots into launches of 16: the same planes and results"""
    r = run("segment_limits")
    print("census", dict(r.census))
    assert r.census["windows"] > 4 * 16
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "kinetics_child.py"), "segment_limits"], env=dict(os.environ, CCSX_POLISH_MAX_BLOCKS="16"),
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    sha = [line.split() for line in out.stdout.splitlines() if line.startswith("sha ")]
    assert len(sha) == 1 and sha[0][1] == hashlib.sha256(Lab.result_bytes(r.res)).hexdigest() and int(sha[0][3]) == int(r.res.n_windows.sum())


# ---------------------------------------------------------------- the stitch
@gpu
def test_window_blocks_of_the_stitch():
    """k_stitch compacts 64 windows at a time: ZMWs of exactly 64, of 65 and of more windows"""
    r = run("many_windows")
    c = r.census
    print("windows per ZMW", [len(z.tpls) for z in r.zmws])
    assert c["zmw_of_64_windows"] >= 1 and c["zmw_of_65_windows"] >= 1 and c["zmw_above_65_windows"] >= 1, c
    assert (r.res.status == 0).all() and r.res.n_windows.tolist() == [len(z.tpls) for z in r.zmws]
    r.plain_run_is_identical()


@gpu
def test_low_rq_is_reported():
    h = handle(min_rq=Lab.MIN_RQ_LOW)
    r = Run(h, Lab.low_rq())
    assert r.compare() == []                                                              # no ZMW so near min_rq that its status is not checked
    want = [r.ref[z]["status"] for z in range(r.b.n_zmw)]
    print("census", dict(r.census), "reference statuses", want, "rq_ref", [round(r.ref[z]["rq_ref"], 6) for z in range(r.b.n_zmw)])
    assert want.count(K.LOW_RQ) >= 2 and want.count(K.SUCCESS) >= 2 and set(want) == {K.LOW_RQ, K.SUCCESS}, want
    assert [int(s) for s in r.res.status] == want
    assert all(r.res.seq_len[z] > 0 and r.res.kinetics(z).any() for z in range(r.b.n_zmw))          # a LOW_RQ ZMW keeps its consensus and planes
    r.plain_run_is_identical()


@gpu
def test_max_qv_93():
    r = Run(handle(max_qv=93), Lab.low_rq())
    r.compare()
    above = sum(int((r.ref[z]["qual"] > 50).sum()) for z in r.ref)
    print("census", dict(r.census), "reference qual bytes above 50:", above)
    assert above > 100 and (r.res.status == 0).sum() >= 4                                 # the cap of the default max_qv is gone
    base = run("strand_reference")
    again = Run(handle(max_qv=93), base.b)
    again.compare()
    assert [int(s) for s in again.res.status] == [int(s) for s in base.res.status] and (again.res.rq >= base.res.rq).all()

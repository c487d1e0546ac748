"""ccs --orient-passes (DESIGN.md §2 "Pass orientation", §7): the option's usage, and on an MI355X a subreads BAM whose cx tags carry adapter bits only — clean
ZMWs, one whose third subread is missing (every later pass breaks the alternation), one that opens with a reverse pass, one whose subreads carry direction
bits.  With the option every ZMW gives the read the library gives on the true strands, np = its full-length passes; without it the driver does what it did — the
alternation guess — and the damaged ZMW loses passes or its read."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bam_util
from test_cli_fail_reads import CCS, HDR, _ccs, _records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
COMMON = ["--min-passes", "3", "--min-rq", "0.9"]


def test_usage(built, tmp_path):
    for order in (["--orient-passes", "--by-strand"], ["--by-strand", "--orient-passes"]):
        p = subprocess.run([CCS, "in.bam", "out.bam", *order], capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert p.returncode == 2 and "--orient-passes" in p.stderr and "--by-strand" in p.stderr and "not supported" in p.stderr
    p = subprocess.run([CCS, "in.bam", "out.bam", "--orient-passes"], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert p.returncode != 2 and "--orient-passes" not in p.stderr           # accepted: the run fails on the missing input
    assert "--orient-passes" in subprocess.run([CCS, "--help"], capture_output=True, text=True, timeout=60).stderr


# ---------------------------------------------------------------- GPU
def _zmws(seed=811):
    """(zm, kind, passes as (bases, pw, ipd, true strand, cx)): templates of 900-1100 bases, 6-8 passes"""
    import lowcx
    rng = np.random.default_rng(seed)
    out = []
    for zm, kind in enumerate(("clean", "clean", "third_removed", "opens_reverse", "third_removed", "given", "clean"), start=700):
        t = rng.integers(0, 4, int(rng.integers(900, 1101))).astype(np.uint8)
        n = int(rng.integers(6, 9))
        strands = [(k + (kind == "opens_reverse")) & 1 for k in range(n + 1)]
        if kind == "third_removed":
            del strands[2]
        ps = []
        for s in strands[:n]:
            b, p = lowcx.sequence_read(rng, t)
            if s:
                b, p = (3 - b[::-1]).astype(np.uint8), p[::-1]
            ps.append((b, p, rng.integers(1, 61, len(b)).astype(np.uint8), s, 3 | ((32 if s else 16) if kind == "given" else 0)))
        out.append((zm, kind, ps))
    return out


def _write(path, zmws):
    recs = []
    for zm, _, ps in zmws:
        q = 0
        for b, p, ip, _, cx in ps:
            recs.append(bam_util.record(f"m1/{zm}/{q}_{q + len(b)}", "".join("ACGT"[c] for c in b),
                                        [("zm", "i", zm), ("sn", "Bf", [9.0, 16.0, 8.0, 13.0]), ("pw", "BC", p), ("ip", "BC", ip), ("cx", "i", cx)]))
            q += len(b) + 45
    bam_util.write_bam(path, HDR, recs)


def _library(zmws, alternate):
    """{zm: (status, np, sequence, quals)} of the library on the true strands, or on the driver's guess (alternation where cx has no direction bit)"""
    from ccs_amd import api
    zid, ro, bo, fl, bs, pw, ip = [], [0], [0], [], [], [], []
    for zm, kind, ps in zmws:
        zid.append(zm)
        for k, (b, p, i, s, cx) in enumerate(ps):
            bs.append(b); pw.append(p); ip.append(i); bo.append(bo[-1] + len(b))
            fl.append((k & 1) if alternate and not cx & 48 else s)
        ro.append(ro[-1] + len(ps))
    b = api.Batch(np.array(zid, np.int32), np.tile(np.array([9.0, 16.0, 8.0, 13.0], np.float32), (len(zid), 1)), np.array(ro, np.int32), np.array(bo, np.int64),
                  np.concatenate(bs).astype(np.uint8), np.concatenate(pw).astype(np.uint8), np.concatenate(ip).astype(np.uint8), np.array(fl, np.uint8))
    o = api.default_opts()
    o.min_passes, o.min_rq = 3, 0.9
    h = api.Handle(0, opts=o)
    res = h.consensus(b)
    h.close()
    return {zm: (int(res.status[z]), int(res.np_[z]), res.sequence(z).copy(), res.quals(z).copy()) for z, zm in enumerate(zid)}


@pytest.fixture(scope="module")
def runs(tmp_path_factory, built):
    d = tmp_path_factory.mktemp("orient")
    zmws = _zmws()
    bam = d / "in.subreads.bam"
    _write(bam, zmws)
    _ccs(bam, d / "off.bam", *COMMON)
    p = _ccs(bam, d / "on.bam", *COMMON, "--orient-passes", "--log-level", "INFO")
    return zmws, d, p.stderr


def _reads(path):
    return {r["tags"]["zm"]: r for r, _ in _records(path)[1]}


@pytest.mark.gpu
def test_every_zmw_gives_the_read_of_its_true_strands(runs):
    zmws, d, log = runs
    lib = _library(zmws, alternate=False)
    on = _reads(d / "on.bam")
    assert set(on) == {zm for zm, _, _ in zmws} and all(st == 0 for st, _, _, _ in lib.values())
    for zm, kind, ps in zmws:
        st, np_, seq, qual = lib[zm]
        r = on[zm]
        assert r["tags"]["np"] == np_ == len(ps), (zm, kind)
        assert np.array_equal(r["seq"], seq) and np.array_equal(r["qual"], qual), (zm, kind)
    unknown = sum(len(ps) for _, kind, ps in zmws if kind != "given")
    assert f"--orient-passes: {unknown} passes submitted strand-unknown" in log


@pytest.mark.gpu
def test_without_the_option_the_driver_alternates(runs):
    zmws, d, log = runs
    guess = _library(zmws, alternate=True)
    off, on = _reads(d / "off.bam"), _reads(d / "on.bam")
    assert set(off) == {zm for zm, (st, _, _, _) in guess.items() if st == 0}
    for zm, r in off.items():
        assert r["tags"]["np"] == guess[zm][1] and np.array_equal(r["seq"], guess[zm][2]) and np.array_equal(r["qual"], guess[zm][3]), zm
    damaged = [zm for zm, kind, _ in zmws if kind == "third_removed"]
    for zm in damaged:                                                  # fewer mapped passes, or no read at all
        assert zm not in off or off[zm]["tags"]["np"] < on[zm]["tags"]["np"], zm
    for zm, kind, ps in zmws:                                           # the others lose nothing: only relative orientation reaches a result
        if kind != "third_removed":
            assert off[zm]["tags"]["np"] == len(ps) and np.array_equal(off[zm]["seq"], on[zm]["seq"]), (zm, kind)
    assert "--orient-passes" not in _ccs(d / "in.subreads.bam", d / "off2.bam", *COMMON, "--log-level", "INFO").stderr
    assert [x for _, x in _records(d / "off2.bam")[1]] == [x for _, x in _records(d / "off.bam")[1]]

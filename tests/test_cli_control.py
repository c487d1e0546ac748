"""ccs --control FILE.fasta (DESIGN.md §2 "Control screen", §7; docs/faq/fail-reads.md fail class 0x2, docs/faq/reports-aux-files.md:42-43): the option's usage
errors, and on an MI355X a subreads BAM of control molecules in both orientations (some with too few clean passes for --min-rq), templates that hold a part of
the control, adapter dimers and normal ZMWs: without the option no output knows of controls; with it the main output loses exactly the ZMWs the library reports
as FOUND on the same passes, the two report rows, the JSON keys, the metrics statuses and the index agree with that set, --fail-reads writes those with a consensus
with ff 0x2 beside the other bits, and the output does not depend on the number of packing threads or the batch size.

The oracle on the CPU (tests/oracle_lib.py consensus_batch on the same passes) for the seed below: every ZMW ends as SUCCESS or LOW_RQ, so every planted control is
tested; the set the driver must remove is nevertheless taken from the library's report, not from the planting."""
import gzip
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bam_util
from test_cli_fail_reads import CCS, MIN_RQ, _ccs, _records, _write

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
ROWS = ("ZMW with control failure", "ZMW with control success")


def _fasta(path, recs):
    path.write_text("".join(f">{n}\n{s}\n" for n, s in recs))
    return path


def _run(tmp_path, *args):
    return subprocess.run([CCS, "in.bam", "out.bam", *map(str, args)], capture_output=True, text=True, timeout=60, cwd=tmp_path)


# ---------------------------------------------------------------- CPU: usage
def test_bad_control_files_name_what_is_wrong(built, tmp_path):
    good = "ACGTTGCAAGGCTTAACCGGTTAGCATGCA" * 140                      # 4200 bases
    cases = [([("one", good[:100]), ("another one", good[:100])], "record 2 (>another one)", "more than one record"),
             ([("short", good[:63])], "record 1 (>short)", "63 bases"),
             ([("long", good[:4097])], "record 1 (>long)", "more than 4096"),
             ([("withN", good[:70] + "N" + good[:70])], "record 1 (>withN)", "'N'")]
    for recs, where, what in cases:
        f = _fasta(tmp_path / "bad.fasta", recs)
        p = _run(tmp_path, "--control", f)
        assert p.returncode == 2 and "--control" in p.stderr and where in p.stderr and what in p.stderr, p.stderr
    p = _run(tmp_path, "--control", "missing.fasta")
    assert p.returncode == 2 and "missing.fasta" in p.stderr and "cannot open" in p.stderr
    p = _run(tmp_path, "--control")
    assert p.returncode == 2 and "missing value for --control" in p.stderr
    (tmp_path / "empty.fasta").write_text("\n")
    p = _run(tmp_path, "--control", "empty.fasta")
    assert p.returncode == 2 and "no FASTA record" in p.stderr
    (tmp_path / "headless.fasta").write_text(good[:100] + "\n")
    p = _run(tmp_path, "--control", "headless.fasta")
    assert p.returncode == 2 and "before the first '>'" in p.stderr
    # the limits are accepted (the run then fails on the missing input, not on the option), in either case and over several lines; --fail-reads is not needed
    for n in (64, 4096):
        f = _fasta(tmp_path / "ok.fasta", [("ok", "\n".join(good[:n].lower()[k:k + 60] for k in range(0, n, 60)))])
        p = _run(tmp_path, "--control", f)
        assert p.returncode != 2 and "--control" not in p.stderr, p.stderr
    p = _run(tmp_path, "--control", f, "--fail-reads", "f.bam", "--by-strand")
    assert p.returncode == 2 and "not supported" in p.stderr
    usage = subprocess.run([CCS, "--help"], capture_output=True, text=True, timeout=60).stderr
    assert "--control" in usage and "0x2" in usage


# ---------------------------------------------------------------- GPU
COUNTS = (("control", 5), ("control_rc", 5), ("control_lowrq", 4), ("partial", 4), ("dimer", 3), ("normal", 5), ("lowrq", 3))


def _zmws(seed=2041, zm0=700):
    """(zm, kind, passes as (bases, pw, ipd, full)) of every ZMW.  control / control_rc: the 2000-base test control at 8 passes; control_lowrq: the control at 3
    noisy passes; partial: 2000-3000 random bases with 30-45 % of the control inside; dimer: 10-30 copies of the test adapter; normal; lowrq: 3 noisy passes"""
    import adapter_synth as A
    import control_synth as S
    import lowcx
    rng = np.random.default_rng(seed)
    c = S.encode(S.TEST_CONTROL)
    ad = A.encode(A.TEST_ADAPTER)
    rnd = lambda m: rng.integers(0, 4, int(m)).astype(np.uint8)
    out = []

    def passes(t, n, channel=1.0):
        ps = []
        for k in range(n):
            b, p = lowcx.sequence_read(rng, t, channel)
            if k & 1:
                b, p = (3 - b[::-1]).astype(np.uint8), p[::-1]
            ps.append((b, p, rng.integers(1, 61, len(b)).astype(np.uint8), True))
        return ps
    zm = zm0
    for kind, n in COUNTS:
        for _ in range(n):
            L = int(rng.integers(2000, 3001))
            if kind in ("control", "control_rc", "partial"):
                t = S.template(rng, kind, L, c)
            elif kind == "control_lowrq":
                t = c
            elif kind == "dimer":
                parts = []
                for _ in range(int(rng.integers(10, 31))):
                    parts += [ad, rnd(rng.integers(0, 61))]
                t = np.concatenate(parts[:-1])
            else:
                t = rnd(L)
            out.append((zm, kind, passes(t, 3, 2.0) if kind in ("lowrq", "control_lowrq") else passes(t, 8)))
            zm += 1
    return out


def _library_verdicts(zmws):
    """what the library reports for the same passes: {zm: (control verdict, final status)}"""
    from ccs_amd import api
    import control_synth as S
    zid, snr, ro, bo, fl, bs, pw, ip = [], [], [0], [0], [], [], [], []
    for zm, _, ps in zmws:
        zid.append(zm); snr.append([9.0, 16.0, 8.0, 13.0])
        for k, (b, p, i, _) in enumerate(ps):
            bs.append(b); pw.append(p); ip.append(i); fl.append(k & 1); bo.append(bo[-1] + len(b))
        ro.append(ro[-1] + len(ps))
    b = api.Batch(np.array(zid, np.int32), np.array(snr, np.float32), np.array(ro, np.int32), np.array(bo, np.int64), np.concatenate(bs).astype(np.uint8),
                  np.concatenate(pw).astype(np.uint8), np.concatenate(ip).astype(np.uint8), np.array(fl, np.uint8))
    o = api.default_opts()
    o.min_rq = float(MIN_RQ)
    h = api.Handle(0, opts=o)
    res, rep, _, _, _, _ = h.consensus_control(b, api.ControlSeq.from_string(S.TEST_CONTROL))
    h.close()
    return {zm: (int(rep.verdict[z]), int(res.status[z])) for z, (zm, _, _) in enumerate(zmws)}


@pytest.fixture(scope="module")
def runs(tmp_path_factory, built):
    import adapter_synth as A
    import control_synth as S
    d = tmp_path_factory.mktemp("control")
    zmws = _zmws()
    bam = d / "in.subreads.bam"
    _write(bam, zmws)
    fa = _fasta(d / "control.fasta", [("test control", "\n".join(S.TEST_CONTROL[k:k + 70].lower() for k in range(0, 2000, 70)))])
    ad = _fasta(d / "adapters.fasta", [("test_adapter", A.TEST_ADAPTER)])
    common = ["--min-rq", MIN_RQ, "--min-passes", "3"]
    rep = lambda n: ["--report-json", d / (n + ".json"), "--report-file", d / (n + ".txt"), "--metrics-json", d / (n + ".metrics.json.gz")]
    _ccs(bam, d / "off.bam", *common, *rep("off"))
    _ccs(bam, d / "on.bam", *common, "--control", fa, *rep("on"))
    _ccs(bam, d / "on2.bam", *common, "--control", fa, "--workers-per-gpu", "1", "--batch-size", "5", *rep("on2"))
    _ccs(bam, d / "fr_off.bam", *common, "--fail-reads", d / "fr_off.fail.bam", "--adapters", ad, *rep("fr_off"))
    _ccs(bam, d / "fr.bam", *common, "--fail-reads", d / "fr.fail.bam", "--adapters", ad, "--control", fa, *rep("fr"))
    _ccs(bam, d / "fr2.bam", *common, "--fail-reads", d / "fr2.fail.bam", "--adapters", ad, "--control", fa, "--workers-per-gpu", "2", "--batch-size", "7")
    _ccs(bam, d / "fq.fastq.gz", *common, "--control", fa)
    _ccs(bam, d / "bs.bam", "--min-rq", "0.9", "--min-passes", "3", "--control", fa, "--by-strand", "--hifi-kinetics", "--pileup-summary",
         "--metrics-json", d / "bs.metrics.json.gz")
    return zmws, _library_verdicts(zmws), d


@pytest.mark.gpu
def test_without_the_option_no_output_knows_of_controls(runs):
    zmws, lib, d = runs
    ex = json.load(open(d / "off.json"))["exclusive_failed_counts"]
    txt = open(d / "off.txt").read()
    for row in ROWS:
        assert row not in ex and row not in txt
    with gzip.open(d / "off.metrics.json.gz", "rt") as f:
        assert not any(x["status"].startswith("CONTROL") for x in json.load(f)["zmws"])
    _, ffr = _records(d / "fr_off.fail.bam")
    assert not any(r["tags"]["ff"] & 0x2 for r, _ in ffr)
    _, off = _records(d / "off.bam")
    assert {r["tags"]["zm"] for r, _ in off} >= {zm for zm, (v, st) in lib.items() if st == 0}


@pytest.mark.gpu
def test_main_output_loses_exactly_the_found_zmws(runs):
    zmws, lib, d = runs
    kind = {zm: k for zm, k, _ in zmws}
    found = {zm for zm, (v, st) in lib.items() if v == 2}
    assert found >= {zm for zm, k in kind.items() if k in ("control", "control_rc")} and not any(kind[zm] in ("partial", "dimer", "normal", "lowrq") for zm in found)
    _, off = _records(d / "off.bam")
    _, on = _records(d / "on.bam")
    assert [x for r, x in off if r["tags"]["zm"] not in found] == [x for _, x in on]                  # the others byte for byte
    assert len(on) < len(off)
    pbi = bam_util.read_pbi(str(d / "on.bam") + ".pbi")
    assert np.array_equal(pbi["file_offset"], bam_util.record_virtual_offsets(d / "on.bam"))
    assert list(pbi["hole"]) == [r["tags"]["zm"] for r, _ in on]


@pytest.mark.gpu
def test_report_rows_json_keys_and_metrics(runs):
    zmws, lib, d = runs
    ok = {zm for zm, (v, st) in lib.items() if v == 2 and st == 0}
    bad = {zm for zm, (v, st) in lib.items() if v == 2 and st != 0}
    assert len(ok) >= 1 and len(bad) >= 1                                                           # both rows are exercised
    _, on = _records(d / "on.bam")
    for name in ("on", "fr"):
        rep = json.load(open(d / (name + ".json")))
        ex = rep["exclusive_failed_counts"]
        assert ex["ZMW with control success"] == len(ok) and ex["ZMW with control failure"] == len(bad), (name, ex)
        txt = open(d / (name + ".txt")).read()
        assert f"ZMW with control failure      : {len(bad)} (" in txt and f"ZMW with control success      : {len(ok)} (" in txt
        assert txt.index("ZMW with control failure") < txt.index("ZMW with control success") < txt.index("CCS below minimum RQ")
        with gzip.open(d / (name + ".metrics.json.gz"), "rt") as f:
            m = {x["zmw"]: x for x in json.load(f)["zmws"]}
        assert {k for k, v in m.items() if v["status"] == "CONTROL_SUCCESS"} == {f"m1/{z}" for z in ok}
        assert {k for k, v in m.items() if v["status"] == "CONTROL_FAILURE"} == {f"m1/{z}" for z in bad}
        assert sum(ex.values()) - (ex.get("ZMW with full-length subread", 0)) == rep["zmws_fail_filters"]     # a ZMW is counted once
    assert json.load(open(d / "on.json"))["zmws_pass_filters"] == len(on)
    p = _ccs(d / "in.subreads.bam", d / "info.bam", "--min-rq", MIN_RQ, "--min-passes", "3", "--control", d / "control.fasta", "--log-level", "INFO")
    assert f", {len(ok) + len(bad)} control ZMWs" in p.stderr


@pytest.mark.gpu
def test_fail_reads_carry_the_control_bit(runs):
    zmws, lib, d = runs
    kind = {zm: k for zm, k, _ in zmws}
    found = {zm for zm, (v, st) in lib.items() if v == 2}
    with_consensus = {zm for zm in found if lib[zm][1] in (0, 7)}
    _, fr_off = _records(d / "fr_off.bam")
    _, ffr_off = _records(d / "fr_off.fail.bam")
    _, fr = _records(d / "fr.bam")
    _, fail = _records(d / "fr.fail.bam")
    assert [x for r, x in fr_off if r["tags"]["zm"] not in found] == [x for _, x in fr]
    assert {r["tags"]["zm"] for r, _ in fail if r["tags"]["ff"] & 0x2} == with_consensus
    old = {r["tags"]["zm"]: (r, x) for r, x in ffr_off}
    order = [r["tags"]["zm"] for r, _ in fail]
    assert order == sorted(order) and set(order) == set(old) | with_consensus
    for r, x in fail:
        t = r["tags"]
        if not t["ff"] & 0x2:
            assert x == old[t["zm"]][1]                                                               # every other record byte for byte
            continue
        assert r["name"] == f"m1/{t['zm']}/ccs" and bool(t["ff"] & 0x1) == (t["rq"] < float(MIN_RQ))
        if t["zm"] in old:                                                                            # it was a fail read already: its bits combine
            assert t["ff"] == old[t["zm"]][0]["tags"]["ff"] | 0x2
    dimers = {r["tags"]["zm"]: r["tags"]["ff"] for r, _ in fail if kind[r["tags"]["zm"]] == "dimer"}
    assert len(dimers) == 3 and all(f & 0x50 and not f & 0x2 for f in dimers.values()), dimers
    assert any(t & 0x1 for t in (r["tags"]["ff"] for r, _ in fail if r["tags"]["ff"] & 0x2)), "no control below --min-rq: 0x1 | 0x2 is not exercised"
    pbi = bam_util.read_pbi(str(d / "fr.fail.bam") + ".pbi")
    assert np.array_equal(pbi["file_offset"], bam_util.record_virtual_offsets(d / "fr.fail.bam"))
    assert list(pbi["hole"]) == order


@pytest.mark.gpu
def test_independent_of_workers_and_batch_size(runs):
    _, _, d = runs
    assert [x for _, x in _records(d / "on.bam")[1]] == [x for _, x in _records(d / "on2.bam")[1]]
    assert [x for _, x in _records(d / "fr.bam")[1]] == [x for _, x in _records(d / "fr2.bam")[1]]
    assert [x for _, x in _records(d / "fr.fail.bam")[1]] == [x for _, x in _records(d / "fr2.fail.bam")[1]]
    assert json.load(open(d / "on.json")) == json.load(open(d / "on2.json"))


@pytest.mark.gpu
def test_fastq_and_by_strand(runs):
    zmws, lib, d = runs
    kind = {zm: k for zm, k, _ in zmws}
    found = {zm for zm, (v, st) in lib.items() if v == 2}
    with gzip.open(d / "fq.fastq.gz", "rt") as f:
        names = [ln[1:].strip() for ln in f if ln.startswith("@m1/")]
    assert names == [r["name"] for r, _ in _records(d / "on.bam")[1]] and not any(int(n.split("/")[1]) in found for n in names)
    # --by-strand: every strand entity is screened on its own draft; no strand of a clean planted control reaches the output, both strands of normal ZMWs do
    _, bs = _records(d / "bs.bam")
    zs = [r["tags"]["zm"] for r, _ in bs]
    assert not any(kind[z] in ("control", "control_rc") for z in zs)
    assert sum(kind[z] == "normal" for z in zs) >= 6 and all(r["name"].endswith(("/fwd", "/rev")) for r, _ in bs)      # (4 passes per strand: --min-rq 0.9)
    with gzip.open(d / "bs.metrics.json.gz", "rt") as f:
        m = {x["zmw"]: x["status"] for x in json.load(f)["zmws"]}
    for zm, k in kind.items():
        if k in ("control", "control_rc"):
            assert m[f"m1/{zm}/fwd"].startswith("CONTROL_") and m[f"m1/{zm}/rev"].startswith("CONTROL_"), (zm, m[f"m1/{zm}/fwd"], m[f"m1/{zm}/rev"])
    assert not any(v.startswith("CONTROL_") for z, v in m.items() if kind[int(z.split("/")[1])] in ("partial", "dimer", "normal", "lowrq"))

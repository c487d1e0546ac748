"""ccs --coverage-filters (DESIGN.md §2 "Coverage rule", §7; docs/faq/reports-aux-files.md:28-35,149-155): the options' usage errors, and on an MI355X a subreads
BAM of planted layouts — clean ZMWs, a block of bases in half of the passes, passes with unique foreign blocks that do not span, a ZMW with a foreign pass, passes
of unrelated molecules: without the flag no output knows of the screen; with it the main output and its index lose exactly the ZMWs the library gates on the same
passes, the four report rows, the JSON keys and the metrics statuses agree with the library's statuses, --fail-reads writes the 0x8 record of a gated ZMW, and
the output does not depend on workers or batch size.  On --write-synthetic input (which has the index --chunk needs) the chunks add up to the whole, and the flag removes nothing: both outputs are the same bytes."""
import gzip
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bam_util
from test_cli_fail_reads import CCS, _ccs, _records, _write

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
ROWS = ("Coverage drops", "Insufficient draft cov", "Draft too different")
NAMES = {11: "TOO_FEW_PASSES_AFTER_DRAFT_ALIGNMENT", 12: "INSUFFICIENT_SPANS", 13: "COVERAGE_DROPS", 14: "TOO_MANY_UNUSABLE", 3: "INSUFFICIENT_SPANS"}
ROW_OF = {11: "Draft too different", 12: "Insufficient draft cov", 13: "Coverage drops", 14: "Reads failed polishing", 3: "Insufficient draft cov"}


def _run(tmp_path, *args):
    return subprocess.run([CCS, "in.bam", "out.bam", *map(str, args)], capture_output=True, text=True, timeout=60, cwd=tmp_path)


# ---------------------------------------------------------------- CPU: usage
def test_usage_errors(built, tmp_path):
    for opt, bad, rng in (("--coverage-drop-percent", ("-1", "101", "x", "5x", ""), "0 .. 100"), ("--coverage-block", ("0", "4097", "-3", "b", ""), "1 .. 4096")):
        for v in bad:
            p = _run(tmp_path, "--coverage-filters", opt, v)
            assert p.returncode == 2 and opt in p.stderr and rng in p.stderr, (opt, v, p.stderr)
        p = _run(tmp_path, "--coverage-filters", opt)
        assert p.returncode == 2 and "missing value for " + opt in p.stderr
        p = _run(tmp_path, opt, "20")
        assert p.returncode == 2 and "need --coverage-filters" in p.stderr
    # the limits are accepted (the run then fails on the missing input, not on the options), with the other output options beside them
    for args in (("--coverage-filters",), ("--coverage-filters", "--coverage-drop-percent", "0", "--coverage-block", "1"),
                 ("--coverage-block", "4096", "--coverage-drop-percent", "100", "--coverage-filters", "--by-strand"),
                 ("--coverage-filters", "--fail-reads", "f.bam", "--chunk", "1/2")):
        p = _run(tmp_path, *args)
        assert p.returncode != 2 and "--coverage" not in p.stderr, (args, p.stderr)
    p = subprocess.run([CCS, "in.bam", "--fit-model", "m.json", "--coverage-filters"], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert p.returncode == 2 and "--coverage-filters" in p.stderr and "not supported" in p.stderr
    usage = subprocess.run([CCS, "--help"], capture_output=True, text=True, timeout=60).stderr
    for word in ("--coverage-filters", "--coverage-drop-percent", "--coverage-block", "Coverage drops", "Insufficient draft cov", "Draft too different",
                 "failed polishing"):
        assert word in usage, word


# ---------------------------------------------------------------- GPU
COUNTS = (("clean", 5), ("block300", 3), ("block100", 2), ("unique_blocks", 2), ("foreign_pass", 2), ("unrelated", 2), ("block300_2of8", 2))


def _zmws(seed=3107, zm0=900):
    """(zm, kind, passes as (bases, pw, ipd, full)) of every ZMW, 600-900-base templates, odd passes on the reverse strand.  clean: 8 passes; block300 / block100:
    the block in the last four of 8 passes; unique_blocks: two clean passes, then six that each carry three foreign blocks of their own (they align as a prefix
    and a suffix and do not span); foreign_pass: three passes, the last one of another molecule; unrelated: six passes of six molecules; block300_2of8"""
    import coverage_synth as S
    import lowcx
    rng = np.random.default_rng(seed)
    out = []
    zm = zm0
    for kind, n in COUNTS:
        for _ in range(n):
            L = int(rng.integers(600, 901))
            t = S.rnd(rng, L)
            if kind == "clean":
                tp = [t] * 8
            elif kind in ("block300", "block100"):
                tp = [t] * 4 + [S.with_block(t, S.rnd(rng, 300 if kind == "block300" else 100), L // 2)] * 4
            elif kind == "block300_2of8":
                tp = [t] * 5 + [S.with_block(t, S.rnd(rng, 300), L // 3)] * 2 + [t]
            elif kind == "unique_blocks":
                tp = [t, t]
                for _ in range(6):
                    u = t
                    for f in (0.8, 0.5, 0.2):
                        u = S.with_block(u, S.rnd(rng, 160), int(L * f))
                    tp.append(u)
            elif kind == "foreign_pass":
                tp = [t, t, S.rnd(rng, L)]
            else:
                tp = [S.rnd(rng, L) for _ in range(6)]
            ps = []
            for k, x in enumerate(tp):
                b, p = lowcx.sequence_read(rng, x)
                if k & 1:
                    b, p = S.rc(b), p[::-1]
                ps.append((b, p, rng.integers(1, 61, len(b)).astype(np.uint8), True))
            out.append((zm, kind, ps))
            zm += 1
    return out


def _batch(zmws):
    from ccs_amd import api
    zid, snr, ro, bo, fl, bs, pw, ip = [], [], [0], [0], [], [], [], []
    for zm, _, ps in zmws:
        zid.append(zm); snr.append([9.0, 16.0, 8.0, 13.0])
        for k, (b, p, i, _) in enumerate(ps):
            bs.append(b); pw.append(p); ip.append(i); fl.append(k & 1); bo.append(bo[-1] + len(b))
        ro.append(ro[-1] + len(ps))
    return api.Batch(np.array(zid, np.int32), np.array(snr, np.float32), np.array(ro, np.int32), np.array(bo, np.int64), np.concatenate(bs).astype(np.uint8),
                     np.concatenate(pw).astype(np.uint8), np.concatenate(ip).astype(np.uint8), np.array(fl, np.uint8))


def _library(zmws, **kw):
    """what the library reports for the same passes: {zm: (status without the request, status with every gate bit, verdict)}"""
    from ccs_amd import api
    b = _batch(zmws)
    h = api.Handle(0)
    plain = h.consensus(b)
    o = api.coverage_opts_default()
    for k, v in kw.items():
        setattr(o, k, v)
    res, rep, *_ = h.consensus_coverage(b, o, gate=api.COVERAGE_GATE_ALL)
    h.close()
    return {zm: (int(plain.status[z]), int(res.status[z]), int(rep.verdict[z])) for z, (zm, _, _) in enumerate(zmws)}


@pytest.fixture(scope="module")
def runs(tmp_path_factory, built):
    d = tmp_path_factory.mktemp("coverage")
    zmws = _zmws()
    bam = d / "in.subreads.bam"
    _write(bam, zmws)
    common = ["--min-passes", "3"]
    rep = lambda n: ["--report-json", d / (n + ".json"), "--report-file", d / (n + ".txt"), "--metrics-json", d / (n + ".metrics.json.gz")]
    _ccs(bam, d / "off.bam", *common, *rep("off"))
    p = _ccs(bam, d / "on.bam", *common, "--coverage-filters", "--log-level", "INFO", *rep("on"))
    (d / "on.log").write_text(p.stderr)
    _ccs(bam, d / "on2.bam", *common, "--coverage-filters", "--workers-per-gpu", "1", "--batch-size", "5", *rep("on2"))
    _ccs(bam, d / "blk.bam", *common, "--coverage-filters", "--coverage-block", "400", "--coverage-drop-percent", "40", *rep("blk"))
    _ccs(bam, d / "fr_off.bam", *common, "--fail-reads", d / "fr_off.fail.bam")
    _ccs(bam, d / "fr.bam", *common, "--fail-reads", d / "fr.fail.bam", "--coverage-filters", *rep("fr"))
    _ccs(bam, d / "bs.bam", "--min-passes", "3", "--min-rq", "0.9", "--coverage-filters", "--by-strand", "--metrics-json", d / "bs.metrics.json.gz")
    _ccs("--write-synthetic", "12,6,700,5", d / "syn.subreads.bam")
    _ccs(d / "syn.subreads.bam", d / "syn_off.bam", *rep("syn_off"))
    _ccs(d / "syn.subreads.bam", d / "syn_on.bam", "--coverage-filters", *rep("syn_on"))
    for i in (1, 2):                                               # (--chunk needs the input's .pbi: the synthetic BAM has one)
        _ccs(d / "syn.subreads.bam", d / f"c{i}.bam", "--coverage-filters", "--chunk", f"{i}/2", "--report-json", d / f"c{i}.json")
    return zmws, _library(zmws), d


def _metrics(path):
    with gzip.open(path, "rt") as f:
        return {x["zmw"]: x for x in json.load(f)["zmws"]}


@pytest.mark.gpu
def test_without_the_flag_no_output_knows_of_the_screen(runs):
    zmws, lib, d = runs
    ex = json.load(open(d / "off.json"))["exclusive_failed_counts"]
    txt = open(d / "off.txt").read()
    for row in ROWS:
        assert row not in ex and row not in txt
    m = _metrics(d / "off.metrics.json.gz")
    assert not {x["status"] for x in m.values()} & {"COVERAGE_DROPS", "INSUFFICIENT_SPANS", "TOO_FEW_PASSES_AFTER_DRAFT_ALIGNMENT"}
    # the "more than half must map" rule is counted where it always was
    unusable = {zm for zm, (st, _, _) in lib.items() if st == 3}
    assert len(unusable) >= 2 and ex["Reads failed polishing"] == len(unusable)
    assert {k for k, x in m.items() if x["status"] == "TOO_MANY_UNUSABLE"} == {f"m1/{z}" for z in unusable}
    _, off = _records(d / "off.bam")
    assert {r["tags"]["zm"] for r, _ in off} == {zm for zm, (st, _, _) in lib.items() if st == 0}
    # on --write-synthetic input the flag removes nothing: the same bytes, the same counts in the rows both reports have
    assert open(d / "syn_on.bam", "rb").read() == open(d / "syn_off.bam", "rb").read()
    assert open(str(d / "syn_on.bam") + ".pbi", "rb").read() == open(str(d / "syn_off.bam") + ".pbi", "rb").read()
    a, b = json.load(open(d / "syn_off.json")), json.load(open(d / "syn_on.json"))
    assert a["zmws_pass_filters"] == b["zmws_pass_filters"] == 12
    assert {k: v for k, v in b["exclusive_failed_counts"].items() if k not in ROWS} == a["exclusive_failed_counts"]
    assert all(b["exclusive_failed_counts"][k] == 0 for k in ROWS)
    assert _metrics(d / "syn_on.metrics.json.gz") == _metrics(d / "syn_off.metrics.json.gz")


@pytest.mark.gpu
def test_main_output_loses_exactly_the_gated_zmws(runs):
    zmws, lib, d = runs
    kind = {zm: k for zm, k, _ in zmws}
    gated = {zm for zm, (_, st, _) in lib.items() if 11 <= st <= 14}
    # the plantings do what they are planted for
    assert {zm for zm, k in kind.items() if k in ("block300", "block100")} == {zm for zm, (_, st, _) in lib.items() if st == 13}
    assert {zm for zm, k in kind.items() if k == "unique_blocks"} == {zm for zm, (_, st, _) in lib.items() if st == 12}
    assert {zm for zm, k in kind.items() if k == "foreign_pass"} == {zm for zm, (_, st, _) in lib.items() if st == 11}
    assert not any(kind[zm] in ("clean", "block300_2of8") for zm in gated)
    for zm, (st0, st1, v) in lib.items():
        assert st1 == (9 + v if v >= 2 else st0), (zm, kind[zm], st0, st1, v)
    _, off = _records(d / "off.bam")
    _, on = _records(d / "on.bam")
    assert [x for r, x in off if r["tags"]["zm"] not in gated] == [x for _, x in on]                  # the others byte for byte
    assert len(on) >= 7 and not any(r["tags"]["zm"] in gated for r, _ in on)
    pbi = bam_util.read_pbi(str(d / "on.bam") + ".pbi")
    assert np.array_equal(pbi["file_offset"], bam_util.record_virtual_offsets(d / "on.bam"))
    assert list(pbi["hole"]) == [r["tags"]["zm"] for r, _ in on]


@pytest.mark.gpu
def test_report_rows_json_keys_and_metrics(runs):
    zmws, lib, d = runs
    want = {}
    for zm, (_, st, _) in lib.items():
        if st in ROW_OF:
            want[ROW_OF[st]] = want.get(ROW_OF[st], 0) + 1
    assert want["Coverage drops"] == 5 and want["Draft too different"] == 2 and want["Insufficient draft cov"] == 4    # (two of them by the half-must-map rule)
    _, on = _records(d / "on.bam")
    for name in ("on", "fr", "on2"):
        rep = json.load(open(d / (name + ".json")))
        ex = rep["exclusive_failed_counts"]
        txt = open(d / (name + ".txt")).read()
        for row in ROWS + ("Reads failed polishing",):
            assert ex[row] == want.get(row, 0), (name, row, ex)
            assert f"{row:<30}: {want.get(row, 0)} (" in txt, (name, row)
        order = ["Lacking full passes", "Coverage drops", "Insufficient draft cov", "Draft too different", "Draft generation error", "Draft above --max-length",
                 "Draft below --min-length", "Reads failed polishing", "Empty coverage windows", "CCS did not converge"]
        at = [txt.index(k) for k in order]
        assert at == sorted(at), name
        keys = [k for k in ex if k in order]
        assert keys == order, keys
        m = _metrics(d / (name + ".metrics.json.gz"))
        for zm, (_, st, _) in lib.items():
            if st in NAMES:
                assert m[f"m1/{zm}"]["status"] == NAMES[st], (name, zm, st, m[f"m1/{zm}"])
                assert m[f"m1/{zm}"]["predicted_accuracy"] == -1.0
        assert sum(ex.values()) - ex.get("ZMW with full-length subread", 0) == rep["zmws_fail_filters"]               # a ZMW is counted once
    assert json.load(open(d / "on.json"))["zmws_pass_filters"] == len(on)
    n_gated = sum(11 <= st <= 14 for _, st, _ in lib.values())
    assert f", {n_gated} ZMWs failed the coverage filters" in open(d / "on.log").read()


@pytest.mark.gpu
def test_fail_reads_write_the_gated_zmws_as_full_length_subreads(runs):
    zmws, lib, d = runs
    gated = {zm for zm, (_, st, _) in lib.items() if 11 <= st <= 14}
    _, fr_off = _records(d / "fr_off.bam")
    _, fr = _records(d / "fr.bam")
    _, fail_off = _records(d / "fr_off.fail.bam")
    _, fail = _records(d / "fr.fail.bam")
    assert [x for r, x in fr_off if r["tags"]["zm"] not in gated] == [x for _, x in fr]
    old = {r["tags"]["zm"]: x for r, x in fail_off}
    got = {r["tags"]["zm"]: (r, x) for r, x in fail}
    assert set(got) >= gated and set(got) - gated == set(old) - gated
    for zm, (r, x) in got.items():
        if zm in gated:
            assert r["tags"]["ff"] == 0x8 and r["tags"]["rq"] == -1.0 and not r["name"].endswith("/ccs"), (zm, r["name"], r["tags"])
        else:
            assert x == old[zm]
    order = [r["tags"]["zm"] for r, _ in fail]
    assert order == sorted(order)
    pbi = bam_util.read_pbi(str(d / "fr.fail.bam") + ".pbi")
    assert np.array_equal(pbi["file_offset"], bam_util.record_virtual_offsets(d / "fr.fail.bam")) and list(pbi["hole"]) == order
    assert json.load(open(d / "fr.json"))["exclusive_failed_counts"]["ZMW with full-length subread"] >= len(gated)


@pytest.mark.gpu
def test_independent_of_workers_batch_size_and_chunks(runs):
    _, _, d = runs
    on = [x for _, x in _records(d / "on.bam")[1]]
    assert on == [x for _, x in _records(d / "on2.bam")[1]]
    assert json.load(open(d / "on.json")) == json.load(open(d / "on2.json"))
    syn = [x for _, x in _records(d / "syn_on.bam")[1]]
    assert len(syn) == 12 and syn == [x for _, x in _records(d / "c1.bam")[1]] + [x for _, x in _records(d / "c2.bam")[1]]
    c1, c2, whole = (json.load(open(d / f"{n}.json"))["exclusive_failed_counts"] for n in ("c1", "c2", "syn_on"))
    assert list(c1) == list(whole) and {k: c1[k] + c2[k] for k in whole} == whole


@pytest.mark.gpu
def test_overrides_and_by_strand(runs):
    zmws, lib, d = runs
    kind = {zm: k for zm, k, _ in zmws}
    # --coverage-block 400: a 300-base block is no block; what the library says under the same options is what leaves
    lib2 = _library(zmws, block=400, drop_percent=40)
    gated2 = {zm for zm, (_, st, _) in lib2.items() if 11 <= st <= 14}
    assert not any(kind[zm] in ("block300", "block100") for zm in gated2) and any(kind[zm] == "unique_blocks" for zm in gated2)
    _, off = _records(d / "off.bam")
    _, blk = _records(d / "blk.bam")
    assert [x for r, x in off if r["tags"]["zm"] not in gated2] == [x for _, x in blk]
    assert json.load(open(d / "blk.json"))["exclusive_failed_counts"]["Coverage drops"] == 0
    # --by-strand: every strand entity is screened on its own (four passes per strand); both strands of the clean ZMWs come out, every entity has a status
    _, bs = _records(d / "bs.bam")
    assert all(r["name"].endswith(("/fwd", "/rev")) for r, _ in bs)
    zs = [r["tags"]["zm"] for r, _ in bs]
    assert sum(kind[z] == "clean" for z in zs) >= 8
    m = _metrics(d / "bs.metrics.json.gz")
    for zm, k in kind.items():
        if k in ("clean", "block300", "block100", "block300_2of8"):
            assert f"m1/{zm}/fwd" in m and f"m1/{zm}/rev" in m
    # the block sits in passes 4 .. 7: two of the four passes of either strand
    assert any(m[f"m1/{zm}/{s}"]["status"] == "COVERAGE_DROPS" for zm, k in kind.items() if k == "block300" for s in ("fwd", "rev"))

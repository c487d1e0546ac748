"""ccs --adapters FILE.fasta|default (DESIGN.md §2 "Adapter screen", §7; docs/faq/fail-reads.md fail classes 0x10 and 0x40): the option's usage errors, and on an
MI355X a subreads BAM of adapter dimers, short-arm near-end ZMWs, adapter-bearing palindromes, interior-adapter, low-rq and normal ZMWs: without the option the
outputs are those of --fail-reads alone; with it the main output loses exactly the ZMWs with a verdict, FAIL.bam gains them with ff 0x10 / 0x40, the index, report
rows, JSON keys and metrics agree with the records, and the output does not depend on the number of packing threads or the batch size.

Which planted ZMWs reach a consensus was decided with the oracle on the CPU for the seeds below (tests/oracle_lib.py consensus_batch on the same passes): all 21
of the test-adapter set and all 6 of the built-in-adapter set end as SUCCESS or LOW_RQ, so every planted ZMW is tested and the sets below are asserted whole."""
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
BITS = {"dimer": 0x50, "near_end": 0x40, "palindrome": 0x20, "interior": 0, "normal": 0, "lowrq": 0}


def _fasta(path, recs):
    path.write_text("".join(f">{n}\n{s}\n" for n, s in recs))
    return path


# ---------------------------------------------------------------- CPU: usage
def test_adapters_needs_fail_reads(built, tmp_path):
    for a in ("default", "x.fasta"):
        p = subprocess.run([CCS, "in.bam", "out.bam", "--adapters", a], capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert p.returncode == 2 and "--adapters" in p.stderr and "--fail-reads" in p.stderr
    p = subprocess.run([CCS, "in.bam", "out.bam", "--adapters", "default", "--fail-reads", "f.bam", "--by-strand"], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert p.returncode == 2 and "not supported" in p.stderr
    usage = subprocess.run([CCS, "--help"], capture_output=True, text=True, timeout=60).stderr
    assert "--adapters" in usage and "default" in usage


def test_bad_fasta_names_the_record(built, tmp_path):
    good = "ACGTTGCAAGGCTTAACCGGTTAGC"
    cases = [([(f"a{k}", good) for k in range(9)], "record 9 (>a8)", "more than 8"),
             ([("first", good), ("short one", good[:15])], "record 2 (>short one)", "15 bases"),
             ([("first", good), ("second", good), ("withN", good[:10] + "N" + good[10:])], "record 3 (>withN)", "'N'"),
             ([("long", good * 3)], "record 1 (>long)", "more than 64")]
    for recs, where, what in cases:
        f = _fasta(tmp_path / "bad.fasta", recs)
        p = subprocess.run([CCS, "in.bam", "out.bam", "--fail-reads", "f.bam", "--adapters", str(f)], capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert p.returncode == 2 and where in p.stderr and what in p.stderr, p.stderr
    p = subprocess.run([CCS, "in.bam", "out.bam", "--fail-reads", "f.bam", "--adapters", "missing.fasta"], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert p.returncode == 2 and "missing.fasta" in p.stderr
    (tmp_path / "empty.fasta").write_text("\n")
    p = subprocess.run([CCS, "in.bam", "out.bam", "--fail-reads", "f.bam", "--adapters", "empty.fasta"], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert p.returncode == 2 and "no FASTA record" in p.stderr


# ---------------------------------------------------------------- GPU
def _zmws(adapter, counts, seed, zm0):
    """(zm, kind, passes as (bases, pw, ipd, full)) of every ZMW.  dimer: 10-30 copies of the adapter in one orientation (no inverted repeat: k_fold stays
    silent) with spacers of 0-60 bases; near_end: the short-arm X·A·rc(X) of adapter_synth; palindrome: arms of 1000-1500 bases around the adapter; interior;
    normal; lowrq: 3 noisy passes of a random template"""
    import adapter_synth as S
    import lowcx
    rng = np.random.default_rng(seed)
    A = S.encode(adapter)
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
    for kind, n in counts:
        for _ in range(n):
            L = int(rng.integers(2000, 3200))
            if kind == "dimer":
                parts = []
                for _ in range(int(rng.integers(10, 31))):
                    parts += [A, rnd(rng.integers(0, 61))]
                t = np.concatenate(parts[:-1])
            elif kind in ("near_end", "interior", "palindrome"):
                t = S.template(rng, kind, L, A)
            else:
                t = rnd(L)
            out.append((zm, kind, passes(t, 3, 2.0) if kind == "lowrq" else passes(t, 8)))
            zm += 1
    return out


TEST_COUNTS = (("dimer", 4), ("near_end", 4), ("palindrome", 3), ("interior", 3), ("normal", 4), ("lowrq", 3))
BUILTIN_COUNTS = (("dimer", 2), ("near_end", 2), ("normal", 2))


@pytest.fixture(scope="module")
def runs(tmp_path_factory, built):
    import adapter_synth as S
    d = tmp_path_factory.mktemp("adapters")
    zmws = _zmws(S.TEST_ADAPTER, TEST_COUNTS, 2031, 300)
    bam = d / "in.subreads.bam"
    _write(bam, zmws)
    fa = _fasta(d / "adapters.fasta", [("decoy a random 25-mer", "ACGTTGCAAGGCTTAACCGGTTAGC"), ("test_adapter", S.TEST_ADAPTER.lower())])
    common = ["--min-rq", MIN_RQ, "--min-passes", "3"]
    _ccs(bam, d / "off.bam", *common)
    _ccs(bam, d / "fr.bam", *common, "--fail-reads", d / "fr.fail.bam", "--report-json", d / "fr.json")
    _ccs(bam, d / "on.bam", *common, "--fail-reads", d / "fail.bam", "--adapters", fa, "--report-json", d / "on.json", "--report-file", d / "on.txt",
         "--metrics-json", d / "on.metrics.json.gz")
    _ccs(bam, d / "on2.bam", *common, "--fail-reads", d / "fail2.bam", "--adapters", fa, "--workers-per-gpu", "1", "--batch-size", "5")
    zb = _zmws(S.SMRTBELL, BUILTIN_COUNTS, 2032, 500)
    _write(d / "builtin.subreads.bam", zb)
    _ccs(d / "builtin.subreads.bam", d / "b.bam", *common, "--fail-reads", d / "b.fail.bam", "--adapters", "default")
    _ccs(d / "builtin.subreads.bam", d / "b_off.bam", *common, "--fail-reads", d / "b_off.fail.bam")
    return zmws, zb, d


@pytest.mark.gpu
def test_without_the_option_nothing_changes(runs):
    zmws, _, d = runs
    _, off = _records(d / "off.bam")
    _, fr = _records(d / "fr.bam")
    _, ffr = _records(d / "fr.fail.bam")
    assert {r["tags"]["ff"] for r, _ in ffr} <= {0x1, 0x8, 0x20, 0x21}
    pal = {r["tags"]["zm"] for r, _ in ffr if r["tags"]["ff"] & 0x20}
    assert pal == {zm for zm, kind, _ in zmws if kind == "palindrome"}
    assert [x for r, x in off if r["tags"]["zm"] not in pal] == [x for _, x in fr]
    ex = json.load(open(d / "fr.json"))["exclusive_failed_counts"]
    assert "CCS adapter concatenation" not in ex and "CCS adapter near end" not in ex


@pytest.mark.gpu
def test_main_output_loses_exactly_the_flagged_zmws(runs):
    zmws, _, d = runs
    _, fr = _records(d / "fr.bam")
    _, ffr = _records(d / "fr.fail.bam")
    text_on, on = _records(d / "on.bam")
    _, fail = _records(d / "fail.bam")
    kind = {zm: k for zm, k, _ in zmws}
    flagged = {r["tags"]["zm"] for r, _ in fail if r["tags"]["ff"] & 0x50}
    assert flagged == {zm for zm, k in kind.items() if k in ("dimer", "near_end")}            # every planted one, nothing else
    assert [x for r, x in fr if r["tags"]["zm"] not in flagged] == [x for _, x in on]           # the others byte for byte
    assert {r["tags"]["zm"] for r, _ in on} >= {zm for zm, k in kind.items() if k in ("interior", "normal")} - \
        {r["tags"]["zm"] for r, _ in ffr}                                                        # (those below --min-rq were fail reads before)
    assert text_on == bam_util.read_bam(d / "fail.bam")[0]
    # FAIL.bam: what --fail-reads alone wrote, byte for byte, plus the flagged ZMWs in input order
    old = {r["tags"]["zm"]: x for r, x in ffr}
    order = [r["tags"]["zm"] for r, _ in fail]
    assert order == sorted(order) and set(order) == set(old) | flagged
    for r, x in fail:
        t = r["tags"]
        if not t["ff"] & 0x50:
            assert x == old[t["zm"]]
            continue
        assert r["name"] == f"m1/{t['zm']}/ccs" and t["ff"] & ~0x1 == BITS[kind[t["zm"]]], (t["zm"], kind[t["zm"]], hex(t["ff"]))
        assert bool(t["ff"] & 0x1) == (t["rq"] < float(MIN_RQ))
    for r, _ in fail:                                                                             # palindromes with the adapter at the fold: 0x20, no 0x40
        if kind[r["tags"]["zm"]] == "palindrome":
            assert r["tags"]["ff"] & ~0x1 == 0x20


@pytest.mark.gpu
def test_index_reports_and_metrics(runs):
    zmws, _, d = runs
    _, fail = _records(d / "fail.bam")
    _, on = _records(d / "on.bam")
    pbi = bam_util.read_pbi(str(d / "fail.bam") + ".pbi")
    assert np.array_equal(pbi["file_offset"], bam_util.record_virtual_offsets(d / "fail.bam"))
    assert list(pbi["hole"]) == [r["tags"]["zm"] for r, _ in fail]
    pbi = bam_util.read_pbi(str(d / "on.bam") + ".pbi")
    assert np.array_equal(pbi["file_offset"], bam_util.record_virtual_offsets(d / "on.bam"))
    assert list(pbi["hole"]) == [r["tags"]["zm"] for r, _ in on]
    ff = {r["tags"]["zm"]: r["tags"]["ff"] for r, _ in fail}
    pal = {z for z, f in ff.items() if f & 0x20}
    con = {z for z, f in ff.items() if f & 0x10} - pal
    near = {z for z, f in ff.items() if f & 0x40} - pal - con
    assert len(con) == 4 and len(near) == 4 and len(pal) == 3
    rep = json.load(open(d / "on.json"))
    ex = rep["exclusive_failed_counts"]
    assert ex["CCS adapter palindrome"] == len(pal) and ex["CCS adapter concatenation"] == len(con) and ex["CCS adapter near end"] == len(near)
    assert rep["zmws_pass_filters"] == len(on)
    txt = open(d / "on.txt").read()
    assert f"CCS adapter concatenation     : {len(con)} (" in txt and f"CCS adapter near end          : {len(near)} (" in txt
    with gzip.open(d / "on.metrics.json.gz", "rt") as f:
        m = {x["zmw"]: x for x in json.load(f)["zmws"]}
    for name, zs in (("ADAPTER_PALINDROME", pal), ("ADAPTER_CONCATENATION", con), ("ADAPTER_NEAR_END", near)):
        assert {k for k, v in m.items() if v["status"] == name} == {f"m1/{z}" for z in zs}, name


@pytest.mark.gpu
def test_independent_of_workers_and_batch_size(runs):
    _, _, d = runs
    assert [x for _, x in _records(d / "on.bam")[1]] == [x for _, x in _records(d / "on2.bam")[1]]
    assert [x for _, x in _records(d / "fail.bam")[1]] == [x for _, x in _records(d / "fail2.bam")[1]]


@pytest.mark.gpu
def test_the_builtin_adapter(runs):
    _, zb, d = runs
    kind = {zm: k for zm, k, _ in zb}
    _, off = _records(d / "b_off.bam")
    _, on = _records(d / "b.bam")
    _, fail = _records(d / "b.fail.bam")
    flagged = {r["tags"]["zm"]: r["tags"]["ff"] for r, _ in fail if r["tags"]["ff"] & 0x50}
    assert set(flagged) == {zm for zm, k in kind.items() if k in ("dimer", "near_end")}
    assert all(f & ~0x1 == BITS[kind[z]] for z, f in flagged.items()), flagged
    assert [x for r, x in off if r["tags"]["zm"] not in flagged] == [x for _, x in on]

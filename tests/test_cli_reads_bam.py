"""ccs --reads-bam on an MI355X (DESIGN.md §2 "Representative rule", §7; the reference's --all, docs/faq/mode-all.md): a --write-synthetic input of six ZMWs that
polish, with hand-built ZMWs around them — one full-length subread, one-adapter subreads only, a subread with no adapter flag, four full-length passes of
unrelated sequence.  One record per ZMW in input order; rq -1 and all-'+' qualities on exactly the draft and subread records; subread bases unaltered; kinetics
tags where the rule says; the index, the report, the JSON and the metrics file agree with the records; without the option the output is what the same filters
give without it; the refusals (no GPU needed)."""
import gzip
import json
import subprocess

import numpy as np
import pytest

import bam_util
from test_cli_fail_reads import CCS, _ccs, _records

MOVIE = "m64000_synth"
FIXED = ["--min-passes", "2", "--min-rq", "0", "--max-length", str(65535 + 65535 // 4 + 64)]   # what --reads-bam sets


def _rec(zm, q, bases, cx, rng):
    return bam_util.record(f"{MOVIE}/{zm}/{q}_{q + len(bases)}", "".join("ACGT"[c] for c in bases),
                           [("zm", "i", zm), ("sn", "Bf", [9.0, 16.0, 8.0, 13.0]), ("pw", "BC", rng.integers(1, 4, len(bases)).astype(np.uint8)),
                            ("ip", "BC", rng.integers(1, 61, len(bases)).astype(np.uint8)), ("cx", "i", cx)])


def _hand_built():
    """zm -> (kind, [(bases, cx)]): cx 3 = adapters on both sides, 1 / 2 = one adapter, 0 = none; 16 / 32 = forward / reverse pass"""
    rng = np.random.default_rng(41)
    rnd = lambda L: rng.integers(0, 4, L).astype(np.uint8)
    return {500: ("single", [(rnd(311), 3 | 16)]),
            501: ("partial_only", [(rnd(180), 2 | 16), (rnd(260), 1 | 32)]),
            2000: ("cx0", [(rnd(277), 16)]),
            2001: ("unrelated", [(rnd(300 + 17 * k), 3 | (32 if k & 1 else 16)) for k in range(4)])}


@pytest.fixture(scope="module")
def runs(tmp_path_factory, built):
    d = tmp_path_factory.mktemp("reads_bam")
    _ccs("--write-synthetic", "6,5,400,3", d / "synth.bam")
    text, raw = bam_util.read_bam_raw_records(d / "synth.bam")
    rng = np.random.default_rng(43)
    hand = _hand_built()

    def recs(zm):
        out, q = [], 0
        for b, cx in hand[zm][1]:
            out.append(_rec(zm, q, b, cx, rng)); q += len(b) + 45
        return out
    bam = d / "in.subreads.bam"
    bam_util.write_bam(bam, text, recs(500) + recs(501) + raw + recs(2000) + recs(2001))
    rep = lambda k: ["--report-json", d / f"{k}.json", "--report-file", d / f"{k}.txt", "--metrics-json", d / f"{k}.metrics.json.gz"]
    _ccs(bam, d / "off.bam", *FIXED, *rep("off"))
    _ccs(bam, d / "on.bam", "--reads-bam", *rep("on"))
    _ccs(bam, d / "on2.bam", "--reads-bam", "--workers-per-gpu", "1", "--batch-size", "3")
    _ccs(bam, d / "kin.bam", "--reads-bam", "--reads-bam-kinetics")
    _ccs(bam, d / "hk.bam", *FIXED, "--hifi-kinetics")
    _ccs(bam, d / "fb.bam", "--reads-bam", "--reads-bam-subread-fallback")
    _ccs(bam, d / "on.fastq.gz", "--reads-bam")
    subreads = {}
    for r in bam_util.read_bam(bam)[1]:
        subreads.setdefault(r["tags"]["zm"], []).append(r)
    return d, hand, subreads


ORDER = [500, 501] + list(range(1000, 1006)) + [2000, 2001]


def _unpolished(r):
    return r["tags"]["rq"] == -1.0


@pytest.mark.gpu
def test_one_record_per_zmw_in_input_order(runs):
    d, hand, subreads = runs
    _, on = _records(d / "on.bam")
    assert [r["tags"]["zm"] for r, _ in on] == ORDER and all(r["name"] == f"{MOVIE}/{r['tags']['zm']}/ccs" for r, _ in on)
    for r, _ in on:
        zm = r["tags"]["zm"]
        assert {"zm", "RG", "sn", "np", "rq"} <= set(r["tags"])
        if zm in hand:                                               # rq -1 and all-'+' qualities (QV 10) on exactly the draft / subread records
            assert _unpolished(r) and (r["qual"] == 10).all() and "ec" not in r["tags"] and len(r["seq"]) > 0, zm
        else:
            assert r["tags"]["rq"] >= 0 and "ec" in r["tags"] and not (r["qual"] == 10).all(), zm
        assert "fi" not in r["tags"]
    by = {r["tags"]["zm"]: r for r, _ in on}
    for zm, want in ((500, 0), (501, 1), (2000, 0)):                 # subread bases unaltered; of two one-adapter subreads: rank 1 by length, the longer
        assert np.array_equal(by[zm]["seq"], subreads[zm][want]["seq"]), zm
    assert [x for _, x in on] == [x for _, x in _records(d / "on2.bam")[1]]                 # independent of packing threads and batch size


@pytest.mark.gpu
def test_fallback_and_kinetics_where_the_rule_says(runs):
    d, hand, subreads = runs
    by = lambda p: {r["tags"]["zm"]: r for r, _ in _records(d / p)[1]}
    on, fb, kin, hk = by("on.bam"), by("fb.bam"), by("kin.bam"), by("hk.bam")
    assert list(fb) == ORDER and list(kin) == ORDER
    lens = [len(s["seq"]) for s in subreads[2001]]                   # the unrelated passes: a draft without the fallback, with it the pass of rank 2 of 4
    want = sorted((l, q) for q, l in enumerate(lens))[2][1]
    assert np.array_equal(fb[2001]["seq"], subreads[2001][want]["seq"]) and _unpolished(fb[2001])
    assert all(np.array_equal(fb[zm]["seq"], on[zm]["seq"]) for zm in ORDER if zm != 2001)
    for zm in ORDER:
        t = kin[zm]["tags"]
        if zm == 2001:                                               # an unpolished draft: no kinetics
            assert not {"fi", "fp", "ri", "rp", "fn", "rn"} & set(t)
        elif zm in hand:                                             # a subread: its own ip / pw as fi / fp, fn 1, rn 0
            src = subreads[zm][{500: 0, 501: 1, 2000: 0}[zm]]["tags"]
            assert np.array_equal(t["fi"], src["ip"]) and np.array_equal(t["fp"], src["pw"]) and t["fn"] == 1 and t["rn"] == 0 and "ri" not in t and "rp" not in t
        else:                                                        # a polished read: what --hifi-kinetics gives
            assert {k: np.asarray(v).tolist() for k, v in t.items()} == {k: np.asarray(v).tolist() for k, v in hk[zm]["tags"].items()}, zm
        assert np.array_equal(kin[zm]["seq"], on[zm]["seq"])


@pytest.mark.gpu
def test_index_reports_and_fastq_agree_with_the_records(runs):
    d, hand, subreads = runs
    _, on = _records(d / "on.bam")
    pbi = bam_util.read_pbi(str(d / "on.bam") + ".pbi")
    assert np.array_equal(pbi["file_offset"], bam_util.record_virtual_offsets(d / "on.bam"))
    assert pbi["hole"].tolist() == ORDER and pbi["q_end"].tolist() == [len(r["seq"]) for r, _ in on]
    assert pbi["read_qual"].tolist() == [r["tags"]["rq"] for r, _ in on]
    want = {"polished": 6, "draft": 1, "subread": 3}
    j, j0 = json.load(open(d / "on.json")), json.load(open(d / "off.json"))
    assert j["representative_reads"] == want and "representative_reads" not in j0
    txt, txt0 = open(d / "on.txt").read(), open(d / "off.txt").read()
    for label, c in (("Polished reads", 6), ("Unpolished drafts", 1), ("Unaltered subreads", 3)):
        assert f"{label:<30}: {c}" in txt
    assert "Representative" not in txt0 and txt[txt.index("HiFi Reads"):] == txt0[txt0.index("HiFi Reads"):]   # HiFi statistics: the polished reads only
    m, m0 = json.load(gzip.open(d / "on.metrics.json.gz")), json.load(gzip.open(d / "off.metrics.json.gz"))
    assert m["representative_reads"] == want and "representative_reads" not in m0 and len(m["zmws"]) == len(ORDER)
    fq = gzip.open(d / "on.fastq.gz", "rt").read().splitlines()
    assert fq[0::4] == [f"@{MOVIE}/{zm}/ccs" for zm in ORDER]
    for (r, _), s, q in zip(on, fq[1::4], fq[3::4]):
        assert s == "".join("ACGT"[c] for c in r["seq"]) and (set(q) == {"+"}) == _unpolished(r)


@pytest.mark.gpu
def test_without_the_option_nothing_changes(runs):
    """the same filters without --reads-bam: the polished records byte for byte, no record for the others"""
    d, hand, subreads = runs
    _, on = _records(d / "on.bam")
    _, off = _records(d / "off.bam")
    assert [x for r, x in on if r["tags"]["zm"] not in hand] == [x for _, x in off] and len(off) == 6


@pytest.mark.parametrize("args,words", [
    (["--reads-bam", "--min-passes", "3"], "can't be changed"), (["--min-rq", "0.9", "--reads-bam"], "can't be changed"),
    (["--reads-bam", "--max-length", "9000"], "can't be changed"), (["--reads-bam", "--by-strand"], "not supported"),
    (["--fail-reads", "f.bam", "--reads-bam"], "not supported"), (["--reads-bam", "--coverage-filters"], "not supported"),
    (["--reads-bam", "--barcodes", "b.fasta"], "not supported"), (["--reads-bam", "--fit-model", "m.json"], "not supported"),
    (["--reads-bam-kinetics"], "need --reads-bam"), (["--reads-bam-subread-fallback"], "need --reads-bam")])
def test_refusals(built, tmp_path, args, words):
    p = subprocess.run([CCS, "in.bam", "out.bam", *args], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert p.returncode == 2 and words in p.stderr, p.stderr


def test_usage_names_the_options(built):
    usage = subprocess.run([CCS, "--help"], capture_output=True, text=True, timeout=60).stderr
    assert all(k in usage for k in ("--reads-bam ", "--reads-bam-kinetics", "--reads-bam-subread-fallback"))

"""ccs --min-tandem-repeat-length (docs/faq/low-complexity.md:8-18, docs/faq/reports-aux-files.md:22,115): the option's usage errors, and on an
MI355X a BAM of planted-tract and random ZMWs: has_tandem_repeat and the report row agree with the library on the same passes, flagged ZMWs'
records equal a --disable-heuristics run's, the others a default run's, alone and combined with the other modes."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

from ccs_amd import api
import bam_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CCS = os.path.join(ROOT, "ccs_amd", "bin", "ccs")
HDR = ("@HD\tVN:1.6\tSO:unknown\tpb:5.0.0\n@RG\tID:x\tPL:PACBIO\tDS:READTYPE=SUBREAD;Ipd:CodecV1=ip;PulseWidth:CodecV1=pw;"
       "BINDINGKIT=101-789-500;SEQUENCINGKIT=101-826-100;BASECALLERVERSION=5.0.0;FRAMERATEHZ=100.000000\tPU:m1\tPM:SEQUELII\n")
ZM0 = 100
THR = 600


def _ccs(*args, check=True):
    return subprocess.run([CCS, *map(str, args)], capture_output=True, text=True, check=check, timeout=900)


@pytest.mark.parametrize("val", [None, "0", "-5", "abc", "12x"])
def test_bad_values_are_usage_errors(built, tmp_path, val):
    args = [CCS, "in.bam", "out.bam", "--min-tandem-repeat-length"] + ([] if val is None else [val])
    p = subprocess.run(args, capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert p.returncode == 2 and "--min-tandem-repeat-length" in p.stderr


def test_option_is_documented(built):
    usage = subprocess.run([CCS, "--help"], capture_output=True, text=True, timeout=60).stderr
    assert "--min-tandem-repeat-length" in usage and "1000" in usage


def _write_bam(path, b):
    recs = []
    for z in range(b.n_zmw):
        for r in range(int(b.read_off[z]), int(b.read_off[z + 1])):
            bases, pw = b.read(r)
            ipd = b.ipd[int(b.base_off[r]):int(b.base_off[r + 1])]
            k = r - int(b.read_off[z])
            n = len(bases)
            recs.append(bam_util.record(f"m1/{ZM0 + z}/{k * 20000}_{k * 20000 + n}", "".join("ACGT"[c] for c in bases),
                                        [("zm", "i", ZM0 + z), ("sn", "Bf", [float(v) for v in b.snr[z]]), ("pw", "BC", pw), ("ip", "BC", ipd),
                                         ("cx", "i", 3 | (32 if k & 1 else 16))]))
    bam_util.write_bam(path, HDR, recs)


def _metrics(path):
    with gzip.open(path, "rt") as f:
        return {m["zmw"]: m for m in json.load(f)["zmws"]}


def _records(path):
    _, raw = bam_util.read_bam_raw_records(path)
    _, recs = bam_util.read_bam(path)
    return {r["name"]: bytes(x) for r, x in zip(recs, raw)}


@pytest.fixture(scope="module")
def tract_bam(tmp_path_factory, built):
    import tandem_synth
    b, tracts = tandem_synth.make(24, 8, (2500, 4000), seed=77, frac=0.5, tract=(500, 1800))
    d = tmp_path_factory.mktemp("tandem_cli")
    bam = d / "t.subreads.bam"
    _write_bam(bam, b)
    return b, tracts, bam, d


def _check_split(d, tag, extra, flagged_names):
    """the run with the option equals the --disable-heuristics run on flagged entities and the default run on the rest"""
    on, off, dis = (_records(d / f"{tag}_{k}.bam") for k in ("on", "off", "dis"))
    assert set(on) == {n for n in set(off) | set(dis) if (n in dis if n in flagged_names else n in off)}
    for n, rec in on.items():
        assert rec == (dis[n] if n in flagged_names else off[n]), (tag, n)


@pytest.mark.gpu
def test_cli_flags_match_the_library_and_switch_heuristics_per_zmw(tract_bam):
    b, tracts, bam, d = tract_bam
    h = api.Handle(0)
    _, tl, _ = h.consensus_extras(b, tandem=True)
    h.close()
    want = {f"m1/{ZM0 + z}" for z in range(b.n_zmw) if tl[z] >= THR}
    assert 0 < len(want) < b.n_zmw
    _ccs(bam, d / "a_off.bam", "--metrics-json", d / "a_off.json.gz", "--report-file", d / "a_off.txt")
    _ccs(bam, d / "a_dis.bam", "--disable-heuristics", "--suppress-reports")
    _ccs(bam, d / "a_on.bam", "--min-tandem-repeat-length", THR, "--metrics-json", d / "a_on.json.gz", "--report-file", d / "a_on.txt",
         "--report-json", d / "a_on.rep.json", "--log-level", "INFO")
    m = _metrics(d / "a_on.json.gz")
    assert {k for k, v in m.items() if v["has_tandem_repeat"]} == want
    assert not any(v["has_tandem_repeat"] for v in _metrics(d / "a_off.json.gz").values())
    rep = (d / "a_on.txt").read_text()
    row = f"ZMWs with tandem repeats      : {len(want)} ({100.0 * len(want) / b.n_zmw:.2f}%)"
    assert row in rep
    lines = rep.split("\n")
    assert lines.index(row) == lines.index("Exclusive failed counts") - 2 and lines[lines.index(row) - 1] == ""
    assert "tandem" not in (d / "a_off.txt").read_text()                       # default reports are unchanged
    assert json.loads((d / "a_on.rep.json").read_text())["zmws_with_tandem_repeats"] == len(want)
    _check_split(d, "a", [], {n + "/ccs" for n in want})


@pytest.mark.gpu
def test_cli_by_strand_and_other_modes(tract_bam):
    b, tracts, bam, d = tract_bam
    # --by-strand: every strand is its own entity with its own draft and flag
    for k, flags in (("off", []), ("dis", ["--disable-heuristics"]), ("on", ["--min-tandem-repeat-length", THR])):
        _ccs(bam, d / f"s_{k}.bam", "--by-strand", "--min-rq", 0.9, "--metrics-json", d / f"s_{k}.json.gz", "--report-file", d / f"s_{k}.txt", *flags)
    m = _metrics(d / "s_on.json.gz")
    flagged = {k for k, v in m.items() if v["has_tandem_repeat"]}
    assert flagged and all(k.endswith(("/fwd", "/rev")) for k in flagged)
    names = {n.rsplit("/", 1)[0] + "/ccs/" + n.rsplit("/", 1)[1] for n in flagged}
    _check_split(d, "s", [], names)
    # kinetics + pileup summary + two workers on one device + small batches: the same split
    common = ["--hifi-kinetics", "--pileup-summary", "--gpus", "0,0", "--workers-per-gpu", 2, "--batch-size", 5, "--suppress-reports"]
    _ccs(bam, d / "k_off.bam", *common)
    _ccs(bam, d / "k_dis.bam", *common, "--disable-heuristics")
    _ccs(bam, d / "k_on.bam", *common, "--min-tandem-repeat-length", THR, "--metrics-json", d / "k_on.json.gz")
    m = _metrics(d / "k_on.json.gz")
    _check_split(d, "k", [], {k + "/ccs" for k, v in m.items() if v["has_tandem_repeat"]})
    # --chunk (needs the input's .pbi: the synthetic BAM has one) and FASTQ output: the chunks' flags add up to the whole run's.  At 7 bases (a
    # homopolymer of 7) about a third of random 3 kb drafts are flagged
    syn = d / "syn.subreads.bam"
    _ccs("--write-synthetic", "48,6,3000,5", syn)
    _ccs(syn, d / "whole.fastq.gz", "--min-tandem-repeat-length", 7, "--report-file", d / "whole.txt", "--metrics-json", d / "whole.json.gz")
    whole = sum(v["has_tandem_repeat"] for v in _metrics(d / "whole.json.gz").values())
    total = 0
    for i in (1, 2):
        _ccs(syn, d / f"c{i}.fastq.gz", "--chunk", f"{i}/2", "--min-tandem-repeat-length", 7, "--report-file", d / f"c{i}.txt",
             "--metrics-json", d / f"c{i}.json.gz")
        total += sum(v["has_tandem_repeat"] for v in _metrics(d / f"c{i}.json.gz").values())
        assert "ZMWs with tandem repeats" in (d / f"c{i}.txt").read_text()
        with gzip.open(d / f"c{i}.fastq.gz", "rt") as f:
            assert f.read().count("\n+\n") > 0
    assert 0 < total == whole

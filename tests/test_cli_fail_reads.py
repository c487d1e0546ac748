"""ccs --fail-reads FAIL.bam (docs/faq/fail-reads.md, docs/faq/reports-aux-files.md:39-41): the option's usage errors, and on an MI355X a BAM of adapter
palindromes, low-rq ZMWs with few passes, ZMWs with one or two full passes and normal ZMWs: the main output loses exactly the palindromes, FAIL.bam holds one
record per ZMW without a HiFi read that has a consensus (ff 0x1 / 0x20) or a full pass (ff 0x8, the median full-length subread), its .pbi matches, the report
rows and metrics agree, and the output does not depend on the number of packing threads or the batch size."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

import bam_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CCS = os.path.join(ROOT, "ccs_amd", "bin", "ccs")
HDR = ("@HD\tVN:1.6\tSO:unknown\tpb:5.0.0\n@RG\tID:x\tPL:PACBIO\tDS:READTYPE=SUBREAD;Ipd:CodecV1=ip;PulseWidth:CodecV1=pw;"
       "BINDINGKIT=101-789-500;SEQUENCINGKIT=101-826-100;BASECALLERVERSION=5.0.0;FRAMERATEHZ=100.000000\tPU:m1\tPM:SEQUELII\n")
MIN_RQ = "0.999"


def _ccs(*args, check=True, cwd=None):
    return subprocess.run([CCS, *map(str, args)], capture_output=True, text=True, check=check, timeout=900, cwd=cwd)


@pytest.mark.parametrize("path", ["fail.fastq.gz", "fail", "fail.sam", ".bam"])
def test_fail_reads_needs_a_bam_path(built, tmp_path, path):
    p = subprocess.run([CCS, "in.bam", "out.bam", "--fail-reads", path], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert p.returncode == 2 and "--fail-reads" in p.stderr and ".bam" in p.stderr


def test_fail_reads_with_by_strand_is_refused(built, tmp_path):
    for order in (["--by-strand", "--fail-reads", "f.bam"], ["--fail-reads", "f.bam", "--by-strand"]):
        p = subprocess.run([CCS, "in.bam", "out.bam", *order], capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert p.returncode == 2 and "not supported" in p.stderr
    usage = subprocess.run([CCS, "--help"], capture_output=True, text=True, timeout=60).stderr
    assert "--fail-reads" in usage


# ---------------------------------------------------------------- GPU
def _zmws():
    """(zm, kind, passes as (bases, pw, ipd, full)) of every ZMW: 6 palindromes, 6 low-pass noisy ZMWs, 3 with one full pass, 2 with two full passes of
    different lengths, 6 normal ZMWs"""
    import fold_synth
    import lowcx
    rng = np.random.default_rng(2027)
    out = []

    def passes(t, n, channel=1.0):
        ps = []
        for k in range(n):
            b, p = lowcx.sequence_read(rng, t, channel)
            if k & 1:
                b, p = (3 - b[::-1]).astype(np.uint8), p[::-1]
            ps.append((b, p, rng.integers(1, 61, len(b)).astype(np.uint8), True))
        return ps
    zm = 200
    for kind, n in (("palindrome", 6), ("lowrq", 6), ("one", 3), ("two", 2), ("normal", 6)):
        for _ in range(n):
            L = int(rng.integers(2000, 3200))
            if kind == "palindrome":
                t, _ = fold_synth.template(rng, "palindrome", L)
                ps = passes(t, 8)
            elif kind == "lowrq":
                ps = passes(rng.integers(0, 4, L).astype(np.uint8), 3, channel=2.0)
            elif kind == "one":
                ps = passes(rng.integers(0, 4, L).astype(np.uint8), 1)
            elif kind == "two":
                ps = passes(rng.integers(0, 4, L).astype(np.uint8), 2)
            else:
                ps = passes(rng.integers(0, 4, L).astype(np.uint8), 8)
            out.append((zm, kind, ps))
            zm += 1
    return out


def _write(path, zmws):
    recs = []
    for zm, _, ps in zmws:
        q = 0
        for k, (b, p, ip, _) in enumerate(ps):
            recs.append(bam_util.record(f"m1/{zm}/{q}_{q + len(b)}", "".join("ACGT"[c] for c in b),
                                        [("zm", "i", zm), ("sn", "Bf", [9.0, 16.0, 8.0, 13.0]), ("pw", "BC", p), ("ip", "BC", ip),
                                         ("cx", "i", 3 | (32 if k & 1 else 16))]))
            q += len(b) + 45
    bam_util.write_bam(path, HDR, recs)


def _records(path):
    _, raw = bam_util.read_bam_raw_records(path)
    text, recs = bam_util.read_bam(path)
    return text, [(r, bytes(x)) for r, x in zip(recs, raw)]


@pytest.fixture(scope="module")
def runs(tmp_path_factory, built):
    d = tmp_path_factory.mktemp("fail_reads")
    zmws = _zmws()
    bam = d / "in.subreads.bam"
    _write(bam, zmws)
    common = ["--min-rq", MIN_RQ, "--min-passes", "3"]
    _ccs(bam, d / "off.bam", *common, "--report-json", d / "off.json")
    _ccs(bam, d / "on.bam", *common, "--fail-reads", d / "fail.bam", "--report-json", d / "on.json", "--report-file", d / "on.txt",
         "--metrics-json", d / "on.metrics.json.gz")
    _ccs(bam, d / "on2.bam", *common, "--fail-reads", d / "fail2.bam", "--workers-per-gpu", "1", "--batch-size", "5")
    return zmws, d


@pytest.mark.gpu
def test_main_output_loses_exactly_the_palindromes(runs):
    zmws, d = runs
    _, off = _records(d / "off.bam")
    text_on, on = _records(d / "on.bam")
    _, fail = _records(d / "fail.bam")
    pal = {r["tags"]["zm"] for r, _ in fail if r["tags"]["ff"] & 0x20}
    assert pal == {zm for zm, kind, _ in zmws if kind == "palindrome"}            # every planted palindrome, nothing else
    assert [x for r, x in off if r["tags"]["zm"] not in pal] == [x for _, x in on]
    assert text_on == bam_util.read_bam(d / "fail.bam")[0]                        # the same header


@pytest.mark.gpu
def test_fail_records(runs):
    zmws, d = runs
    _, on = _records(d / "on.bam")
    _, fail = _records(d / "fail.bam")
    by_zm = {zm: (kind, ps) for zm, kind, ps in zmws}
    order = [r["tags"]["zm"] for r, _ in fail]
    assert order == sorted(order) and len(set(order)) == len(order)                # input order, one record per ZMW
    main = {r["tags"]["zm"] for r, _ in on}
    assert not main & set(order)
    lowrq = sub = 0
    for r, _ in fail:
        t, kind = r["tags"], by_zm[r["tags"]["zm"]][0]
        assert t["RG"] == "ccsamd01" and "sn" in t and "np" in t
        if t["ff"] == 0x8:
            sub += 1
            fl = [p for p in by_zm[t["zm"]][1] if p[3]]
            lens = sorted(len(p[0]) for p in fl)
            med = next(p for p in fl if len(p[0]) == lens[len(lens) // 2])
            assert r["name"].startswith(f"m1/{t['zm']}/") and not r["name"].endswith("/ccs")
            assert np.array_equal(r["seq"], med[0]) and t["np"] == len(fl) and t["rq"] == -1.0
            assert "ec" not in t and "fi" not in t and "ip" not in t
        else:
            assert r["name"] == f"m1/{t['zm']}/ccs" and t["ff"] in (0x1, 0x20, 0x21)
            assert bool(t["ff"] & 0x1) == (t["rq"] < float(MIN_RQ))
            assert bool(t["ff"] & 0x20) == (kind == "palindrome")
            lowrq += t["ff"] == 0x1
    assert lowrq > 0 and sub >= 5
    # together: every ZMW with a consensus or a full pass
    assert main | set(order) == set(by_zm)


@pytest.mark.gpu
def test_index_reports_and_metrics(runs):
    zmws, d = runs
    _, fail = _records(d / "fail.bam")
    pbi = bam_util.read_pbi(str(d / "fail.bam") + ".pbi")
    assert np.array_equal(pbi["file_offset"], bam_util.record_virtual_offsets(d / "fail.bam"))
    assert list(pbi["hole"]) == [r["tags"]["zm"] for r, _ in fail]
    n_pal = sum(1 for r, _ in fail if r["tags"]["ff"] & 0x20)
    n_sub = sum(1 for r, _ in fail if r["tags"]["ff"] == 0x8)
    on, off = json.load(open(d / "on.json")), json.load(open(d / "off.json"))
    ex = on["exclusive_failed_counts"]
    assert ex["CCS adapter palindrome"] == n_pal and ex["ZMW with full-length subread"] == n_sub
    assert "CCS adapter palindrome" not in off["exclusive_failed_counts"]
    assert on["zmws_pass_filters"] == off["zmws_pass_filters"] - sum(1 for r, _ in fail if r["tags"]["ff"] == 0x20)   # (0x21: below --min-rq either way)
    txt = open(d / "on.txt").read()
    assert f"CCS adapter palindrome        : {n_pal} (" in txt and f"ZMW with full-length subread  : {n_sub} (" in txt
    with gzip.open(d / "on.metrics.json.gz", "rt") as f:
        m = {x["zmw"]: x for x in json.load(f)["zmws"]}
    pal = {r["tags"]["zm"] for r, _ in fail if r["tags"]["ff"] & 0x20}
    assert {k for k, v in m.items() if v["status"] == "ADAPTER_PALINDROME"} == {f"m1/{z}" for z in pal}


@pytest.mark.gpu
def test_independent_of_workers_and_batch_size(runs):
    _, d = runs
    assert [x for _, x in _records(d / "on.bam")[1]] == [x for _, x in _records(d / "on2.bam")[1]]
    assert [x for _, x in _records(d / "fail.bam")[1]] == [x for _, x in _records(d / "fail2.bam")[1]]

"""ccs --heteroduplexes split|drop (docs/faq/mode-heteroduplex-filtering.md, docs/how-does-ccs-work.md:65-72, docs/faq/fail-reads.md class 0x4):
the option's usage errors and refused combinations, and on an MI355X a subreads BAM of planted heteroduplexes (substitutions, a 30-bp insertion on one strand),
homoduplex controls, a low-pass group with partial passes and plain ZMWs: `split` against api.consensus_hd_stream on the same passes, against the run without
the option and against --by-strand; the read groups, the index, the two-column report, the summary and the metrics file recomputed from the written records and
the library's verdicts; small batches with one and two packing threads; `drop`; --fail-reads; kinetics, pileup tags and binned QVs; and the run without the
option against what the parent commit's driver wrote for the same input (tests/golden/hd_cli_parent.json)."""
import gzip
import hashlib
import json
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

import bam_util
from test_cli_fail_reads import CCS, HDR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
GOLDEN = os.path.join(ROOT, "tests", "golden", "hd_cli_parent.json")
MIN_RQ = "0.999"
RG = {"": "ccsamd01", "/fwd": "ccsamd02", "/rev": "ccsamd03"}
FAIL_LABEL = {1: "Lacking full passes", 2: "Draft generation error", 3: "Reads failed polishing", 4: "CCS did not converge", 5: "Draft below --min-length",
              6: "Draft above --max-length", 7: "CCS below minimum RQ", 8: "Empty coverage windows", 9: "Consensus outgrew its buffer"}
STATUS_NAME = {0: "SUCCESS", 1: "TOO_FEW_PASSES", 2: "DRAFT_FAILURE", 3: "TOO_MANY_UNUSABLE", 4: "NON_CONVERGENT", 5: "TOO_SHORT", 6: "TOO_LONG", 7: "POOR_QUALITY",
               8: "EMPTY_WINDOW_DURING_POLISHING", 9: "CAPACITY", 10: "HETERODUPLEXES"}


def _run(tmp_path, *args):
    return subprocess.run([CCS, "in.bam", "out.bam", *map(str, args)], capture_output=True, text=True, timeout=60, cwd=tmp_path)


# ---------------------------------------------------------------- CPU: usage
def test_the_value_is_split_or_drop(built, tmp_path):
    for v in ("on", "", "SPLIT", "split,drop"):
        p = _run(tmp_path, "--heteroduplexes", v)
        assert p.returncode == 2 and "--heteroduplexes needs 'split' or 'drop'" in p.stderr and f"'{v}'" in p.stderr, p.stderr
    p = _run(tmp_path, "--heteroduplexes")
    assert p.returncode == 2 and "missing value for --heteroduplexes" in p.stderr
    for v in ("split", "drop"):                                      # accepted: the run then fails on the missing input, not on the option
        p = _run(tmp_path, "--heteroduplexes", v)
        assert p.returncode != 2 and "--heteroduplexes" not in p.stderr, p.stderr
    usage = subprocess.run([CCS, "--help"], capture_output=True, text=True, timeout=60).stderr
    assert "--heteroduplexes split|drop" in usage and "0x4" in usage and "Heteroduplex insertions" in usage


@pytest.mark.parametrize("mode", ["split", "drop"])
@pytest.mark.parametrize("other", [("--by-strand",), ("--reads-bam",), ("--barcodes", "bc.fasta"), ("--fit-model", "m.json"), ("--orient-passes",)])
def test_refused_combinations(built, tmp_path, mode, other):
    """each by its message, exit 2, before any input is opened (in.bam does not exist, neither does bc.fasta)"""
    for args in ((*other, "--heteroduplexes", mode), ("--heteroduplexes", mode, *other)):
        p = _run(tmp_path, *args)
        assert p.returncode == 2 and f"--heteroduplexes combined with {other[0]} is not supported" in p.stderr, p.stderr
        assert "in.bam" not in p.stderr and "bc.fasta" not in p.stderr


def test_the_reference_spellings_stay_refused(built, tmp_path):
    for a in ("--hd-finder", "--split-heteroduplexes"):
        p = _run(tmp_path, a)
        assert p.returncode == 2 and f"{a} is not supported by this build" in p.stderr


# ---------------------------------------------------------------- GPU
def planted():
    """(batch, passes per strand of every ZMW): the planted set of tests/test_hd_requests.py with hole numbers from 1000"""
    import test_hd_requests as T
    b = T.planted()
    b.zmw_id = np.arange(1000, 1000 + b.n_zmw, dtype=np.int32)
    per_strand = []
    for z in range(b.n_zmw):
        f = b.flags[b.read_off[z]:b.read_off[z + 1]]
        full = f[(f & 2) == 0]
        per_strand.append((int(((full & 1) == 0).sum()), int(((full & 1) == 1).sum())))
    return b, per_strand


def write_subreads(path, b):
    """the batch as a subreads BAM: cx carries the adapter flags (a partial pass has one) and the direction bit, sn the ZMW's SNR"""
    recs = []
    for z in range(b.n_zmw):
        q = 0
        for r in range(int(b.read_off[z]), int(b.read_off[z + 1])):
            o, e, f = int(b.base_off[r]), int(b.base_off[r + 1]), int(b.flags[r])
            cx = (3 if not f & 2 else (2 if f & 4 else 1)) | (32 if f & 1 else 16)
            recs.append(bam_util.record(f"m1/{int(b.zmw_id[z])}/{q}_{q + e - o}", "".join("ACGT"[c] for c in b.bases[o:e]),
                                        [("zm", "i", int(b.zmw_id[z])), ("sn", "Bf", b.snr[z]), ("pw", "BC", b.pw[o:e]), ("ip", "BC", b.ipd[o:e]), ("cx", "i", cx)]))
            q += e - o + 45
    bam_util.write_bam(path, HDR, recs)


def _records(path):
    _, raw = bam_util.read_bam_raw_records(path)
    text, recs = bam_util.read_bam(path)
    return text, [(r, bytes(x)) for r, x in zip(recs, raw)]


def _suffix(name):
    """"", "/fwd" or "/rev" of a CCS record's name ("" for a subread's, which a 0x8 fail record keeps)"""
    return name[name.index("/ccs") + 4:] if "/ccs" in name else ""


def _ccs(d, out, *args, timeout=300):
    """one run of the driver in d: (process, seconds)"""
    t0 = time.time()
    p = subprocess.run([CCS, d / "in.subreads.bam", d / out, "--log-level", "INFO", *map(str, args)], capture_output=True, text=True, timeout=timeout, cwd=d)
    assert p.returncode == 0, p.stderr[-3000:]
    return p, time.time() - t0


_LIB = {}


def library(min_rq=None, **requests):
    """api.consensus_hd_stream on the planted passes (records, report), once per option set; the planted set yields every kind (test_hd_requests.planted_yields)"""
    from ccs_amd import api
    import test_hd_requests as T
    key = (min_rq, tuple(sorted(requests)))
    if key not in _LIB:
        b, _ = planted()
        o = api.default_opts()
        if min_rq is not None:
            o.min_rq = float(min_rq)
        h = api.Handle(0, opts=o)
        (recs, rep), = list(api.consensus_hd_stream(h, [b], **requests))
        h.close()
        T.planted_yields(rep)
        _LIB[key] = (b, recs, rep)
    return _LIB[key]


@pytest.fixture(scope="module")
def runs(tmp_path_factory, built):
    d = tmp_path_factory.mktemp("heteroduplex")
    b, per_strand = planted()
    write_subreads(d / "in.subreads.bam", b)
    out = {"d": d, "b": b, "per_strand": per_strand}
    out["off"] = _ccs(d, "off.bam", "--report-file", d / "off.txt", "--metrics-json", d / "off.metrics.json.gz", "--report-json", d / "off.json")
    out["split"] = _ccs(d, "split.bam", "--heteroduplexes", "split", "--report-file", d / "split.txt", "--metrics-json", d / "split.metrics.json.gz",
                        "--report-json", d / "split.json")
    out["strand"] = _ccs(d, "strand.bam", "--by-strand")
    return out


@pytest.mark.gpu
def test_split_equals_the_stream(runs):
    d = runs["d"]
    b, recs, rep = library()
    _, got = _records(d / "split.bam")
    want = [r for r in recs if r.status == 0]
    assert [r["name"] for r, _ in got] == [f"m1/{w.zmw_id}/ccs" + ("" if w.group == "DS" else "/" + w.group) for w in want]
    assert sum(w.group != "DS" for w in want) >= 8
    for (r, _), w in zip(got, want):
        assert np.array_equal(r["seq"], w.seq) and np.array_equal(r["qual"], w.qual), r["name"]
        assert np.float32(r["tags"]["rq"]).tobytes() == np.float32(w.rq).tobytes() and r["tags"]["np"] == w.np_ and r["tags"]["zm"] == w.zmw_id, r["name"]


@pytest.mark.gpu
def test_split_leaves_double_strand_records_alone_and_equals_by_strand(runs):
    from ccs_amd import api
    d, per_strand = runs["d"], runs["per_strand"]
    b, recs, rep = library()
    het = {int(b.zmw_id[z]) for z in np.flatnonzero(rep.verdict == api.HD_HETERODUPLEX)}
    _, off = _records(d / "off.bam")
    text, got = _records(d / "split.bam")
    _, strand = _records(d / "strand.bam")
    # every DS record is byte for byte the record of the run without the option, in its order
    assert [x for r, x in got if _suffix(r["name"]) == ""] == [x for r, x in off if r["tags"]["zm"] not in het]
    assert not [r for r, _ in got if _suffix(r["name"]) == "" and r["tags"]["zm"] in het]
    # the /fwd and /rev records of the split ZMWs with at least 7 passes per strand: those of --by-strand, tag for tag but for the read group
    deep = {int(b.zmw_id[z]) for z in range(b.n_zmw) if min(per_strand[z]) >= 7} & het
    assert len(deep) >= 8
    by_name = {r["name"]: r for r, _ in strand}
    n = 0
    for r, _ in got:
        if r["tags"]["zm"] not in deep:
            continue
        w = by_name[r["name"]]
        assert _suffix(r["name"]) in ("/fwd", "/rev") and np.array_equal(r["seq"], w["seq"]) and np.array_equal(r["qual"], w["qual"]), r["name"]
        assert list(r["tags"]) == list(w["tags"]), r["name"]
        for k, v in r["tags"].items():
            assert k == "RG" or np.array_equal(v, w["tags"][k]), (r["name"], k)
        n += 1
    assert n == sum(1 for x in by_name.values() if x["tags"]["zm"] in deep) >= 16
    # a split ZMW's /fwd record stands before its /rev record, at the ZMW's place
    zms = [r["tags"]["zm"] for r, _ in got]
    assert zms == sorted(zms)
    for zm in het:
        sfx = [_suffix(r["name"]) for r, _ in got if r["tags"]["zm"] == zm]
        assert sfx in (["/fwd", "/rev"], ["/fwd"], ["/rev"], []), (zm, sfx)
    # three read groups, each record names its own; without the option the header is what it was
    rgs = [ln for ln in text.split("\n") if ln.startswith("@RG")]
    assert len(rgs) == 3 and [ln.split("\t")[1] for ln in rgs] == ["ID:ccsamd01", "ID:ccsamd02", "ID:ccsamd03"]
    assert "DS:READTYPE=CCS\t" in rgs[0] and "DS:READTYPE=CCS;STRAND=FORWARD\t" in rgs[1] and "DS:READTYPE=CCS;STRAND=REVERSE\t" in rgs[2]
    assert all(r["tags"]["RG"] == RG[_suffix(r["name"])] for r, _ in got)
    assert len([ln for ln in bam_util.read_bam(d / "off.bam")[0].split("\n") if ln.startswith("@RG")]) == 1
    # the index
    pbi = bam_util.read_pbi(str(d / "split.bam") + ".pbi")
    assert np.array_equal(pbi["file_offset"], bam_util.record_virtual_offsets(d / "split.bam"))
    assert [int(v) for v in pbi["rg_id"]] == [["", "/fwd", "/rev"].index(_suffix(r["name"])) for r, _ in got]
    assert [int(v) for v in pbi["hole"]] == zms and [int(v) for v in pbi["q_end"]] == [len(r["seq"]) for r, _ in got]


def _columns(text):
    """the rows of a two-column report: {label: (DS count, DS percent, SS count, SS percent)}"""
    rows = {}
    for ln in text.split("\n"):
        m = re.match(r"^(.{30}): +(\d+) \( *([\d.]+)%\) +(\d+) \( *([\d.]+)%\)$", ln)
        if m:
            rows[m.group(1).strip()] = (int(m.group(2)), float(m.group(3)), int(m.group(4)), float(m.group(5)))
    return rows


@pytest.mark.gpu
def test_split_reports(runs):
    from ccs_amd import api
    d = runs["d"]
    b, recs, rep = library()
    het = rep.verdict == api.HD_HETERODUPLEX
    n_in = b.n_zmw
    ds = [r for r in recs if r.group == "DS"]
    ss = [r for r in recs if r.group != "DS"]
    assert len(ds) == n_in - het.sum() and len(ss) >= 16
    text = (d / "split.txt").read_text()
    rows = _columns(text)
    assert "Double-Strand Reads" in text.split("\n")[0] and "Single-Strand Reads" in text.split("\n")[0] and "ZMWs input" not in text
    pct = lambda a, n: 100.0 * a / n if n else 0.0
    want = {"Inputs": (len(ds), pct(len(ds), n_in), len(ss), pct(len(ss), n_in))}
    for name, col in (("Passed", lambda rs: sum(r.status == 0 for r in rs)), ("Failed", lambda rs: sum(r.status != 0 for r in rs))):
        want[name] = (col(ds), pct(col(ds), len(ds)), col(ss), pct(col(ss), len(ss)))
    fd, fs = want["Failed"][0], want["Failed"][2]
    for st, label in FAIL_LABEL.items():
        a, c = sum(r.status == st for r in ds), sum(r.status == st for r in ss)
        if label in rows or a or c:
            want[label] = (a, pct(a, fd), c, pct(c, fs))
    assert "Heteroduplex insertions" not in rows and set(want) <= set(rows)
    for k, (a, pa, c, pc) in want.items():
        assert rows[k][0] == a and rows[k][2] == c and abs(rows[k][1] - pa) < 0.006 and abs(rows[k][3] - pc) < 0.006, (k, rows[k], want[k])
    assert sum(v[0] for k, v in rows.items() if k not in ("Inputs", "Passed", "Failed")) == fd
    assert sum(v[2] for k, v in rows.items() if k not in ("Inputs", "Passed", "Failed")) == fs and want["Lacking full passes"][0] >= 1
    js = json.load(open(d / "split.json"))
    assert js["double_strand_reads"] == dict(inputs=len(ds), passed=want["Passed"][0], failed=fd, tandem_repeats=0)
    sj = js["single_strand_reads"]
    assert (sj["inputs"], sj["passed"], sj["failed"]) == (len(ss), want["Passed"][2], fs)
    assert {k: v for k, v in sj["exclusive_failed_counts"].items() if v} == {k: v[2] for k, v in want.items() if k in FAIL_LABEL.values() and v[2]}
    assert {k: v for k, v in js["exclusive_failed_counts"].items() if v} == {k: v[0] for k, v in want.items() if k in FAIL_LABEL.values() and v[0]}
    assert js["zmws_input"] == n_in and "double_strand_reads" not in json.load(open(d / "off.json"))
    # the DS / SS summary, recomputed from the records of OUT
    _, got = _records(d / "split.bam")
    longest, hifi = ({}, {}), ({}, {})
    reads = [0, 0]
    for r, _ in got:
        c, zm, n = int(_suffix(r["name"]) != ""), r["tags"]["zm"], len(r["seq"])
        longest[c][zm] = max(longest[c].get(zm, 0), n)
        if r["tags"]["rq"] >= np.float32(0.99):
            hifi[c][zm] = max(hifi[c].get(zm, 0), n); reads[c] += 1
    err = runs["split"][0].stderr
    pairs = [tuple(int(v) for v in m) for m in re.findall(r"^ - DS / SS    : (\d+) / (\d+)$", err, re.M)]
    assert pairs == [(len(longest[0]), len(longest[1])), (sum(longest[0].values()), sum(longest[1].values())),
                     (sum(hifi[0].values()), sum(hifi[1].values())), tuple(reads)] and pairs[0][1] >= 8
    assert re.search(r"^ZMWs Input    : %d$" % n_in, err, re.M) and re.search(r"^ZMWs Written  : %d$" % sum(pairs[0]), err, re.M)
    assert re.search(r"^HiFi Yield    : %d bases$" % sum(pairs[2]), err, re.M) and re.search(r"^HiFi Reads    : %d$" % sum(reads), err, re.M)
    assert " - DS / SS " not in runs["off"][0].stderr
    # the metrics file: one entry per input ZMW, a split ZMW with its strands
    zm = json.load(gzip.open(d / "split.metrics.json.gz"))["zmws"]
    assert [e["zmw"] for e in zm] == [f"m1/{int(v)}" for v in b.zmw_id]
    by = {}
    for r in ss:
        by.setdefault(r.zmw, []).append(r)
    for z, e in enumerate(zm):
        if not het[z]:
            assert "_strands" not in e and e["status"] != "HETERODUPLEXES"
            continue
        assert e["status"] == "HETERODUPLEXES" and [s["strand"] for s in e["_strands"]] == [r.group for r in by[z]]
        for s, r in zip(e["_strands"], by[z]):
            have = len(r.seq) > 0
            assert s["status"] == STATUS_NAME[r.status] and s["insert_size"] == len(r.seq), (z, s)
            assert abs(s["predicted_accuracy"] - (float(r.rq) if have else -1.0)) < 1e-6
    assert all("_strands" not in e for e in json.load(gzip.open(d / "off.metrics.json.gz"))["zmws"])


@pytest.mark.gpu
def test_small_batches_with_one_and_two_packing_threads(runs):
    """most batches of five hold a heteroduplex, so nearly every ticket is followed by a strand ticket: the same records in the same order; a stall in the
    second-ticket path ends the subprocess at a limit taken from the default run instead of hanging the suite"""
    d = runs["d"]
    limit = max(30.0, 10.0 * runs["split"][1])
    _, want = _records(d / "split.bam")
    for workers in (1, 2):
        p, _ = _ccs(d, f"small{workers}.bam", "--heteroduplexes", "split", "--batch-size", "5", "--workers-per-gpu", workers, timeout=limit)
        _, got = _records(d / f"small{workers}.bam")
        assert [x for _, x in got] == [x for _, x in want], workers
        assert int(re.search(r"single-strand tickets, (\d+) tickets", p.stderr).group(1)) >= 4


@pytest.mark.gpu
def test_drop(runs):
    from ccs_amd import api
    d = runs["d"]
    b, recs, rep = library()
    het = rep.verdict == api.HD_HETERODUPLEX
    hz = {int(b.zmw_id[z]) for z in np.flatnonzero(het)}
    _ccs(d, "drop.bam", "--heteroduplexes", "drop", "--report-file", d / "drop.txt", "--metrics-json", d / "drop.metrics.json.gz", "--report-json", d / "drop.json")
    text_off, off = _records(d / "off.bam")
    text, got = _records(d / "drop.bam")
    assert text == text_off and [x for _, x in got] == [x for r, x in off if r["tags"]["zm"] not in hz] and len(got) < len(off)
    pbi = bam_util.read_pbi(str(d / "drop.bam") + ".pbi")
    assert np.array_equal(pbi["file_offset"], bam_util.record_virtual_offsets(d / "drop.bam")) and not pbi["rg_id"].any()
    js, js_off = json.load(open(d / "drop.json")), json.load(open(d / "off.json"))
    assert js["exclusive_failed_counts"]["Heteroduplex insertions"] == int(het.sum()) >= 8 and "Heteroduplex insertions" not in js_off["exclusive_failed_counts"]
    assert "double_strand_reads" not in js and js["zmws_pass_filters"] == len(got)
    rows = dict(re.findall(r"^(.{30}): (\d+) \(", (d / "drop.txt").read_text(), re.M))
    assert int(rows["Heteroduplex insertions".ljust(30)]) == int(het.sum()) and "Heteroduplex insertions" not in (d / "off.txt").read_text()
    labels = [k.strip() for k in re.findall(r"^(.{30}): ", (d / "drop.txt").read_text(), re.M)]
    assert labels.index("Heteroduplex insertions") == labels.index("Lacking full passes") + 1
    zm = json.load(gzip.open(d / "drop.metrics.json.gz"))["zmws"]
    zm_off = json.load(gzip.open(d / "off.metrics.json.gz"))["zmws"]
    assert len(zm) == b.n_zmw
    for z, (e, e0) in enumerate(zip(zm, zm_off)):
        if het[z]:
            assert e["status"] == "HETERODUPLEXES" and "_strands" not in e and e["predicted_accuracy"] == -1.0
        else:
            assert e == e0
    assert " - DS / SS " not in _ccs(d, "drop2.bam", "--heteroduplexes", "drop")[0].stderr


@pytest.mark.gpu
def test_fail_reads(runs):
    """--fail-reads with --control and --adapters default: the single-strand reads are in FAIL.bam only, each with ff 0x4, with 0x1 exactly below --min-rq; OUT
    and its statistics hold double-strand reads only"""
    from ccs_amd import api
    import control_synth as CS
    d = runs["d"]
    (d / "control.fasta").write_text(">control\n" + CS.TEST_CONTROL + "\n")
    common = ["--min-rq", MIN_RQ, "--fail-reads", d / "fail.bam", "--control", d / "control.fasta", "--adapters", "default"]
    _ccs(d, "fr_off.bam", *common[:2], "--fail-reads", d / "fail_off.bam", *common[4:])
    _ccs(d, "fr.bam", *common, "--heteroduplexes", "split", "--hifi-summary-json", d / "fr.hifi.json", "--report-json", d / "fr.json")
    b, recs, rep = library(min_rq=MIN_RQ)
    het = {int(b.zmw_id[z]) for z in np.flatnonzero(rep.verdict == api.HD_HETERODUPLEX)}
    text, out = _records(d / "fr.bam")
    _, fail = _records(d / "fail.bam")
    _, out_off = _records(d / "fr_off.bam")
    assert all(_suffix(r["name"]) == "" and r["tags"]["RG"] == "ccsamd01" for r, _ in out)
    assert [x for _, x in out] == [x for r, x in out_off if r["tags"]["zm"] not in het]
    ss = [r for r, _ in fail if _suffix(r["name"]) != ""]
    assert len(ss) >= 8 and all(r["tags"]["ff"] & 0x4 and r["tags"]["RG"] == RG[_suffix(r["name"])] for r in ss)
    assert all(not r["tags"]["ff"] & 0x4 for r, _ in fail if _suffix(r["name"]) == "")
    want = {f"m1/{r.zmw_id}/ccs/{r.group}": r for r in recs if r.group != "DS" and len(r.seq) > 0 and r.status in (0, 7)}
    assert {r["name"] for r in ss} == set(want)                      # a strand without a consensus writes nothing
    for r in ss:
        w = want[r["name"]]
        assert bool(r["tags"]["ff"] & 0x1) == (w.status == 7) == bool(r["tags"]["rq"] < np.float32(MIN_RQ)), r["name"]
        assert r["tags"]["ff"] & ~0x5 == 0 and np.array_equal(r["seq"], w.seq) and np.array_equal(r["qual"], w.qual)
    assert text == bam_util.read_bam(d / "fail.bam")[0] and len([ln for ln in text.split("\n") if ln.startswith("@RG")]) == 3
    fpbi = bam_util.read_pbi(str(d / "fail.bam") + ".pbi")
    assert np.array_equal(fpbi["file_offset"], bam_util.record_virtual_offsets(d / "fail.bam"))
    assert [int(v) for v in fpbi["rg_id"]] == [["", "/fwd", "/rev"].index(_suffix(r["name"])) if "/ccs" in r["name"] else 0 for r, _ in fail]
    hs = json.load(open(d / "fr.hifi.json"))
    assert hs["hifi"]["reads"] + hs["below_q20"]["reads"] == len(out) and hs["bases"] == sum(len(r["seq"]) for r, _ in out)
    js = json.load(open(d / "fr.json"))
    assert js["single_strand_reads"]["passed"] == sum(not r["tags"]["ff"] & 0x1 for r in ss) and js["double_strand_reads"]["passed"] == len(out)


@pytest.mark.gpu
def test_kinetics_pileup_and_binned_qvs(runs):
    from ccs_amd import api
    d, per_strand = runs["d"], runs["per_strand"]
    b, recs, rep = library()
    het = {int(b.zmw_id[z]) for z in np.flatnonzero(rep.verdict == api.HD_HETERODUPLEX)}
    deep = {int(b.zmw_id[z]) for z in range(b.n_zmw) if min(per_strand[z]) >= 7} & het
    tags = ["--hifi-kinetics", "--pileup-summary", "--qv-binning"]
    _ccs(d, "k_off.bam", *tags)
    _ccs(d, "k_split.bam", *tags, "--heteroduplexes", "split")
    _ccs(d, "k_strand.bam", *tags, "--by-strand")
    _ccs(d, "k_split.fastq.gz", *tags, "--heteroduplexes", "split")
    _, off = _records(d / "k_off.bam")
    text, got = _records(d / "k_split.bam")
    _, strand = _records(d / "k_strand.bam")
    ds = [(r, x) for r, x in got if _suffix(r["name"]) == ""]
    assert [x for _, x in ds] == [x for r, x in off if r["tags"]["zm"] not in het] and len(ds) >= 16
    assert all({"fi", "fp", "fn", "ri", "rp", "rn", "sa", "sm", "sx"} <= set(r["tags"]) and "ip" not in r["tags"] for r, _ in ds)
    by_name = {r["name"]: r for r, _ in strand}
    n = 0
    for r, _ in got:
        if _suffix(r["name"]) == "":
            continue
        assert {"ip", "pw", "sa", "sm", "sx"} <= set(r["tags"]) and "fi" not in r["tags"] and "ri" not in r["tags"], r["name"]
        assert set(np.unique(r["qual"])) <= {3, 10, 17, 22, 27, 35, 40}
        if r["tags"]["zm"] in deep:
            w = by_name[r["name"]]
            assert list(r["tags"]) == list(w["tags"]) and np.array_equal(r["seq"], w["seq"]) and np.array_equal(r["qual"], w["qual"])
            for k, v in r["tags"].items():
                assert k == "RG" or np.array_equal(v, w["tags"][k]), (r["name"], k)
            n += 1
    assert n >= 16
    rgs = [ln for ln in text.split("\n") if ln.startswith("@RG")]
    assert "Ipd:CodecV1=ip;PulseWidth:CodecV1=pw" not in rgs[0] and all("Ipd:CodecV1=ip;PulseWidth:CodecV1=pw" in ln for ln in rgs[1:]) and len(rgs) == 3
    fq = gzip.open(d / "k_split.fastq.gz", "rt").read().split("\n")
    assert fq[0::4][:-1] == ["@" + r["name"] for r, _ in got]
    assert fq[1::4] == ["".join("ACGT"[c] for c in r["seq"]) for r, _ in got]
    assert fq[3::4] == ["".join(chr(33 + int(q)) for q in r["qual"]) for r, _ in got]


def _digests(d, stem):
    """sha256 of what the four output files hold (the BGZF / gzip containers inflated: their compressed bytes belong to the zlib at hand)"""
    files = {"bam": gzip.open(d / f"{stem}.bam").read(), "pbi": gzip.open(str(d / f"{stem}.bam") + ".pbi").read(),
             "report": open(d / f"{stem}.txt", "rb").read(), "metrics": gzip.open(d / f"{stem}.metrics.json.gz").read()}
    return {k: hashlib.sha256(v).hexdigest() for k, v in files.items()}


@pytest.mark.gpu
def test_without_the_option_nothing_changes(runs):
    """BAM, .pbi, report and metrics of the run without the option against the digests of what the parent commit's driver wrote for the same input
    (`python tests/test_cli_heteroduplex.py --golden PARENT_CCS` made the file with that binary, on an MI355X)"""
    want = json.load(open(GOLDEN))
    assert hashlib.sha256(open(runs["d"] / "in.subreads.bam", "rb").read()).hexdigest() == want["input"], "the planted input is not the one the golden run read"
    assert _digests(runs["d"], "off") == want["outputs"]


if __name__ == "__main__":                                           # --golden CCS: the digests of what that driver writes for the planted input
    import tempfile
    from pathlib import Path
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
    ccs = os.path.abspath(sys.argv[sys.argv.index("--golden") + 1])
    with tempfile.TemporaryDirectory() as tmp:
        d = Path(tmp)
        write_subreads(d / "in.subreads.bam", planted()[0])
        subprocess.run([ccs, d / "in.subreads.bam", d / "off.bam", "--log-level", "INFO", "--report-file", d / "off.txt", "--metrics-json", d / "off.metrics.json.gz",
                        "--report-json", d / "off.json"], check=True, timeout=300, cwd=d)
        out = {"input": hashlib.sha256(open(d / "in.subreads.bam", "rb").read()).hexdigest(), "outputs": _digests(d, "off")}
    json.dump(out, open(GOLDEN, "w"), indent=1)
    print(json.dumps(out))

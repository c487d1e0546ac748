"""ccs --segment-adapters FILE.fasta on an MI355X (DESIGN.md §2 "Segment rule", §7): a subreads BAM of the molecules of tests/segment_lab.py — whole arrays on
either strand, partial arrays, arrays without their middle adapter, molecules without adapters, and ZMWs of two passes that yield no HiFi read.  Against the
same run without the option (with --hifi-kinetics, --pileup-summary and --qv-binning, so every per-base tag is there): every record is the slice of its
parent that the restatement (tests/segment_ref.py) makes of the parent's own sequence; the index, the report block, the JSON keys and the counts TSV agree
with the records; the output does not depend on the packing threads or the batch size; the FASTQ output uses the same names; FAIL.bam is unchanged.

Which ZMWs reach a HiFi read was looked at with the oracle on the CPU for segment_lab.SEED (see tests/test_segment_gpu.py): the ZMWs of eight passes do, so
reads with four, three, two and no segments occur; the tests assert that on the records themselves."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

import bam_util
import segment_lab as LAB
import segment_ref as R
from test_cli_fail_reads import CCS, _ccs, _records, _write

N_ZMW = 12
MIN_RQ = "0.99"


def _zmws():
    """(zm, kind, passes as (bases, pw, ipd, full)) of every ZMW"""
    import lowcx
    tpls, npass, kinds = LAB.templates(N_ZMW)
    rng = np.random.default_rng(LAB.SEED + 2)
    out = []
    for z, (t, n, kind) in enumerate(zip(tpls, npass, kinds)):
        ps = []
        for k in range(n):
            b, p = lowcx.sequence_read(rng, t, 1.0)
            if k & 1:
                b, p = R.rc(b), p[::-1]
            ps.append((b, p, rng.integers(1, 61, len(b)).astype(np.uint8), True))
        out.append((300 + z, kind, ps))
    return out


@pytest.fixture(scope="module")
def runs(tmp_path_factory, built):
    d = tmp_path_factory.mktemp("segments")
    bam = d / "in.subreads.bam"
    _write(bam, _zmws())
    S = LAB.adapter_set()
    (d / "sg.fasta").write_text("".join(f">ad{a} adapter {a}\n{''.join('ACGT'[c] for c in p).lower() if a & 1 else ''.join('ACGT'[c] for c in p)}\n"
                                        for a, p in enumerate(S)))
    common = ["--min-rq", MIN_RQ, "--min-passes", "3", "--hifi-kinetics", "--pileup-summary", "--qv-binning"]
    _ccs(bam, d / "off.bam", *common, "--fail-reads", d / "off.fail.bam", "--report-json", d / "off.json", "--report-file", d / "off.txt")
    on = ["--segment-adapters", d / "sg.fasta", "--segment-counts"]
    _ccs(bam, d / "on.bam", *common, "--fail-reads", d / "on.fail.bam", *on, d / "on.tsv", "--report-json", d / "on.json", "--report-file", d / "on.txt")
    _ccs(bam, d / "on2.bam", *common, "--fail-reads", d / "on2.fail.bam", *on, d / "on2.tsv", "--workers-per-gpu", "1", "--batch-size", "5")
    _ccs(bam, d / "m400.bam", *common, *on, d / "m400.tsv", "--segment-min-length", "400")
    _ccs(bam, d / "on.fastq.gz", *common, "--segment-adapters", d / "sg.fasta")
    return d, S


def _rle(cov):
    out, q = [], 0
    while q < len(cov):
        e = q + 1
        while e < len(cov) and cov[e] == cov[q]:
            e += 1
        out += [e - q, int(cov[q])]
        q = e
    return out


def _expected_records(off, S, **opts):
    """(name, parent record, start, end, di, dl, dr) of every record the option writes, from the parents' own sequences; and the restatement's report"""
    want = R.segment_reads(S, [r["seq"] for r, _ in off], **{**R.DEFAULTS, **opts})
    out = []
    for z, (r, _) in enumerate(off):
        for p in want["pieces"][z, : int(want["n_segments"][z])]:
            st, en, idx, rev = int(p["start"]), int(p["end"]), int(p["index"]), int(p["reverse"])
            out.append((f"{r['name']}/{st}_{en}", r, st, en, idx, idx + rev, idx + 1 - rev))
    return out, want


def _check_records(on, off, S, **opts):
    exp, want = _expected_records(off, S, **opts)
    assert [r["name"] for r, _ in on] == [e[0] for e in exp] and len(exp) > 0
    for (r, _), (name, par, st, en, di, dl, dr) in zip(on, exp):
        L, t, pt = len(par["seq"]), r["tags"], par["tags"]
        assert np.array_equal(r["seq"], par["seq"][st:en]) and np.array_equal(r["qual"], par["qual"][st:en]), name
        assert (t["di"], t["dl"], t["dr"]) == (di, dl, dr), name
        for k in ("RG", "ec", "np", "rq", "zm", "fn", "rn"):              # the parent's scalar tags
            assert t[k] == pt[k], (name, k)
        assert np.array_equal(t["sn"], pt["sn"])
        for k in ("fi", "fp", "sm", "sx"):                                  # per-base, in SEQ's orientation
            assert len(pt[k]) == L and np.array_equal(t[k], pt[k][st:en]), (name, k)
        for k in ("ri", "rp"):                                              # per-base, stored reversed: the slice is taken in SEQ coordinates
            assert len(pt[k]) == L and np.array_equal(t[k], pt[k][L - en: L - st]), (name, k)
        cov = np.repeat(pt["sa"][1::2], pt["sa"][0::2])
        assert len(cov) == L and t["sa"].tolist() == _rle(cov[st:en]), name
        assert set(t) == set(pt) | {"di", "dl", "dr"}, name
    return want


@pytest.mark.gpu
def test_every_record_is_the_stated_slice_of_its_parent(runs):
    d, S = runs
    _, off = _records(d / "off.bam")
    text, on = _records(d / "on.bam")
    assert text == bam_util.read_bam(d / "off.bam")[0]                             # the same header
    want = _check_records(on, off, S)
    assert {0, 2, 3, 4} <= set(want["n_segments"].tolist()) and {-1, 0, 1} <= set(want["orient"].tolist()) and (want["tested"] == 1).all()
    assert set(np.unique(np.concatenate([r["qual"] for r, _ in on])).tolist()) <= {3, 10, 17, 22, 27, 35, 40}          # binned, as the parent
    _, m400 = _records(d / "m400.bam")
    _check_records(m400, off, S, min_len=400)
    assert len(m400) < len(on)


@pytest.mark.gpu
def test_index_reports_and_counts_agree_with_the_records(runs):
    d, S = runs
    _, off = _records(d / "off.bam")
    _, on = _records(d / "on.bam")
    exp, want = _expected_records(off, S)
    pbi = bam_util.read_pbi(str(d / "on.bam") + ".pbi")
    assert np.array_equal(pbi["file_offset"], bam_util.record_virtual_offsets(d / "on.bam"))
    assert pbi["q_start"].tolist() == [e[2] for e in exp] and pbi["q_end"].tolist() == [e[3] for e in exp]
    assert pbi["hole"].tolist() == [e[1]["tags"]["zm"] for e in exp] and np.array_equal(pbi["read_qual"], np.array([e[1]["tags"]["rq"] for e in exp], np.float32))
    n = len(off)
    without = int(((want["n_segments"] == 0) & (want["overflow"] == 0)).sum())
    block_want = {"tested": n, "complete_arrays": int(want["complete"].sum()), "with_segments": int((want["n_segments"] > 0).sum()), "without_segments": without,
                  "overflow": int(want["overflow"].sum()), "segments_written": len(on), "leftover_bases": int(want["leftover_bases"].sum())}
    assert without > 0 and block_want["complete_arrays"] > 0
    j, j0 = json.load(open(d / "on.json")), json.load(open(d / "off.json"))
    assert j["segmentation"] == block_want
    assert "segmentation" not in j0 and {k: v for k, v in j.items() if k != "segmentation"} == j0
    txt, txt0 = open(d / "on.txt").read(), open(d / "off.txt").read()
    block = txt[txt.index("Segmentation\n"): txt.index("Exclusive failed counts")]
    for label, key in (("HiFi reads tested", "tested"), ("Complete arrays", "complete_arrays"), ("Reads with segments", "with_segments"),
                       ("Reads without segments", "without_segments"), ("Reads with adapter overflow", "overflow"), ("Segments written", "segments_written"),
                       ("Leftover bases", "leftover_bases")):
        assert f"{label:<30}: {block_want[key]}" in block, (label, block)
    head = txt.replace(block, "")
    cut = head.index("- - - -")
    assert head[:cut] == txt0[:cut] and "Segmentation" not in txt0               # the HiFi statistics below are over the records written
    lens = sorted(len(r["seq"]) for r, _ in on)
    assert f"HiFi Reads                    : {len(on)}" in txt and f"HiFi Yield (bp)               : {sum(lens):,}" in txt
    classes = {}
    for z in range(n):
        key = (int(want["n_segments"][z]), int(want["orient"][z]), int(want["complete"][z]))
        classes[key] = classes.get(key, 0) + 1
    lines = [ln.split("\t") for ln in open(d / "on.tsv").read().splitlines()]
    assert lines == [[str(a), str(b), str(c), str(v)] for (a, b, c), v in sorted(classes.items())] and len(lines) >= 4


@pytest.mark.gpu
def test_independent_of_workers_and_batch_size_fastq_names_and_fail_reads_unchanged(runs):
    d, _ = runs
    on = _records(d / "on.bam")[1]
    assert [x for _, x in on] == [x for _, x in _records(d / "on2.bam")[1]]
    assert open(d / "on.tsv").read() == open(d / "on2.tsv").read()
    fq = gzip.open(d / "on.fastq.gz", "rt").read().splitlines()
    assert fq[0::4] == ["@" + r["name"] for r, _ in on]
    assert fq[1::4] == ["".join("ACGT"[c] for c in r["seq"]) for r, _ in on] and fq[3::4] == ["".join(chr(33 + q) for q in r["qual"]) for r, _ in on]
    fail0 = [x for _, x in _records(d / "off.fail.bam")[1]]
    assert len(fail0) > 0 and fail0 == [x for _, x in _records(d / "on.fail.bam")[1]] == [x for _, x in _records(d / "on2.fail.bam")[1]]
    assert open(str(d / "off.fail.bam") + ".pbi", "rb").read() == open(str(d / "on.fail.bam") + ".pbi", "rb").read()


# ---------------------------------------------------------------- the driver's usage errors (no GPU is reached)
GOOD = "ACGTTGCAAGGCTTAACCGGTTAGC"


def _fasta(path, recs):
    path.write_text("".join(f">{n}\n{s}\n" for n, s in recs))
    return path


def _run(tmp_path, *args):
    return subprocess.run([CCS, "in.bam", "out.bam", *map(str, args)], capture_output=True, text=True, timeout=60, cwd=tmp_path)


def test_ccs_bad_segment_fasta_names_record_and_cause(built, tmp_path):
    cases = [([(f"a{k}", GOOD) for k in range(34)], "record 34 (>a33)", "more than 33"),
             ([("only", GOOD)], "record 1 (>only)", "at least 2"),
             ([("first", GOOD), ("short one", GOOD[:7])], "record 2 (>short one)", "7 bases"),
             ([("first", GOOD), ("long", (GOOD * 3)[:65])], "record 2 (>long)", "more than 64"),
             ([("first", GOOD), ("second", GOOD), ("withN", GOOD[:10] + "N" + GOOD[10:])], "record 3 (>withN)", "'N'")]
    for recs, where, what in cases:
        p = _run(tmp_path, "--segment-adapters", _fasta(tmp_path / "bad.fasta", recs))
        assert p.returncode == 2 and where in p.stderr and what in p.stderr, p.stderr
    (tmp_path / "empty.fasta").write_text("\n")
    p = _run(tmp_path, "--segment-adapters", "empty.fasta")
    assert p.returncode == 2 and "no FASTA record" in p.stderr
    p = _run(tmp_path, "--segment-adapters", "missing.fasta")
    assert p.returncode == 2 and "missing.fasta" in p.stderr and "cannot open" in p.stderr


def test_ccs_segment_option_errors_and_refusals(built, tmp_path):
    good = _fasta(tmp_path / "sg.fasta", [("a", GOOD[:8]), ("b", (GOOD * 3)[:64]), ("c", GOOD.lower())])
    bc = _fasta(tmp_path / "bc.fasta", [("x", GOOD[:16])])
    for extra in (["--segment-min-length", "32"], ["--segment-counts", "c.tsv"]):
        p = _run(tmp_path, *extra)
        assert p.returncode == 2 and "--segment-adapters" in p.stderr, p.stderr
    for w in ("0", "65536", "-3", "abc", "64x"):
        p = _run(tmp_path, "--segment-adapters", good, "--segment-min-length", w)
        assert p.returncode == 2 and "--segment-min-length" in p.stderr and "1 .. 65535" in p.stderr, (w, p.stderr)
    for extra in (["--by-strand"], ["--barcodes", str(bc)], ["--reads-bam"], ["--heteroduplexes", "drop"], ["--heteroduplexes", "split"], ["--fit-model", "m.json"]):
        p = subprocess.run([CCS, "in.bam", *([] if extra[0] == "--fit-model" else ["out.bam"]), "--segment-adapters", str(good), *extra], capture_output=True,
                           text=True, timeout=60, cwd=tmp_path)
        assert p.returncode == 2 and "not supported" in p.stderr and "--segment-adapters" in p.stderr and extra[0] in p.stderr, (extra, p.stderr)
    assert not os.path.exists(tmp_path / "out.bam")
    usage = subprocess.run([CCS, "--help"], capture_output=True, text=True, timeout=60).stderr
    assert "--segment-adapters" in usage and "--segment-min-length" in usage and "--segment-counts" in usage and "1-65535" in usage
    # a good set at the limits of every range gets past the options: what fails next is the missing input file
    for n in ("1", "65535"):
        p = _run(tmp_path, "--segment-adapters", good, "--segment-min-length", n, "--segment-counts", "c.tsv")
        assert p.returncode != 2 and "--segment" not in p.stderr, p.stderr

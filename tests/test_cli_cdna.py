"""ccs --cdna-primers FILE.fasta on an MI355X (DESIGN.md §2 "cDNA rule", §7): a subreads BAM of the molecules of tests/cdna_lab.py — full-length molecules on
either strand, molecules without a tail, concatemers, molecules with one primer, with the 5' primer at both ends and without primers, and ZMWs of two passes
that yield no HiFi read.  Against the same run without the option (with --hifi-kinetics, --pileup-summary and --qv-binning, so every per-base tag is there):
every record is the slice of its parent that the restatement (tests/cdna_ref.py) makes of the parent's own sequence, with the four tags the restatement gives;
the index, the report block, the JSON keys and the counts TSV add up to the HiFi reads; the output does not depend on the packing threads or the batch size;
the FASTQ output uses the same names; FAIL.bam is unchanged.

Which ZMWs reach a HiFi read was looked at with the oracle on the CPU for cdna_lab.SEED (see tests/test_cdna_gpu.py): the ZMWs of eight passes do, so reads of
the classes FULL_LENGTH (both strands), NO_TAIL, CONCATEMER, ONE_END, SAME_ROLE and NO_PRIMER occur; the tests assert that on the restatement of the parents."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

import bam_util
import cdna_lab as LAB
import cdna_ref as R
from test_cli_fail_reads import CCS, _ccs, _records, _write
from test_cli_segments import _rle

N_ZMW = 14
MIN_RQ = "0.99"
NAMES = ("NO_PRIMER", "ONE_END", "SAME_ROLE", "SHORT", "CONCATEMER", "NO_TAIL", "FULL_LENGTH")
JSON_KEYS = ("no_primer", "one_end", "same_role", "short", "concatemer", "no_tail", "full_length")
ROWS = ("No primer", "Primer at one end only", "Both primers of one role", "Insert too short", "Concatemers", "No poly(A) tail", "Full-length reads written")


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
    d = tmp_path_factory.mktemp("cdna")
    bam = d / "in.subreads.bam"
    _write(bam, _zmws())
    S, roles = LAB.primers()
    seqs = ["".join("ACGT"[c] for c in p) for p in S]
    (d / "pr.fasta").write_text(f">NEB_5p the 5' primer\n{seqs[0]}\n>Clontech_3p\n{seqs[1].lower()}\n")
    common = ["--min-rq", MIN_RQ, "--min-passes", "3", "--hifi-kinetics", "--pileup-summary", "--qv-binning"]
    _ccs(bam, d / "off.bam", *common, "--fail-reads", d / "off.fail.bam", "--report-json", d / "off.json", "--report-file", d / "off.txt")
    on = ["--cdna-primers", d / "pr.fasta", "--cdna-counts"]
    _ccs(bam, d / "on.bam", *common, "--fail-reads", d / "on.fail.bam", *on, d / "on.tsv", "--report-json", d / "on.json", "--report-file", d / "on.txt")
    _ccs(bam, d / "on2.bam", *common, "--fail-reads", d / "on2.fail.bam", *on, d / "on2.tsv", "--workers-per-gpu", "1", "--batch-size", "5")
    _ccs(bam, d / "loose.bam", *common, *on, d / "loose.tsv", "--cdna-min-polya", "0", "--cdna-min-length", "700")
    _ccs(bam, d / "on.fastq.gz", *common, "--cdna-primers", d / "pr.fasta")
    return d, S, roles


def _expected_records(off, S, roles, **opts):
    """(name, parent record, start, end, ts, pa, pr, pq) of every record the option writes, from the parents' own sequences; and the restatement's report"""
    want = R.cdna_reads(S, roles, [r["seq"] for r, _ in off], **opts)
    out = []
    for z, (r, _) in enumerate(off):
        if want["cls"][z] != R.FULL_LENGTH:
            continue
        st, en, strand = int(want["start"][z]), int(want["end"][z]), int(want["strand"][z])
        idx, dist = want["idx"][z].tolist(), want["dist"][z].tolist()
        pq = min(100 * (len(S[idx[e]]) - dist[e]) // len(S[idx[e]]) for e in range(2))
        out.append((f"{r['name']}/{st}_{en}", r, st, en, b"-" if strand else b"+", int(want["polya_len"][z]), [idx[strand], idx[1 - strand]], pq))
    return out, want


def _check_records(on, off, S, roles, **opts):
    exp, want = _expected_records(off, S, roles, **opts)
    assert [r["name"] for r, _ in on] == [e[0] for e in exp] and len(exp) > 0
    for (r, _), (name, par, st, en, ts, pa, pr, pq) in zip(on, exp):
        L, t, pt = len(par["seq"]), r["tags"], par["tags"]
        assert np.array_equal(r["seq"], par["seq"][st:en]) and np.array_equal(r["qual"], par["qual"][st:en]), name
        assert (t["ts"], t["pa"], list(t["pr"]), t["pq"]) == (ts, pa, pr, pq), (name, t["ts"], t["pa"], t["pr"], t["pq"])
        for k in ("RG", "ec", "np", "rq", "zm", "fn", "rn"):              # the parent's scalar tags
            assert t[k] == pt[k], (name, k)
        assert np.array_equal(t["sn"], pt["sn"])
        for k in ("fi", "fp", "sm", "sx"):                                  # per-base, in SEQ's orientation
            assert len(pt[k]) == L and np.array_equal(t[k], pt[k][st:en]), (name, k)
        for k in ("ri", "rp"):                                              # per-base, stored reversed: the slice is taken in SEQ coordinates
            assert len(pt[k]) == L and np.array_equal(t[k], pt[k][L - en: L - st]), (name, k)
        cov = np.repeat(pt["sa"][1::2], pt["sa"][0::2])
        assert len(cov) == L and t["sa"].tolist() == _rle(cov[st:en]), name
        assert set(t) == set(pt) | {"ts", "pa", "pr", "pq"}, name
    return exp, want


@pytest.mark.gpu
def test_every_record_is_the_stated_slice_of_its_parent(runs):
    d, S, roles = runs
    _, off = _records(d / "off.bam")
    text, on = _records(d / "on.bam")
    assert text == bam_util.read_bam(d / "off.bam")[0]                             # the same header
    exp, want = _check_records(on, off, S, roles)
    assert {R.NO_PRIMER, R.ONE_END, R.SAME_ROLE, R.CONCATEMER, R.NO_TAIL, R.FULL_LENGTH} <= set(want["cls"].tolist()) and (want["tested"] == 1).all()
    assert {e[4] for e in exp} == {b"+", b"-"} and all(28 <= e[5] <= 32 and e[6] == [0, 1] and e[7] == 100 for e in exp)
    assert set(np.unique(np.concatenate([r["qual"] for r, _ in on])).tolist()) <= {3, 10, 17, 22, 27, 35, 40}          # binned, as the parent
    _, loose = _records(d / "loose.bam")
    lexp, lwant = _check_records(loose, off, S, roles, min_polya=0, min_len=700)
    assert [e[0] for e in lexp] != [e[0] for e in exp] and (lwant["cls"] == R.NO_TAIL).sum() == 0 and (lwant["cls"] == R.SHORT).sum() > 0


@pytest.mark.gpu
def test_index_reports_and_counts_add_up_to_the_hifi_reads(runs):
    d, S, roles = runs
    _, off = _records(d / "off.bam")
    _, on = _records(d / "on.bam")
    exp, want = _expected_records(off, S, roles)
    pbi = bam_util.read_pbi(str(d / "on.bam") + ".pbi")
    assert np.array_equal(pbi["file_offset"], bam_util.record_virtual_offsets(d / "on.bam"))
    assert pbi["q_start"].tolist() == [e[2] for e in exp] and pbi["q_end"].tolist() == [e[3] for e in exp]
    assert pbi["hole"].tolist() == [e[1]["tags"]["zm"] for e in exp] and np.array_equal(pbi["read_qual"], np.array([e[1]["tags"]["rq"] for e in exp], np.float32))
    n = len(off)
    block_want = {"tested": n, **{key: int((want["cls"] == c).sum()) for c, key in enumerate(JSON_KEYS)}}
    assert sum(block_want[k] for k in JSON_KEYS) == n and block_want["full_length"] == len(on) > 0
    j, j0 = json.load(open(d / "on.json")), json.load(open(d / "off.json"))
    assert j["cdna_reads"] == block_want
    assert "cdna_reads" not in j0 and {k: v for k, v in j.items() if k != "cdna_reads"} == j0
    txt, txt0 = open(d / "on.txt").read(), open(d / "off.txt").read()
    block = txt[txt.index("cDNA reads\n"): txt.index("Exclusive failed counts")]
    assert f"{'HiFi reads tested':<30}: {n}" in block
    for label, key in zip(ROWS, JSON_KEYS):
        assert f"{label:<30}: {block_want[key]} (" in block, (label, block)
    head = txt.replace(block, "")
    cut = head.index("- - - -")
    assert head[:cut] == txt0[:cut] and "cDNA reads" not in txt0                 # the HiFi statistics below are over the records written
    lens = sorted(len(r["seq"]) for r, _ in on)
    assert f"HiFi Reads                    : {len(on)}" in txt and f"HiFi Yield (bp)               : {sum(lens):,}" in txt
    classes = {}
    for z in range(n):
        key = (int(want["cls"][z]), int(want["strand"][z]))
        classes[key] = classes.get(key, 0) + 1
    lines = [ln.split("\t") for ln in open(d / "on.tsv").read().splitlines()]
    assert lines == [[str(c), NAMES[c], str(s), str(v)] for (c, s), v in sorted(classes.items())] and len(lines) >= 6
    assert sum(int(ln[3]) for ln in lines) == n


@pytest.mark.gpu
def test_independent_of_workers_and_batch_size_fastq_names_and_fail_reads_unchanged(runs):
    d = runs[0]
    on = _records(d / "on.bam")[1]
    assert [x for _, x in on] == [x for _, x in _records(d / "on2.bam")[1]]
    assert open(d / "on.tsv").read() == open(d / "on2.tsv").read()
    fq = gzip.open(d / "on.fastq.gz", "rt").read().splitlines()
    assert fq[0::4] == ["@" + r["name"] for r, _ in on]
    assert fq[1::4] == ["".join("ACGT"[c] for c in r["seq"]) for r, _ in on] and fq[3::4] == ["".join(chr(33 + q) for q in r["qual"]) for r, _ in on]
    fail0 = [x for _, x in _records(d / "off.fail.bam")[1]]
    assert len(fail0) > 0 and fail0 == [x for _, x in _records(d / "on.fail.bam")[1]] == [x for _, x in _records(d / "on2.fail.bam")[1]]
    assert open(d / "off.fail.bam", "rb").read() == open(d / "on.fail.bam", "rb").read()          # byte for byte
    assert open(str(d / "off.fail.bam") + ".pbi", "rb").read() == open(str(d / "on.fail.bam") + ".pbi", "rb").read()


# ---------------------------------------------------------------- the driver's usage errors (no GPU is reached)
GOOD = "ACGTTGCAAGGCTTAACCGGTTAGC"


def _fasta(path, recs):
    path.write_text("".join(f">{n}\n{s}\n" for n, s in recs))
    return path


def _run(tmp_path, *args):
    return subprocess.run([CCS, "in.bam", "out.bam", *map(str, args)], capture_output=True, text=True, timeout=60, cwd=tmp_path)


def test_ccs_bad_primer_fasta_names_record_and_cause(built, tmp_path):
    cases = [([(f"a{k}_5p", GOOD) for k in range(65)], "record 65 (>a64_5p)", "more than 64"),
             ([("only_5p", GOOD)], "record 1 (>only_5p)", "a 5' and a 3' primer"),
             ([("first_5p", GOOD), ("short_3p one", GOOD[:7])], "record 2 (>short_3p one)", "7 bases"),
             ([("first_5p", GOOD), ("long_3p", (GOOD * 3)[:65])], "record 2 (>long_3p)", "more than 64"),
             ([("first_5p", GOOD), ("second_3p", GOOD), ("withN_3p", GOOD[:10] + "N" + GOOD[10:])], "record 3 (>withN_3p)", "'N'"),
             ([("first_5p", GOOD), ("second", GOOD)], "record 2 (>second)", "neither _5p nor _3p"),
             ([("first_5p", GOOD), ("second_3p extra_5p", GOOD), ("x_5P", GOOD)], "record 3 (>x_5P)", "neither _5p nor _3p"),
             ([("first_5p", GOOD), ("second_5p", GOOD)], "--cdna-primers", "needs a _5p and a _3p record")]
    for recs, where, what in cases:
        p = _run(tmp_path, "--cdna-primers", _fasta(tmp_path / "bad.fasta", recs))
        assert p.returncode == 2 and where in p.stderr and what in p.stderr, p.stderr
    (tmp_path / "empty.fasta").write_text("\n")
    p = _run(tmp_path, "--cdna-primers", "empty.fasta")
    assert p.returncode == 2 and "no FASTA record" in p.stderr
    p = _run(tmp_path, "--cdna-primers", "missing.fasta")
    assert p.returncode == 2 and "missing.fasta" in p.stderr and "cannot open" in p.stderr


def test_ccs_cdna_option_errors_and_refusals(built, tmp_path):
    good = _fasta(tmp_path / "pr.fasta", [("a_5p", GOOD[:8]), ("b_3p", (GOOD * 3)[:64]), ("c_3p third", GOOD.lower())])
    bc = _fasta(tmp_path / "bc.fasta", [("x", GOOD[:16]), ("y", GOOD[:17])])
    for extra in (["--cdna-min-length", "32"], ["--cdna-counts", "c.tsv"], ["--cdna-min-polya", "10"]):
        p = _run(tmp_path, *extra)
        assert p.returncode == 2 and "--cdna-primers" in p.stderr, p.stderr
    for w in ("0", "65536", "-3", "abc", "64x"):
        p = _run(tmp_path, "--cdna-primers", good, "--cdna-min-length", w)
        assert p.returncode == 2 and "--cdna-min-length" in p.stderr and "1 .. 65535" in p.stderr, (w, p.stderr)
    for w in ("256", "-1", "abc"):
        p = _run(tmp_path, "--cdna-primers", good, "--cdna-min-polya", w)
        assert p.returncode == 2 and "--cdna-min-polya" in p.stderr and "0 .. 255" in p.stderr, (w, p.stderr)
    for extra in (["--by-strand"], ["--barcodes", str(bc)], ["--segment-adapters", str(bc)], ["--reads-bam"], ["--heteroduplexes", "drop"],
                  ["--heteroduplexes", "split"], ["--fit-model", "m.json"]):
        p = subprocess.run([CCS, "in.bam", *([] if extra[0] == "--fit-model" else ["out.bam"]), "--cdna-primers", str(good), *extra], capture_output=True,
                           text=True, timeout=60, cwd=tmp_path)
        assert p.returncode == 2 and "not supported" in p.stderr and "--cdna-primers" in p.stderr and extra[0] in p.stderr, (extra, p.stderr)
    assert not os.path.exists(tmp_path / "out.bam")
    usage = subprocess.run([CCS, "--help"], capture_output=True, text=True, timeout=60).stderr
    assert "--cdna-primers" in usage and "--cdna-min-polya" in usage and "--cdna-min-length" in usage and "--cdna-counts" in usage
    # a good set at the limits of every range gets past the options: what fails next is the missing input file
    for n, a in (("1", "0"), ("65535", "255")):
        p = _run(tmp_path, "--cdna-primers", good, "--cdna-min-length", n, "--cdna-min-polya", a, "--cdna-counts", "c.tsv")
        assert p.returncode != 2 and "--cdna" not in p.stderr, p.stderr

"""ccs --mark-duplicates on an MI355X (DESIGN.md §2 "Duplicate rule", §7): an unaligned BAM of about forty short reads with planted sets of two and three (one
member reverse-complemented), singletons, a read shorter than the window and rq tags that fix the representatives.  Every record of OUT is its input record
byte for byte but for FLAG 0x400 and the ds / du tags that tests/dup_ref.py gives; --dup-remove drops exactly the duplicates; --dup-within-barcodes splits a
set whose members carry different bc tags; the report block and the counts file; the refusals, which exit with 2 before any input is opened."""
import struct

import numpy as np
import pytest

import bam_util
import dup_ref as R
from test_cli_fail_reads import _ccs

pytestmark = pytest.mark.gpu
HDR = "@HD\tVN:1.6\tSO:unknown\tpb:5.0.0\n@RG\tID:ab12cd34\tPL:PACBIO\tDS:READTYPE=CCS\tPU:m1\n"
L = 240


def _reads():
    """[(name, codes, rq or None, bc or None)] and nothing else: the expectation comes from dup_ref on these"""
    rng = np.random.default_rng(77)
    rnd = lambda n=L: rng.integers(0, 4, n).astype(np.uint8)
    a, b, c, d = rnd(), rnd(), rnd(), rnd()
    a1 = R.rc(R.edited(rng, a, R.opts(), "sub", 1))
    out = []

    def add(codes, rq=None, bc=None):
        out.append((f"m1/{100 + len(out)}/ccs", codes, rq, bc))
    add(rnd(), 0.999)
    add(a, 0.9991, (0, 1))             # set A of three: the reverse-complemented member has the largest rq
    add(rnd(), 0.995)
    add(b, 0.9993)                     # set B of two: equal rq, the first stays
    add(a1, 0.99995, (0, 1))
    add(rnd(20), 0.9999)               # shorter than the window: untested
    add(c, 0.9992, (2, 3))             # set C: two bc pairs, split by --dup-within-barcodes
    add(b.copy(), 0.9993)
    for _ in range(12):
        add(rnd(int(rng.integers(60, 400))), float(rng.uniform(0.99, 1.0)))
    add(a.copy(), None, (0, 1))        # no rq tag: score 0
    add(c.copy(), 0.9999, (3, 2))
    add(d, 0.99, (5, 5))               # set D: one bc pair, whole under --dup-within-barcodes
    add(d.copy(), 0.999, (5, 5))
    for _ in range(16):
        add(rnd(int(rng.integers(60, 400))), None if rng.random() < 0.3 else float(rng.uniform(0.99, 1.0)), (1, 1) if rng.random() < 0.5 else None)
    return out


def _record(name, codes, rq, bc):
    tags = [("zm", "i", int(name.split("/")[1])), ("np", "i", 9)]
    if rq is not None:
        tags.append(("rq", "f", rq))
    if bc is not None:
        tags += [("bc", "BS", list(bc)), ("bq", "i", 90)]
    return bam_util.record(name, "".join("ACGT"[c] for c in codes), tags)


def _expected(reads, within=False, **o):
    score = [0 if rq is None else int(np.floor(float(np.float32(rq)) * 1e6)) for _, _, rq, _ in reads]
    group = [0 if (bc is None or not within) else 1 + bc[0] * 65536 + bc[1] for _, _, _, bc in reads]
    return R.mark([r[1] for r in reads], R.opts(**o), group, score)[1]


def _marked(raw, rep, z, names):
    """input record z as OUT carries it"""
    if rep["set_size"][z] < 2:
        return raw
    body = bytearray(raw[4:])
    if rep["dup"][z]:
        flag, = struct.unpack_from("<H", body, 14)
        struct.pack_into("<H", body, 14, flag | 0x400)
    body += b"dsi" + struct.pack("<i", int(rep["set_size"][z]))
    if rep["dup"][z]:
        body += b"duZ" + names[int(rep["rep"][z])].encode() + b"\0"
    return struct.pack("<i", len(body)) + bytes(body)


@pytest.fixture(scope="module")
def runs(tmp_path_factory, built):
    d = tmp_path_factory.mktemp("markdup")
    reads = _reads()
    bam_util.write_bam(d / "in.bam", HDR, [_record(*r) for r in reads], block=3000)
    _ccs("--mark-duplicates", d / "in.bam", d / "out.bam", "--report-file", d / "out.txt", "--dup-counts", d / "out.tsv")
    _ccs("--mark-duplicates", d / "in.bam", d / "rm.bam", "--dup-remove", "-j", 2)
    _ccs("--mark-duplicates", d / "in.bam", d / "bc.bam", "--dup-within-barcodes", "--report-file", d / "bc.txt")
    _ccs("--mark-duplicates", d / "in.bam", d / "w16.bam", "--dup-window", 16, "--dup-kmer", 8, "--dup-max-dist-pct", 0, "--dup-max-len-diff-pct", 0)
    return d, reads


def _check(d, reads, out, rep, remove=False):
    text_in, raw_in = bam_util.read_bam_raw_records(d / "in.bam")
    text, raw = bam_util.read_bam_raw_records(d / out)
    names = [r[0] for r in reads]
    want = [_marked(x, rep, z, names) for z, x in enumerate(raw_in) if not (remove and rep["dup"][z])]
    assert text == text_in and len(raw) == len(want)
    for z, (g, w) in enumerate(zip(raw, want)):
        assert g == w, (out, z)


def test_every_record_is_its_input_record_with_the_marks_of_the_rule(runs):
    d, reads = runs
    rep = _expected(reads)
    names = [r[0] for r in reads]
    # the planted sets are what the restatement finds: A of three under its reverse-complemented member, B under its first, C and D of two, the short read untested
    assert rep["rep"][[1, 4, 20]].tolist() == [4, 4, 4] and rep["set_size"][4] == 3 and rep["rep"][[3, 7]].tolist() == [3, 3]
    assert rep["rep"][[6, 21]].tolist() == [21, 21] and rep["rep"][[22, 23]].tolist() == [23, 23] and rep["status"][5] == R.UNTESTED
    assert int(rep["dup"].sum()) == 5 and int((rep["set_size"] > 1).sum()) == 9
    _check(d, reads, "out.bam", rep)
    _, recs = bam_util.read_bam(d / "out.bam")
    for z, r in enumerate(recs):                                     # (and through the tests' own reader)
        assert r["name"] == names[z] and np.array_equal(r["seq"], reads[z][1] & 3)
        assert bool(r["flag"] & 0x400) == bool(rep["dup"][z]) and r["tags"].get("ds") == (int(rep["set_size"][z]) if rep["set_size"][z] > 1 else None)
        assert r["tags"].get("du") == (names[int(rep["rep"][z])] if rep["dup"][z] else None)
    assert not (d / "out.bam.pbi").exists()


def test_dup_remove_drops_exactly_the_duplicates(runs):
    d, reads = runs
    _check(d, reads, "rm.bam", _expected(reads), remove=True)


def test_within_barcodes_splits_a_set_with_two_bc_pairs(runs):
    d, reads = runs
    rep = _expected(reads, within=True)
    assert rep["set_size"][[6, 21]].tolist() == [1, 1] and rep["rep"][[22, 23]].tolist() == [23, 23] and rep["rep"][[1, 4, 20]].tolist() == [4, 4, 4]
    _check(d, reads, "bc.bam", rep)
    assert "within barcodes" in (d / "bc.txt").read_text()


def test_the_rule_options_reach_the_rule(runs):
    d, reads = runs
    rep = _expected(reads, window=16, kmer=8, max_dist_pct=0, max_len_diff_pct=0)
    assert rep["status"][5] == R.TESTED and rep["rep"][[1, 20]].tolist() == [1, 1] and rep["rep"][[6, 21]].tolist() == [21, 21]   # (20 bases are a window of 16)
    assert R.diff(rep, _expected(reads)) != []
    _check(d, reads, "w16.bam", rep)


def test_report_block_and_counts(runs):
    d, reads = runs
    rep = _expected(reads)
    rows = dict(line.split(":") for line in (d / "out.txt").read_text().splitlines()[1:])
    rows = {k.strip(): int(v) for k, v in rows.items()}
    sizes = [int(rep["set_size"][z]) for z in range(len(reads)) if rep["status"][z] == R.TESTED and rep["rep"][z] == z]
    assert rows == {"Reads input": len(reads), "Reads tested": len(reads) - 1, "Reads untested": 1, "Reads in overflowed buckets": 0,
                    "Duplicate sets": sum(s > 1 for s in sizes), "Duplicates": int(rep["dup"].sum()), "Largest set": 3, "Reads written": len(reads)}
    assert (d / "out.txt").read_text().startswith("Duplicate marking (rule 1: window 32, kmer 12, max_dist_pct 10, max_len_diff_pct 2)")
    lines = (d / "out.tsv").read_text().splitlines()
    assert lines[0] == "set_size\tsets" and [tuple(map(int, x.split("\t"))) for x in lines[1:]] == sorted((s, sizes.count(s)) for s in set(sizes))


@pytest.mark.parametrize("extra", [["--by-strand"], ["--min-passes", "3"], ["--min-rq", "0.9"], ["--fail-reads", "f.bam"], ["--barcodes", "b.fasta"],
                                   ["--segment-adapters", "s.fasta"], ["--cdna-primers", "p.fasta"], ["--reads-bam"], ["--heteroduplexes", "split"],
                                   ["--hifi-kinetics"], ["--chunk", "1/2"], ["--gpu-inflate"], ["--gpu-deflate"], ["--fit-model", "m.json"],
                                   ["--model-file", "m.json"], ["--batch-size", "64"], ["--metrics-json", "m.json.gz"], ["--gpus", "0,1"]],
                         ids=lambda e: e[0])
def test_refusals_exit_2_before_any_input_is_opened(built, tmp_path, extra):
    for args in (["--mark-duplicates", "missing.bam", "out.bam", *extra], [*extra, "missing.bam", "out.bam", "--mark-duplicates"]):
        p = _ccs(*args, check=False, cwd=tmp_path)
        assert p.returncode == 2 and "not supported" in p.stderr and "--mark-duplicates" in p.stderr, (args, p.stderr)
        assert "cannot open" not in p.stderr and not (tmp_path / "out.bam").exists()


def test_stdin_and_stray_options_are_refused(built, tmp_path):
    p = _ccs("--mark-duplicates", "-", "out.bam", check=False, cwd=tmp_path)
    assert p.returncode == 2 and "stdin" in p.stderr and "not supported" in p.stderr
    p = _ccs("--dup-remove", "in.bam", "out.bam", check=False, cwd=tmp_path)
    assert p.returncode == 2 and "need --mark-duplicates" in p.stderr
    p = _ccs("--mark-duplicates", "in.bam", "out.bam", "--dup-window", 16, "--dup-kmer", 12, "--dup-window", 65, check=False, cwd=tmp_path)
    assert p.returncode == 2 and "16 .. 64" in p.stderr

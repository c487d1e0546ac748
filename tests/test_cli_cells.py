"""ccs --cell-reads on an MI355X (DESIGN.md §2 "Cell-tag rule", §7): a small unaligned BAM of planted single-cell cDNA molecules.  Every written record is its
input record with SEQ, QUAL and the per-base B tags cut to the slice tests/cell_ref.py gives (ri from the read's other end), every other tag byte for byte, and the
tags ts, pa, pr, pq, XM, XC and CB behind them: the expected record is built whole and compared as bytes.  The counts file and the report block add up; the
options reach the rule; the refusals exit with 2 before any input is opened.  Then ccs --mark-duplicates --dup-within-cells on the output: two copies of one
molecule with equal (CB, XM) form a set, the same sequence under another UMI or in another cell does not, and without the option it does."""
import struct

import numpy as np
import pytest

import bam_util
import cell_ref as R
from test_cli_fail_reads import _ccs

pytestmark = pytest.mark.gpu
HDR = "@HD\tVN:1.6\tSO:unknown\tpb:5.0.0\n@RG\tID:ab12cd34\tPL:PACBIO\tDS:READTYPE=CCS\tPU:m1\n"
D = dict(R.DESIGN)                                                  # T-12U-16B
TEXT = lambda c: "".join("ACGT"[int(x) & 3] for x in c)            # noqa: E731


def _record(name, codes, qual, tags):
    """a record, block_size first; tags: (tag, type, value), type A i f Z BC Bf"""
    n = len(codes)
    nib = np.array([1, 2, 4, 8], np.uint8)[np.asarray(codes, np.uint8) & 3]
    if n & 1:
        nib = np.append(nib, np.uint8(0))
    packed = ((nib[0::2] << 4) | nib[1::2]).astype(np.uint8).tobytes()
    body = struct.pack("<iiBBHHHiiii", -1, -1, len(name) + 1, 255, 4680, 0, 4, n, -1, -1, 0) + name.encode() + b"\0" + packed + np.asarray(qual, np.uint8).tobytes()
    for tag, ty, v in tags:
        body += tag.encode()
        if ty == "A": body += b"A" + v.encode()
        elif ty == "i": body += b"i" + struct.pack("<i", v)
        elif ty == "f": body += b"f" + struct.pack("<f", v)
        elif ty == "Z": body += b"Z" + v.encode() + b"\0"
        elif ty == "BC": body += b"BC" + struct.pack("<i", len(v)) + np.asarray(v, np.uint8).tobytes()
        elif ty == "Bf": body += b"Bf" + struct.pack("<i", len(v)) + np.asarray(v, "<f4").tobytes()
        else: raise ValueError(ty)
    return struct.pack("<i", len(body)) + body


def _world():
    """primers, whitelist and [(name, codes)]: the expectation comes from cell_ref on these"""
    rng = np.random.default_rng(404)
    p5, p3 = R.random_set(rng, 2, [25])
    wl = R.whitelist(rng, 20, 16, steady_first=20)
    ins, umi, umi2 = R.body(rng, 150), R.steady(rng, 12), R.steady(rng, 12)
    mols = [R.cmol(D, p5, p3, ins, wl[3], umi),                       # 0: the molecule ...
            R.rc(R.cmol(D, p5, p3, R.body(rng, 90), wl[5], R.steady(rng, 12))),
            R.cmol(D, p5, p3, ins, wl[3], umi),                       # 2: ... a second copy of it
            R.cmol(D, p5, p3, R.body(rng, 120), R.sub(wl[7], 4), R.steady(rng, 12)),
            R.cmol(D, p5, p3, ins, wl[3], umi2),                      # 4: the same sequence under another UMI
            R.rc(R.cmol(D, p5, p3, R.body(rng, 101), R.lost(wl[9], 6), R.steady(rng, 12))),
            R.cmol(D, p5, p3, ins, wl[11], umi),                      # 6: ... and in another cell
            R.cmol(D, p5, p3, R.body(rng, 77), R.gained(wl[0], 9), R.steady(rng, 12)),
            R.cmol(D, p5, p3, R.body(rng, 130), R.rand(rng, 16), R.steady(rng, 12)),          # 8: nobody's barcode: ABSENT, written without CB
            R.cmol(D, p5, p3, R.body(rng, 130), wl[2], R.steady(rng, 12), 4),                 # no tail
            R.rand(rng, 300),                                                                 # no primer
            R.cat(p5, R.body(rng, 200)),                                                      # one end
            R.rc(R.cmol(D, p5, p3, R.rc(ins), wl[19], R.steady(rng, 12)))]
    return (p5, p3), wl, [(f"m1/{100 + k}/ccs", c) for k, c in enumerate(mols)]


def _input_record(rng, name, codes):
    L = len(codes)
    qual, fi, ri = rng.integers(0, 94, L), rng.integers(0, 256, L), rng.integers(0, 256, L)
    tags = [("zm", "i", int(name.split("/")[1])), ("rq", "f", 0.999), ("fi", "BC", fi), ("ri", "BC", ri), ("sn", "Bf", [9.0, 8.5, 7.25, 6.0]), ("zz", "BC", [1, 2, 3, 4, 5]),
            ("mg", "Z", "as it is")]
    return qual, tags


def _expected_records(reads, want, wl, recs_in, require=False):
    """the records OUT must hold, as bytes"""
    out = []
    for z, (name, c) in enumerate(reads):
        listed = int(want["tag"][z]) in (R.EXACT, R.CORRECTED)
        if want["cls"][z] != R.FULL_LENGTH or (require and not listed):
            continue
        s, e, L = int(want["start"][z]), int(want["end"][z]), len(c)
        qual, tags = recs_in[z]
        cut = {"fi": lambda v: v[s:e], "ri": lambda v: v[L - e: L - s]}
        tags = [(t, ty, cut[t](v) if t in cut else v) for t, ty, v in tags]
        st = int(want["strand"][z])
        idx, dist = want["idx"][z], want["dist"][z]
        tags += [("ts", "A", "-" if st else "+"), ("pa", "i", int(want["polya_len"][z])), ("pr", "BC", [int(idx[st]), int(idx[1 - st])]),
                 ("pq", "i", min(100 * (25 - int(dist[0])) // 25, 100 * (25 - int(dist[1])) // 25)),
                 ("XM", "Z", TEXT(R.unpack(int(want["umi"][z]), 12))), ("XC", "Z", TEXT(R.unpack(int(want["bc_raw"][z]), 16)))]
        if listed:
            tags.append(("CB", "Z", TEXT(wl[int(want["bc"][z])])))
        out.append(_record(name, c[s:e], qual[s:e], tags))
    return out


@pytest.fixture(scope="module")
def runs(tmp_path_factory, built):
    d = tmp_path_factory.mktemp("cells")
    (p5, p3), wl, reads = _world()
    rng = np.random.default_rng(5)
    recs_in = [_input_record(rng, name, c) for name, c in reads]
    bam_util.write_bam(d / "in.bam", HDR, [_record(name, c, q, t) for (name, c), (q, t) in zip(reads, recs_in)], block=3000)
    (d / "primers.fasta").write_text(f">five_5p\n{TEXT(p5)}\n>three_3p\n{TEXT(p3)}\n")
    (d / "wl.txt").write_text("\n".join(TEXT(w) if k % 2 else TEXT(w).lower() for k, w in enumerate(wl)) + "\n\n")
    base = ["--cell-reads", d / "in.bam"]
    common = ["--cdna-primers", d / "primers.fasta", "--cell-design", "T-12U-16B"]
    _ccs(*base, d / "out.bam", *common, "--cell-whitelist", d / "wl.txt", "--report-file", d / "out.txt", "--cell-counts", d / "out.tsv")
    _ccs(*base, d / "req.bam", *common, "--cell-whitelist", d / "wl.txt", "--cell-require-barcode", "--cell-no-indels", "-j", 2)
    _ccs(*base, d / "raw.bam", *common, "--cdna-min-polya", 0, "--cdna-min-length", 100)
    _ccs("--mark-duplicates", d / "out.bam", d / "cells.bam", "--dup-within-cells", "--report-file", d / "cells.txt")
    _ccs("--mark-duplicates", d / "out.bam", d / "plain.bam")
    return d, (p5, p3), wl, reads, recs_in


def _want(runs, wl="wl", design=None, **o):
    d, S, whitelist, reads, _ = runs
    return R.cell_reads(S, (0, 1), [c for _, c in reads], {**D, **(design or {})}, whitelist if wl else None, **o)


def test_every_written_record_is_the_slice_of_its_input_with_the_tags_of_the_rule(runs):
    d, S, wl, reads, recs_in = runs
    want = _want(runs)
    # the planted molecules are what the restatement finds
    assert want["cls"].tolist() == [R.FULL_LENGTH] * 9 + [R.NO_TAIL, 0, 1, R.FULL_LENGTH] and want["strand"][:9].tolist() == [0, 1, 0, 0, 0, 1, 0, 0, 0]
    assert want["tag"][:9].tolist() == [R.EXACT, R.EXACT, R.EXACT, R.CORRECTED, R.EXACT, R.CORRECTED, R.EXACT, R.CORRECTED, R.ABSENT]
    assert want["shift"][:9].tolist() == [0, 0, 0, 0, 0, -1, 0, 1, 0] and want["bc"][:9].tolist() == [3, 5, 3, 7, 3, 9, 11, 0, -1]
    text, raw = bam_util.read_bam_raw_records(d / "out.bam")
    exp = _expected_records(reads, want, wl, recs_in)
    assert text == HDR and len(raw) == len(exp) == 10
    for k, (g, w) in enumerate(zip(raw, exp)):
        assert g == w, k
    _, recs = bam_util.read_bam(d / "out.bam")                       # (and through the tests' own reader)
    assert [r["tags"].get("CB") for r in recs[:9]] == [TEXT(wl[k]) for k in (3, 5, 3, 7, 3, 9, 11, 0)] + [None]
    assert recs[0]["tags"]["XM"] == recs[2]["tags"]["XM"] != recs[4]["tags"]["XM"] and len(recs[0]["seq"]) == 150 and recs[0]["tags"]["pa"] == 30
    assert not (d / "out.bam.pbi").exists()


def test_the_options_reach_the_rule(runs):
    d, S, wl, reads, recs_in = runs
    want = _want(runs, design=dict(indels=0))
    assert want["tag"][[5, 7]].tolist() == [R.ABSENT] * 2
    _, raw = bam_util.read_bam_raw_records(d / "req.bam")
    exp = _expected_records(reads, want, wl, recs_in, require=True)
    assert len(exp) == 7 and raw == exp
    want = _want(runs, wl=None, min_polya=0, min_len=100)
    assert (want["tag"][:10] == R.RAW).all() and want["cls"][:10].tolist() == [R.FULL_LENGTH, R.SHORT] + [R.FULL_LENGTH] * 5 + [R.SHORT] + [R.FULL_LENGTH] * 2
    _, raw = bam_util.read_bam_raw_records(d / "raw.bam")
    assert raw == _expected_records(reads, want, wl, recs_in)


def test_report_block_and_counts_add_up(runs):
    d, S, wl, reads, _ = runs
    want = _want(runs)
    lines = (d / "out.txt").read_text().splitlines()
    assert lines[0] == "Cell reads (rule 1: design T-12U-16B, 20 barcodes, indels on; cDNA rule 1: min_polya 20, min_len 50)"
    rows = {k.strip(): int(v) for k, v in (line.split(":") for line in lines[1:])}
    cls = {f"Class {n}": int((want["cls"] == k).sum()) for k, n in enumerate(("NO_PRIMER", "ONE_END", "SAME_ROLE", "SHORT", "CONCATEMER", "NO_TAIL", "FULL_LENGTH"))}
    tag = {f"Tag {n}": int((want["tag"] == k).sum()) for k, n in enumerate(("NONE", "RAW", "EXACT", "CORRECTED", "AMBIGUOUS", "ABSENT"))}
    assert rows == {"Reads input": 13, **cls, **tag, "Full-length, no barcode": 0, "Reads written": 10}
    assert sum(cls.values()) == 13 == sum(tag.values())
    tsv = [x.split("\t") for x in (d / "out.tsv").read_text().splitlines()]
    assert tsv[0] == ["index", "barcode", "reads"]
    per = [(int(a), b, int(c)) for a, b, c in tsv[1:] if a not in ("tag", "class")]
    full = want["cls"] == R.FULL_LENGTH
    called = [int(b) for b, t, f in zip(want["bc"], want["tag"], full) if f and t in (R.EXACT, R.CORRECTED)]
    assert per == [(k, TEXT(wl[k]), called.count(k)) for k in sorted(set(called))] and sum(p[2] for p in per) == 9
    assert [x for x in tsv if x[0] == "tag"] == [["tag", k[4:], str(v)] for k, v in tag.items()]
    assert [x for x in tsv if x[0] == "class"] == [["class", k[6:], str(v)] for k, v in cls.items()]


def test_within_cells_a_set_is_one_molecule(runs):
    """reads 0, 2, 4 and 6 are one sequence: 0 and 2 share (CB, XM), 4 has another UMI, 6 another cell; read 12 is its reverse complement in a third cell"""
    d = runs[0]
    _, cells = bam_util.read_bam(d / "cells.bam")
    _, plain = bam_util.read_bam(d / "plain.bam")
    assert [r["name"] for r in cells] == [r["name"] for r in plain] and len(cells) == 10
    same = [0, 2, 4, 6, 9]                                           # (records of OUT: inputs 0, 2, 4, 6 and 12)
    assert [cells[k]["tags"].get("ds") for k in same] == [2, 2, None, None, None]
    assert [bool(cells[k]["flag"] & 0x400) for k in same].count(True) == 1
    assert [plain[k]["tags"].get("ds") for k in same] == [5] * 5 and sum(bool(plain[k]["flag"] & 0x400) for k in same) == 4
    assert all(r["tags"].get("ds") is None for k, r in enumerate(cells) if k not in same)
    assert "within cells" in (d / "cells.txt").read_text().splitlines()[0]


@pytest.mark.parametrize("extra", [["--by-strand"], ["--min-passes", "3"], ["--fail-reads", "f.bam"], ["--barcodes", "b.fasta"], ["--segment-adapters", "s.fasta"],
                                   ["--cdna-counts", "c.tsv"], ["--reads-bam"], ["--hifi-kinetics"], ["--chunk", "1/2"], ["--gpu-inflate"], ["--gpu-deflate"],
                                   ["--mark-duplicates"], ["--metrics-json", "m.json.gz"], ["--gpus", "0,1"]], ids=lambda e: e[0])
def test_refusals_exit_2_before_any_input_is_opened(built, tmp_path, extra):
    for args in (["--cell-reads", "missing.bam", "out.bam", "--cdna-primers", "p.fasta", "--cell-design", "T-12U-16B", *extra],
                 [*extra, "missing.bam", "out.bam", "--cell-design", "T-12U-16B", "--cell-reads", "--cdna-primers", "p.fasta"]):
        p = _ccs(*args, check=False, cwd=tmp_path)
        assert p.returncode == 2 and "not supported" in p.stderr and ("--cell-reads" in p.stderr or "--mark-duplicates" in p.stderr), (args, p.stderr)
        assert "cannot open" not in p.stderr and not (tmp_path / "out.bam").exists()


def test_usage_errors_of_the_mode(runs, tmp_path):
    d = runs[0]
    ok = ["--cell-reads", d / "in.bam", "out.bam", "--cdna-primers", d / "primers.fasta"]

    def refused(*args, say):
        p = _ccs(*args, check=False, cwd=tmp_path)
        assert p.returncode == 2 and say in p.stderr and not (tmp_path / "out.bam").exists(), (args, p.stderr)
    refused("--cell-reads", "-", "out.bam", "--cdna-primers", d / "primers.fasta", "--cell-design", "T-12U-16B", say="stdin (-) is not supported")
    refused("--cell-design", "T-12U-16B", "in.bam", "out.bam", say="need --cell-reads")
    refused("--cell-no-indels", "in.bam", "out.bam", say="need --cell-reads")
    refused("--mark-duplicates", "in.bam", "out.bam", "--dup-within-cells", "--dup-within-barcodes", say="--dup-within-cells combined with --dup-within-barcodes is not supported")
    refused("--dup-within-cells", "in.bam", "out.bam", say="need --mark-duplicates")
    refused("--cell-reads", d / "in.bam", "out.bam", "--cell-design", "T-12U-16B", say="needs --cdna-primers and --cell-design")
    refused(*ok, say="needs --cdna-primers and --cell-design")
    for design, say in (("12U-T-16B", "fields on both sides of T"), ("T", "no field"), ("12U-16B", "names the transcript T once"), ("T-12U-T", "names the transcript T once"),
                        ("T-12U-4U", "more than one U field"), ("8B-8B-T", "more than one B field"), ("T-17B", "not a length 1 .. 16"), ("T-0U", "not a length 1 .. 16"),
                        ("T-12X", "not a length 1 .. 16"), ("T-U", "not a length 1 .. 16"), ("T--12U", "not a length 1 .. 16")):
        refused(*ok, "--cell-design", design, say=say)
    refused(*ok, "--cell-design", "T-12U", "--cell-whitelist", d / "wl.txt", say="the design has no barcode field")
    refused(*ok, "--cell-design", "T-12U-16B", "--cell-require-barcode", say="needs --cell-whitelist")
    for k, (text, say) in enumerate((("ACGTACGTACGTACGT\nACGTACGTACGTACG\n", "line 2: not a barcode of 16 bases"), ("ACGTACGTACGTACGT\n\nACGTACGTACGTACGN\n", "line 3: not ACGT"),
                                     ("\n\n", "holds no barcode"), ("ACGTACGTACGTACGT\nAAAAAAAAAAAAAAAA\nacgtacgtacgtacgt\n", "barcodes 0 and 2 are the same"))):
        (tmp_path / f"w{k}.txt").write_text(text)
        refused(*ok, "--cell-design", "T-12U-16B", "--cell-whitelist", tmp_path / f"w{k}.txt", say=say)
    (tmp_path / "w.gz").write_bytes(b"\x1f\x8b\x08\x00" + b"\0" * 20)
    refused(*ok, "--cell-design", "T-12U-16B", "--cell-whitelist", tmp_path / "w.gz", say="compressed files are not read")


def test_design_strings_place_the_fields(runs, tmp_path):
    """16B-12U-T: the 5' side, the barcode next to the primer; T-16B-12U: the 3' side, the UMI next to the primer.  The molecules are built for each design"""
    d, (p5, p3), wl, _, _ = runs
    rng = np.random.default_rng(8)
    for text, design in (("16B-12U-T", dict(side=0, bc_first=1)), ("T-16B-12U", dict(side=1, bc_first=0)), ("12U-16B-T", dict(side=0, bc_first=0))):
        dd = {**D, **design}
        umi = R.steady(rng, 12)
        reads = [R.cmol(dd, p5, p3, R.body(rng, 100), wl[4], umi), R.rc(R.cmol(dd, p5, p3, R.body(rng, 100), R.sub(wl[6], 2), umi))]
        bam_util.write_bam(tmp_path / "in.bam", HDR, [_record(f"m1/{k}/ccs", c, np.full(len(c), 40), [("zm", "i", k)]) for k, c in enumerate(reads)])
        _ccs("--cell-reads", tmp_path / "in.bam", tmp_path / "out.bam", "--cdna-primers", d / "primers.fasta", "--cell-design", text, "--cell-whitelist", d / "wl.txt")
        _, recs = bam_util.read_bam(tmp_path / "out.bam")
        assert [(r["tags"]["CB"], r["tags"]["XM"], len(r["seq"]), r["tags"]["ts"]) for r in recs] == [(TEXT(wl[4]), TEXT(umi), 100, b"+"), (TEXT(wl[6]), TEXT(umi), 100, b"-")], text


def test_aligned_and_already_tagged_input_end_the_run(runs, tmp_path):
    d, S, wl, reads, recs_in = runs
    args = ["--cdna-primers", d / "primers.fasta", "--cell-design", "T-12U-16B"]
    name, c = reads[0]
    bam_util.write_bam(tmp_path / "tagged.bam", HDR, [_record(name, c, recs_in[0][0], [("zm", "i", 1), ("XM", "Z", "ACGT")])])
    p = _ccs("--cell-reads", tmp_path / "tagged.bam", tmp_path / "o.bam", *args, check=False)
    assert p.returncode == 1 and "already carries an XM, XC or CB tag" in p.stderr and name in p.stderr
    data = b"BAM\x01" + struct.pack("<i", len(HDR)) + HDR.encode() + struct.pack("<i", 1) + struct.pack("<i", 5) + b"chr1\0" + struct.pack("<i", 1000)
    (tmp_path / "aligned.bam").write_bytes(bam_util._bgzf_block(data) + bam_util.BGZF_EOF)
    p = _ccs("--cell-reads", tmp_path / "aligned.bam", tmp_path / "o2.bam", *args, check=False)
    assert p.returncode == 1 and "reference sequences" in p.stderr and not (tmp_path / "o2.bam").exists()

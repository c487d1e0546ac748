"""ccs --barcodes FILE.fasta on an MI355X (DESIGN.md §2 "Barcode calls", §7): a subreads BAM of the molecules of tests/barcode_lab.py — barcodes at both ends, at
the head only, at the tail only, none, and ZMWs of two passes that yield no HiFi read.  With the option exactly the records whose own sequence the restatement
(tests/barcode_ref.py) calls at both ends carry bc / bq with its values; every other byte of every record is what it is without the option; the index, the report
block, the JSON keys and the counts TSV agree with the records; the output does not depend on the packing threads or the batch size; FAIL.bam is unchanged.

Which ZMWs reach a HiFi read was looked at with the oracle on the CPU for barcode_lab.SEED (see tests/test_barcode_gpu.py): the ZMWs of eight passes do, so all
four calls occur among the records; the tests assert that on the records themselves."""
import json
import struct

import numpy as np
import pytest

import bam_util
import barcode_lab as LAB
import barcode_ref as R
from test_cli_fail_reads import _ccs, _records, _write

pytestmark = pytest.mark.gpu
N_ZMW = 18
MIN_RQ = "0.99"


def _zmws():
    """(zm, kind, passes as (bases, pw, ipd, full)) of every ZMW"""
    import lowcx
    tpls, npass, kinds, _ = LAB.templates(N_ZMW)
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
    d = tmp_path_factory.mktemp("barcodes")
    bam = d / "in.subreads.bam"
    _write(bam, _zmws())
    S = LAB.barcode_set()
    (d / "bc.fasta").write_text("".join(f">bc{b:03d} barcode {b}\n{''.join('ACGT'[c] for c in p).lower() if b & 1 else ''.join('ACGT'[c] for c in p)}\n"
                                        for b, p in enumerate(S)))
    common = ["--min-rq", MIN_RQ, "--min-passes", "3"]
    _ccs(bam, d / "off.bam", *common, "--fail-reads", d / "off.fail.bam", "--report-json", d / "off.json", "--report-file", d / "off.txt")
    on = ["--barcodes", d / "bc.fasta", "--barcode-counts"]
    _ccs(bam, d / "on.bam", *common, "--fail-reads", d / "on.fail.bam", *on, d / "on.tsv", "--report-json", d / "on.json", "--report-file", d / "on.txt")
    _ccs(bam, d / "on2.bam", *common, "--fail-reads", d / "on2.fail.bam", *on, d / "on2.tsv", "--workers-per-gpu", "1", "--batch-size", "5")
    _ccs(bam, d / "w24.bam", *common, *on, d / "w24.tsv", "--barcode-window", "24")
    return d, S


def _want(recs, S, **opts):
    return R.call_reads(S, [r["seq"] for r, _ in recs], **{**R.DEFAULTS, **opts})


def _tag_bytes(idx, bq):
    return b"bcBS" + struct.pack("<IHH", 2, int(idx[0]), int(idx[1])) + b"bqi" + struct.pack("<i", int(bq))


def _check_records(on, off, S, **opts):
    """every record of `on` against the same record of `off` and the restatement on its own sequence; returns the restatement's report"""
    assert len(on) == len(off) > 0
    want = _want(on, S, **opts)
    for z, ((r, raw), (_, raw0)) in enumerate(zip(on, off)):
        if want["call"][z] == 3:
            assert list(r["tags"]["bc"]) == want["idx"][z].tolist() and r["tags"]["bq"] == want["bq"][z], (r["name"], r["tags"].get("bc"), want["idx"][z])
            extra = _tag_bytes(want["idx"][z], want["bq"][z])
            assert raw[4:] == raw0[4:] + extra and struct.unpack("<i", raw[:4])[0] == struct.unpack("<i", raw0[:4])[0] + len(extra), r["name"]
        else:
            assert "bc" not in r["tags"] and "bq" not in r["tags"] and raw == raw0, r["name"]
    return want


def test_exactly_the_reads_called_at_both_ends_are_tagged(runs):
    d, S = runs
    _, off = _records(d / "off.bam")
    text, on = _records(d / "on.bam")
    assert text == bam_util.read_bam(d / "off.bam")[0]                             # the same header
    want = _check_records(on, off, S)
    assert set(want["call"].tolist()) == {0, 1, 2, 3} and (want["tested"] == 1).all()
    _, w24 = _records(d / "w24.bam")
    _check_records(w24, off, S, window=24)


def test_index_reports_and_counts_agree_with_the_records(runs):
    d, S = runs
    _, on = _records(d / "on.bam")
    want = _want(on, S)
    pbi, pbi0 = bam_util.read_pbi(str(d / "on.bam") + ".pbi"), bam_util.read_pbi(str(d / "off.bam") + ".pbi")
    assert np.array_equal(pbi["file_offset"], bam_util.record_virtual_offsets(d / "on.bam"))
    for k in ("rg_id", "q_start", "q_end", "hole", "read_qual", "ctxt"):
        assert np.array_equal(pbi[k], pbi0[k]), k
    n = {c: int((want["call"] == c).sum()) for c in range(4)}
    j, j0 = json.load(open(d / "on.json")), json.load(open(d / "off.json"))
    assert j["barcode_calls"] == {"tested": len(on), "both_ends": n[3], "head_only": n[1], "tail_only": n[2], "none": n[0]}
    assert "barcode_calls" not in j0 and {k: v for k, v in j.items() if k != "barcode_calls"} == j0
    txt, txt0 = open(d / "on.txt").read(), open(d / "off.txt").read()
    block = txt[txt.index("Barcode calls\n"): txt.index("Exclusive failed counts")]
    for label, c in (("HiFi reads tested", len(on)), ("Barcodes at both ends", n[3]), ("Barcode at the head only", n[1]), ("Barcode at the tail only", n[2]),
                     ("No barcode", n[0])):
        assert f"{label:<30}: {c}" in block, (label, block)
    assert txt.replace(block, "") == txt0 and "Barcode" not in txt0
    pairs = {}
    for z in np.flatnonzero(want["call"] == 3):
        key = tuple(want["idx"][z].tolist())
        pairs[key] = pairs.get(key, 0) + 1
    lines = [ln.split("\t") for ln in open(d / "on.tsv").read().splitlines()]
    assert lines == [[f"bc{a:03d}", f"bc{b:03d}", str(c)] for (a, b), c in sorted(pairs.items())] and len(lines) > 0


def test_independent_of_workers_and_batch_size_and_fail_reads_unchanged(runs):
    d, _ = runs
    assert [x for _, x in _records(d / "on.bam")[1]] == [x for _, x in _records(d / "on2.bam")[1]]
    assert open(d / "on.tsv").read() == open(d / "on2.tsv").read()
    fail0 = [x for _, x in _records(d / "off.fail.bam")[1]]
    assert len(fail0) > 0 and fail0 == [x for _, x in _records(d / "on.fail.bam")[1]] == [x for _, x in _records(d / "on2.fail.bam")[1]]
    assert all("bc" not in r["tags"] and "bq" not in r["tags"] for r, _ in _records(d / "on.fail.bam")[1])

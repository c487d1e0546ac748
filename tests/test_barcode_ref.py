"""The barcode rule on the CPU (DESIGN.md §2 "Barcode calls"): tests/barcode_ref.py against the brute force over every substring, ccsx_barcode_reads_host
against barcode_ref on the limit set, the structs against the header, and every argument error of the four entry points."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from ccs_amd import api
import barcode_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = R.limit_cases()


def _opts(d):
    o = api.BarcodeOpts()
    o.window, o.max_dist_pct, o.min_margin = d["window"], d["max_dist_pct"], d["min_margin"]
    return o


@pytest.mark.parametrize("seed", range(4))
def test_restatement_equals_the_bruteforce(seed):
    """short reads, so that every substring can be tried: L 0 .. 14 against 8- and 9-mers, windows shorter than, equal to and longer than the read"""
    rng = np.random.default_rng(seed)
    S = R.random_set(rng, 4, [8, 9])
    S[3] = S[1].copy()
    reads = [R.molecule(rng, int(L), S[int(rng.integers(0, 4))], S[int(rng.integers(0, 4))], head_at=int(rng.integers(0, 3))) for L in rng.integers(1, 15, 10)]
    reads += [np.zeros(0, np.uint8), np.zeros(9, np.uint8)]
    for window, pct, margin in ((8, 20, 1), (10, 30, 0), (64, 0, 1)):
        want = R.call_reads_brute(S, reads, window, pct, margin)
        got = R.call_reads(S, reads, window, pct, margin)
        assert R.diff(got, want) == [], (window, R.diff(got, want))


def test_the_limit_set_holds_what_it_is_for():
    """the cases are there, and the values the issue names occur in what the restatement says about them"""
    names = [c[0] for c in CASES]
    for nb in (1, 2, 64, 65, 128, 129, 384):
        assert f"n{nb}" in names
    assert 2 * 128 == R.THREADS and 2 * 129 > R.THREADS          # the boundary the 128 | 129 pair is about
    calls = set()
    for i, (name, S, o, reads) in enumerate(CASES):
        w = R.expected(i)
        calls |= set(int(c) for c in w["call"][w["tested"] == 1])
        if name == "n1":
            assert (w["second"][w["tested"] == 1] == 255).all()
        if name == "content_p15_g1":                              # identical barcodes 2 and 5: the lower index, margin 0, not called; called at margin 0
            assert w["idx"][9].tolist() == [2, 2] and w["dist"][9].tolist() == [0, 0] and w["second"][9].tolist() == [0, 0] and w["call"][9] == 0
            assert R.expected(names.index("content_p15_g0"))["call"][9] == 3
            assert w["call"][0] == 3 and w["call"][1] == 3 and w["call"][2] == 0      # 1 and 2 substitutions called, 3 not
            assert w["idx"][11].tolist() == [6, 6] and w["call"][11] == 3             # its own reverse complement at both ends
        if name == "placement":
            assert w["clip"][11].tolist() == [19, 18] and w["call"][11] == 3          # twice in the window: the first
            assert [int(c) for c in w["clip"][1:6, 0]] == [17, 18, 19, 20, 21]
            assert w["dist"][6].tolist() == [1, 1] and (w["dist"][6:11] <= np.array([1, 4, 8, 12, 15])[:, None]).all()   # straddling the edge: k bases of it inside
            assert w["call"][10] == 0
    assert calls == {0, 1, 2, 3}


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0] for c in CASES])
def test_the_host_rule_equals_the_restatement(built, i):
    name, S, o, reads = CASES[i]
    rep = api.barcode_reads_host(api.BarcodeSet.from_codes(S), list(reads), _opts(o))
    assert R.diff(rep, R.expected(i)) == [], (name, R.diff(rep, R.expected(i)))


def test_structs_match_the_header(built, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ccsx.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d %d\\n", '
                   'sizeof(ccsx_barcode_opts), offsetof(ccsx_barcode_opts, min_margin), sizeof(ccsx_barcode_set), offsetof(ccsx_barcode_set, len), '
                   'offsetof(ccsx_barcode_set, seq), sizeof(ccsx_barcode_report), offsetof(ccsx_barcode_report, tested), offsetof(ccsx_barcode_report, idx), '
                   'offsetof(ccsx_barcode_report, clip), sizeof(ccsx_barcode_request), offsetof(ccsx_barcode_request, opts), offsetof(ccsx_barcode_request, set), '
                   'offsetof(ccsx_barcode_request, report), offsetof(ccsx_barcode_request, reserved), sizeof(ccsx_requests), offsetof(ccsx_requests, reserved), '
                   'CCSX_BARCODE_MAX, CCSX_BARCODE_MIN_LEN, CCSX_BARCODE_MAX_LEN, CCSX_BARCODE_MAX_WINDOW, CCSX_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    O, S, Rp, Q, Rq = api.BarcodeOpts, api.BarcodeSet, api.CBarcodeReport, api.CBarcodeRequest, api.CRequests
    assert got == [C.sizeof(O), O.min_margin.offset, C.sizeof(S), S.len.offset, S.seq.offset, C.sizeof(Rp), Rp.tested.offset, Rp.idx.offset, Rp.clip.offset,
                   C.sizeof(Q), Q.opts.offset, Q.set.offset, Q.report.offset, Q.reserved.offset, C.sizeof(Rq), Rq.reserved.offset,
                   api.BARCODE_MAX, api.BARCODE_MIN_LEN, api.BARCODE_MAX_LEN, api.BARCODE_MAX_WINDOW, 6]
    assert got[0] == 12 and got[2] == 4 + 384 * 4 + 384 * 64 and got[5] == 64 and got[9] == 32 and got[14] == 64 and got[15] == 40
    L = api.lib()
    assert L.ccsx_barcode_rule_version() == 1 and L.ccsx_abi_version() == 6 and L.ccsx_spec_version() == 8
    o = api.barcode_opts_default()
    assert dict(window=o.window, max_dist_pct=o.max_dist_pct, min_margin=o.min_margin) == R.DEFAULTS
    assert [c.tolist() for c in api.BarcodeSet.from_strings(["acgtACGT", [3, 2, 1, 0, 0, 1, 2, 3, 3]]).codes()] == [[0, 1, 2, 3] * 2, [3, 2, 1, 0, 0, 1, 2, 3, 3]]


# ---------------------------------------------------------------- argument errors: refused before anything is enqueued (no handle is ever needed to be refused)
def _set(lens, poke=None, n=None):
    s = api.BarcodeSet.from_strings([("ACGT" * 16)[:m] for m in lens])
    if poke:
        s.seq[poke[0]][poke[1]] = poke[2]
    if n is not None:
        s.n_barcodes = n
    return s


def _bad_sets_and_opts():
    """(message, set, opts kwargs)"""
    bad = [("n_barcodes outside 1 .. 384", _set([16], n=0), {}), ("n_barcodes outside 1 .. 384", _set([16] * 384, n=385), {}),
           ("barcode 1: length outside 8 .. 64", _set([16, 7, 30]), {}), ("barcode 0: length outside 8 .. 64", _set([0]), {}),
           ("barcode 2: length outside 8 .. 64", _set([8, 64, 64], n=3), {"poke_len": (2, 65)}),
           ("barcode 2: code above 3", _set([64, 16, 40], poke=(2, 39, 4)), {})]
    for kw in (dict(window=7), dict(window=1025), dict(max_dist_pct=-1), dict(max_dist_pct=31), dict(min_margin=-1), dict(min_margin=65)):
        bad.append(("barcode options out of range", _set([16]), kw))
    return bad


def _mk_opts(kw):
    o = api.barcode_opts_default()
    for k, v in kw.items():
        if k != "poke_len":
            setattr(o, k, v)
    return o


@pytest.mark.parametrize("entry", ["ccsx_barcode_reads_host", "ccsx_barcode_reads"])
def test_the_read_forms_refuse_bad_arguments(built, entry):
    L = api.lib()
    reads = [np.zeros(30, np.uint8), np.zeros(0, np.uint8)]

    def call(bset, opts, rep, poke=None, null=()):
        args, _, keep = api._barcode_reads_args(bset if bset is not None else _set([16]), opts, reads, rep)
        args = list(args)
        if bset is None:
            args[0] = None
        for k in null:
            args[k] = None
        if poke:
            poke(keep)
        return getattr(L, entry)(*(([None] if entry == "ccsx_barcode_reads" else []) + args))

    for msg, s, kw in _bad_sets_and_opts():
        if "poke_len" in kw:
            s.len[kw["poke_len"][0]] = kw["poke_len"][1]
        assert call(s, _mk_opts(kw), None) < 0 and msg.encode() in L.ccsx_last_error(), (msg, L.ccsx_last_error())
    assert call(None, None, None) < 0 and b"null barcode set" in L.ccsx_last_error()
    assert call(_set([16]), None, None, null=(6,)) < 0 and b"null barcode report" in L.ccsx_last_error()
    assert call(_set([16]), None, api.BarcodeReport.allocate(3)) < 0 and b"sized for another batch" in L.ccsx_last_error()
    for k in (2, 3, 4):
        assert call(_set([16]), None, None, null=(k,)) < 0 and b"null argument" in L.ccsx_last_error(), k

    def neg(keep):
        keep[3][0] = -1
    assert call(_set([16]), None, None, poke=neg) < 0 and b"read 0: negative seq_off" in L.ccsx_last_error()
    if entry == "ccsx_barcode_reads":                            # valid arguments at the limits of every range: the handle is what is missing
        for kw in (dict(window=8, max_dist_pct=0, min_margin=0), dict(window=1024, max_dist_pct=30, min_margin=64)):
            assert call(_set([8, 64] * 192), _mk_opts(kw), None) < 0 and b"null argument" in L.ccsx_last_error(), L.ccsx_last_error()
    else:
        assert call(_set([8, 64] * 192), _mk_opts(dict(window=1024, max_dist_pct=30, min_margin=64)), None) == 0


@pytest.mark.parametrize("entry", ["ccsx_consensus_barcodes", "ccsx_submit_barcodes"])
def test_the_fused_forms_refuse_bad_requests(built, entry):
    L = api.lib()
    b = api.synth(3, 4, 300, seed=2)
    res = api.Results.allocate(b)
    rep = api.BarcodeReport.allocate(b.n_zmw)

    def call(q, rq=None, batch=b):
        cb, cr = batch.c_struct() if batch is not None else None, res.c_struct()
        t = C.c_int64()
        args = [None, C.byref(cb) if cb is not None else None, C.byref(cr), rq, q]
        return getattr(L, entry)(*(args + [C.byref(t)] if entry == "ccsx_submit_barcodes" else args))

    def request(bset, opts=None, report=rep, reserved=(0, 0)):
        cr = report.c_struct() if report is not None else None
        q = api.CBarcodeRequest(C.pointer(opts) if opts is not None else None, C.pointer(bset) if bset is not None else None,
                                C.pointer(cr) if cr is not None else None, (C.c_int32 * 2)(*reserved))
        return q, (bset, opts, cr)

    for msg, s, kw in _bad_sets_and_opts():
        if "poke_len" in kw:
            s.len[kw["poke_len"][0]] = kw["poke_len"][1]
        q, keep = request(s, _mk_opts(kw))
        assert call(C.byref(q)) < 0 and msg.encode() in L.ccsx_last_error(), (msg, L.ccsx_last_error())
    for msg, (q, keep) in (("null barcode set", request(None)), ("null barcode report", request(_set([16]), report=None)),
                           ("reserved must be 0", request(_set([16]), reserved=(0, 1))), ("reserved must be 0", request(_set([16]), reserved=(5, 0))),
                           ("sized for another batch", request(_set([16]), report=api.BarcodeReport.allocate(b.n_zmw + 1)))):
        assert call(C.byref(q)) < 0 and msg.encode() in L.ccsx_last_error(), (msg, L.ccsx_last_error())
    assert call(None) < 0 and b"null barcode request" in L.ccsx_last_error()
    q, keep = request(_set([16]))
    assert call(C.byref(q), batch=None) < 0 and b"null argument" in L.ccsx_last_error()
    # a bad member of the ccsx_requests beside a good barcode request is refused by that member's message; nonzero reserved pointers of the struct too
    frep = api.FoldReport.allocate(b.n_zmw + 1).c_struct()
    fq = api.CFoldRequest(None, C.pointer(frep), (C.c_int32 * 2)(0, 0))
    rq = api.CRequests(None, C.pointer(fq), None, None, None, (C.c_void_p * 3)())
    assert call(C.byref(q), C.byref(rq)) < 0 and b"sized for another batch" in L.ccsx_last_error()
    rq = api.CRequests(None, None, None, None, None, (C.c_void_p * 3)(0, 1, 0))
    assert call(C.byref(q), C.byref(rq)) < 0 and b"reserved must be NULL" in L.ccsx_last_error()
    # valid requests (NULL options = the defaults, the limits of every range): the handle is what is missing
    for q, keep in (request(_set([16])), request(_set([8, 64] * 192), _mk_opts(dict(window=1024, max_dist_pct=30, min_margin=64))),
                    request(_set([8]), _mk_opts(dict(window=8, max_dist_pct=0, min_margin=0)))):
        assert call(C.byref(q)) < 0 and b"null argument" in L.ccsx_last_error(), L.ccsx_last_error()


# ---------------------------------------------------------------- the driver's usage errors (no GPU is reached)
CCS = os.path.join(ROOT, "ccs_amd", "bin", "ccs")
GOOD = "ACGTTGCAAGGCTTAACCGGTTAGC"


def _fasta(path, recs):
    path.write_text("".join(f">{n}\n{s}\n" for n, s in recs))
    return path


def _run(tmp_path, *args):
    return subprocess.run([CCS, "in.bam", "out.bam", *map(str, args)], capture_output=True, text=True, timeout=60, cwd=tmp_path)


def test_ccs_bad_barcode_fasta_names_record_and_cause(built, tmp_path):
    cases = [([(f"b{k}", GOOD) for k in range(385)], "record 385 (>b384)", "more than 384"),
             ([("first", GOOD), ("short one", GOOD[:7])], "record 2 (>short one)", "7 bases"),
             ([("first", GOOD), ("long", (GOOD * 3)[:65])], "record 2 (>long)", "more than 64"),
             ([("first", GOOD), ("second", GOOD), ("withN", GOOD[:10] + "N" + GOOD[10:])], "record 3 (>withN)", "'N'")]
    for recs, where, what in cases:
        p = _run(tmp_path, "--barcodes", _fasta(tmp_path / "bad.fasta", recs))
        assert p.returncode == 2 and where in p.stderr and what in p.stderr, p.stderr
    (tmp_path / "empty.fasta").write_text("\n")
    p = _run(tmp_path, "--barcodes", "empty.fasta")
    assert p.returncode == 2 and "no FASTA record" in p.stderr
    p = _run(tmp_path, "--barcodes", "missing.fasta")
    assert p.returncode == 2 and "missing.fasta" in p.stderr and "cannot open" in p.stderr


def test_ccs_barcode_option_errors(built, tmp_path):
    good = _fasta(tmp_path / "bc.fasta", [("a", GOOD[:8]), ("b", (GOOD * 3)[:64]), ("c", GOOD.lower())])
    for extra in (["--barcode-window", "32"], ["--barcode-counts", "c.tsv"]):
        p = _run(tmp_path, *extra)
        assert p.returncode == 2 and "--barcodes" in p.stderr, p.stderr
    for w in ("7", "1025", "0", "-3", "abc", "64x"):
        p = _run(tmp_path, "--barcodes", good, "--barcode-window", w)
        assert p.returncode == 2 and "--barcode-window" in p.stderr and "8 .. 1024" in p.stderr, (w, p.stderr)
    for extra in (["--by-strand"], ["--fit-model", "m.json"]):
        p = subprocess.run([CCS, "in.bam", *(["out.bam"] if extra[0] == "--by-strand" else []), "--barcodes", str(good), *extra], capture_output=True, text=True,
                           timeout=60, cwd=tmp_path)
        assert p.returncode == 2 and "not supported" in p.stderr and "--barcodes" in p.stderr, p.stderr
    usage = subprocess.run([CCS, "--help"], capture_output=True, text=True, timeout=60).stderr
    assert "--barcodes" in usage and "--barcode-window" in usage and "--barcode-counts" in usage and "8-1024" in usage
    # a good set at the limits of every range gets past the options: what fails next is the missing input file
    p = _run(tmp_path, "--barcodes", good, "--barcode-window", "8", "--barcode-counts", "c.tsv")
    assert p.returncode != 2 and "--barcode" not in p.stderr, p.stderr

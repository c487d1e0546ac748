"""The segment rule on the CPU (DESIGN.md §2 "Segment rule"): tests/segment_ref.py against the brute force over every substring, ccsx_segment_reads_host
against segment_ref on the limit set (on poisoned planes, and again with the reads in reverse order), the structs against the header, and every argument error
of the four entry points."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from ccs_amd import api
import segment_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = R.limit_cases()
NAMES = [c[0] for c in CASES]


def _opts(d):
    o = api.SegmentOpts()
    o.max_dist_pct, o.min_len = d["max_dist_pct"], d["min_len"]
    return o


def poisoned(n):
    """a report whose every byte is 0xA5: what the rule does not write shows"""
    rep = api.SegmentReport.allocate(n)
    for k in R.FIELDS:
        getattr(rep, k).view(np.uint8)[...] = 0xA5
    return rep


@pytest.mark.parametrize("seed", range(4))
def test_restatement_equals_the_bruteforce(seed):
    """short reads, so that every substring can be tried: 8- and 9-mers, three adapters, reads of 1 .. 40 bases that hold whole, cut and edited adapters"""
    rng = np.random.default_rng(seed)
    S = R.random_set(rng, 3, [8, 9])
    reads = [np.zeros(0, np.uint8), S[0][:7], S[0].copy(), R.cat(S[0], R.rand(rng, 6), S[1]), R.rc(R.cat(S[0], R.rand(rng, 6), S[1], R.rand(rng, 5), S[2])),
             R.cat(S[1], S[2]), R.cat(R.rand(rng, 3), R.edit(rng, S[1], "sub", 1), R.rand(rng, 7), R.edit(rng, S[2], "del", 1), R.rand(rng, 2)),
             R.cat(S[0], S[0][4:], S[0])]
    reads += [R.rand(rng, int(L)) for L in rng.integers(1, 30, 4)]
    for pct, min_len in ((15, 5), (30, 1), (0, 6)):
        want = R.segment_reads_brute(S, reads, pct, min_len)
        got = R.segment_reads(S, reads, pct, min_len)
        assert R.diff(got, want) == [], (pct, R.diff(got, want))


def test_the_limit_set_holds_what_it_is_for(built):
    """the cases are there, and the values the issue names occur in what the restatement says about them"""
    assert api.lib().ccsx_segment_chunk() == R.CHUNK
    for name in ("n2", "n3", "n32", "n33", "m8", "m25", "m63", "m64", "mixed", "chunks", "longest", "edits_p15", "pieces", "order", "ties", "counts"):
        assert name in NAMES
    E = {name: R.expected(i) for i, name in enumerate(NAMES)}
    for na in (2, 3, 32, 33):                                    # the whole array, both ways; the set's last segments
        w = E[f"n{na}"]
        assert w["complete"][:2].tolist() == [1, 1] and w["orient"][:2].tolist() == [0, 1] and w["n_segments"][:2].tolist() == [na - 1] * 2
        assert w["pieces"][0, 0]["start"] == 7 + 25 and w["pieces"][0, na - 2]["index"] == na - 2 and w["pieces"][1, 0]["index"] == na - 2
        assert w["pieces"][2, int(w["n_segments"][2]) - 1]["index"] == na - 2 and w["tested"][3] == 0 and w["orient"][3] == -1
        assert w["leftover_bases"][0] == 12 and w["n_segments"][4] == 0
    for name in ("m8", "m25", "m63", "m64"):                     # m - 1 bases of an adapter: m = 8 allows one edit, so its 7-mer hits; m, m + 1 and the rc hit
        w, m = E[name], int(name[1:])
        assert w["n_hits"][1] >= (1 if m * 15 // 100 >= 1 else 0) and w["n_hits"][2] >= 1 and w["n_hits"][3] >= 1 and w["n_hits"][4] >= 1 and w["n_segments"][1:5].sum() == 0
        assert len(CASES[NAMES.index(name)][3][-1]) == 3001
        if m >= 25:
            z = 5                                                    # exactly A0 S A1: an adapter at 0 and one that ends at L
            assert w["n_segments"][z] == 1 and w["pieces"][z, 0].tolist() == (m, m + 70, 0, 0, 0, 0) and w["leftover_bases"][z] == 0
    w = E["chunks"]
    ends = (R.CHUNK - 1, R.CHUNK, R.CHUNK + 1, R.CHUNK + 4, R.CHUNK + 12, 2 * R.CHUNK - 1, 2 * R.CHUNK, 2 * R.CHUNK + 1, 2 * R.CHUNK + 12)
    for i, end in enumerate(ends):
        assert w["complete"][2 * i] == 1 and w["pieces"][2 * i, 0]["end"] == end - 25 and w["pieces"][2 * i, 1]["start"] == end, (i, end)
        assert w["complete"][2 * i + 1] == 1 and w["orient"][2 * i + 1] == 1
    assert w["complete"][-1] == 1 and w["pieces"][-1, 1]["start"] == R.CHUNK + 25
    w = E["longest"]
    assert w["n_segments"][0] == 2 and w["pieces"][0, 0]["start"] == 28 and w["pieces"][0, 1]["end"] == R.LONGEST - 25 and w["orient"][0] == 0
    w = E["edits_p15"]                                           # per kind: 0, k, k + 1 edits; with k + 1 the two pieces become one leftover
    for kind in range(3):
        assert w["n_segments"][3 * kind: 3 * kind + 3].tolist() == [2, 2, 0] and w["n_cuts"][3 * kind: 3 * kind + 3].tolist() == [3, 3, 2], kind
        assert w["pieces"][3 * kind + 1, 0]["dist_right"] == R.K25 and w["leftover_bases"][3 * kind + 2] >= 250
    assert E["edits_p0"]["n_segments"].tolist() == [2, 0, 0] * 3 and (E["edits_p30"]["n_segments"] == 2).all()
    w = E["pieces"]                                              # back to back: a piece of length 0; 49 is no segment, 50 is one
    assert w["n_cuts"][0] == 3 and w["n_segments"][0] == 1 and w["leftover_bases"][0] == 0
    assert [int(p["index"]) for p in w["pieces"][1, :2]] == [1, 2] and w["n_segments"][1] == 2 and w["leftover_bases"][1] == 49
    assert w["n_segments"][2] == 2 and w["n_cuts"][3] == 4 and w["n_segments"][3] == 0 and w["leftover_bases"][3] == 0
    assert E["pieces_min1"]["n_segments"].tolist() == [1, 3, 3, 0, 3] and E["pieces_min1"]["complete"].tolist() == [0, 1, 1, 0, 1]
    assert (E["pieces_min65535"]["n_segments"] == 0).all()
    w = E["order"]
    assert w["n_segments"][:2].tolist() == [0, 0] and w["n_cuts"][:2].tolist() == [2, 2]
    assert (w["complete"][2], w["orient"][2]) == (1, 1) and (w["complete"][3], w["orient"][3], w["n_segments"][3]) == (0, 2, 6)
    assert (w["complete"][4], w["orient"][4], w["n_segments"][4]) == (0, 0, 6) and (w["complete"][5], w["orient"][5]) == (0, 1) and w["orient"][6] == 2
    w = E["ties"]
    assert w["n_hits"][0] == 3 and w["n_cuts"][0] == 2 and w["pieces"][0, 0].tolist()[2:] == (0, 0, 0, 0)           # adapter 1 at dist 0 beats adapter 2 at dist 2
    assert w["n_hits"][1] == 2 and w["n_cuts"][1] == 1 and w["leftover_bases"][1] == 40 + 50                        # u v taken, v w not
    assert w["n_segments"][2] == 1 and w["pieces"][2, 0]["index"] == 4 and w["n_hits"][2] == 5                      # 4 | 5, then 5 == 6: search 10 taken twice, not 12
    assert w["n_segments"][3] == 1 and w["pieces"][3, 0].tolist()[2:4] == (7, 0) and w["n_hits"][3] == 5            # 6 (as 5) | 7: not a segment; 7 | 8 forward: search 14 beats 15
    assert w["n_hits"][4] == 3 and w["n_cuts"][4] == 1 and w["leftover_bases"][4] == 30 + 19 + 19 + 30
    w = E["counts"]
    assert w["n_hits"].tolist() == [64, 65, 100, 3, 63] and w["overflow"].tolist() == [0, 1, 1, 0, 0] and w["n_cuts"].tolist() == [64, 0, 0, 3, 63]
    assert w["tested"].tolist() == [1] * 5 and w["orient"].tolist() == [-1] * 5 and w["leftover_bases"].tolist() == [256, 0, 0, 0, 252]


@pytest.mark.parametrize("i", range(len(CASES)), ids=NAMES)
def test_the_host_rule_equals_the_restatement(built, i):
    name, S, o, reads = CASES[i]
    sset = api.SegmentSet.from_codes(S)
    rep = api.segment_reads_host(sset, list(reads), _opts(o), poisoned(len(reads)))
    assert R.diff(rep, R.expected(i)) == [], (name, R.diff(rep, R.expected(i)))
    rep = api.segment_reads_host(sset, list(reads)[::-1], _opts(o), poisoned(len(reads)))
    assert R.diff(rep, R.reversed_order(R.expected(i))) == [], (name, "reversed", R.diff(rep, R.reversed_order(R.expected(i))))


def test_structs_match_the_header(built, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ccsx.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu '
                   '%d %d %d %d %d %d\\n", '
                   'sizeof(ccsx_segment_opts), offsetof(ccsx_segment_opts, min_len), sizeof(ccsx_segment_set), offsetof(ccsx_segment_set, len), '
                   'offsetof(ccsx_segment_set, seq), sizeof(ccsx_segment_piece), offsetof(ccsx_segment_piece, end), offsetof(ccsx_segment_piece, index), '
                   'offsetof(ccsx_segment_piece, dist_right), sizeof(ccsx_segment_report), offsetof(ccsx_segment_report, tested), '
                   'offsetof(ccsx_segment_report, leftover_bases), offsetof(ccsx_segment_report, pieces), sizeof(ccsx_segment_request), '
                   'offsetof(ccsx_segment_request, set), offsetof(ccsx_segment_request, report), offsetof(ccsx_segment_request, reserved), '
                   'CCSX_SEGMENT_MAX_ADAPTERS, CCSX_SEGMENT_MIN_LEN, CCSX_SEGMENT_MAX_LEN, CCSX_SEGMENT_MAX_HITS, CCSX_SEGMENT_MAX_PIECES, CCSX_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    O, S, P, Rp, Q = api.SegmentOpts, api.SegmentSet, api.CSegmentPiece, api.CSegmentReport, api.CSegmentRequest
    assert got == [C.sizeof(O), O.min_len.offset, C.sizeof(S), S.len.offset, S.seq.offset, C.sizeof(P), P.end.offset, P.index.offset, P.dist_right.offset,
                   C.sizeof(Rp), Rp.tested.offset, Rp.leftover_bases.offset, Rp.pieces.offset, C.sizeof(Q), Q.set.offset, Q.report.offset, Q.reserved.offset,
                   api.SEGMENT_MAX_ADAPTERS, api.SEGMENT_MIN_LEN, api.SEGMENT_MAX_LEN, api.SEGMENT_MAX_HITS, api.SEGMENT_MAX_PIECES, 6]
    assert got[0] == 8 and got[2] == 4 + 33 * 4 + 33 * 64 and got[5] == 12 and got[9] == 80 and got[13] == 32
    assert api.SEGMENT_PIECE_DTYPE.itemsize == 12 and api.SEGMENT_PIECE_DTYPE == R.PIECE_DTYPE and R.PLANES == api.SEGMENT_PLANES
    L = api.lib()
    assert L.ccsx_segment_rule_version() == 1 and L.ccsx_abi_version() == 6
    o = api.segment_opts_default()
    assert dict(max_dist_pct=o.max_dist_pct, min_len=o.min_len) == R.DEFAULTS
    assert [c.tolist() for c in api.SegmentSet.from_codes(["acgtACGT", [3, 2, 1, 0, 0, 1, 2, 3, 3]]).codes()] == [[0, 1, 2, 3] * 2, [3, 2, 1, 0, 0, 1, 2, 3, 3]]


# ---------------------------------------------------------------- argument errors: refused before anything is enqueued (no handle is ever needed to be refused)
def _set(lens, poke=None, n=None):
    s = api.SegmentSet.from_codes([("ACGT" * 16)[:m] for m in lens])
    if poke:
        s.seq[poke[0]][poke[1]] = poke[2]
    if n is not None:
        s.n_adapters = n
    return s


def _bad_sets_and_opts():
    """(message, set, opts kwargs, (adapter, length) to poke)"""
    bad = [("n_adapters outside 2 .. 33", _set([16], n=1), {}, None), ("n_adapters outside 2 .. 33", _set([16] * 33, n=34), {}, None),
           ("n_adapters outside 2 .. 33", _set([16, 16], n=0), {}, None),
           ("adapter 1: length outside 8 .. 64", _set([16, 7, 30]), {}, None), ("adapter 0: length outside 8 .. 64", _set([0, 16]), {}, None),
           ("adapter 2: length outside 8 .. 64", _set([8, 64, 64]), {}, (2, 65)),
           ("adapter 2: code above 3", _set([64, 16, 40], poke=(2, 39, 4)), {}, None)]
    for kw in (dict(max_dist_pct=-1), dict(max_dist_pct=31), dict(min_len=0), dict(min_len=65536)):
        bad.append(("segment options out of range", _set([16, 16]), kw, None))
    for msg, s, kw, poke in bad:
        if poke:
            s.len[poke[0]] = poke[1]
    return bad


def _mk_opts(kw):
    o = api.segment_opts_default()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


LIMITS = (dict(max_dist_pct=0, min_len=1), dict(max_dist_pct=30, min_len=65535))


@pytest.mark.parametrize("entry", ["ccsx_segment_reads_host", "ccsx_segment_reads"])
def test_the_read_forms_refuse_bad_arguments(built, entry):
    L = api.lib()
    reads = [np.zeros(30, np.uint8), np.zeros(0, np.uint8)]

    def call(sset, opts, rep, poke=None, null=()):
        args, _, keep = api._segment_reads_args(sset if sset is not None else _set([16, 16]), opts, reads, rep)
        args = list(args)
        if sset is None:
            args[0] = None
        for k in null:
            args[k] = None
        if poke:
            poke(keep)
        return getattr(L, entry)(*(([None] if entry == "ccsx_segment_reads" else []) + args))

    for msg, s, kw, _ in _bad_sets_and_opts():
        assert call(s, _mk_opts(kw), None) < 0 and msg.encode() in L.ccsx_last_error(), (msg, L.ccsx_last_error())
    assert call(None, None, None) < 0 and b"null segment set" in L.ccsx_last_error()
    assert call(_set([16, 16]), None, None, null=(6,)) < 0 and b"null segment report" in L.ccsx_last_error()
    assert call(_set([16, 16]), None, api.SegmentReport.allocate(3)) < 0 and b"sized for another batch" in L.ccsx_last_error()
    for k in (2, 3, 4):
        assert call(_set([16, 16]), None, None, null=(k,)) < 0 and b"null argument" in L.ccsx_last_error(), k

    def neg(keep):
        keep[3][0] = -1
    assert call(_set([16, 16]), None, None, poke=neg) < 0 and b"read 0: negative seq_off" in L.ccsx_last_error()
    for kw in LIMITS:                                            # valid arguments at the limits of every range: only the handle is missing, where one is needed
        rc = call(_set([8, 64] * 16 + [8]), _mk_opts(kw), None)
        if entry == "ccsx_segment_reads":
            assert rc < 0 and b"null argument" in L.ccsx_last_error(), L.ccsx_last_error()
        else:
            assert rc == 0, L.ccsx_last_error()


@pytest.mark.parametrize("entry", ["ccsx_consensus_segments", "ccsx_submit_segments"])
def test_the_fused_forms_refuse_bad_requests(built, entry):
    L = api.lib()
    b = api.synth(3, 4, 300, seed=2)
    res = api.Results.allocate(b)
    rep = api.SegmentReport.allocate(b.n_zmw)

    def call(q, rq=None, batch=b):
        cb, cr = batch.c_struct() if batch is not None else None, res.c_struct()
        t = C.c_int64()
        args = [None, C.byref(cb) if cb is not None else None, C.byref(cr), rq, q]
        return getattr(L, entry)(*(args + [C.byref(t)] if entry == "ccsx_submit_segments" else args))

    def request(sset, opts=None, report=rep, reserved=(0, 0)):
        cr = report.c_struct() if report is not None else None
        q = api.CSegmentRequest(C.pointer(opts) if opts is not None else None, C.pointer(sset) if sset is not None else None,
                                C.pointer(cr) if cr is not None else None, (C.c_int32 * 2)(*reserved))
        return q, (sset, opts, cr)

    for msg, s, kw, _ in _bad_sets_and_opts():
        q, keep = request(s, _mk_opts(kw))
        assert call(C.byref(q)) < 0 and msg.encode() in L.ccsx_last_error(), (msg, L.ccsx_last_error())
    for msg, (q, keep) in (("null segment set", request(None)), ("null segment report", request(_set([16, 16]), report=None)),
                           ("reserved must be 0", request(_set([16, 16]), reserved=(0, 1))), ("reserved must be 0", request(_set([16, 16]), reserved=(5, 0))),
                           ("sized for another batch", request(_set([16, 16]), report=api.SegmentReport.allocate(b.n_zmw + 1)))):
        assert call(C.byref(q)) < 0 and msg.encode() in L.ccsx_last_error(), (msg, L.ccsx_last_error())
    assert call(None) < 0 and b"null segment request" in L.ccsx_last_error()
    q, keep = request(_set([16, 16]))
    assert call(C.byref(q), batch=None) < 0 and b"null argument" in L.ccsx_last_error()
    # a bad member of the ccsx_requests beside a good segment request is refused by that member's message; nonzero reserved pointers of the struct too
    frep = api.FoldReport.allocate(b.n_zmw + 1).c_struct()
    fq = api.CFoldRequest(None, C.pointer(frep), (C.c_int32 * 2)(0, 0))
    rq = api.CRequests(None, C.pointer(fq), None, None, None, (C.c_void_p * 3)())
    assert call(C.byref(q), C.byref(rq)) < 0 and b"sized for another batch" in L.ccsx_last_error()
    rq = api.CRequests(None, None, None, None, None, (C.c_void_p * 3)(0, 1, 0))
    assert call(C.byref(q), C.byref(rq)) < 0 and b"reserved must be NULL" in L.ccsx_last_error()
    # valid requests (NULL options = the defaults, the limits of every range): the handle is what is missing
    for q, keep in (request(_set([16, 16])), request(_set([8, 64] * 16 + [8]), _mk_opts(LIMITS[1])), request(_set([8, 8]), _mk_opts(LIMITS[0]))):
        assert call(C.byref(q)) < 0 and b"null argument" in L.ccsx_last_error(), L.ccsx_last_error()


def test_the_mirror_refuses_the_combinations_no_entry_point_takes(built):
    """the segment request goes beside the members of ccsx_requests only: hd, hand-off, barcode and represent requests have entry points of their own, and none
    takes two.  Handle.submit says so before it looks at anything else (no handle state is touched: the check comes first)"""
    b = api.synth(2, 4, 300, seed=2)
    res, rep = api.Results.allocate(b), api.SegmentReport.allocate(b.n_zmw)
    sset = _set([16, 16])
    others = (dict(hd=api.HdReport.allocate(b.n_zmw)), dict(handoff=object()), dict(barcodes=api.BarcodeReport.allocate(b.n_zmw), barcode_set=object()),
              dict(represent=api.RepresentReport.allocate(b.n_zmw)))
    for kw in others:
        with pytest.raises(ValueError, match="segment request is not combined"):
            api.Handle.submit(None, b, res, segments=rep, segment_set=sset, **kw)

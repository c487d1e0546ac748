"""The polisher hand-off (ccsx_consensus_handoff / ccsx_submit_handoff; DESIGN.md §2 "Polisher hand-off") against tests/handoff_ref.py: every tile the engine
selects is compared with the numpy restatement on the engine's own stages, integer for integer.  Every test asserts that the limit it is about occurred."""
import ctypes as C
import hashlib
import os
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest

import handoff_ref as R
from ccs_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu
FIELDS = api.Handoff.FIELDS


def hopts(T=100, R_=20, skip=94):
    o = api.handoff_opts_default()
    o.tile_len, o.max_rows, o.skip_above = T, R_, skip
    return o


@pytest.fixture(scope="module")
def handle(built):
    h = api.Handle(0)
    yield h
    h.close()


def same(got: api.Handoff, exp: dict):
    """every array of the written slots equals the restatement's"""
    got = got.host()
    assert got.counts.tolist() == exp["counts"].tolist()
    m = got.n_tiles
    assert m == len(exp["tile_zmw"])
    for k in FIELDS[1:]:
        a, b = np.asarray(getattr(got, k))[:m], exp[k]
        assert np.array_equal(a, b), (k, np.argwhere(a != b)[:5].tolist())
    return m


def run_and_compare(h, b, o, max_tiles=None, ipd=True, **kw):
    res, ho = h.consensus_handoff(b, opts=o, max_tiles=max_tiles, **kw)
    exp, zmws = R.from_engine(h, b, res, o, ho.max_tiles, ipd)
    same(ho, exp)
    return res, ho, exp, zmws


def census(exp, zmws) -> Counter:
    """what the compared tiles contain, for the tests' own assertions"""
    c = Counter()
    for g in range(len(exp["tile_zmw"])):
        z, start, ln, rows = (int(exp[k][g]) for k in ("tile_zmw", "tile_start", "tile_len", "tile_rows"))
        st = np.concatenate([[0], np.cumsum([ce - cs for cs, ce in zmws[z].cores])])
        pos = start + np.arange(ln)
        first, later_first, last = np.isin(pos, st[:-1]), np.isin(pos, st[1:-1]), np.isin(pos, st[1:] - 1)
        c["short_tile"] += ln < exp["cells"].shape[2]; c["tile_of_1"] += ln == 1; c["opposite_rows"] += int(exp["row_strand"][g].sum())
        c["missing_rows"] += int((exp["row_pass"][g] == 255).sum())
        for k in range(rows):
            base, ins = exp["cells"][g, k, :ln, 0].astype(int), exp["cells"][g, k, :ln, 3].astype(int)
            c["ins>=12"] += int((ins >= 12).sum()); c["del_first_core_col"] += int(((base == 4) & first).sum()); c["del_last_core_col"] += int(((base == 4) & last).sum())
            c["seam_insertion"] += int(((base < 4) & (ins > 0) & later_first).sum())
            # leading inserted bases, counted where the first core starts at template column 0: no column, so no DIAG, lies to the left of position 0
            lead = int(((base < 4) & (ins > 0) & (pos == 0)).sum()) if zmws[z].cores[0][0] == 0 else 0
            c["leading_insertion"] += lead; c["leading_insertion_opposite" if exp["row_strand"][g][k] else "leading_insertion_forward"] += lead
            have = np.flatnonzero(base < 5)
            if len(have):
                c["code5_inside_a_row"] += int((base[have[0]:have[-1] + 1] == 5).any())
                c["code5_to_the_tile_end"] += int(have[-1] < ln - 1 or have[0] > 0)
            else:
                c["row_all_5"] += 1
    return c


def segment_lengths(zmws, max_rows) -> Counter:
    """usable segments of the row passes by the wave layout they take: paired (<= 31 bases), unpaired (32 .. 63), and unusable ones"""
    c = Counter()
    for z in zmws:
        nw = len(z.tpls)
        for w in range(nw):
            iws, iwe = (0 if w == 0 else 2 * w - 1), (2 * nw - 1 if w == nw - 1 else 2 * (w + 1))
            for p in R.row_passes(z, max_rows):
                n = int(z.reads[p][3][iwe]) - int(z.reads[p][3][iws])
                c["unusable" if (n < 0 or n > 63) else ("paired" if n <= 31 else "unpaired")] += 1
    return c


def planted(seed, both=True):
    """ZMWs of given passes (tools/coverage_synth.py): both strands, partial passes, 20-base insertions in three passes and a 70-base insertion in one, 36 passes with two of
    random sequence among the first 32, a ZMW of three unrelated passes between two good ones, three extra bases in front of the molecule in passes of both strands"""
    import coverage_synth as S
    rng = np.random.default_rng(seed)
    t = [S.rnd(rng, n) for n in (300, 201, 128, 100, 257, 66, 60, 420)]
    # (the kinetics alignment prefers DIAG on ties, so a random block is shredded: its bases take the neighbouring columns one by one and the displaced ones
    # become short insertions.  A run of one base that differs from both neighbours stays one insertion)
    run = lambda at: np.full(20, [x for x in range(4) if x not in (t[0][at - 1], t[0][at])][0], np.uint8)
    z0 = S.blocked(t[0], run(147), 147, {3, 4}, 10, both)
    z0[8] = S.Pass(S.with_block(t[0], run(63), 63), z0[8].rev)
    z0[6] = S.Pass(S.with_block(t[0], S.rnd(rng, 70), 211), z0[6].rev)
    z1 = S.with_partials(t[1], 8, (0.6, 0.5), both)
    bad = [S.Pass(S.rnd(rng, 200), False) for _ in range(3)]
    z3 = S.clean(t[7], 36, both)
    z3[5], z3[17] = S.Pass(S.rnd(rng, 420), z3[5].rev), S.Pass(S.rnd(rng, 420), z3[17].rev)
    zs = [z0, z1, bad, z3] + [S.clean(x, 12, both) for x in t[2:7]]
    # leading inserted bases: three extra bases in front of the molecule (for a pass of the opposite strand that is the end of its read), in a pass of each strand
    for z, ps in ((0, (2, 5)), (4, (4, 7))):
        for q in ps:
            x = zs[z][q].tpl
            zs[z][q] = S.Pass(S.with_block(x, np.full(3, (int(x[0]) + 2) % 4, np.uint8), 0), zs[z][q].rev)
    return S.batch(zs, rng), zs


# ---------------------------------------------------------------- parity
@gpu
@pytest.mark.parametrize("seed,T,R_", [(1, 100, 20), (2, 22, 32), (3, 128, 5)])
def test_parity_on_synthetic_batches(handle, seed, T, R_):
    rng = np.random.default_rng(seed)
    b = api.synth(int(rng.integers(4, 13)), (3, 40), (60, 700), seed=seed)
    res, ho, exp, zmws = run_and_compare(handle, b, hopts(T, R_))
    c, s = census(exp, zmws), segment_lengths(zmws, R_)
    assert ho.n_tiles == int(ho.counts[0]) > b.n_zmw and c["opposite_rows"] > 0 and c["short_tile"] > 0
    assert s["paired"] > 100 and min(c["del_first_core_col"], c["del_last_core_col"], c["seam_insertion"]) > 0, (c, s)
    if R_ == 32:
        assert c["missing_rows"] > 0 and (exp["tile_rows"] == 32).any()          # ZMWs with fewer and with more than 32 passes


@gpu
def test_planted_rows_and_both_trace_backs(handle):
    b, zs = planted(7)
    o = hopts(22, 32)
    res, ho, exp, zmws = run_and_compare(handle, b, o)
    c, s = census(exp, zmws), segment_lengths(zmws, 32)
    assert res.seq_len[2] == 0 and res.seq_len[1] > 0 and res.seq_len[3] > 0                  # the failing ZMW between two good ones
    assert sorted(set(exp["tile_zmw"].tolist())) == [0, 1] + list(range(3, b.n_zmw))
    assert s["paired"] > 0 and s["unpaired"] > 0 and s["unusable"] > 0, s
    print("census", dict(c), "segments", dict(s))
    assert c["ins>=12"] > 0 and c["code5_to_the_tile_end"] > 0, c
    assert c["leading_insertion_forward"] > 0 and c["leading_insertion_opposite"] > 0, c          # both "no DIAG to the left" branches: ins = r, and n - 1 - r
    # the planted ones (the channel may take one of the three away, or the base on position 0): on consensus position 0 a planted pass of each strand carries
    # two inserted bases or more
    lead = {}
    for z, ps in ((0, (2, 5)), (4, (4, 7))):
        g = exp["tile_zmw"].tolist().index(z)
        assert exp["tile_start"][g] == 0 and zmws[z].cores[0][0] == 0
        rp = exp["row_pass"][g].tolist()
        lead.update({(z, p): (int(exp["row_strand"][g, rp.index(p)]), int(exp["cells"][g, rp.index(p), 0, 3])) for p in ps})
    assert {st for st, ins in lead.values() if ins >= 2} == {0, 1}, lead
    assert min(c["del_first_core_col"], c["del_last_core_col"], c["seam_insertion"], c["opposite_rows"]) > 0, c
    # the 70-base insertion: pass 6 of ZMW 0 has no segment in one window and is covered on both sides of it
    g0 = [g for g in range(ho.n_tiles) if exp["tile_zmw"][g] == 0]
    row6 = np.concatenate([exp["cells"][g, list(exp["row_pass"][g]).index(6), :exp["tile_len"][g], 0] for g in g0])
    five = np.flatnonzero(row6 == 5)
    assert 0 < len(five) <= 64 and five[0] > 0 and five[-1] < len(row6) - 1 and (np.diff(five) == 1).all(), five
    # 36 passes, two of the first 32 invalid: the 32 rows take passes beyond the first group of 32
    g3 = [g for g in range(ho.n_tiles) if exp["tile_zmw"][g] == 3]
    rp = exp["row_pass"][g3[0]].tolist()
    assert len(g3) > 0 and exp["tile_rows"][g3[0]] == 32 and 5 not in rp and 17 not in rp and rp[-1] == 33 and rp == sorted(rp), rp
    # the partial passes of ZMW 1 stop short: their rows are 5 from some window on (or up to one)
    valid1 = R.row_passes(zmws[1], 32)
    assert any(p >= 8 for p in valid1), valid1
    g1 = [g for g in range(ho.n_tiles) if exp["tile_zmw"][g] == 1]
    part = np.concatenate([exp["cells"][g, valid1.index(max(valid1)), :exp["tile_len"][g], 0] for g in g1])
    assert (part == 5).sum() > 40 and (part < 5).sum() > 40, Counter(part.tolist())


@gpu
@pytest.mark.parametrize("R_", [1, 20])
def test_rows_at_the_capacity(built, R_):
    """ZMWs of R - 1, R and R + 1 valid passes (R = 1: one with none, which has no consensus, one with 1 and one with 2, under min_passes 1)"""
    import coverage_synth as S
    rng = np.random.default_rng(20 + R_)
    op = api.default_opts()
    op.min_passes = 1
    op.min_rq = 0.0
    h = api.Handle(0, opts=op)
    try:
        t = S.rnd(rng, 150)
        counts = [max(R_ - 1, 0), R_, R_ + 1]
        zs = [S.clean(t, k, True) if k else [S.Pass(S.rnd(rng, 12), False)] for k in counts]
        b = S.batch(zs, rng)
        res, ho, exp, zmws = run_and_compare(h, b, hopts(16, R_))
        got = {int(z): int(exp["tile_rows"][list(exp["tile_zmw"]).index(z)]) for z in set(exp["tile_zmw"].tolist())}
        valid = {z: len(R.row_passes(zmws[z], 255)) for z in got}
        assert got == {z: min(R_, valid[z]) for z in got} and set(got) >= {1, 2} and sorted(valid.values())[-2:] == [R_, R_ + 1], (got, valid)
        if R_ == 20:
            assert valid[0] == 19 and census(exp, zmws)["missing_rows"] > 0
    finally:
        h.close()


# ---------------------------------------------------------------- tile seams against window seams
@gpu
@pytest.mark.parametrize("T", [16, 22, 100, 128])
def test_tile_seams(handle, T):
    import coverage_synth as S
    rng = np.random.default_rng(T)
    short = T - 30 if T >= 100 else T - 4                                                          # (opts.min_length is 10: a consensus of 12 bases exists)
    lens = [T * 3, T * 3, T * 2 + 1, T * 2 + 1, T * 4 + 1, T, T, short, short]
    b = S.batch([S.clean(S.rnd(rng, n), 14, True) for n in lens], rng)
    res, ho, exp, zmws = run_and_compare(handle, b, hopts(T, 8))
    L = res.seq_len
    assert any(l % T == 0 and l > T for l in L) and any(l % T == 1 for l in L), L.tolist()            # L = kT, and a last tile of one position
    assert census(exp, zmws)["tile_of_1"] > 0
    assert any(l == T for l in L) and any(0 < l < T for l in L), L.tolist()                        # L = T and L < T
    for z in range(b.n_zmw):                                                                       # the tiles of a ZMW cover its consensus once
        g = [i for i in range(ho.n_tiles) if exp["tile_zmw"][i] == z]
        assert exp["tile_start"][g].tolist() == list(range(0, int(L[z]), T)) and int(exp["tile_len"][g].sum()) == int(L[z])


# ---------------------------------------------------------------- selection
@gpu
def test_selection_at_the_qv_cap(built):
    op = api.default_opts()
    op.max_qv = 20
    h = api.Handle(0, opts=op)
    try:
        b = api.synth(6, (6, 12), (150, 500), seed=5)
        plain = h.consensus(b)
        T = 22
        res20, ho20, exp20, _ = run_and_compare(h, b, hopts(T, 4, 20))
        res21, ho21, exp21, _ = run_and_compare(h, b, hopts(T, 4, 21))
        _, ho0, _, _ = run_and_compare(h, b, hopts(T, 4, 0))
        _, ho94, exp94, _ = run_and_compare(h, b, hopts(T, 4, 94))
        assert ho0.counts[1] == 0 and ho94.counts[1] == ho94.counts[0] == sum((int(l) + T - 1) // T for l in plain.seq_len)
        capped = {(int(z), int(s)) for z, s, ln, q in zip(exp94["tile_zmw"], exp94["tile_start"], exp94["tile_len"], exp94["tile_qsum"]) if q == 20 * ln}
        in20 = set(zip(exp20["tile_zmw"].tolist(), exp20["tile_start"].tolist())); in21 = set(zip(exp21["tile_zmw"].tolist(), exp21["tile_start"].tolist()))
        assert len(capped) > 3 and not (capped & in20) and capped <= in21 and in21 == set(zip(exp94["tile_zmw"].tolist(), exp94["tile_start"].tolist()))
        assert 0 < len(in20) < len(in21)
        for z, s, ln, q in zip(ho94.tile_zmw, ho94.tile_start, ho94.tile_len, ho94.tile_qsum):            # qsum against a plain consensus run's qual bytes
            assert int(q) == int(plain.quals(int(z))[int(s):int(s) + int(ln)].astype(np.int64).sum())
    finally:
        h.close()


# ---------------------------------------------------------------- order and capacity
GUARD = 0xA5


def guarded(b, max_tiles, o, pinned=False):
    """a Handoff whose arrays are followed by 64 guard bytes each"""
    keep, arrays = [], {}
    for k, (sh, dt) in api.Handoff.shapes(max_tiles, o).items():
        nb = int(np.prod(sh)) * np.dtype(dt).itemsize
        raw = api._pinned_array(nb + 64, np.uint8, keep) if pinned else np.zeros(nb + 64, np.uint8)
        raw[...] = GUARD
        arrays[k] = raw[:nb].view(dt).reshape(sh)
        keep.append(raw)
    return api.Handoff(o, max_tiles, arrays, False, keep), [r for r in keep if isinstance(r, np.ndarray)]


@gpu
@pytest.mark.parametrize("form", ["consensus", "submit"])
def test_capacity_and_guards(handle, form):
    b, _ = planted(9)
    o = hopts(100, 6, 94)
    _, full, exp, _ = run_and_compare(handle, b, o)
    nsel = int(full.counts[1])
    assert nsel > 6
    for m in (nsel - 1, nsel, nsel + 3):
        ho, raws = guarded(b, m, o, pinned=form == "submit")
        if form == "submit":
            res = api.Results.allocate(b, pinned=True)
            t = handle.submit(b, res, handoff=ho)
            handle.wait(t); handle.release(t)
        else:
            handle.consensus_handoff(b, handoff=ho)
        assert ho.counts.tolist() == [int(full.counts[0]), nsel] and ho.n_tiles == min(m, nsel)
        for k in FIELDS[1:]:
            assert np.array_equal(getattr(ho, k)[:ho.n_tiles], getattr(full, k)[:ho.n_tiles]), (m, k)
        for r in raws:
            assert (r[-64:] == GUARD).all(), m


# ---------------------------------------------------------------- invariance
def res_bytes(res):
    n = res.seq_off[-1]
    out = [res.status, res.seq_len, res.rq, res.np_, res.ec, res.iters, res.n_windows, res.fn, res.rn]
    for z in range(len(res.status)):
        out += [res.sequence(z), res.quals(z), res.raw(z)] + ([res.kinetics(z)] if res.kin is not None else [])
    return b"".join(np.ascontiguousarray(a).tobytes() for a in out)


def ho_bytes(ho):
    ho = ho.host()
    return b"".join(np.ascontiguousarray(getattr(ho, k)[:(2 if k == "counts" else ho.n_tiles)]).tobytes() for k in FIELDS)


@gpu
def test_results_do_not_change_and_runs_repeat(built):
    op = api.default_opts()
    op.hifi_kinetics = 1
    h = api.Handle(0, opts=op)
    try:
        b = api.synth(5, (4, 14), (200, 600), seed=12)
        res0 = api.Results.allocate(b, kinetics=True)
        p0 = api.Pileup.allocate(res0)
        h._fused("consensus", b, res0, api._requests(p0))
        res1 = api.Results.allocate(b, kinetics=True)
        p1 = api.Pileup.allocate(res1)
        _, ho1 = h.consensus_handoff(b, opts=hopts(100, 20, 94), res=res1, pileup=p1)
        exp, _ = R.from_engine(h, b, res1, ho1.opts, ho1.max_tiles)
        assert same(ho1, exp) > 5
        assert res_bytes(res0) == res_bytes(res1) and all(np.array_equal(getattr(p0, k), getattr(p1, k)) for k in ("coverage", "matches", "mismatches"))
        assert res1.kin is not None and res1.kin.any() and p1.coverage.any()
        _, ho2 = h.consensus_handoff(b, opts=hopts(100, 20, 94))
        assert ho_bytes(ho1) == ho_bytes(ho2)                                                     # two runs, with and without the other requests
    finally:
        h.close()


CHILD_BATCH, CHILD_OPTS = ((6, (5, 12), (200, 700)), 14), (100, 20, 94)      # tests/handoff_child.py: the batch and options of the fresh processes


def child(mode, **env):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "handoff_child.py"), mode], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    return dict(line.split()[1:3] for line in out.stdout.splitlines() if line.startswith("sha "))


@gpu
def test_tickets_in_flight_each_get_their_own(handle):
    b = api.synth(*CHILD_BATCH[0], seed=CHILD_BATCH[1]).pinned()
    optss = [hopts(*CHILD_OPTS), hopts(16, 3, 94), hopts(128, 32, 45)]
    want = []
    for o in optss:
        _, ho, exp, _ = run_and_compare(handle, b, o)
        want.append(ho_bytes(ho))
    assert len(set(want)) == 3 and all(len(w) > 1000 for w in want[:2])
    hos = [api.Handoff.allocate(b, None, o, pinned=True) for o in optss]
    ress = [api.Results.allocate(b, pinned=True) for _ in hos]
    ts = [handle.submit(b, r, handoff=ho) for r, ho in zip(ress, hos)]
    for t in ts:
        handle.wait(t)
    for t in ts:
        handle.release(t)
    assert [ho_bytes(ho) for ho in hos] == want                                                   # the ticketed form agrees with the synchronous one
    plain = handle.consensus(b)
    assert all(res_bytes(r) == res_bytes(plain) for r in ress)


@gpu
def test_device_destination(handle):
    """torch tensors on the handle's GPU as the destination, synchronous and ticketed: moved to the host, the bytes of a host destination"""
    b = api.synth(*CHILD_BATCH[0], seed=CHILD_BATCH[1])
    want = hashlib.sha256(ho_bytes(handle.consensus_handoff(b, opts=hopts(*CHILD_OPTS))[1])).hexdigest()
    assert child("device") == {"sync": want, "ticket": want}


@gpu
def test_launch_pieces(handle):
    """a small CCSX_POLISH_MAX_BLOCKS (read once per process) forces k_tile_rows into pieces of 16 window slots: the same bytes"""
    b = api.synth(*CHILD_BATCH[0], seed=CHILD_BATCH[1])
    res, ho = handle.consensus_handoff(b, opts=hopts(*CHILD_OPTS))
    assert int(res.n_windows.sum()) > 64
    assert child("pieces", CCSX_POLISH_MAX_BLOCKS="16") == {"sync": hashlib.sha256(ho_bytes(ho)).hexdigest()}


@gpu
def test_ip_is_zero_without_ipd(handle):
    b = api.synth(4, 6, 300, seed=15)
    o = hopts(100, 6, 94)
    res = api.Results.allocate(b)
    ho = api.Handoff.allocate(b, None, o)
    cb, cr = b.c_struct(), res.c_struct()
    cb.ipd = None
    hreq = api._handoff_request(ho)
    assert api.lib().ccsx_consensus_handoff(handle._h, C.byref(cb), C.byref(cr), None, C.byref(hreq[0])) == 0, api.lib().ccsx_last_error()
    exp, _ = R.from_engine(handle, b, res, o, ho.max_tiles, ipd=False)
    assert same(ho, exp) > 0 and not ho.cells[..., 2].any() and ho.cells[..., 1].any()
    _, ho2, _, _ = run_and_compare(handle, b, o)
    assert ho2.cells[..., 2].any()


# ---------------------------------------------------------------- arguments
def test_structs_match_the_header(built, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ccsx.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d\\n", '
                   'sizeof(ccsx_handoff_opts), offsetof(ccsx_handoff_opts, skip_above), offsetof(ccsx_handoff_opts, reserved), sizeof(ccsx_handoff_out), '
                   'offsetof(ccsx_handoff_out, counts), offsetof(ccsx_handoff_out, tile_rows), offsetof(ccsx_handoff_out, row_pass), offsetof(ccsx_handoff_out, cells), '
                   'sizeof(ccsx_handoff_request), offsetof(ccsx_handoff_request, out), offsetof(ccsx_handoff_request, reserved), sizeof(ccsx_requests), '
                   'CCSX_ABI_VERSION, CCSX_SPEC_VERSION);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    Op, Out, Q = api.HandoffOpts, api.CHandoffOut, api.CHandoffRequest
    assert got == [C.sizeof(Op), Op.skip_above.offset, Op.reserved.offset, C.sizeof(Out), Out.counts.offset, Out.tile_rows.offset, Out.row_pass.offset, Out.cells.offset,
                   C.sizeof(Q), Q.out.offset, Q.reserved.offset, C.sizeof(api.CRequests), 6, 8]
    assert got[0] == 16 and got[3] == 80 and got[8] == 32 and got[11] == 64
    L = api.lib()
    assert L.ccsx_handoff_rule_version() == 1 and L.ccsx_abi_version() == 6 and L.ccsx_spec_version() == 8
    o = api.handoff_opts_default()
    assert (o.tile_len, o.max_rows, o.skip_above, o.reserved) == (100, 20, 45, 0)
    assert (api.HANDOFF_NO_BASE, api.HANDOFF_NO_SEGMENT) == (R.NO_BASE, R.NO_SEGMENT) == (4, 5)
    assert {"ccsx_handoff_opts_default", "ccsx_handoff_rule_version", "ccsx_consensus_handoff", "ccsx_submit_handoff"} <= set(api.EXPORTS)


def bad_requests(b):
    """(message, request, keep) of every refusal"""
    out = []

    def req(opts=None, reserved=(0, 0), drop=None, max_tiles=4, no_out=False):
        o = opts if opts is not None else hopts()
        ho = api.Handoff.allocate(b, 4, hopts())
        co = ho.c_struct()
        co.max_tiles = max_tiles
        if drop:
            setattr(co, drop, None)
        return api.CHandoffRequest(C.pointer(o), None if no_out else C.pointer(co), (C.c_int64 * 2)(*reserved)), (o, ho, co)
    out.append(("null handoff out", *req(no_out=True)))
    for k in FIELDS:
        out.append(("handoff out arrays missing", *req(drop=k)))
    for m in (0, -3, (1 << 26) + 1):
        out.append(("max_tiles must be", *req(max_tiles=m)))
    for T, R_, s in ((15, 20, 45), (129, 20, 45), (100, 0, 45), (100, 33, 45), (100, 20, -1), (100, 20, 95)):
        out.append(("handoff options out of range", *req(opts=hopts(T, R_, s))))
    o = hopts()
    o.reserved = 1
    out.append(("handoff options: reserved must be 0", *req(opts=o)))
    out.append(("handoff request: reserved must be 0", *req(reserved=(0, 1))))
    out.append(("handoff request: reserved must be 0", *req(reserved=(5, 0))))
    return out


def call(entry, h, b, res, q, rq=None):
    cb, cr = b.c_struct(), res.c_struct()
    t = C.c_int64(-7)
    args = [h, C.byref(cb), C.byref(cr), C.byref(rq) if rq is not None else None, C.byref(q) if q is not None else None]
    rc = getattr(api.lib(), entry)(*(args + [C.byref(t)] if entry == "ccsx_submit_handoff" else args))
    assert rc == 0 or t.value == -7                                     # a refused submit hands out no ticket
    return rc


@pytest.mark.parametrize("entry", ["ccsx_consensus_handoff", "ccsx_submit_handoff"])
def test_entry_points_refuse_bad_requests(built, entry):
    L = api.lib()
    b = api.synth(3, 4, 300, seed=2)
    res = api.Results.allocate(b)
    for msg, q, keep in bad_requests(b):
        assert call(entry, None, b, res, q) < 0 and msg.encode() in L.ccsx_last_error() and entry.encode() in L.ccsx_last_error(), (msg, L.ccsx_last_error())
    assert call(entry, None, b, res, None) < 0 and b"null handoff request" in L.ccsx_last_error()
    q, keep = bad_requests(b)[0][1:]
    rq = api.CRequests(None, None, None, None, None, (C.c_void_p * 3)(None, 8, None))
    assert call(entry, None, b, res, q, rq) < 0 and b"ccsx_requests: reserved must be NULL" in L.ccsx_last_error()


@gpu
@pytest.mark.parametrize("entry", ["ccsx_consensus_handoff", "ccsx_submit_handoff"])
def test_a_refusing_handle_still_works(handle, entry):
    L = api.lib()
    b = api.synth(3, 5, 300, seed=2)
    res = api.Results.allocate(b)
    before = ho_bytes(handle.consensus_handoff(b, opts=hopts(100, 5))[1])
    for msg, q, keep in bad_requests(b):
        assert call(entry, handle._h, b, res, q) < 0 and msg.encode() in L.ccsx_last_error(), (msg, L.ccsx_last_error())
    assert len(before) > 1000 and ho_bytes(handle.consensus_handoff(b, opts=hopts(100, 5))[1]) == before
    t = handle.submit(b, api.Results.allocate(b, pinned=True))
    handle.wait(t); handle.release(t)

"""The polisher hand-back on the GPU (ccsx_refine_batch / ccsx_submit_refine; DESIGN.md §2 "Polisher hand-back"): the results against the polish seam on drafts
spliced in numpy (byte for byte), the report against tests/refine_ref.py (integer for integer, rq_merged bit for bit).  Every test asserts that the case it is
about occurred."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import refine_ref as R
from ccs_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu
QV_TOL = 1e-4          # per-base QVs against the CPU restatement (tests/test_gpu_parity.py)
NO_CONSENSUS = 4       # the ZMW of two passes


def lab_batch():
    """twelve ZMWs of 5-8 passes and 300-1500 bases; ZMW 3 is long enough for 300 tiles, ZMW 4 has two passes and so no consensus"""
    return api.concat([api.synth(3, (5, 8), (400, 900), seed=31), api.synth(1, 6, 1500, seed=32), api.synth(1, 2, 400, seed=33),
                       api.synth(7, (5, 8), (300, 1500), seed=34)])


class Lab:
    def __init__(self, handle, batch=None):
        self.batch = batch if batch is not None else lab_batch()
        self.base = handle.consensus(self.batch)
        drafts = handle.draft(self.batch)                              # (kept until the copy below is made: its arrays are page-locked blocks of its own)
        self.backbone = drafts.backbone.copy()                         # the draft's orientation is SEQ's
        self.L = self.base.seq_len
        self.C = np.diff(self.base.seq_off)
        self.passes = np.diff(self.batch.read_off)

    def ref(self, tiles: api.RefineTiles, backbone=None) -> dict:
        t = tiles.host()
        return R.refine(self.base.seq_off, self.L, self.base.seq, self.base.qual, self.passes, self.backbone if backbone is None else backbone,
                        {k: getattr(t, k) for k in t.FIELDS}, t.stride)


def lab_opts():
    """min_rq 0: a refined sequence carries the errors the tests put into it, and QV_ONLY scores them low; the reads come back all the same"""
    op = api.default_opts()
    op.min_rq = 0.0
    return op


@pytest.fixture(scope="module")
def handle(built):
    h = api.Handle(0, opts=lab_opts())
    yield h
    h.close()


@pytest.fixture(scope="module")
def lab(handle):
    return Lab(handle)


def res_bytes(res):
    out = [res.status, res.seq_len, res.rq, res.np_, res.ec, res.iters, res.n_windows, res.fn, res.rn]
    for z in range(len(res.status)):
        out += [res.sequence(z), res.quals(z), res.raw(z)] + ([res.kinetics(z)] if res.kin is not None else [])
    return b"".join(np.ascontiguousarray(a).tobytes() for a in out)


def rep_bytes(rep):
    out = [rep.counts, rep.code, rep.n_applied, rep.new_len, rep.rq_merged] + [rep.quals(z) for z in range(len(rep.code))]
    return b"".join(np.ascontiguousarray(a).tobytes() for a in out)


def same_results(a, b):
    for k in ("status", "seq_len", "np_", "iters", "n_windows", "fn", "rn", "rq", "ec"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k
    for z in range(len(a.status)):
        assert np.array_equal(a.sequence(z), b.sequence(z)) and np.array_equal(a.quals(z), b.quals(z)) and a.raw(z).tobytes() == b.raw(z).tobytes(), z
        if a.kin is not None:
            assert np.array_equal(a.kinetics(z), b.kinetics(z)), z


def same_report(rep, ref):
    for k in ("counts", "code", "n_applied", "new_len"):
        assert getattr(rep, k).tolist() == ref[k].tolist(), (k, getattr(rep, k).tolist(), ref[k].tolist())
    assert rep.rq_merged.tobytes() == ref["rq_merged"].tobytes(), (rep.rq_merged, ref["rq_merged"])
    for z in range(len(rep.code)):
        assert np.array_equal(rep.quals(z), ref["quals"][z]), z


def run_and_compare(handle, lab, tiles, backbone=None):
    """the engine against the restatement: results against the polish seam on the numpy-spliced drafts, the report against refine_ref"""
    bb = lab.backbone if backbone is None else backbone
    ref = lab.ref(tiles, bb)
    res, rep = handle.refine(lab.batch, lab.base, tiles, bb)
    same_report(rep, ref)
    same_results(res, handle.polish(lab.batch, R.spliced_drafts(lab.batch, ref, bb), flags=api.QV_ONLY))
    return res, rep, ref


def tiles_of(rows, stride=128, **kw) -> api.RefineTiles:
    """rows: (zmw, start, len, new_seq, new_qual) or (zmw, start, len, new_seq, new_qual, new_len) in list order"""
    nl = [r[5] if len(r) > 5 else len(r[3]) for r in rows]
    return api.RefineTiles.from_arrays([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], nl, [r[3] for r in rows], [r[4] for r in rows],
                                       stride=stride, **kw)


def rnd_row(rng, k):
    return rng.integers(0, 4, k).astype(np.uint8), rng.integers(0, 94, k).astype(np.uint8)


def edited(rng, seg, k):
    """what a polisher returns for the bases seg: the same bases with a few changed, and bases taken out or put in to reach the length k; random quals"""
    row = [int(x) for x in seg]
    for i in range(0, len(row), 17):
        row[i] = (row[i] + 1 + int(rng.integers(0, 3))) & 3
    while len(row) > k:
        del row[int(rng.integers(0, len(row)))]
    while len(row) < k:
        row.insert(int(rng.integers(0, len(row) + 1)), int(rng.integers(0, 4)))
    return np.array(row, np.uint8), rng.integers(0, 94, k).astype(np.uint8)


def half_of_the_tiles(lab, rng, zs, T=100, keep=0):
    """every second T-base tile of the ZMWs zs replaced by a row of about the same length (the first replaced tile: keep + 2 k)"""
    rows = []
    for z in zs:
        for t, s in enumerate(range(0, int(lab.L[z]), T)):
            if t % 2 == keep:
                ln = min(T, int(lab.L[z]) - s)
                rows.append((z, s, ln, *edited(rng, lab.base.sequence(z)[s:s + ln], max(0, ln + int(rng.integers(-3, 4))))))
    return rows


# ---------------------------------------------------------------- 1: identity
@gpu
@pytest.mark.parametrize("kinetics", [False, True])
def test_no_tiles_is_the_qv_only_polish_of_the_base(built, kinetics):
    op = api.default_opts()
    op.hifi_kinetics = int(kinetics)
    h = api.Handle(0, opts=op)
    try:
        lab = Lab(h)
        assert lab.L[NO_CONSENSUS] == 0 and (np.delete(lab.L, NO_CONSENSUS) > 250).all()
        tiles = api.RefineTiles.allocate(0, 128)
        res, rep, ref = run_and_compare(h, lab, tiles)
        assert (res.kin is not None) == kinetics
        want = [1] * lab.batch.n_zmw
        want[NO_CONSENSUS] = 0
        assert rep.code.tolist() == want and rep.counts.tolist() == [0, 0, 0] and rep.n_applied.sum() == 0
        perr = R.perr_table()
        for z in range(lab.batch.n_zmw):
            assert np.array_equal(res.sequence(z), lab.base.sequence(z)) and np.array_equal(rep.quals(z), lab.base.quals(z))
            assert rep.rq_merged[z].tobytes() == R.rq_of(lab.base.quals(z), perr).tobytes()
        assert rep.rq_merged[NO_CONSENSUS] == 0 and 0.9 < rep.rq_merged[0] < 1
    finally:
        h.close()


# ---------------------------------------------------------------- 2: the splice lab
def lab_rows(lab, rng, U):
    L = lab.L
    rows = []
    # ZMW 0: a substitution-only tile starting at 0, new_len = len - 3, len + 5 and 0, a short last tile ending exactly at L
    z = 0
    sub = lab.base.sequence(z)[:100].copy()
    sub[::7] = (sub[::7] + 1) & 3
    seg = lambda a, k: lab.base.sequence(z)[a:a + k]
    rows += [(z, 0, 100, sub, rnd_row(rng, 100)[1]), (z, 100, 50, *edited(rng, seg(100, 50), 47)), (z, 160, 40, *edited(rng, seg(160, 40), 45)), (z, 210, 10, *rnd_row(rng, 0)),
             (z, int(L[z]) - 17, 17, *edited(rng, seg(int(L[z]) - 17, 17), 20))]
    # ZMW 1: adjacent tiles (end == next start), tile_len 1, new_len == U
    z = 1
    rows += [(z, 30, 20, *rnd_row(rng, 20)), (z, 50, 1, *rnd_row(rng, 3)), (z, 51, 30, *rnd_row(rng, 28)), (z, 200, 1, *rnd_row(rng, U)), (z, 201, 100, *rnd_row(rng, 60))]
    # ZMW 2: 70 tiles, ZMW 3: 300 tiles, of length 1-3 (more than a wave's lanes, more than a workgroup's threads)
    for z, cnt in ((2, 70), (3, 300)):
        for k in range(cnt):
            rows.append((z, 3 + 4 * k, int(rng.integers(1, 4)), *rnd_row(rng, int(rng.integers(0, 5)))))
    # ZMW 4 has no consensus; 5 and 6 have no tiles; 7 and 9-11 have every second 100-base tile replaced; 8 has tiles and backbone -1
    rows += half_of_the_tiles(lab, rng, [7, 8, 9, 10, 11])
    return rows


@gpu
def test_splice_lab(handle, lab):
    U = 127
    rng = np.random.default_rng(61)
    rows = lab_rows(lab, rng, U)
    tiles = tiles_of(rows, stride=U)
    bb = lab.backbone.copy()
    bb[8] = -1
    assert lab.L[2] > 3 + 4 * 70 and lab.L[3] > 3 + 4 * 300 and lab.L[0] > 300 and lab.L[1] > 320
    res, rep, ref = run_and_compare(handle, lab, tiles, bb)
    assert rep.code.tolist() == [2, 2, 2, 2, 0, 1, 1, 2, 0, 2, 2, 2], rep.code.tolist()
    assert rep.n_applied[:4].tolist() == [5, 5, 70, 300] and rep.counts.tolist() == [8, int(rep.n_applied.sum()), 0]
    assert int(tiles.new_len.max()) == U == 127 and (tiles.new_len == 0).any() and (tiles.tile_len == 1).any()
    assert rep.new_len[0] == lab.L[0] - 3 + 5 - 10 + 3 and (rep.new_len[[5, 6]] == lab.L[[5, 6]]).all() and rep.new_len[8] == 0
    assert res.seq_len[8] == 0 and res.status[8] != 0 and (res.status[[0, 7, 9, 10, 11]] == 0).all(), res.status.tolist()
    for z in (0, 7, 9, 10, 11):                            # QV_ONLY: the sequence that comes back is the spliced one
        assert np.array_equal(res.sequence(z), ref["drafts"][z]) and not np.array_equal(res.sequence(z), lab.base.sequence(z)), z
        assert res.rq[z] < lab.base.rq[z]                  # the planted errors are scored: res.rq is the re-score's own
    # two ZMWs against the CPU restatement of the polish seam
    for z in (0, 1):
        one = lab.batch.slice(z, z + 1)
        d = api.Drafts.allocate(one)
        d.set_draft(0, ref["drafts"][z], backbone=int(bb[z]))
        want = O.polish_batch(handle.model, handle.opts, one, d, api.Results.allocate(one), flags=api.QV_ONLY)
        assert res.status[z] == want.status[0] and np.array_equal(res.sequence(z), want.sequence(0)) and np.array_equal(res.quals(z), want.quals(0)), z
        assert np.allclose(res.raw(z), want.raw(0), atol=QV_TOL, rtol=0) and abs(float(res.rq[z]) - float(want.rq[0])) < 1e-6, z


# ---------------------------------------------------------------- 3: refused tiles
@gpu
def test_refused_tiles_keep_the_base_sequence(handle, lab):
    U = 128
    rng = np.random.default_rng(62)
    L, C_ = lab.L, lab.C
    big = 2 ** 31 - 1
    sym, q94 = rnd_row(rng, 10), rnd_row(rng, 10)
    sym[0][9], q94[1][9] = 4, 94                           # at the last read entry
    beyond = (np.concatenate([rnd_row(rng, 10)[0], [7]]).astype(np.uint8), np.concatenate([rnd_row(rng, 10)[1], [200]]).astype(np.uint8))
    # ZMW 7 grows to exactly its capacity (accepted), ZMW 9 to one more (TOO_LONG): tiles of length 1 replaced by full rows, the last one by what is left
    def grow(z, by):
        rows, left, s = [], by, 5
        while left > 0:
            k = min(U - 1, left)
            rows.append((z, s, 1, *rnd_row(rng, k + 1)))
            left, s = left - k, s + 2
        return rows
    rows = [(0, big, 5, *rnd_row(rng, 5)),                                                 # -1: start = 2^31 - 1
            (1, 10, 5, *rnd_row(rng, 5)), (1, 20, big, *rnd_row(rng, 5)),                  # -1: len = 2^31 - 1, after a good tile
            (2, 10, 5, *rnd_row(rng, 5), -1),                                              # -1: new_len = -1
            (3, 10, 5, *rnd_row(rng, 5), U + 1),                                           # -1: new_len = U + 1
            (5, 40, 10, *rnd_row(rng, 9)), (5, 49, 5, *rnd_row(rng, 5)),                   # -2: starts on its predecessor's last position
            (6, 10, 10, *sym)] + grow(7, int(C_[7] - L[7])) + [                           # -3: symbol 4; ZMW 7: L' = C
            (8, 10, 10, *q94)] + grow(9, int(C_[9] - L[9]) + 1) + [                       # -3: qual 94; ZMW 9: L' = C + 1
            (10, 10, 10, *beyond, 10),                                                     # refined: the bad entries lie beyond new_len
            (11, 10, 5, *rnd_row(rng, 5))]                                                 # -6 below: backbone = pass count
    tiles = tiles_of(rows, stride=U)
    bb = lab.backbone.copy()
    bb[11] = lab.passes[11]
    res, rep, ref = run_and_compare(handle, lab, tiles, bb)
    assert rep.code.tolist() == [-1, -1, -1, -1, 0, -2, -3, 2, -3, -4, 2, -6], rep.code.tolist()
    assert rep.new_len[7] == C_[7] > L[7] and rep.new_len[11] == 0 and res.seq_len[11] == 0
    for z in (0, 1, 2, 3, 5, 6, 8, 9):                     # each keeps the base sequence, whole
        assert rep.new_len[z] == L[z] and rep.n_applied[z] == 0 and np.array_equal(res.sequence(z), lab.base.sequence(z)) and np.array_equal(rep.quals(z), lab.base.quals(z))
    # L' = 0: a ZMW of its own batch whose one tile deletes everything (U bounds nothing here: new_len = 0)
    one = Lab(handle, lab.batch.slice(5, 7))
    res1, rep1, _ = run_and_compare(handle, one, tiles_of([(0, 0, int(one.L[0]), *rnd_row(rng, 0)), (1, 0, 5, *rnd_row(rng, 5))], stride=U))
    assert rep1.code.tolist() == [-5, 2] and np.array_equal(res1.sequence(0), one.base.sequence(0))
    # the list's order: one tile_zmw below its predecessor, one equal to n_zmw
    good = half_of_the_tiles(lab, rng, [0, 1, 2])
    assert good[0][0] == 0 and good[1][0] == 0 and good[-1][0] == 2
    bad = good[:1] + [(3, 10, 5, *rnd_row(rng, 5))] + good[1:] + [(lab.batch.n_zmw, 0, 5, *rnd_row(rng, 5))]   # ZMW 3 between tiles of ZMW 0: the tile behind it is the violation
    res2, rep2, _ = run_and_compare(handle, lab, tiles_of(bad, stride=U))
    want = [-7] * lab.batch.n_zmw
    want[NO_CONSENSUS] = 0
    assert rep2.counts.tolist() == [0, 0, 2] and rep2.code.tolist() == want and rep2.n_applied.sum() == 0
    for z in range(lab.batch.n_zmw):
        assert np.array_equal(res2.sequence(z), lab.base.sequence(z)) or res2.status[z] != 0


# ---------------------------------------------------------------- 4: round trip with the hand-off
@gpu
def test_round_trip_with_the_handoff(handle, lab):
    o = api.handoff_opts_default()
    o.skip_above = 94                                      # every tile is selected
    base, ho = handle.consensus_handoff(lab.batch, opts=o)
    ho = ho.host()
    n, T = ho.n_tiles, int(o.tile_len)
    assert n == int(ho.counts[0]) > lab.batch.n_zmw and res_bytes(base) == res_bytes(lab.base)
    rows = []
    for g in range(n):
        z, s, ln = int(ho.tile_zmw[g]), int(ho.tile_start[g]), int(ho.tile_len[g])
        a = int(base.seq_off[z]) + s
        rows.append((z, s, ln, base.seq[a:a + ln].copy(), base.qual[a:a + ln].copy()))
    bb = ho.backbones(lab.batch.n_zmw)
    assert bb[NO_CONSENSUS] == -1 and (np.delete(bb, NO_CONSENSUS) >= 0).all()
    res, rep, ref = run_and_compare(handle, lab, tiles_of(rows, stride=T), bb)
    want = [2] * lab.batch.n_zmw
    want[NO_CONSENSUS] = 0
    assert rep.code.tolist() == want and rep.counts.tolist() == [lab.batch.n_zmw - 1, n, 0]
    for z in range(lab.batch.n_zmw):
        assert np.array_equal(ref["drafts"][z], lab.base.sequence(z)) and np.array_equal(rep.quals(z), lab.base.quals(z))
    ident, _ = handle.refine(lab.batch, lab.base, api.RefineTiles.allocate(0, 128), lab.backbone)
    same_results(res, ident)                               # the hand-off's backbones give what the draft's own give


# ---------------------------------------------------------------- 5, 6: device-resident tiles, tickets
CHILD_SEED = 63


def child_rows(lab):
    return half_of_the_tiles(lab, np.random.default_rng(CHILD_SEED), [0, 1, 2, 3, 7, 9])


@gpu
def test_device_resident_tiles(handle, lab):
    """torch tensors on the handle's GPU as the tile list, synchronous and ticketed, in a fresh process that opens torch first: the bytes of the host form"""
    res, rep, _ = run_and_compare(handle, lab, tiles_of(child_rows(lab)))
    assert rep.counts[0] == 6
    want = hashlib.sha256(res_bytes(res) + rep_bytes(rep)).hexdigest()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "refine_child.py")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    got = dict(line.split()[1:3] for line in out.stdout.splitlines() if line.startswith("sha "))
    assert got == {"sync": want, "ticket": want}


@gpu
def test_tickets_in_flight_each_get_their_own(handle, lab):
    b = lab.batch.pinned()
    rng = np.random.default_rng(64)
    sets = [half_of_the_tiles(lab, rng, [0, 1, 2, 3], keep=0), half_of_the_tiles(lab, rng, [5, 6, 7, 9, 10, 11], T=50, keep=1), []]
    plain = res_bytes(handle.consensus(b))
    want = []
    for rows in sets:
        res, rep, _ = run_and_compare(handle, lab, tiles_of(rows))
        want.append(res_bytes(res) + rep_bytes(rep))
    assert len(set(want)) == 3
    for _ in range(2):                                     # two runs give the same bytes
        tl = [tiles_of(rows, pinned=True) for rows in sets]
        ress = [api.Results.allocate(b, pinned=True) for _ in sets]
        reps = [api.RefineReport.allocate(b, pinned=True) for _ in sets]
        ts = [handle.submit_refine(b, lab.base, t, lab.backbone, r, p) for t, r, p in zip(tl, ress, reps)]
        for t in ts:
            handle.wait(t)
        for t in ts:
            handle.release(t)
        assert [res_bytes(r) + rep_bytes(p) for r, p in zip(ress, reps)] == want
    assert res_bytes(handle.consensus(b)) == plain         # a plain consensus afterwards is unchanged


# ---------------------------------------------------------------- 7: arguments
@gpu
def test_bad_arguments_are_refused_and_the_handle_stays_usable(handle, lab):
    L_ = api.lib()
    b, base = lab.batch, lab.base
    rows = half_of_the_tiles(lab, np.random.default_rng(65), [0])
    good = tiles_of(rows)
    res, rep = api.Results.allocate(b), api.RefineReport.allocate(b)
    bb = np.ascontiguousarray(lab.backbone, np.int32)
    other = api.synth(3, 5, 300, seed=66)

    def call(batch=b, base_=base, backbone=bb, tiles=good, res_=res, rep_=rep, edit=None, null=None, ticket=False):
        cs = dict(b=batch.c_struct(), base=base_.c_struct(), t=tiles.c_struct(), res=res_.c_struct(), rep=rep_.c_struct())
        if edit:
            edit(cs)
        a = dict(b=C.byref(cs["b"]), base=C.byref(cs["base"]), bb=backbone.ctypes.data_as(C.POINTER(C.c_int32)), t=C.byref(cs["t"]), res=C.byref(cs["res"]),
                 rep=C.byref(cs["rep"]))
        if null:
            a[null] = None
        tk = C.c_int64(-1)
        args = (handle._h, a["b"], a["base"], a["bb"], a["t"], a["res"], a["rep"])
        rc = L_.ccsx_submit_refine(*args, C.byref(tk)) if ticket else L_.ccsx_refine_batch(*args)
        assert tk.value == -1
        return rc, L_.ccsx_last_error().decode()

    def setter(which, field, value):
        return lambda cs: setattr(cs[which], field, value)

    def reserved(i):
        def f(cs):
            cs["t"].reserved[i] = 1
        return f
    cases = [(dict(null=k), "null argument") for k in ("b", "base", "bb", "t", "res", "rep")]
    cases += [(dict(edit=setter("t", "n_tiles", -1)), "n_tiles"), (dict(edit=setter("t", "stride", 0)), "stride"), (dict(edit=setter("t", "stride", 257)), "stride"),
              (dict(edit=setter("t", "reserved0", 1)), "reserved"), (dict(edit=reserved(0)), "reserved"), (dict(edit=reserved(1)), "reserved")]
    cases += [(dict(edit=setter("t", k, None)), "arrays missing") for k in api.RefineTiles.FIELDS]
    cases += [(dict(edit=setter("rep", "code", None)), "report"), (dict(base_=api.Results.allocate(other)), "another batch"),
              (dict(res_=api.Results.allocate(other)), "too small"), (dict(edit=setter("base", "seq_capacity", 5)), "capacity layout")]
    shifted = api.Results.allocate(b)
    shifted.seq_off[1:-1] += 1
    cases.append((dict(base_=shifted), "capacity layout"))
    for kw, msg in cases:
        for ticket in (False, True):
            rc, err = call(ticket=ticket, **kw)
            assert rc == -1 and msg in err, (kw, rc, err)
    with pytest.raises(RuntimeError, match="null argument"):
        handle._check(L_.ccsx_submit_refine(handle._h, *[None] * 6, None), "ccsx_submit_refine")
    got, grep = handle.refine(b, base, api.RefineTiles.allocate(0, 128), lab.backbone)      # the same handle then runs test 1's case
    same_results(got, handle.polish(b, R.spliced_drafts(b, lab.ref(api.RefineTiles.allocate(0, 128)), lab.backbone), flags=api.QV_ONLY))
    assert grep.code.tolist() == [1, 1, 1, 1, 0] + [1] * 7

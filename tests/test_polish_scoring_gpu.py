"""k_polish_t scores a unit's rows as a two-deep pipeline of row-steps: a row-step's gamma, beta and table pairs are loaded while the row-step before it computes,
and the row's observation byte comes from registers — a chain's next twelve bytes of its read's observation row, loaded as four aligned words and shifted into
place by the residue of the first row's address.  The lane constants of both strands stay packed in one word between units.  The arithmetic of a chain and its
order are unchanged, so every case below runs the whole engine and compares with the CPU restatement BIT FOR BIT — status, seq_len, iters, n_windows, np, rq,
sequence, raw QVs as uint32 — on the shapes at which the new loops can go wrong, and asserts on the restatement's side alone (its alignments, its window bounds,
its counters) that the shape the case is about occurs.  The seeds were chosen on the CPU.  Small batches: a second or two each.

A (window, pass) pair's shape: J = the window's columns with the overhang, I = the pass's bases between the entry rows of the window's first column and of its
end, Wr = 5 + max(|I - J| - 2, 0), nr = min(I, 2 Wr) + 1 rows per chain, first row i0(c) = clamp(floor((2 c I + J) / (2 J)) - Wr, 0, I + 1 - nr) of the lane at
column c.  The loops take other paths with nr (one block of observation bytes up to twelve rows, two and more above; an odd row behind the row pairs), with
i0 & 3 (the shift of the four words), with the number of a wave's units in a block of lanes (one chain, two chains, two chains of different lengths).

One shape of the issue's list does not exist in the restatement, so no case can assert it: a FAVOURABLE insertion behind a draft's last column.  The lane is
enumerated and scored (it feeds the last base's QV), but no pass can vote for it: a base that a pass carries behind the draft's last column is "emitted while
waiting in column Ld" — the entry row of column Ld is the row at which the path ENTERS it (orc_align's trace-back, oracle/ccs_oracle.c: "rstart[j] = row at which
the optimal path ENTERS column j ... insertions emitted while waiting at state j follow it"), and the last window's segment ends at that row, so the extra base lies
outside every segment.  test_lanes_at_the_last_column asserts exactly that on the restatement's entry rows, and takes its favourable `fin` lanes from the
substitution and the deletion of the last column."""
import difflib

import numpy as np
import pytest

from ccs_amd import api
import oracle_lib as O

pytestmark = pytest.mark.gpu

SCORE_BAND, OBS_ROWS = 5, 12


def _bit_exact(res, ref, batch):
    assert np.array_equal(res.status, ref.status), (res.status, ref.status)
    assert np.array_equal(res.seq_len, ref.seq_len)
    assert np.array_equal(res.iters, ref.iters), (res.iters, ref.iters)
    assert np.array_equal(res.n_windows, ref.n_windows)
    assert np.array_equal(res.np_, ref.np_), (res.np_, ref.np_)
    assert np.array_equal(res.rq.view(np.uint32), ref.rq.view(np.uint32)), (res.rq, ref.rq)
    for z in range(batch.n_zmw):
        assert np.array_equal(res.sequence(z), ref.sequence(z)), f"zmw {z}: sequence differs"
        a, b = res.raw(z), ref.raw(z)
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"zmw {z}: raw QVs differ, max |d| = {np.abs(a - b).max() if a.shape == b.shape else 'shape'}"


def _oracle_polish(model, o, batch, drafts):
    O.lib().orc_counts_sync(); O.counts_reset()
    ref = O.polish_batch(model, o, batch, drafts, api.Results.allocate(batch))
    O.lib().orc_counts_sync()
    ref.paths = O.counts()
    return ref


def _oracle_consensus(model, o, batch):
    ref = api.Results.allocate(batch)
    O.lib().orc_counts_sync(); O.counts_reset()
    O.consensus_batch(model, o, batch, ref, nthreads=8)
    O.lib().orc_counts_sync()
    ref.paths = O.counts()
    return ref


def _read(batch, r):
    return O.orient(batch.bases[int(batch.base_off[r]):int(batch.base_off[r + 1])], int(batch.flags[r]) & 1)


def shapes(batch, drafts, o, zs=None):
    """round 0's (window, pass) pairs on the drafts, from the restatement's alignment cascade and window rule alone: a list of dicts z, w, q (the pass in its ZMW),
    rev, J, I (after the trim of max_insertion_size), raw (before it), trimmed.  Passes without a segment in a window, or with one of more than 63 bases, are left out"""
    maxins = 30 if o.max_insertion_size == 0 else o.max_insertion_size
    out = []
    for z in (range(batch.n_zmw) if zs is None else zs):
        d = drafts[z]
        wb = O.windows(d)
        for r in range(int(batch.read_off[z]), int(batch.read_off[z + 1])):
            if int(batch.flags[r]) & 2: continue
            name, rs, valid, sc, dirty = O.route(_read(batch, r), d, wide=int(o.disable_heuristics))
            if not valid: continue
            for w in range(len(wb) - 1):
                ws, we = max(0, int(wb[w]) - 2), min(len(d), int(wb[w + 1]) + 2)
                if rs[ws] < 0 or rs[we] < 0: continue
                J, raw = we - ws, int(rs[we] - rs[ws])
                trimmed = maxins >= 0 and raw > J + maxins
                I = J if trimmed else raw
                if I > 63: continue
                out.append(dict(z=int(z), w=w, q=r - int(batch.read_off[z]), rev=int(batch.flags[r]) & 1, J=J, I=I, raw=raw, trimmed=trimmed))
    return out


def nrows(s):
    d = abs(s["I"] - s["J"])
    return min(s["I"], 2 * (SCORE_BAND + max(d - 2, 0))) + 1


def row0(s, c):
    """the first row of the lane at column c (k_polish_t's band_row0)"""
    I, J = s["I"], s["J"]
    Wr, nr = SCORE_BAND + max(abs(I - J) - 2, 0), nrows(s)
    return min(max((2 * c * I + J) // (2 * J) - Wr, 0), I + 1 - nr)


def row0s(s):
    return [row0(s, c) for c in range(s["J"] + 1)]


def _noisy(rng, t, sub=0.01, dele=0.01, dup=0.01):
    t = t[rng.random(len(t)) > dele].copy()
    s = rng.random(len(t)) < sub
    t[s] = (t[s] + rng.integers(1, 4, int(s.sum()))) & 3
    return np.repeat(t, 1 + (rng.random(len(t)) < dup)).astype(np.uint8)


def _batch_of(base, reads):
    """the batch `base` with its passes replaced by reads[z][q] (in the draft's orientation; turned by the pass's own flag)"""
    bases, pw, ipd, off = [], [], [], [0]
    rng = np.random.default_rng(5)
    for z in range(base.n_zmw):
        for q, r in enumerate(range(int(base.read_off[z]), int(base.read_off[z + 1]))):
            t = O.orient(np.asarray(reads[z][q], np.uint8), int(base.flags[r]) & 1)
            bases.append(t); pw.append(rng.integers(1, 4, len(t)).astype(np.uint8)); ipd.append(np.full(len(t), 5, np.uint8)); off.append(off[-1] + len(t))
    return api.Batch(base.zmw_id, base.snr, base.read_off, np.array(off, np.int64), np.concatenate(bases), np.concatenate(pw), np.concatenate(ipd),
                     base.flags.copy(), base.tpl_off, base.tpl)


def _polish_case(case, paths):
    """the engine's polish of caller drafts against the restatement's"""
    batch, o, drafts = case
    h = api.Handle(0, opts=o)
    try:
        d = api.Drafts.allocate(batch)
        for z, t in enumerate(drafts): d.set_draft(z, t, backbone=0)
        res = h.polish(batch, d)
        ref = _oracle_polish(h.model, o, batch, d)
    finally:
        h.close()
    paths(ref, batch, shapes(batch, drafts, o))
    _bit_exact(res, ref, batch)
    return res, ref


def _consensus_case(case, paths):
    batch, o = case
    h = api.Handle(0, opts=o)
    try:
        res = h.consensus(batch)
        ref = _oracle_consensus(h.model, o, batch)
    finally:
        h.close()
    paths(ref, batch)
    _bit_exact(res, ref, batch)
    return res, ref


# ---- chain lengths 3 .. 10: short last windows in which the passes end early

def _tpl_24_5(rng):
    """29 bases with (ac)3 at 19 .. 24 and no a behind it: the boundaries 21 - 23 would break the repeat, 24 does not — windows of 26 and of 7 columns"""
    t = rng.integers(0, 4, 29, dtype=np.uint8)
    a = int(rng.integers(0, 4)); c = (a + 1 + int(rng.integers(0, 3))) & 3
    t[19:25] = [a, c, a, c, a, c]
    if t[25] == a: t[25] = (a + 1 + (c == ((a + 1) & 3))) & 3
    return t


SHORT_SEED = 0


def case_short_chains():
    """caller drafts whose last window is short, and ten passes that end inside it.  Even ZMWs: 52 random bases, last window of J = 8 .. 10, pass q
    ends q bases into it; the aligner spreads what is missing, I comes out as 2 .. 9, chains of I + 1 rows (0 and 1: case_empty_segments).  Odd ZMWs: 29 bases with a last window of J = 7; passes of 21 .. 31 bases (the aligner moves a missing
    stretch across the repeat in front of that window, so I stays above 1 there)"""
    rng = np.random.default_rng(1300 + SHORT_SEED)
    base = api.synth(8, 10, 40, seed=1301)
    drafts, reads = [], []
    for z in range(base.n_zmw):
        rs = []
        if z % 2 == 0:
            t = rng.integers(0, 4, 52, dtype=np.uint8)
            ws = int(O.windows(t)[-2]) - 2                             # the last window's first column (42 .. 44: J = 8 .. 10)
            for q in range(10): rs.append(t[:min(ws + q, 52)].copy())
        else:
            t = _tpl_24_5(rng)
            for q in range(10):
                n = 21 + (q + 3 * z) % 11
                rs.append((t[:n] if n <= 29 else np.concatenate([t[:26], rng.integers(0, 4, n - 29, dtype=np.uint8), t[26:]])).copy())
        drafts.append(t); reads.append(rs)
    o = api.default_opts(); o.min_rq = 0.0; o.min_zscore = 0.0; o.disable_heuristics = 1
    return _batch_of(base, reads), o, drafts


def paths_short_chains(ref, batch, sh):
    last = [s for s in sh if s["J"] <= 10]
    assert 7 in set(s["J"] for s in last), sorted(set(s["J"] for s in sh))                                # (a window of J < 8 among them)
    assert set(range(2, 10)) <= set(s["I"] for s in last), sorted(set(s["I"] for s in last))             # I = 2 .. 9 (0 and 1: case_empty_segments)
    assert all(nrows(s) == s["I"] + 1 for s in last if s["I"] <= 9)                                        # nr = I + 1: 3 .. 10 rows, both parities
    assert set(range(2, 10)) <= set(s["I"] for s in last if s["J"] == 7)
    assert any(abs(s["I"] - s["J"]) >= 5 for s in last)                                                    # (|I - J| >= 5 in a small window, too)
    for i in range(2, 10): assert len(set(s["rev"] for s in last if s["I"] == i)) == 2, i                   # every length on both strands
    assert ref.paths["zdrop"] == 0, ref.paths


# ---- chains of one and two rows: segments of 0 and 1 bases

EMPTY_SEED = 0
HEAD, TAIL = 30, 32


def _ends_template(rng, L=257):
    """a random template whose first 30 and last 32 bases are G and T alone, followed by a C / preceded by an A (tests/kinetics_lab.py: ends_template): a pass that
    lacks one of the two ends has one best alignment — the base next to the gap finds no chance match inside it — so a window inside that end keeps no base of it"""
    t = rng.integers(0, 4, L, dtype=np.uint8)
    t[:HEAD] = 2 + rng.integers(0, 2, HEAD)
    t[L - TAIL:] = 2 + rng.integers(0, 2, TAIL)
    t[HEAD], t[L - TAIL - 1] = 1, 0
    return t


def case_empty_segments():
    """caller drafts = ends_template's templates, twelve passes: 0 - 2 and 11 whole; 3 and 4 (one of each strand) lack the head, 5 and 6 the tail: I = 0 in the window
    inside that end; 7 and 8 lack the head but for the template's first base, 9 and 10 the tail but for its last base: that base lands in one window of the end, I = 1"""
    rng = np.random.default_rng(1360 + EMPTY_SEED)
    base = api.synth(6, 12, 257, seed=1361)
    drafts, reads = [], []
    for z in range(base.n_zmw):
        t = _ends_template(rng)
        L = len(t)
        rs = [t.copy() for q in range(12)]
        rs[3], rs[4] = t[HEAD:].copy(), t[HEAD:].copy()
        rs[5], rs[6] = t[:L - TAIL].copy(), t[:L - TAIL].copy()
        rs[7], rs[8] = np.concatenate([t[:1], t[HEAD:]]), np.concatenate([t[:1], t[HEAD:]])
        rs[9], rs[10] = np.concatenate([t[:L - TAIL], t[-1:]]), np.concatenate([t[:L - TAIL], t[-1:]])
        drafts.append(t); reads.append(rs)
    o = api.default_opts(); o.min_rq = 0.0; o.min_zscore = 0.0; o.disable_heuristics = 1
    return _batch_of(base, reads), o, drafts


def paths_empty_segments(ref, batch, sh):
    assert (ref.status == 0).all(), ref.status
    for i in (0, 1):
        e = [s for s in sh if s["I"] == i]
        assert len(e) >= 8 and len(set(s["rev"] for s in e)) == 2, (i, len(e))                             # segments of 0 and of 1 bases, on both strands
        assert all(nrows(s) == i + 1 and s["J"] - i >= 5 for s in e)                                       # chains of ONE row and of TWO rows (|I - J| >= 5: the row layout)
        assert {s["w"] == 0 for s in e} == {True, False}                                                   # in a first window and in a last one
    wins = {}
    for s in sh: wins.setdefault((s["z"], s["w"]), []).append(s)
    assert any(sorted(set(s["I"] for s in v))[:2] == [0, 1] and len(v) == 12 for v in wins.values())      # beside chains of eleven rows in the same chunks
    assert ref.paths["zdrop"] == 0 and ref.paths["trim"] == 0, ref.paths


# ---- chain lengths 11, 13, 15 and the row layout; first rows of every residue; both clamps; long segments; the trim

BLOCKS_SEED = 0


def case_blocks(maxins):
    """caller drafts of 300 random bases, ten passes: light noise everywhere, and in one window per pass a block of k bases inserted or deleted in the middle of the
    core, k = 3, 4, 5 - 8 (|I - J| = k) or 12 (a segment that max_insertion_size = 10 trims)"""
    rng = np.random.default_rng(1310 + BLOCKS_SEED)
    base = api.synth(8, 10, 300, seed=1311)
    drafts, reads = [], []
    ks = [3, -3, 4, -4, 5, -6, 8, 12, 0, 0]
    for z in range(base.n_zmw):
        t = rng.integers(0, 4, 300, dtype=np.uint8)
        wb = O.windows(t)
        rs = []
        for q in range(10):
            k = ks[(q + z) % 10]
            w = int(rng.integers(1, len(wb) - 2))
            m = (int(wb[w]) + int(wb[w + 1])) // 2
            if k > 0: r = np.concatenate([_noisy(rng, t[:m]), rng.integers(0, 4, k, dtype=np.uint8), _noisy(rng, t[m:])])
            elif k < 0: r = np.concatenate([_noisy(rng, t[:m + k // 2]), _noisy(rng, t[m + k // 2 - k:])])
            else: r = _noisy(rng, t)
            rs.append(r)
        drafts.append(t); reads.append(rs)
    o = api.default_opts(); o.min_rq = 0.0; o.max_insertion_size = maxins
    return _batch_of(base, reads), o, drafts


def paths_blocks(ref, batch, sh, maxins):
    dif = np.array([abs(s["I"] - s["J"]) for s in sh]); I = np.array([s["I"] for s in sh]); nr = np.array([nrows(s) for s in sh])
    assert ((I >= 10) & (dif <= 2) & (nr == 11)).sum() >= 100                                             # the usual chain: eleven rows
    assert ((dif == 3) & (nr == 13)).any() and ((dif == 4) & (nr == 15)).any(), np.bincount(dif)          # one row, three rows in a second block of observation bytes
    assert ((dif >= 5) & (nr >= 17)).any(), np.bincount(dif)                                              # the row layout (pitch = S), 17 rows and more
    assert (I > 31).any(), I.max()                                                                        # a segment of more than 31 bases
    assert (nr > 2 * OBS_ROWS).any(), nr.max()                                                            # three blocks of observation bytes
    usual = [s for s in sh if nrows(s) == 11]
    i0 = np.concatenate([row0s(s) for s in usual])
    assert set((i0 & 3).tolist()) == {0, 1, 2, 3}                                                         # every shift of the four words
    assert any(row0s(s)[0] == 0 and row0s(s)[-1] == s["I"] + 1 - nrows(s) for s in usual)                 # both clamps of the first row
    for k in (13, 15):
        assert set((np.concatenate([row0s(s) for s in sh if nrows(s) == k]) & 3).tolist()) == {0, 1, 2, 3}, k
    if maxins > 0:
        assert any(s["trimmed"] for s in sh) and ref.paths["trim"] >= 1, ref.paths                        # a segment trimmed by max_insertion_size
        assert any(not s["trimmed"] and s["I"] - s["J"] >= 5 for s in sh)
    else:
        assert not any(s["trimmed"] for s in sh) and ref.paths["trim"] == 0, ref.paths


# ---- units: one, two and three usable reads in a chunk; pairs of different lengths and of both strands; two blocks of lanes

UNITS_SEED = 0


def case_units(passes):
    """ZMWs of one to three windows with `passes` passes, every mutation lane valid (disable_heuristics): a window of J >= 9 has more than 64 valid lanes, i.e.
    two blocks of lanes and more.  3 passes: one chunk of three reads; 9, 10, 11: a chunk of eight and one of 1, 2, 3 reads.  A chunk's blocks x reads units are
    shared out over four waves: with one or two reads every wave has single chains, with three a wave gets a pair or a pair plus one"""
    o = api.default_opts(); o.min_rq = 0.0; o.disable_heuristics = 1; o.min_zscore = 0.0
    return api.synth(12, passes, (20, 56), seed=1320 + 10 * UNITS_SEED + passes), o


def wave_units(nblk, nv):
    """k_polish_t's share-out of a chunk's nblk x nv units (block-major) over four waves: the units as tuples of the chunk's usable reads, (k0, k0 + 1) for a pair"""
    n, out = nblk * nv, []
    for wave in range(4):
        u, end = wave * n // 4, (wave + 1) * n // 4
        while u < end:
            k0 = u % nv
            two = u + 1 < end and k0 + 1 < nv
            out.append((k0, k0 + 1) if two else (k0,))
            u += 2 if two else 1
    return out


def paths_units(ref, batch, passes):
    assert ref.paths["fallback"] == 0 and ref.paths["third_draft"] == 0, ref.paths
    done = np.flatnonzero(ref.seq_len > 0)
    assert len(done) >= 8 and (ref.np_[done] == passes).all(), (ref.status, ref.np_)
    drafts = {int(z): O.poa_draft(batch, int(z)) for z in done}
    o = api.default_opts(); o.disable_heuristics = 1
    sh = shapes(batch, drafts, o, zs=[int(z) for z in done])
    assert all(s["J"] >= 9 for s in sh)                                                                   # more than 64 valid lanes: 7 J + 4 - (run positions) > 64
    wins = {}
    for s in sh: wins.setdefault((s["z"], s["w"]), []).append(s)
    assert sum(len(v) == passes for v in wins.values()) >= 8                                              # every pass has a segment: chunks of 3, or of 8 and passes - 8 = 1, 2, 3 reads
    # the units of a wave, from the kernel's own share-out: in a window whose passes are all usable (ec = the pass count in every window of the ZMW) and whose J <= 27
    # (eight reads per chunk fit), chunk k holds passes 8 k .. 8 k + 7 in pass order, the list has 7 J + 4 - (positions inside a run) lanes, every lane valid
    shapes_seen, dnr, dst, both = set(), 0, 0, 0
    for (z, w), v in wins.items():
        if len(v) != passes or v[0]["J"] > 27 or ref.ec[z] != passes: continue
        d = drafts[z]; wb = O.windows(d)
        t = d[max(0, int(wb[w]) - 2):min(len(d), int(wb[w + 1]) + 2)]
        nblk = (7 * len(t) + 4 - int((t[1:] == t[:-1]).sum()) + 63) // 64
        v = sorted(v, key=lambda s: s["q"])
        for c0 in range(0, passes, 8):
            chunk = v[c0:c0 + 8]
            for u in wave_units(nblk, len(chunk)):
                shapes_seen.add((len(chunk), len(u)))
                if len(u) == 2:
                    a, b = chunk[u[0]], chunk[u[1]]
                    dnr += nrows(a) != nrows(b); dst += a["rev"] != b["rev"]; both += nrows(a) != nrows(b) and a["rev"] != b["rev"]
    tail = passes - 8 if passes > 8 else passes
    assert (tail, 1) in shapes_seen, shapes_seen                                                          # a chunk of 1, 2, 3 reads with a single chain
    if tail == 3: assert (3, 2) in shapes_seen, shapes_seen                                               # three reads: a wave with a pair (and one with a pair plus one: 4 blocks)
    if passes > 8: assert (8, 2) in shapes_seen
    if passes >= 3: assert dnr >= 1 and dst >= 1 and both >= 1, (dnr, dst, both)                          # a wave's PAIR with nrA != nrB, with the strands mixed, with both


# ---- ten passes (chunks of 8 + 2), the z-score gate inside a chunk, J = 31, an insertion behind the last column, more than 32 passes

TEN_SEED = 0


def case_ten(noisy=True):
    """ten passes, two of them (4 and 5) six times as noisy: the z-score gate drops them from windows — inside the first chunk of eight.  noisy = False: the same
    batch with passes 4 and 5 as quiet as the others (every pass has a generator of its own, so the other eight are the same bases)"""
    base = api.synth(10, 10, 400, seed=1331)
    reads = []
    for z in range(base.n_zmw):
        t = base.tpl[int(base.tpl_off[z]):int(base.tpl_off[z + 1])].copy()
        reads.append([_noisy(np.random.default_rng([1330 + TEN_SEED, z, q]), t, *((0.09, 0.18, 0.12) if noisy and q in (4, 5) else (0.015, 0.03, 0.02))) for q in range(10)])
    o = api.default_opts(); o.min_rq = 0.0
    return _batch_of(base, reads), o


def paths_ten(ref, batch):
    assert ref.paths["fallback"] == 0 and ref.paths["third_draft"] == 0, ref.paths
    done = np.flatnonzero(ref.seq_len > 0)
    assert (ref.np_[done] == 10).sum() >= 6, (ref.status, ref.np_)                                        # ten passes in the polish, in pass order: chunks of passes 0 - 7 and 8 - 9
    assert ref.paths["zdrop"] >= 1, ref.paths                                                             # (read, window) pairs the gate dropped
    assert (ref.iters > ref.n_windows)[done].any()
    quiet, o = case_ten(noisy=False)                                                                      # the drops are passes 4 and 5, i.e. inside the first chunk:
    assert _oracle_consensus(api.default_model(), o, quiet).paths["zdrop"] == 0                           # with those two quiet the gate drops nothing


FIN_SEED = 0


def case_fin():
    """caller drafts with a defect at the last column of the draft, ten clean passes of the template.  The lanes with `fin` set — an insertion behind the last column,
    a substitution or the deletion of the last column — report b and not acc.  ZMW z % 3 == 0: the draft's last base is wrong (repair: a substitution with fin),
    1: the draft has a base too many (repair: the deletion with fin), 2: the draft lacks its last base (the insertion behind the last column is scored — its gain
    feeds the last base's QV — but never favourable: the passes' extra base lies outside the last window's segment, see the module's docstring)"""
    rng = np.random.default_rng(1340 + FIN_SEED)
    base = api.synth(9, 10, 120, seed=1341)
    drafts, reads, tpls = [], [], []
    for z in range(base.n_zmw):
        t = rng.integers(0, 4, 120, dtype=np.uint8)
        while t[-1] == t[-2] or t[-2] == t[-3]: t[-3:] = rng.integers(0, 4, 3)
        if z % 3 == 0: d = t.copy(); d[-1] = (d[-1] + 1) & 3
        elif z % 3 == 1: d = np.concatenate([t, [(t[-1] + 1) & 3]]).astype(np.uint8)
        else: d = t[:-1].copy()
        drafts.append(d); tpls.append(t); reads.append([t.copy() for q in range(10)])
    o = api.default_opts(); o.min_rq = 0.0; o.disable_heuristics = 1
    return _batch_of(base, reads), o, drafts, tpls


def paths_fin(ref, batch, sh, drafts, tpls):
    assert (ref.status == 0).all(), ref.status
    for z in range(batch.n_zmw):
        if z % 3 < 2: assert np.array_equal(ref.sequence(z), tpls[z]), z                                   # the favourable lane with fin was found: the window's result was its b
        else:
            assert np.array_equal(ref.sequence(z), drafts[z]), z
            for r in range(int(batch.read_off[z]), int(batch.read_off[z + 1])):                            # why: the pass's last base lies behind the entry row of column Ld,
                rd = _read(batch, r)                                                                       # outside the last window's segment — no pass votes for the insertion
                name, rs, valid, sc, dirty = O.route(rd, drafts[z], wide=1)
                assert valid and len(rd) == len(drafts[z]) + 1 and rs[len(drafts[z])] == len(rd) - 1, (z, r, rs[len(drafts[z])])
    assert (ref.iters > ref.n_windows).sum() >= 6, (ref.iters, ref.n_windows)


JMAX_SEED = 923


def case_jmax():
    """three passes x 800 bases: the draft's own errors give many rounds, and insertions make windows of 29 and 30 columns grow to CCSX_JMAX = 31"""
    o = api.default_opts(); o.min_rq = 0.0
    return api.synth(8, 3, 800, seed=JMAX_SEED), o


def paths_jmax(ref, batch):
    """a window of the restatement's draft with 29 or 30 columns into which the consensus put as many bases more as make 31 (from an alignment of draft and consensus)"""
    assert ref.paths["fallback"] == 0 and ref.paths["third_draft"] == 0, ref.paths
    hit = 0
    for z in np.flatnonzero(ref.seq_len > 0):
        d, s = O.poa_draft(batch, int(z)), ref.sequence(int(z))
        wb = O.windows(d)
        ins, dl = np.zeros(len(d) + 1, int), np.zeros(len(d) + 1, int)
        for tag, i1, i2, j1, j2 in difflib.SequenceMatcher(None, bytes(d.tolist()), bytes(s.tolist()), autojunk=False).get_opcodes():
            n = (j2 - j1) - (i2 - i1)
            if tag != "equal" and n > 0: ins[i1] += n
            elif tag != "equal" and n < 0: dl[i1:i1 - n] += 1
        for w in range(len(wb) - 1):
            ws, we = max(0, int(wb[w]) - 2), min(len(d), int(wb[w + 1]) + 2)
            hit += (we - ws >= 29) and (we - ws + ins[ws:we + 1].sum() - dl[ws:we].sum() == 31)
    assert hit >= 1


def case_reload():
    o = api.default_opts(); o.min_rq = 0.0
    return api.synth(6, 40, 300, seed=1351), o


def paths_reload(ref, batch):
    done = ref.seq_len > 0
    assert done.sum() >= 5 and (ref.np_[done] == 40).all(), (ref.status, ref.np_)                         # two groups of passes: a reload between the scorings of a round
    assert (ref.iters > ref.n_windows)[done].any(), (ref.iters, ref.n_windows)


def test_chains_of_one_and_two_rows(built):
    _polish_case(case_empty_segments(), paths_empty_segments)


def test_chains_of_three_to_ten_rows(built):
    _polish_case(case_short_chains(), paths_short_chains)


@pytest.mark.parametrize("maxins", [10, -1])
def test_chain_lengths_first_rows_and_trim(built, maxins):
    _polish_case(case_blocks(maxins), lambda ref, batch, sh: paths_blocks(ref, batch, sh, maxins))


@pytest.mark.parametrize("passes", [3, 9, 10, 11])
def test_chunks_of_one_two_and_three_reads(built, passes):
    _consensus_case(case_units(passes), lambda ref, batch: paths_units(ref, batch, passes))


def test_ten_passes_and_the_zscore_gate(built):
    _consensus_case(case_ten(), paths_ten)


def test_window_of_31_columns(built):
    _consensus_case(case_jmax(), paths_jmax)


def test_lanes_at_the_last_column(built):
    batch, o, drafts, tpls = case_fin()
    _polish_case((batch, o, drafts), lambda ref, b, sh: paths_fin(ref, b, sh, drafts, tpls))


def test_more_than_32_passes(built):
    _consensus_case(case_reload(), paths_reload)

"""The alignment lab: a small batch that plants, on purpose, the shapes the alignment cascade (k_align16, k_align16_tb, k_align, k_rescue) has limits for, and for every pass
the CPU restatement's result by route (oracle_lib.route) and the plain unbanded reference (align_ref.Ref).  Most passes are error-free copies of their template (strands
alternating), so the draft IS the template and Ld is what was planted; the edits sit in named passes.  tests/test_align_ref.py checks restatement against reference on it
without a GPU, tests/test_align_gpu.py the engine against both."""
import functools

import numpy as np

from ccs_amd import api
import align_ref as A
import oracle_lib as O

SNR0 = (9.0, 16.0, 8.0, 13.0)
PARTIAL, ADAPTER_AT_END = 2, 4            # pass flags beside bit 0 = strand (include/ccsx.h)


def revcomp(b):
    return (3 - np.asarray(b, np.uint8)[::-1]).astype(np.uint8)


def edited(tpl, ops):
    """the template with ops = [(at, n_deleted, inserted bases)] applied: tpl[:at] + inserted + tpl[at + n_deleted:]"""
    t = [int(b) for b in tpl]
    for at, cut, ins in sorted(ops, key=lambda o: o[0], reverse=True):
        t = t[:at] + [int(b) for b in ins] + t[at + cut:]
    return np.array(t, np.uint8)


def _other(*bases):
    """a base that differs from all of `bases` (at most three)"""
    return next(b for b in range(4) if b not in [int(x) for x in bases])


def _template(rng, Ld, nw_parity=None, ok=None):
    """a random template of exactly Ld bases (whose window count has the given parity, and which satisfies ok(t, edges))"""
    for _ in range(20000):
        t = rng.integers(0, 4, Ld).astype(np.uint8)
        wb = O.windows(t)
        if nw_parity is not None and (len(wb) - 1) % 2 != nw_parity: continue
        if ok is not None and not ok(t, wb): continue
        return t, wb
    raise AssertionError("no such template")


def _isolated(t, p):
    """position p differs from both neighbours: an edit there has one placement"""
    return 0 < p < len(t) - 1 and t[p] != t[p - 1] and t[p] != t[p + 1]


def _mid(wb, w):
    return (int(wb[w]) + int(wb[w + 1])) // 2


def _mm(t, p):
    return (p, 1, [(int(t[p]) + 1) & 3])


class Lab:
    def __init__(self, seed=2):
        rng = np.random.default_rng(seed)
        self.zmws = []           # (name, template, [(oriented bases, flags)])
        self.subopt = set()      # (zmw, pass): planted at a band limit where the 16-row band's valid, unsaturated answer is known to fall short of the unbanded optimum
        self.expect_dirty = {}   # (zmw, pass) -> the positions DESIGN.md §2 "Pile-up evidence" names for the planted single edits
        self.tiny_quad = None    # (zmw, first pass of the quad)
        self.runs = {}           # planted insertion run length -> (zmw, pass)

        def zmw(name, t, ops_by_pass, n, partial=()):
            ps = []
            for k in range(n):
                ops = ops_by_pass.get(k, [])
                ps.append((ops if isinstance(ops, np.ndarray) else edited(t, ops), k & 1))
            for b, fl in partial: ps.append((b, fl))
            self.zmws.append((name, t, ps))
            return len(self.zmws) - 1

        # ---- block and length limits: Ld mod 16 in {1, 15, 0, 0}, Ld in (16 k, 16 k + 16] for k = 6, 7, 7, 8; tail quads of 3, 1, 2, 3 passes; the window
        # counts are planted odd, even, even, odd, so nneed mod 4 is 2, 0, 0, 2
        for name, Ld, n, par in (("ld97", 97, 3, 1), ("ld127", 127, 5, 0), ("ld128", 128, 6, 0), ("ld144", 144, 7, 1)):
            t, wb = _template(rng, Ld, nw_parity=par)         # 5, 6, 6, 7 windows: nneed = 10, 12, 12, 14
            e = {n - 1: [_mm(t, _mid(wb, 1)), (_mid(wb, 3), 1, [])], n - 2: [(_mid(wb, 2), 0, [_other(t[_mid(wb, 2) - 1], t[_mid(wb, 2)])])]}
            zmw(name, t, e, n)
        # ---- band limits in otherwise clean passes, away from the edges.  Insertion runs of 5 .. 11 copies of the following base: while the read emits the run the
        # band's best row stays where it is (a deletion per column, -4, beats a mismatch per column, -5), so the path slides down the band by one row per column until it
        # overtakes (7 m > 4 k columns after a run of k): a run of 5 stays inside the 9 rows below, 6 reaches the last row — trigger (a) — and longer ones leave the band.
        # The boundary pair 5 / 6 is planted beside the runs of 7 .. 11; the evidence test asserts from the routes where the boundary lies
        t, wb = _template(rng, 208)
        z = zmw("ins_runs", t, {3 + k: [(_mid(wb, 1 + k), 0, [t[_mid(wb, 1 + k)]] * (5 + k))] for k in range(7)}, 10)
        for k in range(7): self.runs[5 + k] = (z, 3 + k)
        # deleted stretches of 4 .. 8.  The band has 6 rows above the best row: across a deleted stretch of n >= 6 bases the path stays in its row while every chance match
        # on the old diagonal pulls the band one row further down, so from 6 on the 16-row band CAN lose the optimum and still end valid and unsaturated — whether it does
        # depends on those chance matches.  In this lab the stretches of 6 and 8 do (30 and 35 points below the unbanded optimum) and the stretch of 7 does not: the two
        # are the lab's planted-suboptimal list, check_all asserts score < OPT for each of them (a stale excuse fails), and the 64-row band holds all of them
        t, wb = _template(rng, 208)
        z = zmw("del_runs", t, {3 + k: [(_mid(wb, 2 + k) - 3, 4 + k, [])] for k in range(5)}, 8)
        self.subopt |= {(z, 5), (z, 7)}
        # insertions of 20, 31, 33 random bases; blocks of 40 and 150 (split)
        t, wb = _template(rng, 304)
        blk = lambda n: rng.integers(0, 4, n).tolist()
        zmw("blocks", t, {3: [(_mid(wb, 3), 0, blk(20))], 4: [(_mid(wb, 5), 0, blk(31))], 5: [(_mid(wb, 7), 0, blk(33))], 6: [(_mid(wb, 4), 0, blk(40))],
                          7: [(_mid(wb, 8), 0, blk(150))]}, 8)
        # a 60-base block at the very start / end of a pass, two blocks of 50 in one pass (near the ends: no single split column carries the pass); partial passes with both anchor ends on both strands
        t, wb = _template(rng, 300)
        cut = 170
        partial = [(t[:cut].copy(), PARTIAL | 0), (t[:cut].copy(), PARTIAL | 1 | ADAPTER_AT_END), (t[-cut:].copy(), PARTIAL | ADAPTER_AT_END), (t[-cut:].copy(), PARTIAL | 1)]     # (draft orientation)
        self.z_ends = zmw("ends", t, {4: [(0, 0, blk(60))], 5: [(len(t), 0, blk(60))], 6: [(_mid(wb, 1), 0, blk(50)), (_mid(wb, 11), 0, blk(50))]}, 8, partial)
        # ---- more than 128 window-edge columns (two refills of the edge list), just over 64, and the chunk reload at read row 2048 with an 8-base insertion and a
        # 5-base deletion within 30 columns of it
        t, wb = _template(rng, 1521)
        zmw("edges128", t, {2: [_mm(t, _mid(wb, 40)), (_mid(wb, 66), 1, [])], 3: [(_mid(wb, 33), 0, [_other(t[_mid(wb, 33) - 1], t[_mid(wb, 33)])])]}, 4)
        t, wb = _template(rng, 750)
        zmw("edges64", t, {3: [_mm(t, _mid(wb, 31)), (_mid(wb, 33), 1, [])]}, 4)
        t, wb = _template(rng, 2303)
        self.z_chunk = zmw("chunk2048", t, {1: [(2030, 0, blk(8)), (2062, 5, [])], 2: [(2020, 5, []), (2046, 0, blk(8))]}, 3)
        # ---- saturation trigger (b): (AC)x40 and (AAG)x25 tracts, passes missing 1, 2 and 4 repeat units
        def tracts(t, wb):
            t[60:140] = [0, 1] * 40; t[200:275] = [0, 0, 2] * 25
            return t[59] != 1 and t[140] != 0 and t[199] != 2 and t[275] != 0
        t, wb = _template(rng, 340, ok=tracts)
        self.z_tracts = zmw("tracts", t, {3: [(100, 2, []), (230, 12, [])], 4: [(100, 4, [])], 5: [(100, 8, [])], 6: [(230, 3, [])], 7: [(230, 6, [])]}, 8)
        # ---- edits on the edges themselves (edge column c = c draft bases consumed: an insertion AT c sits before position c, the base OF c is position c - 1)
        def edge_sites(t, wb):
            c = [int(b) for b in wb]
            return len(c) > 8 and all(_isolated(t, p) for p in (c[3] - 3, c[3] + 2, c[3] + 1, c[5] + 1, c[5] - 2, c[5] - 3, 159, 175, 95, 112))
        t, wb = _template(rng, 208, ok=edge_sites)
        c = [int(b) for b in wb]
        x = lambda at: _other(t[at - 1], t[at])
        first, last = _other(t[0]), _other(t[-1])
        e = {3: [(0, 0, [first] * 2), (c[2] - 2, 0, [x(c[2] - 2)]), (c[4] + 2, 0, [x(c[4] + 2)] * 3), _mm(t, 159), _mm(t, 175)],
             4: [(c[2] - 2, 0, [x(c[2] - 2)] * 3), (c[4] + 2, 0, [x(c[4] + 2)]), (len(t), 0, [last] * 2)],
             5: [(c[3] - 3, 1, []), _mm(t, c[5] + 1), _mm(t, 95), _mm(t, 112)],
             6: [(c[3] + 2, 1, []), _mm(t, c[5] - 2)],                     # the bases AFTER the edge columns c[3] + 2 and c[5] - 2
             7: [(c[3] + 1, 1, []), _mm(t, c[5] - 3)]}                     # the bases OF the edge columns c[3] + 2 and c[5] - 2 (pass 5: of c[3] - 2 and c[5] + 2)
        z = zmw("on_edges", t, e, 8)
        self.z_edges = z
        self.expect_dirty[(z, 3)] = {0, c[2] - 3, c[2] - 2, c[4] + 1, c[4] + 2, 159, 175}
        self.expect_dirty[(z, 4)] = {c[2] - 3, c[2] - 2, c[4] + 1, c[4] + 2, len(t) - 1}
        self.expect_dirty[(z, 5)] = {c[3] - 3, c[5] + 1, 95, 112}
        self.expect_dirty[(z, 6)] = {c[3] + 2, c[5] - 2}
        self.expect_dirty[(z, 7)] = {c[3] + 1, c[5] - 3}
        self.expect_dirty[(z, 0)] = set()
        # ---- quads: a pass of half the length among exact ones; a 12-base pass that sends its three neighbours through the `tiny` branch
        t, wb = _template(rng, 122)
        z = zmw("tiny_quad", t, {2: t[:61].copy(), 5: t[40:52].copy()}, 8)
        self.tiny_quad = (z, 4)
        # ---- ZMWs whose passes are themselves shorter than the 16-row band, and passes of 15, 16 and 17 bases
        t, wb = _template(rng, 12)
        self.z_short = zmw("ld12", t, {}, 4)
        t, wb = _template(rng, 16, ok=lambda t, wb: _isolated(t, 8))
        zmw("ld16", t, {3: [(8, 1, [])], 4: [(8, 0, [_other(t[7], t[8])])]}, 5)

    def batch(self):
        reads = [(revcomp(b) if fl & 1 else b, fl) for _, _, ps in self.zmws for b, fl in ps]
        n, tot = len(self.zmws), sum(len(b) for b, _ in reads)
        rng = np.random.default_rng(99)
        return api.Batch(np.arange(n, dtype=np.int32), np.tile(np.array(SNR0, np.float32), (n, 1)), np.concatenate([[0], np.cumsum([len(ps) for _, _, ps in self.zmws])]).astype(np.int32),
                         np.concatenate([[0], np.cumsum([len(b) for b, _ in reads])]).astype(np.int64), np.ascontiguousarray(np.concatenate([b for b, _ in reads])),
                         rng.integers(1, 4, tot).astype(np.uint8), np.full(tot, 5, np.uint8), np.array([fl for _, fl in reads], np.uint8))

    def passes(self):
        """(zmw, pass, oriented bases, draft, from_end of a partial pass or None) for every pass"""
        for z, (_, t, ps) in enumerate(self.zmws):
            for k, (b, fl) in enumerate(ps):
                yield z, k, b, t, ((((fl >> 2) & 1) ^ (fl & 1)) if fl & PARTIAL else None)


@functools.lru_cache(maxsize=None)
def lab():
    return Lab()


@functools.lru_cache(maxsize=None)
def refs():
    """{(zmw, pass): align_ref.Ref} — computed once per process"""
    return {(z, k): A.Ref(b, t, O.need_cols(t)) for z, k, b, t, _ in lab().passes()}


@functools.lru_cache(maxsize=None)
def routes(wide=0):
    """{(zmw, pass): (route, rstart, valid, score, dirty)} of the CPU restatement's cascade, computed once per process"""
    return {(z, k): O.route(b, t, partial=pe, wide=wide) for z, k, b, t, pe in lab().passes()}


def check_all(results, wide=0):
    """the independent properties (align_ref.check_pass) of {(zmw, pass): (route, rstart, valid, score, dirty)} over the whole lab"""
    L, R = lab(), refs()
    sub = set() if wide else L.subopt                     # (the 64-row band holds every planted pass: nothing is excused with opts.disable_heuristics)
    for z, k, b, t, pe in L.passes():
        name, rs, v, sc, dirty = results[(z, k)]
        if (z, k) in sub:
            assert v and name == "narrow" and sc < R[(z, k)].opt, f"zmw {z} pass {k}: on the planted-suboptimal list, but {name} with score {sc} against an optimum of {R[(z, k)].opt}"
        A.check_pass(R[(z, k)], name, v, sc, rs, dirty, (z, k) in sub, partial=pe, tag=f"zmw {z} ({L.zmws[z][0]}) pass {k} [{name}]")


def saturation_triggers():
    """RESTATEMENT-side evidence (the engine reports no trigger; its run enters through valid / score agreeing with the restatement pass by pass):
    {(zmw, pass): (a fired, b fired)} for the passes of route wide_saturated: the 16-row attempt again with one trigger switched off at a time (a pass is saturated by
    (a) iff it no longer is with (a) off ...; both may fire)"""
    out = {}
    try:
        for (z, k, b, t, pe), (name, *_) in zip(lab().passes(), routes(0).values()):
            if name != "wide_saturated": continue
            O.sat_triggers(rows=0); only_b = O.route(b, t)[0] == "wide_saturated"
            O.sat_triggers(gain=-(1 << 30)); only_a = O.route(b, t)[0] == "wide_saturated"
            O.sat_triggers()
            out[(z, k)] = (only_a, only_b)
    finally:
        O.sat_triggers()
    return out


def evidence(results):
    """what a run contained, from {(zmw, pass): (route, rstart, valid, score, dirty)} and the lab's templates.  Route names and the saturation triggers are the restatement's
    (they describe an engine run only because the caller has checked valid pass by pass); the quad sizes follow from the lab's pass counts, the host packing up to four
    CONSECUTIVE full-length passes of a ZMW into a quad (ccsx_upload)"""
    L, R = lab(), refs()
    E = dict(routes={}, sat_a=0, sat_b=0, quad_sizes=set(), ld_mod16=set(), block_parity=set(), nneed_mod4=set(), nneed_max=0, row_above_2048_narrow=0, tiny_quad_exact=0,
             half_length_invalid=0, short_zmw_valid=0, runs={})
    for key, res in results.items(): E["routes"][res[0]] = E["routes"].get(res[0], 0) + 1
    for (a, b) in saturation_triggers().values(): E["sat_a"] += int(a); E["sat_b"] += int(b)
    for z, (name, t, ps) in enumerate(L.zmws):
        nfull = sum(1 for _, fl in ps if not fl & PARTIAL)
        E["quad_sizes"] |= {4} if nfull >= 4 else set()
        if nfull % 4: E["quad_sizes"].add(nfull % 4)
        nneed = len(O.need_cols(t))
        E["ld_mod16"].add(len(t) % 16); E["block_parity"].add(((len(t) + 15) // 16) % 2); E["nneed_mod4"].add(nneed % 4); E["nneed_max"] = max(E["nneed_max"], nneed)
    for (z, k), (name, rs, v, sc, dirty) in results.items():
        if name == "narrow" and v and R[(z, k)].I > 2048 and int(rs[R[(z, k)].L]) > 2048: E["row_above_2048_narrow"] += 1
    z, k0 = L.tiny_quad
    lens = [len(L.zmws[z][2][k][0]) for k in range(k0, k0 + 4)]
    assert sum(1 for n in lens if 9 <= n <= 14) == 1
    E["tiny_quad_exact"] = sum(1 for k in range(k0, k0 + 4) if results[(z, k)][0] == "narrow" and results[(z, k)][3] == R[(z, k)].opt)
    E["half_length_invalid"] = int(not results[(z, 2)][2])
    E["short_zmw_valid"] = sum(int(results[(L.z_short, k)][2]) for k in range(len(L.zmws[L.z_short][2])))
    E["runs"] = {n: results[key][0] for n, key in sorted(L.runs.items())}
    return E


def assert_evidence(E):
    missing = [r for r in O.ROUTES if not E["routes"].get(r)]
    assert not missing, f"routes that did not occur: {missing}"
    assert E["sat_a"] > 0 and E["sat_b"] > 0, "a band-saturation trigger did not fire on its own"
    assert E["quad_sizes"] == {1, 2, 3, 4} and E["ld_mod16"] >= {0, 1, 15} and E["block_parity"] == {0, 1} and E["nneed_mod4"] == {0, 2} and E["nneed_max"] > 128
    assert E["row_above_2048_narrow"] > 0 and E["tiny_quad_exact"] == 3 and E["half_length_invalid"] == 1 and E["short_zmw_valid"] >= 3
    # the boundary pair of the 16-row band: every run up to some length stays narrow, every longer one does not, and both sides were planted
    narrow = [n for n, r in E["runs"].items() if r == "narrow"]
    assert narrow and max(narrow) + 1 in E["runs"] and all(E["runs"][n] == "narrow" for n in E["runs"] if n <= max(narrow)), E["runs"]


# ---- the engine's side (needs a GPU): stage outputs of a run over the lab batch, optionally behind `prefix` synthetic ZMWs
def lab_batch_after(prefix=0):
    """the lab batch, concatenated after `prefix` synthetic ZMWs (api.synth: other lengths, so the length-ordered quads interleave with the lab's)"""
    b = lab().batch()
    if not prefix: return b, 0
    s = api.synth(prefix, (3, 9), (100, 2600), seed=31)
    cat = lambda x, y: np.ascontiguousarray(np.concatenate([x, y]))
    nr, nb = int(s.read_off[-1]), int(s.base_off[-1])
    return api.Batch(np.arange(prefix + b.n_zmw, dtype=np.int32), cat(s.snr, b.snr), cat(s.read_off, b.read_off[1:] + nr).astype(np.int32),
                     cat(s.base_off, b.base_off[1:] + nb).astype(np.int64), cat(s.bases, b.bases), cat(s.pw, b.pw), cat(s.ipd, b.ipd), cat(s.flags, b.flags)), prefix


def stage_outputs(handle, batch, z0=0):
    """upload / run / sync, then per lab pass {(zmw, pass): (rstart [Ld + 1], valid, score, dirty [Ld])} from ccsx_stage_align_ev, and the drafts and windows the run used"""
    handle.upload(batch); handle.run(); handle.sync()
    out, drafts = {}, {}
    for z in range(len(lab().zmws)):
        d = handle.stage_draft(z0 + z); drafts[z] = (d, handle.stage_windows(z0 + z) if len(d) else None)
        r0 = int(batch.read_off[z0 + z])
        for k in range(int(batch.read_off[z0 + z + 1]) - r0):
            rs, v, sc, dirty = handle.stage_align_ev(r0 + k, len(d))
            rs2, v2, sc2 = handle.stage_align(r0 + k, len(d))
            assert np.array_equal(rs, rs2) and (v, sc) == (v2, sc2), "ccsx_stage_align_ev and ccsx_stage_align disagree"
            out[(z, k)] = (rs, v, sc, dirty)
    return out, drafts


def packed(out):
    """the stage outputs as four flat arrays (for byte comparison across processes)"""
    keys = sorted(out)
    return dict(ent=np.concatenate([out[k][0] for k in keys]), valid=np.array([out[k][1] for k in keys], np.int32), score=np.array([out[k][2] for k in keys], np.int64),
                dirty=np.concatenate([out[k][3] for k in keys]))

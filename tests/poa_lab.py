"""The POA lab: a small planted batch that takes the four POA kernels to the limits their code names ("POA draft", the note "Pinned against a plain
reference").  Every ZMW has a name, the class it plants, the passes, and — where a clear majority forces the answer — the planted draft, known by construction and
independent of oracle and engine.  Every ZMW also carries `checks` and `log_checks`: what the per-pass records of the FIRST generator (tests/poa_ref.py PassRecord,
and the five log words of the engine) must show for the class to have occurred; a class that does not occur is a failure, never a skip.

Built deterministically: sequences come from one seeded generator, every edit is placed by construction, nothing is searched for.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

from ccs_amd import api
import poa_ref as R

COV = 14           # opts.max_poa_cov of the lab's runs: every full-length pass of every ZMW enters the POA (no ZMW has more than 14)
PRING = 8          # columns of a graph k_poa_dp keeps in LDS: an in-edge of more positions is far
WORN = (1, 4, 6, 9, 12, 14)     # six mismatches in sixteen bases: 10 * 3 - 6 * 5 = 0


@dataclass
class Zmw:
    name: str
    cls: str
    reads: list
    flags: list
    planted: "np.ndarray | None" = None
    checks: list = field(default_factory=list)      # (what, fn(recs of poa_spec) -> bool): the class occurs, on the reference's records
    log_checks: list = field(default_factory=list)  # (what, fn(log rows [rr, I, score, kend, threaded, nverts]) -> bool): ... and on the five words a log holds
    excused: tuple = ()                             # passes rr allowed to fall short of the unbanded optimum (each must really fall short)
    excused2: tuple = ()                            # ... of the second generator
    fallback: "int | None" = None                   # the first generator is expected to fail or be rejected: the backbone the second one takes
    fails: bool = False                             # the first generator ends in DRAFT_FAILURE


def _rng(tag): return np.random.default_rng(abs(hash_str(tag)) % (1 << 32))


def hash_str(s):
    h = 2166136261
    for c in s.encode(): h = ((h ^ c) * 16777619) & 0xffffffff
    return h


def template(tag, n):
    """n bases without a homopolymer run (no two equal neighbours): an indel then has exactly one optimal placement unless a lab entry plants a repeat"""
    g = _rng(tag)
    t = np.zeros(n, np.uint8)
    prev = 4
    for i in range(n):
        b = int(g.integers(0, 4))
        if b == prev: b = (b + 1 + int(g.integers(0, 3))) & 3
        if b == prev: b = (b + 1) & 3
        t[i] = prev = b
    return t


def snp(t, *at, step=2):
    s = t.copy()
    for p in at: s[p] = (s[p] + step) & 3
    return s


def delete(t, p, n): return np.concatenate([t[:p], t[p + n:]]).astype(np.uint8)
def insert(t, p, bases): return np.concatenate([t[:p], np.asarray(bases, np.uint8), t[p:]]).astype(np.uint8)
def rc(t): return (3 - t[::-1]).astype(np.uint8)
def threaded(recs): return [q.threaded for q in recs]


def _edges(recs, rr): return recs[rr - 1].edges        # (distance, slot, in-edges) of the edges of 7 and more positions that pass rr's DP read


def build():
    Z = []
    add = Z.append

    # ---- ring boundary: an in-edge whose source is exactly d positions back, read by two later passes.  (a) a deletion of d - 1 bases in pass 1 makes the edge
    # (in-edge 1 of its target); (b) a bubble of d - 1 inserted vertices spliced between source and target stretches the chain edge (in-edge 0: CREC_FAR0 beyond 8)
    def fix_neighbours(t, *at):
        for i in at:
            if t[i] == t[i - 1] or t[i] == t[i + 1]: t[i] = next(b for b in (0, 1, 2, 3) if b != t[i - 1] and b != t[i + 1] and b != t[i])
        return t

    for d in (7, 8, 9, 20):
        # a deleted block stays one block (no slide, no split: a tie would be broken towards the diagonal) when neither flanking base occurs in it: the block
        # has the letters 2, 3 (and, for the second step of the 19-base deletion, a run of 1), the flanks are 0
        t = template(f"ring{d}", 120)
        n1 = min(d - 1, 10)
        t[59], t[60:60 + n1] = 0, ([2, 3] * 5)[:n1]
        t[60 + n1:60 + d - 1] = 1
        t[60 + d - 1] = 0
        fix_neighbours(t, 58, 60 + d)
        dels = [delete(t, 60, n) for n in range(10, d - 1, 10)] + [delete(t, 60, d - 1)]      # (the band follows a deletion of ten bases, not of nineteen: in two
        n = len(dels)                                                                       #  steps, the second pass takes the first one's edge and deletes on)
        x = dels[-1]
        add(Zmw(f"ring_del_{d}", "ring boundary", [t] + dels + [x, x], [0] * (n + 3), planted=x if n == 1 else None,
                checks=[(f"the last two passes read an in-edge of distance {d}", lambda r, d=d, n=n: all((d, 1, 2) in _edges(r, k) and r[k - 1].max_dist == d for k in (n + 1, n + 2)))]))
        t = template(f"ringb{d}", 120)
        t[50:70] = [0, 1] * 10                            # around the bubble the template has two letters and the bubble the other two: it cannot slide or break up
        for i in (49, 70):
            if t[i] == t[i - 1] or t[i] == t[i + 1]: t[i] = next(b for b in (2, 3) if b != t[i - 1] and b != t[i + 1])
        bub = np.array([2, 3] * 10, np.uint8)[:d - 1]
        grow = [insert(t, 60, bub[:n]) for n in range(10, d - 1, 10)] + [insert(t, 60, bub)]   # (nor does the band follow nineteen inserted bases)
        n = len(grow)
        add(Zmw(f"ring_bubble_{d}", "ring boundary", [t] + grow + [t, t], [0] * (n + 3), planted=t,
                checks=[(f"the last two passes read an in-edge 0 of distance {d}, a near in-edge 1 beside it",
                         lambda r, d=d, n=n: all((d, 0, n + 1) in _edges(r, k) and r[k - 1].max_dist == d for k in (n + 1, n + 2)))]))

    # ---- far edge slot / in-edge count: vertex p collects in-edges from passes that differ right before it — its chain edge (in-edge 0), the three other bases
    # at p - 1, two deletions of 10 and 12 bases that end at p (edges of 11 and 13 positions: far), two bases inserted before p — in the order of the passes.
    # The deleted blocks stay whole: t[p - 10 .. p) has the letters 2, 3, before it stand 1, then 2, then 0, and t[p] = 0 occurs in neither block
    P = 110
    def fan(tag, kinds, n=160):
        t = template(tag, n)
        t[P - 13:P + 1] = [0, 2, 1] + [2, 3] * 5 + [0]
        fix_neighbours(t, P - 14, P + 1)
        make = {"snp0": lambda: snp(t, P - 1, step=1), "snp1": lambda: snp(t, P - 1, step=2), "snp2": lambda: snp(t, P - 1, step=3),
                "del10": lambda: delete(t, P - 10, 10), "del12": lambda: delete(t, P - 12, 12), "ins1": lambda: insert(t, P, [1]), "ins2": lambda: insert(t, P, [2])}
        return t, [make[k]() for k in kinds]

    far = lambda r, slots, n: {s_ for (d_, s_, n_) in _edges(r, len(r)) if d_ > PRING and n_ == n and s_ in slots}
    for k, kinds in ((3, ("del10", "del12")), (4, ("del10", "del12", "snp0")), (7, ("snp0", "snp1", "del10", "del12", "snp2", "ins1")),
                     (8, ("snp0", "snp1", "del10", "del12", "snp2", "ins1", "ins2"))):
        t, var = fan(f"fan{k}", kinds)
        reads = [t] + var + [var[-1], t]                 # the last edge's pass once more: it scores 3 per base only along its own edge (or, refused, never)
        what = f"a vertex with exactly {min(k, 7)} in-edges" + (", an eighth refused" if k == 8 else "")
        chk = [(what, lambda r, k=k: r[-1].max_indeg == min(k, 7) and any(q.cap_refused for q in r) == (k == 8))]
        if k in (3, 4): chk.append(("far edges in slots 1 and 2 beside the near in-edge 0", lambda r, k=k: far(r, (1, 2), k) == {1, 2}))
        if k >= 7: chk.append(("far edges in the overflow slots 3 and 4 of a vertex with seven in-edges", lambda r: far(r, (3, 4, 5, 6), 7) == {3, 4}))
        # (fan_7: the ten-base deletion of pass 3 comes after two more vertices were spliced in before p: twelve columns are more than the band follows there)
        add(Zmw(f"fan_{k}", "far edge slot" if k in (3, 4) else "in-edge count", reads, [0] * len(reads), checks=chk, excused=(3,) if k == 7 else ()))
    # in-edge 0 far with far edges beside it: deletions end at p, then a bubble of 9 before p stretches the chain edge and all the others
    t, var = fan("far0", ("del10", "del12"))
    y = insert(t, P, [1, 0, 1, 0, 1, 0, 1, 0, 1])
    add(Zmw("far0_with_far_slots", "far edge slot", [t] + var + [y, t, t], [0] * 6,
            checks=[("in-edge 0 far (CREC_FAR0), far in-edges 1 and 2, a near in-edge 3", lambda r: far(r, (0, 1, 2, 3), 4) == {0, 1, 2} and (10, 0, 4) in _edges(r, 5))]))

    # ---- record blocks: vertex counts before a pass of 0, 1, 15 (mod 16) and 0, 1, 63 (mod 64); an edit whose new vertex lands on positions 15 / 16, 63 / 64
    for n in (127, 128, 129):
        t = template(f"blk{n}", n)
        add(Zmw(f"block_{n}", "record blocks", [t, snp(t, 15), snp(t, 16), snp(t, 63, 66), t], [0] * 5, planted=t,
                checks=[(f"{n} vertices before pass 1, new vertices at 15, then 16 (17 after the first), then 63 + 2 = 65 and 68 + 2",
                         lambda r, n=n: r[0].I == n and r[0].new_pos == [15] and r[1].new_pos == [17] and r[2].new_pos == [65, 69])],
                log_checks=[("vertex counts n, n + 1, n + 2, n + 4", lambda g, n=n: [int(x) for x in g[:, 5]] == [n + 1, n + 2, n + 4, n + 4])]))
    t = template("blk64", 190)
    add(Zmw("block_new_at_63_64", "record blocks", [t, snp(t, 63), snp(t, 62), t, t], [0] * 5, planted=t,
            checks=[("new vertices land on positions 63 and 64 - 1", lambda r: r[0].new_pos == [63] and r[1].new_pos == [62])]))
    t = template("blk64b", 190)
    add(Zmw("block_new_at_64", "record blocks", [t, snp(t, 64), t, t], [0] * 4, planted=t, checks=[("a new vertex lands on position 64", lambda r: r[0].new_pos == [64])]))

    # ---- trace-back block: an edge that skips more than 64 positions, made by pass 1 and walked by passes 2 and 3; leading insertions at START
    # (the band cannot follow 70 inserted or deleted bases: a bubble grows by ten vertices a pass between two neighbours of the backbone, whose edge the last two
    # passes then walk from position p + 70 to p - 1, across a whole block of the trace-back)
    t = template("tb", 420)
    t[160:180] = [0, 1] * 10
    fix_neighbours(t, 159, 180)
    bub = np.array([2, 3] * 35, np.uint8)
    add(Zmw("tb_skip_block", "trace-back block", [t] + [insert(t, 170, bub[:10 * k]) for k in range(1, 8)] + [t, t], [0] * 10,
            checks=[("the last two passes walk an edge of 71 positions", lambda r: all(q.threaded for q in r) and all((71, 0, 2) in _edges(r, k) and r[k - 1].score == 1260 for k in (8, 9)))]))
    t = template("lead", 150)
    x = insert(t, 0, [(t[0] + 2) & 3, (t[0] + 1) & 3, (t[0] + 2) & 3])
    add(Zmw("tb_leading_insertions", "trace-back block", [t, x, t, x], [0] * 4,
            checks=[("the trace-back of pass 1 ends in three leading insertions, spliced in at the list head", lambda r: r[0].lead_ins == 3 and r[0].new_pos == [0, 1, 2])]))

    # ---- short reads: the clamp max(0, I - 31), drafts of at most one window
    for n in (1, 2, 28, 29, 30, 31, 32, 33, 63):
        t = template(f"short{n}", n)
        add(Zmw(f"short_{n}", "short reads", [t, t, t], [0] * 3, planted=t if n >= 2 else None, checks=[(f"passes of {n} bases", lambda r, n=n: all(q.I == n for q in r))],
                log_checks=[("threaded at 3 per base", lambda g, n=n: all(int(x[1]) == n and int(x[2]) == 3 * n and int(x[4]) == 1 for x in g))]))
    t = template("short12", 200)
    add(Zmw("short_12_among_200", "short reads", [t, t, t[:12].copy(), t], [0] * 4, planted=t,
            checks=[("a 12-base pass ends on vertex 11", lambda r: r[1].I == 12 and r[1].kend == 11 and r[1].score == 36)]))

    # ---- chunk reload: three passes of about 2100 bases with edits at read rows 2012 .. 2050 (the read chunk of 2048 bases is reloaded once the band passes row 2014)
    t = template("chunk", 2100)
    add(Zmw("chunk_reload", "chunk reload", [t, snp(delete(t, 2020, 1), 2012, 2040), insert(snp(t, 2030), 2047, [(t[2047] + 2) & 3]), snp(t, 2050)], [0] * 4, planted=t,
            checks=[("every band goes beyond row 2048 - 32 - 2, where the read chunk is reloaded, and every pass threads its edits there",
                     lambda r: all(q.threaded and q.max_lo > 2014 and q.new_pos and min(q.new_pos) > 2000 for q in r))]))

    # ---- gate: end scores of exactly I, I + 1, I - 1 (a mismatch costs 8, an inserted base 4 and one more base to pay for), a junk pass, a pass the band loses
    # A clean copy of the 200-base template scores 600.  A mismatch costs 8, an inserted base 4 and one more base of I: score - I = 400 - 8 m - 5 k.
    # m = 50: 0.  m = 48, k = 3: + 1.  m = 47, k = 5: - 1.  A wrong base differs from the template's base and both neighbours, an inserted one from both its
    # neighbours, and they stand apart: no alignment with an indel does better
    t = template("gate", 200)
    def other(*not_these): return next(b for b in range(4) if b not in [int(x) for x in not_these])
    for nm, m, k, diff in (("eq", 50, 0, 0), ("plus1", 48, 3, 1), ("minus1", 47, 5, -1)):
        x = t.copy()
        for i in range(2, 4 * m, 4): x[i] = other(t[i - 1], t[i], t[i + 1])
        for p in reversed(range(200 - 2 * k, 200, 2)): x = insert(x, p, [other(t[p - 1], t[p])])
        add(Zmw(f"gate_{nm}", "gate", [t, t, x, t], [0] * 4, planted=t,
                checks=[(f"pass 2 ends at score I {diff:+d}", lambda r, diff=diff: r[1].score == r[1].I + diff and r[1].threaded == (diff >= 0))],
                log_checks=[(f"score I {diff:+d}", lambda g, diff=diff: int(g[1, 2]) == int(g[1, 1]) + diff and int(g[1, 4]) == int(diff >= 0))]))
    junk = _rng("junk").integers(0, 4, 200).astype(np.uint8)
    add(Zmw("gate_junk", "gate", [t, t, junk, t], [0] * 4, planted=t, excused=(2,), checks=[("a junk pass is refused", lambda r: not r[1].threaded and r[1].nverts == 200)],
            log_checks=[("refused", lambda g: int(g[1, 4]) == 0 and int(g[1, 5]) == 200)]))
    lost = np.concatenate([t, _rng("tail").integers(0, 4, 60).astype(np.uint8)])
    add(Zmw("gate_band_lost", "gate", [t, t, lost, t], [0] * 4, planted=t, excused=(2,),
            checks=[("the band never reaches the last row of pass 2", lambda r: r[1].kend == -1 and r[1].score == R.NEG and not r[1].threaded)],
            log_checks=[("no end cell", lambda g: int(g[1, 3]) == -1 and int(g[1, 2]) == R.NEG and int(g[1, 4]) == 0)]))

    # ---- ties: 2 against 2 at even coverage, a homopolymer indel, two predecessors with equal column maxima and different band starts
    t = template("tie", 150)
    s = snp(t, 70)
    add(Zmw("tie_snp_2v2", "ties", [t, t, s, s], [0] * 4, checks=[("two passes on each side of a SNP", lambda r: [q.nverts for q in r] == [150, 151, 151])]))
    x = delete(t, 70, 1)
    add(Zmw("tie_indel_2v2", "ties", [t, t, x, x], [0] * 4, checks=[("two passes on each side of a deletion", lambda r: all(threaded(r)) and r[-1].nverts == 150)]))
    h = insert(t, 70, [t[70]] * 3)                     # a run of four equal bases
    add(Zmw("tie_homopolymer", "ties", [h, delete(h, 70, 1), h, delete(h, 71, 1)], [0] * 4, planted=None,
            checks=[("a deleted base of a homopolymer: diagonal and deletion tie on the path of the pass that lacks it, nowhere on the full copy's", lambda r: all(threaded(r)) and r[-1].nverts == 153 and r[0].path_ties > 0 and r[1].path_ties == 0)]))
    a, rp, b = template("tieA", 60), template("tieR", 16), template("tieB", 60)
    g = np.concatenate([a, rp, rp, b])
    # a deleted copy of a repeat leaves an edge around one copy (which one: the tie-breaks decide); a pass whose other copy scores 0 in all (ten matches,
    # six mismatches) then finds the column maxima at both ends of that copy equal, eight rows apart
    add(Zmw("tie_colmax", "ties", [g, delete(g, 60, 16), np.concatenate([a, snp(rp, *WORN), rp, b]), np.concatenate([a, rp, snp(rp, *WORN), b])], [0] * 4,
            checks=[("two predecessors with equal column maxima and different band starts", lambda r: r[1].ustar_ties + r[2].ustar_ties > 0)]))

    # the consensus ends at the FIRST maximum: two of four passes have one more base at their end, a vertex of weight 2 * 2 - 4 = 0 behind the last one — the same
    # best score one position later, inside one 64-position block of k_poa_finish (40 bases) and across two (64 bases: positions 63 and 64)
    for n in (40, 64):
        t = template(f"tieend{n}", n)
        x = insert(t, n, [(t[n - 1] + 2) & 3])
        add(Zmw(f"tie_consensus_end_{n}", "ties", [t, x, t, x], [0] * 4, planted=t,
                checks=[("the extra base becomes the last vertex, two of four passes go through it", lambda r, n=n: all(threaded(r)) and r[0].new_pos == [n] and r[-1].nverts == n + 1)]))

    # ---- strands: a reverse-strand backbone with forward passes and the converse, read lengths 0, 1, 15 (mod 16)
    for n in (96, 97, 111):
        t = template(f"strand{n}", n)
        add(Zmw(f"strand_rev_backbone_{n}", "strands", [rc(t), t, t, rc(t)], [1, 0, 0, 1], planted=rc(t), checks=[("both strands in one graph: every pass, oriented to the backbone, scores 3 per base", lambda r: all(q.threaded and q.score == 3 * q.I for q in r))]))
        add(Zmw(f"strand_fwd_backbone_{n}", "strands", [t, rc(t), rc(t)], [0, 1, 1], planted=t, checks=[("both strands in one graph: every pass, oriented to the backbone, scores 3 per base", lambda r: all(q.threaded and q.score == 3 * q.I for q in r))]))

    # ---- coverage option: partial passes follow the full ones and are never threaded; more passes than max_poa_cov
    t = template("cov", 180)
    add(Zmw("cov_partials", "coverage option", [t, snp(t, 50), t, t[:100].copy(), t[90:].copy()], [0, 0, 0, 2, 6], planted=t,
            checks=[("two records: the partial passes are not threaded", lambda r: len(r) == 2)], log_checks=[("two records", lambda g: len(g) == 2)]))
    add(Zmw("cov_eight_passes", "coverage option", [t, snp(t, 20), snp(t, 40), snp(t, 60), snp(t, 80), snp(t, 20), snp(t, 20), snp(t, 20)], [0] * 8,
            checks=[("seven passes threaded", lambda r: len(r) == 7 and all(threaded(r)))], log_checks=[("seven records", lambda g: len(g) == 7)]))

    # ---- fallback: pass 0 is junk, so the second generator runs: backbone = the pass closest to the median length, the others threaded from there, wrapping.
    # Lengths are planted so that the backbone is the middle pass, the last pass, or pass 0 again (junk once more: the last resort takes over)
    t = template("fb", 200)
    good = {203: insert(insert(insert(t, 40, [(t[40] + 2) & 3]), 90, [(t[89] + 2) & 3]), 150, [(t[148] + 2) & 3]), 201: insert(t, 120, [(t[120] + 2) & 3]),
            198: delete(delete(t, 60, 1), 130, 1), 200: t.copy()}
    # (junk against the template: the band finds an alignment, not the best one — excused, pass by pass)
    for nm, jl, lens, bb, ex, ex2 in (("middle", 230, (203, 201, 198, 200), 2, (1, 2, 3, 4), (3,)), ("last", 230, (203, 200, 198, 201), 4, (1, 2, 3, 4), (1,)),
                                      ("first", 201, (203, 200, 198, 201), 0, (2, 3, 4), (2, 3, 4))):
        reads = [_rng("fbjunk" + nm).integers(0, 4, jl).astype(np.uint8)] + [good[n] for n in lens]
        add(Zmw(f"fallback_{nm}", "fallback", reads, [0] * 5, planted=t if bb else None, fallback=bb, excused=ex, excused2=ex2,
                checks=[("nothing threads into the junk backbone", lambda r: not any(threaded(r)))], log_checks=[("nothing threaded", lambda g: not g[:, 4].any())]))

    # ---- overflow: 14 passes of mutually different mismatches on a 400-base template cross the vertex capacity 2.5 * 400 + 256 = 1256.  Pass k has a mismatch
    # at every fifth base, with its own phase and wrong base (fifteen combinations): up to 80 new vertices each (a few find a neighbour's vertex), so that the
    # twelfth would cross the capacity.  The sibling's last passes are worn in their first 250 and 130 bases only and stop a few vertices short
    t = template("over", 400)
    def worn(k, upto=400): return snp(t, *range(k % 5, upto, 5), step=1 + k // 5)
    # (pass 11 of both: a mismatch at every fifth base against a graph that holds ten other passes' — the band settles for a near-optimal path)
    add(Zmw("overflow", "overflow", [t] + [worn(k) for k in range(13)], [0] * 14, fails=True, excused=(11,),
            checks=[("the last pass read would take the graph past its 1256 vertices", lambda r: r[-1].overflow and all(threaded(r[:-1])) and r[-1].nverts + 80 > 1256)],
            log_checks=[("the last pass is not threaded although its score passes the gate", lambda g: g[:-1, 4].all() and int(g[-1, 4]) == 0 and int(g[-1, 5]) + 80 > 1256 and int(g[-1, 2]) >= int(g[-1, 1]))]))
    add(Zmw("overflow_sibling", "overflow", [t] + [worn(k) for k in range(10)] + [worn(10, 250), worn(11, 130), worn(7)], [0] * 14, excused=(11,),
            checks=[("thirteen passes threaded, at most sixteen vertices short of the capacity", lambda r: len(r) == 13 and all(threaded(r)) and 1240 <= r[-1].nverts <= 1256)],
            log_checks=[("thirteen threaded, at most sixteen short", lambda g: len(g) == 13 and g[:, 4].all() and 1240 <= int(g[-1, 5]) <= 1256)]))
    # ---- band limit: the ZMWs of the low-complexity fuzz (tests/test_poa_ref.py FUZZ "lowcx") in which the 32-row band falls short of the unbanded optimum — it
    # settles on another phase of a tandem repeat or homopolymer.  Taken over whole and named, so that the fuzz itself excuses nothing
    import lowcx
    b = lowcx.make(*LOWCX_FUZZ[:-1], tpl=LOWCX_FUZZ[-1])
    for zi, ex in LOWCX_SHORT.items():
        r0, r1 = int(b.read_off[zi]), int(b.read_off[zi + 1])
        reads = [np.array(b.bases[int(b.base_off[r]):int(b.base_off[r + 1])], np.uint8) for r in range(r0, r1)]
        add(Zmw(f"lowcx_{zi}", "band limit", reads, [int(f) for f in b.flags[r0:r1]], excused=ex))   # (the class IS the excuse: each excused pass must fall short)
    return Z


LOWCX_FUZZ = (70, (3, 8), (40, 400), 43, "lowcx")    # lowcx.make arguments of the low-complexity fuzz
LOWCX_SHORT = {2: (3,), 7: (3,), 10: (3,), 34: (1, 3), 39: (2,), 51: (4,), 66: (2, 3, 4)}   # its ZMWs that became lab entries: the passes excused at COV


@lru_cache(maxsize=None)
def lab():
    """the lab's ZMWs, in batch order"""
    return build()


def batch_of(zmws) -> api.Batch:
    reads = [r for z in zmws for r in z.reads]
    ro = np.concatenate([[0], np.cumsum([len(z.reads) for z in zmws])]).astype(np.int32)
    bo = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
    bases = np.ascontiguousarray(np.concatenate(reads).astype(np.uint8))
    n = len(zmws)
    return api.Batch(np.arange(n, dtype=np.int32), np.tile(np.array([[9, 16, 8, 13]], np.float32), (n, 1)), ro, bo, bases,
                     np.full(len(bases), 2, np.uint8), np.ones(len(bases), np.uint8), np.array([f for z in zmws for f in z.flags], np.uint8))

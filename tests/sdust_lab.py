"""The tandem-repeat rule's laboratory (DESIGN.md §2 "Tandem repeats"): a parameterised form of tests/sdust_ref.py's incremental rule and of its
64-lane split, whose knobs are the slips a kernel could plausibly make (MUTANTS); the readers of the limit set tests/golden/sdust_limits.npz
(tests/golden/make_sdust_limits.py writes it); batches that hand k_sdust an exact draft (identical passes: the POA returns the template itself); and the
ZMWs of the deciding-draft cases.  With the default knobs the parameterised form IS sdust_ref.masked_incremental / masked_lanes, bit for bit
(tests/test_tandem_limits.py holds that)."""
from __future__ import annotations

import os
from dataclasses import dataclass

import numpy as np

import sdust_ref as R

W, T, KMAX = R.W, R.T, R.KMAX
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sdust_limits.npz")


@dataclass(frozen=True)
class Knobs:
    warm: int = 0           # a lane's warm-up starts `warm` ends later than W - 3 ends before its range
    leave: int = 0          # the window triplet e - 62 - leave leaves at end e (-1: one end early)
    gate: int = 0           # added to the gate's longest suffix (S_w - 1) / 2
    kmax: int = 0           # added to the longest suffix W - 3
    strict_tie: bool = False  # an interval must beat, not equal, the best perfect interval inside it
    ring: int = 64          # slots of the best-per-start ring
    thr_ge: bool = False    # S * 10 >= T * k: a score of exactly 2.0 counts


DEFAULT = Knobs()
# every mutant is one plausible slip of k_sdust.  ("leave+1", Knobs(leave=1): the triplet leaves one end late.  EQUIVALENT, not a mutant: S_w only bounds a
# suffix's pairs from above, a larger S_w loosens an exact bound and no suffix is scored differently — the 64-slot triplet ring still holds the triplet.)
MUTANTS = {
    "warm-1": Knobs(warm=1),
    "leave-1": Knobs(leave=-1),
    "gate-1": Knobs(gate=-1),
    "kmax-1": Knobs(kmax=-1),
    "tie>": Knobs(strict_tie=True),
    "ring61": Knobs(ring=61),
    "thr>=": Knobs(thr_ge=True),
}
SINGLE_LANE = [m for m in MUTANTS if m != "warm-1"]      # the slips one lane can make alone; warm-1 is a slip of the split


def _tri(seq) -> list:
    return [int(t) for t in R.triplets(seq)]


def lane_ends(tri: list, lo: int, e0: int, e1: int, mask: np.ndarray, K: Knobs = DEFAULT) -> None:
    """sdust_ref.masked_incremental's loop under the knobs K: the ends [e0, e1) of a lane whose warm-up starts at triplet lo, ORed into mask"""
    nt = len(tri)
    ring = K.ring
    best = [0] * ring
    win = [0] * 64
    if nt > lo:
        win[tri[lo]] = 1
    Sw = 0
    leave = W - 2 + K.leave
    kcap = KMAX + K.kmax
    for e in range(lo + 1, e1):
        if e - leave >= lo:
            to = tri[e - leave]
            win[to] -= 1
            Sw -= win[to]
        tn = tri[e]
        Sw += win[tn]
        win[tn] += 1
        best[e % ring] = 0
        cnt = {tn: 1}
        g = max(0, ((Sw - 1) >> 1) + K.gate) if Sw > 0 else 0
        ilo = max(lo, e - kcap, e - g)
        S = MS = Mk = 0
        imn = -1
        for i in range(e - 1, ilo - 1, -1):
            k = e - i
            t = tri[i]
            c = cnt.get(t, 0)
            S += c
            cnt[t] = c + 1
            b = best[i % ring]
            if b and (not Mk or (b >> 8) * Mk > MS * (b & 255)):
                MS, Mk = b >> 8, b & 255
            over = S * 10 >= T * k if K.thr_ge else S * 10 > T * k
            if over and (not Mk or (S * Mk > MS * k if K.strict_tie else S * Mk >= MS * k)):
                MS, Mk = S, k
                best[i % ring] = (S << 8) | k
                imn = i
        if e >= e0 and imn >= 0:
            mask[imn:e + 3] = True


def masked_incremental(seq, K: Knobs = DEFAULT) -> np.ndarray:
    """one lane over the whole draft"""
    tri = _tri(seq)
    mask = np.zeros(len(seq), bool)
    if len(tri) >= 2:
        lane_ends(tri, 0, 1, len(tri), mask, K)
    return mask


def masked_lanes(seq, K: Knobs = DEFAULT, lanes: int = 64) -> np.ndarray:
    """the kernel's split: lane l owns ends [1 + l ch, 1 + (l + 1) ch) and warms up over the W - 3 - K.warm ends before them"""
    tri = _tri(seq)
    mask = np.zeros(len(seq), bool)
    nt = len(tri)
    if nt < 2:
        return mask
    ch = (nt - 1 + lanes - 1) // lanes
    for lane in range(lanes):
        e0 = 1 + lane * ch
        e1 = min(e0 + ch, nt)
        if e0 < e1:
            lane_ends(tri, max(0, e0 - KMAX + K.warm), e0, e1, mask, K)
    return mask


def tandem_len(seq, K: Knobs = DEFAULT) -> int:
    """what a k_sdust with the slip K would report: its 64-lane split, then the longest run"""
    return R.longest_run(masked_lanes(seq, K)) if len(seq) >= 3 else 0


def kills(seq, names=None) -> dict:
    """mutant -> the tandem_len it gives, for the mutants under which tandem_len (not merely the mask) changes"""
    want = tandem_len(seq)
    out = {}
    for m in (names if names is not None else MUTANTS):
        got = tandem_len(seq, MUTANTS[m])
        if got != want:
            out[m] = got
    return out


# ---------------------------------------------------------------- what the kernel's launch makes of a length
def ch_of(Ld: int) -> int:
    """ends per lane: ceil((nt - 1) / 64), nt = Ld - 2 triplets"""
    return max(0, (Ld - 3 + 63) // 64)


def cb_of(Ld: int) -> int:
    """bases per lane of the longest-run scan: ceil(Ld / 64)"""
    return (Ld + 63) // 64


def runs(mask) -> list:
    """the maximal runs of masked bases as (start, end) with end inclusive, in order"""
    m = np.concatenate([[0], np.asarray(mask, np.int8), [0]])
    d = np.diff(m)
    return list(zip(np.flatnonzero(d == 1).tolist(), (np.flatnonzero(d == -1) - 1).tolist()))


def longest(mask):
    """the first longest run (start, end), or None"""
    rr = runs(mask)
    return max(rr, key=lambda r: (r[1] - r[0], -r[0])) if rr else None


def interval_scores(seq) -> list:
    """(i, e, S, k) of every interval of triplets [i, e] inside a window (k = e - i in 1..W - 3), counted directly"""
    tri = _tri(seq)
    out = []
    for i in range(len(tri)):
        cnt, S = {}, 0
        for e in range(i, min(len(tri), i + KMAX + 1)):
            c = cnt.get(tri[e], 0)
            S += c
            cnt[tri[e]] = c + 1
            if e > i:
                out.append((i, e, S, e - i))
    return out


# ---------------------------------------------------------------- the limit set
@dataclass
class Limits:
    names: list             # one per draft, "<group>/<what>"
    drafts: list            # uint8 codes
    expect: np.ndarray      # tandem_len of each, from the written definition (sdust_ref.masked_bruteforce)
    kills: np.ndarray       # [draft, mutant] bool: tandem_len changes under MUTANTS' k-th entry
    mutants: list
    too_short: np.ndarray   # the one draft below opts.min_length: expects 0 and status TOO_SHORT
    unrealised: list        # the properties of (d) the search could not realise

    def index(self, name: str) -> int:
        return self.names.index(name)

    def group(self, prefix: str) -> list:
        return [k for k, n in enumerate(self.names) if n.startswith(prefix)]


def load(path: str = GOLDEN) -> Limits:
    with np.load(path) as f:
        off = f["draft_off"]
        cat = f["drafts"]
        return Limits([str(n) for n in f["names"]], [cat[off[k]:off[k + 1]].copy() for k in range(len(off) - 1)], f["expect"].copy(),
                      f["kills"].astype(bool), [str(m) for m in f["mutants"]], f["too_short"].copy(), [str(u) for u in f["unrealised"]])


# ---------------------------------------------------------------- exact-draft batches
def batch_from_passes(zmws, seed: int = 0):
    """an api.Batch whose ZMW z has the passes zmws[z], each given in the template's orientation: pass q is stored reverse-complemented with strand flag 1
    when q is odd.  pw / ipd as tests/test_fold.py::_from_templates fills them (pulse widths 1..3 at .3 .3 .4, ipd codes 1..60), no read-error channel"""
    from ccs_amd import api
    rng = np.random.default_rng(seed)
    zmw_id, snr, read_off, base_off, flags, bases = [], [], [0], [0], [], [np.zeros(0, np.uint8)]
    for z, passes in enumerate(zmws):
        zmw_id.append(z); snr.append([9.0, 16.0, 8.0, 13.0])
        for q, p in enumerate(passes):
            p = np.asarray(p, np.uint8)
            bases.append(R.revcomp(p) if q & 1 else p); flags.append(q & 1); base_off.append(base_off[-1] + len(p))
        read_off.append(read_off[-1] + len(passes))
    nb = base_off[-1]
    pw = (np.searchsorted([0.3, 0.6], rng.random(nb)) + 1).astype(np.uint8)
    return api.Batch(np.array(zmw_id, np.int32), np.array(snr, np.float32), np.array(read_off, np.int32), np.array(base_off, np.int64),
                     np.ascontiguousarray(np.concatenate(bases), np.uint8), pw, rng.integers(1, 61, nb).astype(np.uint8), np.array(flags, np.uint8))


def batch_from_drafts(drafts, passes: int = 3, seed: int = 0):
    """every ZMW gets `passes` identical passes of its draft on alternating strands: the POA draft is the draft itself, so k_sdust is handed exactly it"""
    return batch_from_passes([[d] * passes for d in drafts], seed)


def passes_of(batch, z: int):
    """(reads in native orientation, flags) of ZMW z: what oracle_lib.poa_generator takes"""
    r0, r1 = int(batch.read_off[z]), int(batch.read_off[z + 1])
    return [np.array(batch.bases[int(batch.base_off[r]):int(batch.base_off[r + 1])], np.uint8) for r in range(r0, r1)], [int(f) for f in batch.flags[r0:r1]]


# ---------------------------------------------------------------- the deciding draft (the first draft the cascade aligns passes to)
def unmasked(rng, n: int) -> np.ndarray:
    """a random sequence of n bases without a masked base"""
    while True:
        x = rng.integers(0, 4, n).astype(np.uint8)
        if not R.masked_incremental(x).any():
            return x


def with_tract(rng, n: int, unit, tract: int) -> np.ndarray:
    """n bases, random but for one tract of `unit` in the middle, whose longest masked run is the tract's (at least `tract` bases)"""
    while True:
        x = rng.integers(0, 4, n).astype(np.uint8)
        p = (n - tract) // 2
        x[p:p + tract] = np.tile(np.asarray(unit, np.uint8), tract // len(unit) + 1)[:tract]
        if tract <= R.tandem_len(x) <= tract + 8:
            return x


@dataclass
class CascadeCase:
    name: str
    passes: list            # in the template's orientation (batch_from_passes)
    first: "np.ndarray | None"   # the first generator's draft (the no_fallback_draft handle's stage_draft), None: it fails (DRAFT_FAILURE)
    first_len: int          # tandem_len of the first draft (0 without one)
    final_len: int          # tandem_len of the draft the polish is given
    expect: int             # tandem_len of the deciding draft
    threshold: int          # strictly between the two candidates


def cascade_cases() -> list:
    """the four ZMWs of the deciding-draft test.  A junk pass 0 is its generator's draft itself (nothing threads into it), most passes do not align to it, and
    the fallback generator takes the pass closest to the median length as backbone; with that one junk too, the last resort takes a pass as the draft"""
    rng = np.random.default_rng(2006)
    acg = np.tile(np.array([0, 1, 2], np.uint8), 60)                       # 180 bases, masked over their whole length
    clean = unmasked(rng, 240)
    tract = with_tract(rng, 420, [0, 2, 2, 2, 2, 3], 300)
    junk = unmasked(rng, 200)
    junk[90:102] = 3                                                       # twelve T: a small value that is not the 0 of "undecided"
    tract3 = with_tract(rng, 380, [1, 3], 260)
    t4 = with_tract(rng, 301, [0, 0, 2], 150)
    t4s = np.delete(t4, 20)                                                # 299 bases: the median of 180 299 299 300 301 301 301 is the junk of 300
    junk4 = unmasked(rng, 300)
    tl = R.tandem_len
    cases = [
        CascadeCase("tandem_junk_then_clean", [acg] + [clean] * 5, acg, tl(acg), tl(clean), tl(acg), 0),
        CascadeCase("random_junk_then_tract", [junk] + [tract] * 5, junk, tl(junk), tl(tract), tl(junk), 0),
        CascadeCase("empty_pass_then_tract", [np.zeros(0, np.uint8)] + [tract3] * 5, None, 0, tl(tract3), tl(tract3), 0),
        CascadeCase("two_junk_backbones", [acg, t4, t4s, junk4, t4, t4s, t4], acg, tl(acg), tl(t4), tl(acg), 0),
    ]
    for c in cases:
        a, b = sorted((c.first_len, c.final_len))
        assert b - a >= 2, c.name
        c.threshold = (a + b + 1) // 2
    assert cases[0].final_len == 0 and cases[0].expect == 180 and 0 < cases[1].expect < 20 < 300 <= cases[1].final_len
    return cases

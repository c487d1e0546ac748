#!/usr/bin/env python3
"""Generates tests/golden/sdust_limits.npz: the limit set of the tandem-repeat rule (DESIGN.md §2 "Tandem repeats").  Drafts of 10..400 bases that place a
masked run against every boundary of k_sdust — a lane's range of ends, its warm-up, the words of the LDS mask, the chunks of the longest-run scan — and
drafts on which a kernel with one of tests/sdust_lab.py's slips (MUTANTS) reports another tandem_len.  Seeded: the same file every time.

Every expectation is the written definition (sdust_ref.masked_bruteforce); the generator asserts that the incremental form and the 64-lane split agree with
it, and that the CPU oracle's draft generator returns every draft exactly from three identical passes (a draft it did not reproduce would be replaced, not
skipped).  tests/test_tandem_limits.py recomputes every claim from the file.     python tests/golden/make_sdust_limits.py
"""
import os
import sys
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import sdust_ref as R  # noqa: E402
import sdust_lab as LAB  # noqa: E402

SEED = 20061028
UNITS = ([0], [0, 1], [0, 2, 3], [1, 1, 3], [0, 1, 2, 3], [2, 0, 0, 1, 3], [0, 2, 2, 2, 2, 3], [0, 1, 2, 3, 3, 1])


def rng_of(*key):
    return np.random.default_rng([SEED, *[int(k) for k in key]])


def tile(unit, n):
    return np.tile(np.asarray(unit, np.uint8), n // len(unit) + 1)[:n]


def planted(Ld, start, n, unit, key):
    """random bases with a tract of n bases of `unit` at `start`"""
    x = rng_of(*key).integers(0, 4, Ld).astype(np.uint8)
    x[start:start + n] = tile(unit, n)
    return x


def mask_of(x):
    return R.masked_incremental(x)


# ---------------------------------------------------------------- (e) lengths: a tract-bearing draft of every length at which the launch changes shape
def length_drafts():
    want = sorted(set(range(10, 71)) | {32 * k + d for k in (2, 3, 4) for d in (-1, 0, 1)} | {67, 68, 131, 132})
    out = []
    for Ld in want:
        g = rng_of(1, Ld)
        n = int(g.integers(9, max(10, min(Ld - 1, 48)) + 1)) if Ld > 10 else 9
        where = int(g.integers(0, 3))                                      # the tract at the start, at the end, inside
        start = 0 if where == 0 else Ld - n if where == 1 else int(g.integers(0, Ld - n + 1))
        out.append((f"len/{Ld}", planted(Ld, start, n, UNITS[int(g.integers(0, len(UNITS)))], (2, Ld))))
    return out


# ---------------------------------------------------------------- (d) mask and scan: each property is a predicate on (Ld, mask); the first candidate that has it is kept
def p_alone(m, pred):
    """the longest run is unique and has the property"""
    rr = LAB.runs(m)
    if not rr:
        return False
    lens = sorted(b - a + 1 for a, b in rr)
    lg = LAB.longest(m)
    return (len(lens) == 1 or lens[-1] > lens[-2]) and pred(*lg)


def cb_class(Ld):
    cb = LAB.cb_of(Ld)
    return "1" if cb == 1 else "2" if cb == 2 else "4+" if cb >= 4 else None


def mask_properties():
    """name -> predicate(Ld, mask)"""
    P = {
        "run/starts_at_0": lambda L, m: not m.all() and p_alone(m, lambda a, b: a == 0),
        "run/ends_at_last": lambda L, m: not m.all() and p_alone(m, lambda a, b: b == L - 1),
        "word/begins_at_bit0": lambda L, m: p_alone(m, lambda a, b: a > 0 and a % 32 == 0 and b % 32 != 31),
        "word/ends_at_bit31": lambda L, m: p_alone(m, lambda a, b: b < L - 1 and b % 32 == 31 and a % 32 != 0),
        "word/three_whole_words": lambda L, m: p_alone(m, lambda a, b: a % 32 != 0 and b % 32 != 31 and (b + 1) // 32 - (a + 31) // 32 >= 3),
        "word/inside_one_word": lambda L, m: p_alone(m, lambda a, b: a % 32 != 0 and b % 32 != 31 and a // 32 == b // 32),
        "gap/one_unmasked_base": lambda L, m: any(c - b == 2 for (a, b), (c, d) in zip(LAB.runs(m), LAB.runs(m)[1:])),
    }
    for cls in ("1", "2", "4+"):
        def in_cls(L, cls=cls):
            return cb_class(L) == cls

        def whole(L, m, cls=cls):             # a whole scan chunk (or more) between two partial ones; at cb = 1 a chunk is one base and none is partial
            cb = LAB.cb_of(L)
            if cb == 1:
                return p_alone(m, lambda a, b: a > 0 and b < L - 1)
            return p_alone(m, lambda a, b: a % cb != 0 and (b + 1) % cb != 0 and (b + 1) // cb - (a + cb - 1) // cb >= 1)

        def one_chunk(L, m):                  # a run that touches one chunk only
            cb = LAB.cb_of(L)
            return p_alone(m, lambda a, b: a // cb == b // cb)

        def two(L, m, first):
            rr = LAB.runs(m)
            if len(rr) != 2:
                return False
            (a, b), (c, d) = rr
            return (b - a > d - c) if first else (d - c > b - a)
        P[f"scan/cb{cls}/inside_one_chunk"] = lambda L, m, f=in_cls, g=one_chunk: f(L) and g(L, m)
        P[f"scan/cb{cls}/whole_chunk_between_partial"] = lambda L, m, f=in_cls, g=whole: f(L) and g(L, m)
        P[f"scan/cb{cls}/longer_first"] = lambda L, m, f=in_cls, g=two: f(L) and g(L, m, True)
        P[f"scan/cb{cls}/longer_second"] = lambda L, m, f=in_cls, g=two: f(L) and g(L, m, False)
    return P


def mask_candidates():
    """a seeded stream of drafts with one or two planted tracts, lengths over the three classes of the scan"""
    k = 0
    while True:
        g = rng_of(3, k)
        cls = k % 3
        Ld = int(g.integers(20, 65)) if cls == 0 else int(g.integers(65, 129)) if cls == 1 else int(g.integers(193, 401))
        x = g.integers(0, 4, Ld).astype(np.uint8)
        for _ in range(int(g.integers(1, 3))):
            n = int(g.integers(7, min(Ld, 130)))
            s = int(g.integers(0, Ld - n + 1))
            x[s:s + n] = tile(UNITS[int(g.integers(0, len(UNITS)))], n)
        yield x
        k += 1


def mask_drafts(budget=20000):
    P = mask_properties()
    found, unrealised = {}, []
    for k, x in zip(range(budget), mask_candidates()):
        m = mask_of(x)
        for name, pred in P.items():
            if name not in found and pred(len(x), m):
                found[name] = x
        if all(n in found or n.endswith("/inside_one_chunk") for n in P):       # (those the stream cannot draw: below)
            break
    # a run that touches one scan chunk only: a masked run has at least 7 bases and drafts of up to 400 bases have cb <= 7, so it is seven equal bases on a chunk
    # of cb = 7 (385..400 bases) with nothing else masked — planted, the stream above does not draw it
    name = "scan/cb4+/inside_one_chunk"
    for k in range(4000):
        g = rng_of(7, k)
        Ld = int(g.integers(385, 401))
        x = g.integers(0, 4, Ld).astype(np.uint8)
        s = 7 * int(g.integers(1, Ld // 7 - 1))
        c = int(g.integers(0, 4))
        x[s:s + 7] = c
        x[s - 1], x[s + 7] = (c + 1) & 3, (c + 2) & 3
        if P[name](Ld, mask_of(x)):
            found[name] = x
            break
    out = [(f"full/{Ld}", tile(u, Ld)) for Ld, u in ((10, [0]), (64, [0, 1]), (65, [0, 2, 2, 2, 2, 3]), (200, [0, 2, 3]))]
    for name in P:
        if name in found:
            out.append((name, found[name]))
        else:
            unrealised.append(name)
    return out, unrealised


# ---------------------------------------------------------------- (a) mutant kills, (b) the gate's limit, (c) the tie
def mix_candidate(k):
    """the random mix: 10..400 bases, up to three planted low-complexity stretches with errors (the kind tests/test_tandem.py's CPU test draws)"""
    g = rng_of(4, k)
    L = int(round(np.exp(g.uniform(np.log(10), np.log(400)))))
    x = g.integers(0, 4, L).astype(np.uint8)
    for _ in range(int(g.integers(1, 4))):
        u = g.integers(0, 4, int(g.integers(1, 9))).astype(np.uint8)
        n = int(g.integers(8, 90))
        p = int(g.integers(0, max(1, L - 8)))
        rep = tile(u, n)[:L - p]
        err = g.random(len(rep)) < 0.04
        rep[err] = g.integers(0, 4, int(err.sum()))
        x[p:p + len(rep)] = rep
    return x


def warm_candidate(cls, k):
    """targeted at the warm-up: a period-6..16 tract of 50..90 bases with 3 % errors; cls 0, 1, 2: ch = 1, 2, at least 3"""
    g = rng_of(5, cls, k)
    L = int(g.integers(66, 68)) if cls == 0 else int(g.integers(68, 132)) if cls == 1 else int(g.integers(132, 400))
    x = g.integers(0, 4, L).astype(np.uint8)
    u = g.integers(0, 4, int(g.integers(6, 17))).astype(np.uint8)
    n = min(int(g.integers(50, 91)), L)
    p = int(g.integers(0, L - n + 1))
    rep = tile(u, n)
    err = g.random(n) < 0.03
    rep[err] = g.integers(0, 4, int(err.sum()))
    x[p:p + n] = rep
    return x


def _kills_mix(k):
    x = mix_candidate(k)
    return k, LAB.kills(x, LAB.SINGLE_LANE)


def _kills_warm(ck):
    x = warm_candidate(*ck)
    return ck, LAB.kills(x, ["warm-1"])


def mutant_drafts(pool, per_mutant=3):
    out = []
    have = {m: [] for m in LAB.SINGLE_LANE}
    step = 256
    for k0 in range(0, 40000, step):
        for k, kl in pool.map(_kills_mix, range(k0, k0 + step), chunksize=8):
            for m in kl:
                if len(have[m]) < per_mutant:
                    have[m].append(k)
        if all(len(v) >= per_mutant for v in have.values()):
            break
    assert all(len(v) >= per_mutant for v in have.values()), {m: len(v) for m, v in have.items()}
    seen = set()
    for m, ks in have.items():
        for j, k in enumerate(sorted(ks, key=lambda k: len(mix_candidate(k)))):      # the shortest first, for the reader's sake
            if k not in seen:                                                         # (a draft that kills two mutants is kept once, under the first one's name)
                seen.add(k)
                out.append((f"kill/{m}/{j}", mix_candidate(k)))
    for cls in range(3):
        hit = []
        for k0 in range(0, 20000, step):
            for ck, kl in pool.map(_kills_warm, [(cls, k) for k in range(k0, k0 + step)], chunksize=8):
                if kl:
                    hit.append(ck[1])
            if len(hit) >= 2:
                break
        assert hit, f"no warm-1 kill in class {cls}"
        for j, k in enumerate(hit[:2]):
            out.append((f"kill/warm-1/ch{cls + 1}/{j}", warm_candidate(cls, k)))
    return out


def gate_limit_draft():
    """a draft whose only interval with a score above 2.0 has S = 2 k + 1, the fewest pairs the gate lets through.  Such an interval is perfect (nothing inside
    it scores above 2.0 at all) and spans the whole evaluation window when it is reached, so S_w = S: a gate one tighter never scores it"""
    found = []
    for k in range(20000):                    # (the shortest of what 20000 perturbed short repeats hold: 19 bases, 17 triplets with S = 33)
        g = rng_of(6, k)
        L = int(g.integers(10, 40))
        p = int(g.integers(1, 7))
        x = tile(g.integers(0, 4, p), L)
        for _ in range(int(g.integers(0, 4))):
            x[int(g.integers(0, L))] = int(g.integers(0, 4))
        over = [(i, e, S, kk) for i, e, S, kk in LAB.interval_scores(x) if S * 10 > LAB.T * kk]
        if len(over) == 1 and over[0][2] == 2 * over[0][3] + 1 and LAB.kills(x, ["gate-1"]):
            found.append(x)
    assert found, "no gate-limit draft"
    return [("gate/limit", min(found, key=len))]


def name_tie_draft(kill_drafts):
    """(c): the first of the tie> kills in which a perfect interval contains a perfect interval of the same score takes the name tie/nested_equal_score"""
    for j, (name, x) in enumerate(kill_drafts):
        if name.startswith("kill/tie>/") and nested_tie(x):
            kill_drafts[j] = ("tie/nested_equal_score", x)
            return
    raise AssertionError("no tie draft among the tie> kills")


def nested_tie(x):
    S, _ = R.pair_table(x)
    per = sorted(R.perfect_intervals_bruteforce(x))
    for i, e in per:
        for a, b in per:
            if (a, b) != (i, e) and i <= a and b <= e and S[a, b - a] * (e - i) == S[i, e - i] * (b - a):
                return True
    return False


# ---------------------------------------------------------------- the oracle hands every draft back
def oracle_returns(x):
    import oracle_lib as O
    b = LAB.batch_from_drafts([x])
    reads, flags = LAB.passes_of(b, 0)
    d, _ = O.poa_generator(reads, flags, 5)
    return d is not None and np.array_equal(d, x)


def _brute(x):
    return R.masked_bruteforce(x)


def _row(x):
    kl = LAB.kills(x)
    return [m in kl for m in LAB.MUTANTS]


def main():
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        items = length_drafts()
        md, unrealised = mask_drafts()
        items += md
        kd = mutant_drafts(pool)
        name_tie_draft(kd)
        items += kd + gate_limit_draft()
        names = [n for n, _ in items]
        drafts = [np.ascontiguousarray(x, np.uint8) for _, x in items]
        assert len(set(names)) == len(names) and all(10 <= len(x) <= 400 for x in drafts)
        for n, x in items:
            assert oracle_returns(x), f"{n}: the oracle's generator does not return this draft; replace it"
        masks = pool.map(_brute, drafts, chunksize=2)
        for n, x, m in zip(names, drafts, masks):
            assert np.array_equal(m, R.masked_incremental(x)) and np.array_equal(m, R.masked_lanes(x)), n
            assert np.array_equal(m, LAB.masked_incremental(x)) and np.array_equal(m, LAB.masked_lanes(x)), n
        expect = np.array([R.longest_run(m) for m in masks], np.int32)
        kills = np.array(pool.map(_row, drafts, chunksize=2), np.uint8)
    # every warm-1 kill is a kmax-1 kill as well (both only lose perfect intervals of 62 triplets, warm-1 a subset of them, and the longest run is monotone in
    # the mask); what tells the split's slip from a lane's is a draft on which warm-1's value is that of no single-lane mutant
    told = [n for n, x, r in zip(names, drafts, kills) if r[0] and LAB.tandem_len(x, LAB.MUTANTS["warm-1"]) not in
            {LAB.tandem_len(x, LAB.MUTANTS[m]) for m in LAB.SINGLE_LANE}]
    assert told, "no draft tells warm-1 from the single-lane mutants"
    too_short = np.zeros(9, np.uint8)
    off = np.concatenate([[0], np.cumsum([len(x) for x in drafts])]).astype(np.int64)
    np.savez_compressed(os.path.join(HERE, "sdust_limits.npz"), names=np.array(names), drafts=np.concatenate(drafts), draft_off=off, expect=expect,
                        kills=kills, mutants=np.array(list(LAB.MUTANTS)), too_short=too_short, unrealised=np.array(unrealised, dtype="U64"))
    print(f"wrote sdust_limits.npz: {len(drafts)} drafts, {int(off[-1])} bases, {int((expect > 0).sum())} with a masked run")
    for j, m in enumerate(LAB.MUTANTS):
        print(f"  {m:8s} kills {int(kills[:, j].sum())}")
    print("  warm-1 told from every single-lane mutant by its value:", told)
    print("  unrealised:", unrealised)


if __name__ == "__main__":
    main()

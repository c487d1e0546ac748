"""The orientation lab: one batch of small ZMWs, each named for the limit of k_orient (DESIGN.md §2 "Pass orientation", §4) it sits on.  batch(opts) builds it
for the options the vote thresholds are measured against (default: orient_ref.DEFAULTS); NAMES[z] names ZMW z.  The prefilter / first-probe collisions are built
from the constants ccsx_kernels.h exports."""
import os
import re

import numpy as np

from ccs_amd import api
import orient_ref as R

K = R.K
U = R.UNKNOWN
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernel_constants():
    """CCSX_ORIENT_* of ccsx_kernels.h as ints"""
    text = open(os.path.join(_ROOT, "ccs_amd", "csrc", "ccsx_kernels.h")).read()
    return {k: int(v, 0) for k, v in re.findall(r"#define\s+CCSX_ORIENT_(\w+)\s+(0x[0-9a-fA-F]+|\d+)", text)}


def fmix32(h):
    h = np.asarray(h, np.uint64) & np.uint64(0xffffffff)
    h ^= h >> np.uint64(16); h = (h * np.uint64(0x85ebca6b)) & np.uint64(0xffffffff)
    h ^= h >> np.uint64(13); h = (h * np.uint64(0xc2b2ae35)) & np.uint64(0xffffffff)
    h ^= h >> np.uint64(16)
    return h


def colliding_codes():
    """two distinct 13-mer codes with the same prefilter bit AND the same first probe in the smallest table (an anchor of exactly 13 bases)"""
    c = kernel_constants()
    assert c["K"] == K and c["FILTER_BITS"] == 1 << (32 - c["FILTER_SHIFT"])
    h = fmix32(np.arange(1 << 23))
    key = ((h >> np.uint64(c["FILTER_SHIFT"])) << np.uint64(16)) | (h & np.uint64(c["MIN_SLOTS"] - 1))
    o = np.argsort(key, kind="stable")
    d = np.flatnonzero(key[o][1:] == key[o][:-1])
    assert len(d), "no colliding pair among the first 2^23 codes"
    return int(o[d[0]]), int(o[d[0] + 1])


def bases_of(code):
    return np.array([(code >> (2 * (K - 1 - i))) & 3 for i in range(K)], np.uint8)


def make_batch(zmws):
    """zmws: per ZMW a list of (bases, flags byte)"""
    read_off, base_off, bases, flags = [0], [0], [], []
    for passes in zmws:
        for b, f in passes:
            bases.append(np.asarray(b, np.uint8)); flags.append(f); base_off.append(base_off[-1] + len(b))
        read_off.append(read_off[-1] + len(passes))
    n = len(zmws)
    cat = np.ascontiguousarray(np.concatenate(bases)) if bases else np.zeros(0, np.uint8)
    pw = ((np.arange(len(cat)) % 3) + 1).astype(np.uint8)
    return api.Batch(np.arange(n, dtype=np.int32), np.full((n, 4), 8.0, np.float32), np.array(read_off, np.int32), np.array(base_off, np.int64), cat, pw,
                     np.zeros(len(cat), np.uint8), np.array(flags, np.uint8), tpl_off=np.zeros(n + 1, np.int64), tpl=np.zeros(0, np.uint8))


def batch(opts=None, seed=5):
    """(batch, names)"""
    op = dict(R.DEFAULTS); op.update(opts or {})
    mv, ra = op["min_votes"], op["ratio"]
    NT = kernel_constants()["THREADS"]
    rng = np.random.default_rng(seed)
    rnd = lambda n: rng.integers(0, 4, int(n)).astype(np.uint8)
    rc = R.revcomp
    Z, names = [], []

    def add(name, passes):
        names.append(name); Z.append(passes)

    a13 = rnd(13)
    add("12 / 13 / 14 bases, anchor of 13", [(a13, U), (a13[:12].copy(), U), (np.concatenate([a13, rnd(1)]), U | 1), (rc(a13), U)])
    a = rnd(NT + 60)
    add("N - K + 1 = threads - 1, threads, threads + 1", [(a, 0)] + [(rc(a)[:NT + K - 1 + d].copy(), U | 2) for d in (-1, 0, 1)] + [(a[:NT + K - 1 + d].copy(), U | 2 | 4 | 1) for d in (-1, 0, 1)])
    add("one pass", [(rnd(200), U | 1)])
    t = rnd(64)
    add("255 passes of 64 bases", [((rc(t) if s else t.copy()), U | int(g)) for s, g in zip(rng.integers(0, 2, 255), rng.integers(0, 2, 255))])
    add("only partial passes", [(rnd(150), U | 2), (rnd(90), U | 2 | 4 | 1)])
    a = rnd(400)
    add("partial passes behind full ones", [(a, 1), (rc(a), U | 1), (a.copy(), U), (rc(a)[:120].copy(), U | 2), (a[250:].copy(), U | 2 | 4 | 1)])
    a = rnd(310)
    add("median tie", [(a[:300].copy(), U), (a, U | 1), (rc(a)[:300].copy(), U), (rc(a), U)])
    add("homopolymer anchor", [(np.zeros(3000, np.uint8), U), (np.full(3000, 3, np.uint8), U), (np.zeros(2990, np.uint8), U | 1), (rnd(2995), U)])
    a = rnd(500)
    at = lambda m, s=0: a[s:s + K + m - 1].copy()                     # m 13-mer positions of the anchor
    add("v_same = min_votes, min_votes - 1", [(a, 1), (at(500), U), (at(mv), U | 2), (at(mv - 1), U | 2), (rc(at(mv, 100)), U | 2 | 1), (rc(at(mv - 1, 100)), U | 2 | 1)])
    x = max(2, (mv + ra - 1) // ra)
    fw = lambda m, s: (at(m, s), int(a[s - 1]), int(a[s + K + m - 1]))                    # a piece of the anchor, the anchor's base before it, the one after it
    bw = lambda m, s: (rc(at(m, s)), 3 - int(a[s + K + m - 1]), 3 - int(a[s - 1]))         # ... reverse-complemented

    def glue(left, right):
        """left + one base + right; the base continues neither piece along the anchor, so no 13-mer across the joint is one of the anchor's"""
        spacer = next(v for v in range(4) if v not in (left[2], right[1]))
        return np.concatenate([left[0], np.array([spacer], np.uint8), right[0]])
    add("v_same = ratio x v_opp, one less", [(a.copy(), 0), (a.copy(), U), (glue(fw(ra * x, 20), bw(x, 200)), U | 2 | 1), (glue(fw(ra * x - 1, 20), bw(x, 200)), U | 2 | 1),
                                             (glue(bw(ra * x, 50), fw(x, 300)), U | 2), (glue(bw(ra * x - 1, 50), fw(x, 300)), U | 2)])
    for name, unit in (("(AT)n", [0, 3]), ("(ACGT)n", [0, 1, 2, 3])):
        u = np.array(unit, np.uint8)
        add(name, [(np.tile(u, 400 // len(u)), U), (np.tile(u, 360 // len(u)), U), (np.tile(u, 360 // len(u)), U | 1), (np.tile(u, 400 // len(u)), U | 1)])
    xx = rnd(150)
    pal = np.concatenate([xx, rc(xx)])
    add("X rc(X)", [(pal, U | 1), (pal.copy(), U), (pal.copy(), U | 1), (pal.copy(), 0)])
    add("junk anchor", [(rnd(300), U), (rnd(300), U | 1), (rnd(290), U), (rnd(310), U | 1)])
    a = rnd(350)
    hi = lambda b: (b | np.uint8(0xA4)).astype(np.uint8)
    add("base bytes with high bits", [(hi(a), U | 1), (hi(rc(a)), U | 1), (hi(a), U), (rc(a), U)])
    add("GIVEN and unknown passes mixed", [(a.copy(), 1), (a.copy(), U), (rc(a), 1), (rc(a), U | 1), (a.copy(), 0), (rc(a), U)])
    c1, c2 = colliding_codes()
    add("prefilter and first-probe collision", [(bases_of(c1), U), (bases_of(c2), U), (rc(bases_of(c2)), U | 1), (bases_of(c1), U | 1), (rc(bases_of(c1)), U)])
    big = rnd(65535)
    noisy = rc(big)
    noisy[::97] = (noisy[::97] + 1) & 3
    add("two passes of 65535 bases", [(big, U), (noisy, U)])
    return make_batch(Z), names


def end_to_end(seed=17, seed_short=39):
    """(batch with its true flags, the same batch through with_unknown_strands(random bits)): 64 ZMWs of 6 x 1500 bases and 4 of 3 x 300.  A pass of 300 bases at
    the generator's error rates keeps about 30 of its 13-mers (tools/orient_study.py), so half of such ZMWs hold a pass below min_votes, which stays UNDETERMINED
    by design: seed_short is one whose 300-base passes all lie above it (tests/test_orient_ref.py checks that on the CPU)"""
    b = api.concat([api.synth(64, 6, 1500, seed=seed), api.synth(4, 3, 300, seed=seed_short)])
    guess = np.random.default_rng(seed).integers(0, 2, len(b.flags))
    return b, b.with_unknown_strands(guess)


def relative_strands_equal(batch, flags_a, flags_b):
    """per ZMW: do the two flag arrays give every pair of passes the same relative orientation (they are equal, or complementary in bit 0, over the ZMW)"""
    x = (np.asarray(flags_a) ^ np.asarray(flags_b)) & 1
    return np.array([len(set(x[int(batch.read_off[z]):int(batch.read_off[z + 1])].tolist())) <= 1 for z in range(batch.n_zmw)])

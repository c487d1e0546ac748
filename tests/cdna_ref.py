"""The cDNA rule restated (DESIGN.md §2 "cDNA rule", rule version 1), and the limit set the library and the kernel are checked on.

cdna_reads() takes the ends from barcode_ref.call_reads (the whole edit-distance table of every primer against either window) and the hits inside the read from
segment_ref.table_hits (the whole table of every search against the whole read, the start from a second, anchored table); neither is stated again here.  What
is this rule's own is plain Python: strand and class from the roles, the poly(A) scan one position after the other (polya_scan), the predicate, class and slice.
polya_brute() is the scan's definition itself, O(K^2): every s_k summed from its first term, every M_k a maximum over all of s_0 .. s_k, then k* and the
arg-max.  Nothing here is bit-parallel, nothing is chunked or done 64 positions at a time, and nothing is shared with cdna_core.h.

limit_cases() lists (name, primers, roles, opts, reads): the smallest shapes at which the kernel can still go wrong (see each block); expected() is cdna_reads()
on a case, computed once per process and shared by the CPU and the GPU tests."""
from __future__ import annotations

import functools

import numpy as np

import barcode_ref
import segment_ref
from segment_ref import cat, codes, edit, rand, rc, random_set   # noqa: F401  (the limit set's helpers; codes / rc for the tests)

READ_PLANES = ("tested", "cls", "strand", "start", "end", "polya_len", "n_internal", "first_internal")
END_PLANES = ("idx", "dist", "second", "clip")
FIELDS = READ_PLANES + END_PLANES
NO_PRIMER, ONE_END, SAME_ROLE, SHORT, CONCATEMER, NO_TAIL, FULL_LENGTH = range(7)
DEFAULTS = dict(window=64, max_dist_pct=15, min_margin=1, polya_mismatch=3, polya_xdrop=3, polya_max=512, min_polya=20, min_len=50)
CHUNK = segment_ref.CHUNK
K25 = segment_ref.K25


def polya_scan(x, mismatch: int, xdrop: int) -> int:
    """polya_len of x[0 .. K) (x[k - 1] = x_k), one position after the other"""
    s = best = arg = 0
    for k, a in enumerate(x, 1):
        s += 1 if a else -mismatch
        if s > best:
            best, arg = s, k
        elif best - s > xdrop:
            break
    return arg


def polya_brute(x, mismatch: int, xdrop: int) -> int:
    """the same by the definition, over every k"""
    K = len(x)
    s = [sum(1 if a else -mismatch for a in x[:k]) for k in range(K + 1)]
    M = [max(s[: k + 1]) for k in range(K + 1)]
    stop = next((k for k in range(1, K + 1) if M[k] - s[k] > xdrop), K + 1)
    top = max(s[:stop])
    return next(k for k in range(stop) if s[k] == top)


def polya_x(c, strand: int, clip0: int, clip1: int, K: int) -> list:
    """x_1 .. x_K of the read c"""
    L = len(c)
    return [int(c[clip0 + k - 1] == 3) if strand else int(c[L - clip1 - k] == 0) for k in range(1, K + 1)]


def cdna_reads(primers, roles, reads, polya=polya_scan, **opts) -> dict:
    o = {**DEFAULTS, **opts}
    n = len(reads)
    ends = barcode_ref.call_reads(primers, reads, window=o["window"], max_dist_pct=o["max_dist_pct"], min_margin=o["min_margin"])
    out = {k: np.zeros(n, np.int32) for k in READ_PLANES}
    out.update({k: ends[k].copy() for k in END_PLANES})
    out["tested"][:] = ends["tested"]
    out["strand"][:] = -1
    out["first_internal"][:] = -1
    for z, c in enumerate(reads):
        c = np.asarray(c, np.uint8) & 3
        L = len(c)
        if L == 0:
            continue
        call, idx, clip = int(ends["call"][z]), ends["idx"][z], ends["clip"][z]
        if call != 3:
            out["cls"][z] = NO_PRIMER if call == 0 else ONE_END
            continue
        if roles[idx[0]] == roles[idx[1]]:
            out["cls"][z] = SAME_ROLE
            continue
        strand = out["strand"][z] = int(roles[idx[0]])
        clip0, clip1 = int(clip[0]), int(clip[1])
        ins_len = L - clip0 - clip1
        if ins_len < 1:
            out["cls"][z] = SHORT
            continue
        tail = polya(polya_x(c, strand, clip0, clip1, min(o["polya_max"], ins_len)), o["polya_mismatch"], o["polya_xdrop"])
        starts = []
        for s in range(2 * len(primers)):
            p = segment_ref.search_pattern(primers, s)
            starts += [s0 for s0, e0, _ in segment_ref.table_hits(p, c, len(p) * o["max_dist_pct"] // 100) if clip0 <= s0 and e0 <= L - clip1]
        out["polya_len"][z], out["n_internal"][z], out["first_internal"][z] = tail, len(starts), min(starts) if starts else -1
        trimmed = ins_len - tail
        cls = SHORT if trimmed < o["min_len"] else CONCATEMER if starts else NO_TAIL if o["min_polya"] > 0 and tail < o["min_polya"] else FULL_LENGTH
        out["cls"][z] = cls
        if cls >= CONCATEMER:
            out["start"][z], out["end"][z] = (clip0 + tail, L - clip1) if strand else (clip0, L - clip1 - tail)
    return out


# ---- the limit set
A, C_, T = 0, 1, 3


def body(rng, n) -> np.ndarray:
    """n random insert bases whose last two are not A, so that the scan stops there under the defaults and a planted tail has the planted length"""
    b = rand(rng, n)
    b[-2:] = C_
    return b


def tail_of(counted) -> np.ndarray:
    """a tail given as it is counted, from the 3' primer towards the insert, as it stands in the sense read"""
    return np.asarray(counted, np.uint8)[::-1]


def mol(p5, p3, insert, tail=30) -> np.ndarray:
    """the sense read 5p . insert . tail . rc(3p); tail: a count of A, or the bases as tail_of gives them"""
    t = np.full(tail, A, np.uint8) if isinstance(tail, int) else tail
    return cat(p5, insert, t, rc(p3))


def both(reads) -> list:
    """every read and its reverse complement"""
    return [r for c in reads for r in (c, rc(c))]


@functools.lru_cache(maxsize=None)
def limit_cases() -> tuple:
    rng = np.random.default_rng(20261021)
    cases = []

    def add(name, primers, roles, reads, **opts):
        assert len(reads) <= 16, name
        cases.append((name, tuple(primers), tuple(roles), {**DEFAULTS, **opts}, tuple(reads)))

    # set sizes 2, 3, 63 | 64 (128 items: waves 0 and 1 full), all of one role but the last primer, and but the first.  Primers at either end of the set at the
    # reads' ends, both strands, an untested read, a read without a primer
    for P in (2, 3, 63, 64):
        S = random_set(rng, P, [25])
        for name, roles in (("last", [0] * (P - 1) + [1]), ("first", [0] + [1] * (P - 1))):
            reads = both([mol(S[0], S[P - 1], body(rng, 120)), mol(S[P - 1], S[0], body(rng, 90), 0)]) + [np.zeros(0, np.uint8), rand(rng, 300)]
            if P > 2:
                reads += both([mol(S[1], S[P - 1], body(rng, 70)), mol(S[0], S[P - 2], body(rng, 70))])
            add(f"n{P}_{name}", S, roles, reads)
    # lengths 8, 25, 63, 64 (top = 1 << 63) and all four in one set.  Reads of 0, m - 1, m and 2 m - 1 bases (the two windows overlap: ins_len < 1), a molecule,
    # 3001 bases
    for name, lens in (("m8", [8]), ("m25", [25]), ("m63", [63]), ("m64", [64]), ("mixed", [8, 25, 63, 64])):
        S = random_set(rng, 4, lens)
        roles = [0, 1, 1, 0]
        reads = [np.zeros(0, np.uint8)]
        for a in range(len(set(lens))):
            m = len(S[a])
            reads += [S[a][: m - 1], S[a].copy(), cat(S[a], rc(S[(a + 1) % 4]))[: 2 * m - 1]]
        reads += [mol(S[0], S[1], body(rng, 80)), rc(mol(S[3], S[2], body(rng, 200), 25)), mol(S[0], S[2], body(rng, 3001 - 30 - len(S[0]) - len(S[2])))]
        add(name, S, roles, reads[:16])
    # overlapping windows with different roles: 5p and rc(3p) share bases, so clip_0 + clip_1 > L and the class is SHORT from step 3
    S = random_set(rng, 2, [25])
    ov = cat(S[0], rc(S[1]))
    add("overlap", S, [0, 1], both([ov, cat(S[0][:20], rc(S[1])), cat(S[0], rand(rng, 1), rc(S[1]))]), min_len=1)
    # windows 8, 64, 1024, and reads of window - 1, window, window + 1 bases: the primers end at the last base of either window, or too far outside it to be called
    for W, m in ((8, 8), (64, 25), (1024, 25)):
        S = random_set(rng, 2, [m])
        reads = []
        for L in (W - 1, W, W + 1):
            reads.append(cat(S[0], rand(rng, L - 2 * m), rc(S[1])) if L >= 2 * m else cat(S[0], rc(S[1]))[:L])
        far, out = W - m, W - m + m * DEFAULTS["max_dist_pct"] // 100 + 1     # (out: k + 1 bases of the primer lie outside the window, more than it may lose)
        reads += [cat(rand(rng, far), S[0], body(rng, 60), np.full(25, A, np.uint8), rc(S[1]), rand(rng, far)),
                  cat(rand(rng, out), S[0], body(rng, 60), np.full(25, A, np.uint8), rc(S[1]), rand(rng, far)),
                  cat(rand(rng, far), S[0], body(rng, 60), np.full(25, A, np.uint8), rc(S[1]), rand(rng, out))]
        add(f"window{W}", S, [0, 1], both(reads), window=W)
    # edits: 0, k and k + 1 edits of each kind (k = K25 = 3) in the head's and in the tail's primer
    S = random_set(rng, 3, [25])
    roles = [0, 1, 0]
    for kind in ("sub", "ins", "del"):
        reads = []
        for k in (0, K25, K25 + 1):
            reads += [mol(edit(rng, S[0], kind, k), S[1], body(rng, 100)), mol(S[0], edit(rng, S[1], kind, k), body(rng, 100))]
        add(f"edits_{kind}", S, roles, both(reads))
    add("edits_p0", S, roles, both(reads), max_dist_pct=0)
    add("edits_p30", S, roles, both(reads), max_dist_pct=30)
    # ties: primers 0 and 1 are the same sequence with opposite roles: the head is uncalled at margin 1 and primer 0 at margin 0 (strand 0); the same with the
    # roles exchanged (strand 1 from the sense layout).  Primer 3 is its own reverse complement: searches 6 and 7 give every hit twice
    X, Y = rand(rng, 25), rand(rng, 25)
    half = rand(rng, 12)
    pal = cat(half, rc(half))
    assert np.array_equal(rc(pal), pal)
    S = [X, X.copy(), Y, pal]
    reads = both([mol(X, Y, body(rng, 100)), mol(pal, Y, body(rng, 100)), mol(X, Y, cat(body(rng, 60), pal, body(rng, 60))), mol(Y, pal, body(rng, 90))])
    for margin in (0, 1, 64):
        add(f"ties_m{margin}", S, [0, 1, 1, 0], reads, min_margin=margin)
        add(f"ties_swapped_m{margin}", S, [1, 0, 0, 1], reads, min_margin=margin)
    # every class on both strands: no primer; one end (head, tail); both ends of one role (5p - 5p, 3p - 3p); SHORT from step 6; concatemer; no tail; full length
    S = random_set(rng, 2, [25])
    p5, p3 = S
    one = mol(p5, p3, body(rng, 150))
    reads = [rand(rng, 400), cat(p5, body(rng, 200)), cat(body(rng, 200), rc(p3)), cat(p5, body(rng, 150), rc(p5)), cat(p3, body(rng, 150), rc(p3)),
             mol(p5, p3, body(rng, 30)), cat(one, mol(p5, p3, body(rng, 140))), mol(p5, p3, body(rng, 150), 5)]
    add("classes", S, [0, 1], both(reads))
    add("classes_full", S, [0, 1], both([one, mol(p5, p3, body(rng, 50)), mol(p5, p3, body(rng, 49))]))   # trimmed = min_len | min_len - 1
    add("classes_min_len", S, [0, 1], both([mol(p5, p3, body(rng, 1), 0), mol(p5, p3, body(rng, 1)), mol(p5, p3, np.zeros(0, np.uint8), 40)]), min_len=1)
    # tails of 0, 1, min_polya - 1, min_polya, 63 | 64 | 65, 127 | 128 | 129 bases (the wave's block edges), each strand a case; under the defaults, with
    # min_polya 0 (no tail is required), polya_mismatch 1 and 8, polya_xdrop 0 and 64
    sense = [mol(p5, p3, body(rng, 100), t) for t in (0, 1, 19, 20, 63, 64, 65, 127, 128, 129)]
    anti = [rc(r) for r in sense]
    variants = (("", {}), ("_nomin", dict(min_polya=0)), ("_mm1", dict(polya_mismatch=1)), ("_mm2", dict(polya_mismatch=2)), ("_mm8", dict(polya_mismatch=8)),
                ("_x0", dict(polya_xdrop=0)), ("_x64", dict(polya_xdrop=64)))
    for suffix, o in variants[:2]:
        add("tails_sense" + suffix, S, [0, 1], sense, **o)
        add("tails_anti" + suffix, S, [0, 1], anti, **o)
    # polya_max - 1 | = | + 1 at both ends of its range's cheap side (16, 512); a tail that runs into the 5' primer (K = ins_len < polya_max)
    for pm in (16, 512):
        add(f"polya_max{pm}", S, [0, 1], both([mol(p5, p3, body(rng, 100), t) for t in (pm - 1, pm, pm + 1)] + [mol(p5, p3, np.zeros(0, np.uint8), 40)]), polya_max=pm)
    # polya_max at the top of its range in reads of 3001 bases: a tail of 2000 bases (32 rounds of the wave, the sum and the maximum carried through all of them), one
    # with a non-A every 700 bases (each a dip of polya_xdrop, recovered in a later block), and under polya_max 2048 a tail of 2500 that the option cuts
    long_tail = [A] * 700 + [C_] + [A] * 700 + [C_] + [A] * 700 + [C_] + [A] * 300
    reads = both([mol(p5, p3, body(rng, 3001 - 50 - 2000), 2000), mol(p5, p3, body(rng, 3001 - 50 - len(long_tail)), tail_of(long_tail)), mol(p5, p3, body(rng, 3001 - 50 - 2500), 2500)])
    add("polya_max4096", S, [0, 1], reads, polya_max=4096)
    add("polya_max2048", S, [0, 1], reads, polya_max=2048)
    # the scan's own edges, the tail given as it is counted from the 3' primer.  One non-A at the last lane of a block (k = 64) and at the first of the next
    # (k = 65), which are dips of exactly polya_xdrop (one non-A at mismatch 3: the scan goes on and recovers), and the same reads at polya_xdrop 2 (the dip is
    # polya_xdrop + 1: it stops); three non-A across the block edge (a dip of polya_xdrop at mismatch 1, a stop under the defaults); A x 10 . C . AA (at mismatch
    # 2, s = 10, 8, 9, 10: the tie goes to the smallest k, 10); a tail of non-A only; two short dips in a row
    a = lambda n: [A] * n                                             # noqa: E731
    c = lambda n: [C_] * n                                            # noqa: E731
    shapes = [a(63) + c(1) + a(40) + c(9), a(64) + c(1) + a(40) + c(9), a(30) + c(1) + a(20) + c(9), a(62) + c(3) + a(20) + c(9), a(63) + c(3) + a(20) + c(9),
              a(10) + c(1) + a(2) + c(9), c(12), a(5) + c(2) + a(3) + c(2) + a(9) + c(9)]
    scan = both([mol(p5, p3, body(rng, 100), tail_of(t)) for t in shapes])
    for suffix, o in variants + (("_x2", dict(polya_xdrop=2)), ("_mm1_x64_max16", dict(polya_mismatch=1, polya_xdrop=64, polya_max=16))):
        add("scan" + suffix, S, [0, 1], scan, **o)
    # internal hits (primer 2, which stands at no end): ending exactly at L - clip_1 and one base past it (its last base is the 3' primer's first), starting at
    # clip_0 and one base before it, inside the poly(A), in both orientations
    Q = rand(rng, 25)
    S3 = [p5, p3, Q]
    Qe, Qs = Q.copy(), Q.copy()
    Qe[-1], Qs[0] = rc(p3)[0], p5[-1]
    reads = [cat(p5, body(rng, 120), Q, rc(p3)), cat(p5, body(rng, 120), Qe[:-1], rc(p3)), cat(p5, Q, body(rng, 120), np.full(30, A, np.uint8), rc(p3)),
             cat(p5, Qs[1:], body(rng, 120), np.full(30, A, np.uint8), rc(p3)), cat(p5, body(rng, 120), np.full(15, A, np.uint8), Q, np.full(15, A, np.uint8), rc(p3)),
             mol(p5, p3, cat(body(rng, 60), rc(Q), body(rng, 60)))]
    # (window 30: a window of 64 would hold the copy next to the end's primer as well, a tie at distance 0 that leaves the end uncalled)
    add("internal_edges", S3, [0, 1, 0], both(reads), window=30)
    add("internal_edges_Qe", [p5, p3, Qe], [0, 1, 1], both(reads[:2]), window=30)
    add("internal_edges_Qs", [p5, p3, Qs], [0, 1, 1], both(reads[2:4]), window=30)
    # ... at, before, after and across a chunk boundary of 256 (k_segment's cases: the run of qualifying ends crosses the boundary, begins just after it, or the
    # hit starts before it and ends well after it), and at the second boundary
    reads = []
    for end in (CHUNK - 1, CHUNK, CHUNK + 1, CHUNK + 4, CHUNK + 12, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1):
        r = mol(p5, p3, cat(body(rng, end - 50), Q, body(rng, 120)))
        assert np.array_equal(r[end - 25:end], Q)
        reads.append(r)
    add("internal_chunks", S3, [0, 1, 0], reads)
    add("internal_chunks_rc", S3, [0, 1, 0], [rc(r) for r in reads])
    # ... with 0, k and k + 1 edits of each kind, and two and three hits in different chunks (first_internal is the smallest start, whichever lane finds it first)
    reads = [mol(p5, p3, cat(body(rng, 100), edit(rng, Q, kind, k), body(rng, 100))) for kind in ("sub", "ins", "del") for k in (0, K25, K25 + 1)]
    reads += [mol(p5, p3, cat(body(rng, 700), Q, body(rng, 40), rc(Q), body(rng, 100))), mol(p5, p3, cat(body(rng, 300), rc(Q), body(rng, 600), Q, body(rng, 20), p5, body(rng, 90))),
              rc(mol(p5, p3, cat(body(rng, 30), p3, body(rng, 900), rc(p3), body(rng, 60))))]
    add("internal_edits", S3, [0, 1, 0], reads)
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def _expected(i: int) -> dict:
    _, primers, roles, opts, reads = limit_cases()[i]
    return cdna_reads(primers, roles, reads, **opts)


def expected(i: int) -> dict:
    return _expected(i)


def reversed_order(want: dict) -> dict:
    """the report of the same reads given in reverse order"""
    return {k: v[::-1] for k, v in want.items()}


def diff(got, want) -> list:
    """the fields and reads at which a report (an object with FIELDS as attributes, or a dict) differs from `want`"""
    bad = []
    for k in FIELDS:
        g = np.asarray(got[k] if isinstance(got, dict) else getattr(got, k))
        w = np.asarray(want[k])
        if g.shape != w.shape:
            bad.append((k, "shape", g.shape, w.shape))
            continue
        ne = (g != w).reshape(len(w), -1).any(axis=1) if len(w) else np.zeros(0, bool)
        for z in np.flatnonzero(ne)[:4]:
            bad.append((k, int(z), g[z].tolist(), w[z].tolist()))
    return bad

"""The segment rule restated (DESIGN.md §2 "Segment rule", rule version 1), and the limit set the library and the kernel are checked on.

segment_reads() fills the whole edit-distance table of every search against the whole read: row 0 is 0 (a match may start anywhere), column 0 is the row index,
unit costs; E[j] is the last row.  The hits are the maximal runs of E <= k; a hit's start comes from a second table, the reversed pattern against the read read
backwards from the hit's end, whose row 0 charges the start.  The selection is a sort of tuples and a test against every hit taken before.  brute_hits() is the
definition itself, without a table shared between substrings: the plain Levenshtein distance of the pattern to every substring.  Nothing here is bit-parallel,
nothing is chunked, and nothing is shared with segment_core.h.

limit_cases() lists (name, adapters, opts, reads): the smallest shapes at which the kernel can still go wrong (see each block); expected() is segment_reads() on
a case, computed once per process and shared by the CPU and the GPU tests."""
from __future__ import annotations

import functools

import numpy as np

PLANES = ("tested", "overflow", "n_hits", "n_cuts", "n_segments", "complete", "orient", "leftover_bases")
FIELDS = PLANES + ("pieces",)
PIECE_DTYPE = np.dtype([("start", np.int32), ("end", np.int32), ("index", np.uint8), ("reverse", np.uint8), ("dist_left", np.uint8), ("dist_right", np.uint8)])
DEFAULTS = dict(max_dist_pct=15, min_len=50)
MAX_HITS = MAX_PIECES = 64
CHUNK = 256            # CCSX_SEGMENT_CHUNK: an item of k_segment is (search, 256 read bases); test_segment_ref.py checks it against ccsx_segment_chunk()
LONGEST = 81982        # the engine's longest result slot, that of a 65535-base subread (ccsx_result_layout: m + m // 4 + 64)
K25 = 25 * DEFAULTS["max_dist_pct"] // 100     # the edits at which a 25-mer still hits under the defaults: 3


def codes(s: str) -> np.ndarray:
    return np.array(["ACGT".index(c) for c in s.upper()], np.uint8)


def rc(c) -> np.ndarray:
    return (3 - np.asarray(c, np.uint8)[::-1]).astype(np.uint8)


def last_row(p, s, anchored: bool) -> np.ndarray:
    """E[j], 0 <= j <= len(s): the last row of pattern p's table against s, every row filled.  anchored: row 0 is j, not 0"""
    n = len(s)
    ar = np.arange(n + 1, dtype=np.int32)
    prev = ar.copy() if anchored else np.zeros(n + 1, np.int32)
    s = np.asarray(s, np.int32)
    for i in range(1, len(p) + 1):
        t = np.empty(n + 1, np.int32)
        t[0] = i
        if n:
            t[1:] = np.minimum(prev[:-1] + (s != int(p[i - 1])), prev[1:] + 1)
        prev = np.minimum.accumulate(t - ar) + ar                   # ... and the cell to the left + 1
    return prev


def search_pattern(adapters, s: int) -> np.ndarray:
    a = np.asarray(adapters[s >> 1], np.uint8)
    return rc(a) if s & 1 else a


def table_hits(p, c, k: int) -> list:
    """(start, end, dist) of every hit of pattern p in c"""
    E = last_row(p, c, False)
    ok = E <= k
    hits = []
    j = 1
    while j <= len(c):
        if not ok[j]:
            j += 1
            continue
        j1 = j
        while j1 + 1 <= len(c) and ok[j1 + 1]:
            j1 += 1
        run = E[j:j1 + 1]
        dist = int(run.min())
        end = j + int(np.argmin(run))                               # (the first minimum)
        back = c[max(0, end - (len(p) + dist)):end][::-1]
        D = last_row(p[::-1], back, True)
        x = int(np.flatnonzero(D == dist)[0])                       # (the shortest)
        hits.append((end - x, end, dist))
        j = j1 + 1
    return hits


def levenshtein(a, b) -> int:
    row = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        new = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            new[j] = min(row[j - 1] + (a[i - 1] != b[j - 1]), row[j] + 1, new[j - 1] + 1)
        row = new
    return row[len(b)]


def brute_hits(p, c, k: int) -> list:
    """the same by the definition: an end j qualifies iff some substring c[i:j] is within k of p, over every substring"""
    p, c = [int(x) for x in p], [int(x) for x in c]
    L = len(c)
    D = [[levenshtein(p, c[i:j]) for i in range(j + 1)] for j in range(L + 1)]      # D[j][i]
    E = [min(row) for row in D]
    hits, j = [], 1
    while j <= L:
        if E[j] > k:
            j += 1
            continue
        j1 = j
        while j1 + 1 <= L and E[j1 + 1] <= k:
            j1 += 1
        dist = min(E[j:j1 + 1])
        end = next(q for q in range(j, j1 + 1) if E[q] == dist)
        start = max(i for i in range(end + 1) if D[end][i] == dist)
        hits.append((start, end, dist))
        j = j1 + 1
    return hits


def finish(n, per_read, n_adapters: int, min_len: int) -> dict:
    """the report from per_read[z] = None (untested) or (L, [(dist, start, search, end) of every hit])"""
    out = {k: np.zeros(n, np.int32) for k in PLANES}
    out["pieces"] = np.zeros((n, MAX_PIECES), PIECE_DTYPE)
    for z in range(n):
        out["orient"][z] = -1
        if per_read[z] is None:
            continue
        L, hits = per_read[z]
        out["tested"][z] = 1
        out["n_hits"][z] = len(hits)
        if len(hits) > MAX_HITS:
            out["overflow"][z] = 1
            continue
        cuts = []
        for d, s0, q, e0 in sorted(hits):
            if not any(s0 < e1 and s1 < e0 for _, s1, _, e1 in cuts):
                cuts.append((d, s0, q, e0))
        cuts.sort(key=lambda h: h[1])
        out["n_cuts"][z] = len(cuts)
        segs, leftover = [], 0
        bounds = [(None, 0)] + [(h, h[3]) for h in cuts]
        for i, (left, frm) in enumerate(bounds):
            right = cuts[i] if i < len(cuts) else None
            to = right[1] if right is not None else L
            kind = None
            if left is not None and right is not None and to - frm >= min_len:
                ls, rs = left[2], right[2]
                if ls % 2 == 0 and rs == ls + 2:
                    kind = (ls // 2, 0)
                elif ls % 2 == 1 and rs == ls - 2:
                    kind = (rs // 2, 1)
            if kind is not None:
                segs.append((frm, to, kind[0], kind[1], left[0], right[0]))
            elif to > frm:
                leftover += to - frm
        out["n_segments"][z] = len(segs)
        out["leftover_bases"][z] = leftover
        for i, sg in enumerate(segs):
            out["pieces"][z, i] = sg
        if segs:
            revs = {sg[3] for sg in segs}
            out["orient"][z] = 2 if len(revs) == 2 else revs.pop()
            idx = [sg[2] for sg in segs]
            want = list(range(n_adapters - 1))
            out["complete"][z] = int(out["orient"][z] in (0, 1) and idx == (want if out["orient"][z] == 0 else want[::-1]))
    return out


def _segment(adapters, reads, max_dist_pct, min_len, hits_of) -> dict:
    per_read = []
    for c in reads:
        c = np.asarray(c, np.uint8) & 3
        if len(c) == 0:
            per_read.append(None)
            continue
        hits = []
        for s in range(2 * len(adapters)):
            p = search_pattern(adapters, s)
            hits += [(d, s0, s, e0) for s0, e0, d in hits_of(p, c, len(p) * max_dist_pct // 100)]
        per_read.append((len(c), hits))
    return finish(len(reads), per_read, len(adapters), min_len)


def segment_reads(adapters, reads, max_dist_pct=DEFAULTS["max_dist_pct"], min_len=DEFAULTS["min_len"]) -> dict:
    return _segment(adapters, reads, max_dist_pct, min_len, table_hits)


def segment_reads_brute(adapters, reads, max_dist_pct=DEFAULTS["max_dist_pct"], min_len=DEFAULTS["min_len"]) -> dict:
    return _segment(adapters, reads, max_dist_pct, min_len, brute_hits)


# ---- the limit set
def random_set(rng, n, lens) -> list:
    """n random adapters, lengths cycling through `lens`"""
    return [rng.integers(0, 4, lens[a % len(lens)]).astype(np.uint8) for a in range(n)]


def rand(rng, L) -> np.ndarray:
    return rng.integers(0, 4, L).astype(np.uint8)


def cat(*parts) -> np.ndarray:
    return np.concatenate([np.asarray(p, np.uint8) for p in parts] + [np.zeros(0, np.uint8)])


def edit(rng, p, kind: str, k: int) -> np.ndarray:
    """p with k edits of one kind at distinct interior positions, no two next to each other (sub: another base; ins: a base; del)"""
    p = [int(x) for x in p]
    pos = []
    while len(pos) < k:
        q = int(rng.integers(2, len(p) - 2))
        if all(abs(q - r) > 1 for r in pos):
            pos.append(q)
    for q in sorted(pos, reverse=True):
        if kind == "sub":
            p[q] = (p[q] + 1 + int(rng.integers(0, 3))) % 4
        elif kind == "ins":
            p.insert(q, int(rng.integers(0, 4)))
        else:
            del p[q]
    return np.array(p, np.uint8)


def array(rng, S, seg_lens, first=0, head=0, tail=0, adapters=None) -> np.ndarray:
    """head random bases, then S[first] seg S[first + 1] seg ... with random segments of seg_lens, then tail random bases.  adapters: what is written in place of
    S[first + i] (edited copies)"""
    parts = [rand(rng, head)]
    for i in range(len(seg_lens) + 1):
        parts.append(adapters[i] if adapters is not None else S[first + i])
        if i < len(seg_lens):
            parts.append(rand(rng, seg_lens[i]))
    return cat(*parts, rand(rng, tail))


@functools.lru_cache(maxsize=None)
def limit_cases() -> tuple:
    rng = np.random.default_rng(20261020)
    cases = []

    def add(name, adapters, reads, **opts):
        cases.append((name, tuple(adapters), {**DEFAULTS, **opts}, tuple(reads)))

    # set sizes 2, 3, 32 | 33: 64 searches are one wave of one chunk, 66 are one wave and two lanes.  The whole array forwards and reverse complemented, its
    # last two segments alone (the last searches of the set), an untested read
    for na in (2, 3, 32, 33):
        S = random_set(rng, na, [25])
        full = array(rng, S, [60] * (na - 1), head=7, tail=5)
        reads = [full, rc(full), array(rng, S, [55] * min(2, na - 1), first=na - 1 - min(2, na - 1)), np.zeros(0, np.uint8), rand(rng, 300)]
        add(f"n{na}", S, reads)
    # lengths 8, 25, 63, 64 (top = 1 << 63) and all four in one set.  Reads of 0, m - 1, m, m + 1 bases that are (part of) an adapter; exactly A0 S A1, so one
    # adapter starts at 0 and one ends at L; 3001 bases
    for name, lens in (("m8", [8]), ("m25", [25]), ("m63", [63]), ("m64", [64]), ("mixed", [8, 25, 63, 64])):
        S = random_set(rng, 4, lens)
        reads = [np.zeros(0, np.uint8)]
        for a in range(len(set(lens))):
            m = len(S[a])
            reads += [S[a][: m - 1], S[a].copy(), cat(S[a], rand(rng, 1)), rc(S[a])]
        reads += [array(rng, S, [70]), array(rng, S, [50, 80], first=1), rc(array(rng, S, [64, 51, 90])), cat(array(rng, S, [900, 1000, 700]), rand(rng, 400))[:3001]]
        add(name, S, reads)
    # chunk edges (25-mers; k = 3, so a perfect copy's run of qualifying ends is end - 3 .. end + 3): a hit that ends at CH - 1, CH, CH + 1 (all three runs cross
    # the boundary; the run of the last begins in chunk 0 and has its minimum in chunk 1: the owner follows it past its chunk), one that ends at CH + 4 (the run
    # begins at CH + 1: chunk 1 owns it, from its warm-up), one that starts before the boundary and ends well after it, and the same at the second boundary.
    # A0 starts at 0: chunk 0 has no warm-up to start from
    S = random_set(rng, 3, [25])
    reads = []
    for end in (CHUNK - 1, CHUNK, CHUNK + 1, CHUNK + 4, CHUNK + 12, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1, 2 * CHUNK + 12):
        r = array(rng, S, [end - 50, 120])
        assert np.array_equal(r[end - 25:end], S[1])
        reads += [r, rc(r)]
    reads.append(cat(S[0], rand(rng, CHUNK - 25), S[1], rand(rng, CHUNK - 25), S[2]))          # adapters begin exactly at the chunk boundaries
    add("chunks", S, reads)
    # the engine's longest slot: hits in its first and in its last chunk only
    r = rand(rng, LONGEST)
    head, tail = array(rng, S, [80]), array(rng, S, [90], first=1)
    r[3: 3 + len(head)] = head
    r[LONGEST - len(tail):] = tail
    add("longest", S, [r])
    # edits: 0, k and k + 1 edits of each kind in the middle adapter (k = K25 = 3); with k + 1 the two pieces beside it become one leftover.  At 0 % and 30 % too
    reads = []
    for kind in ("sub", "ins", "del"):
        for k in (0, K25, K25 + 1):
            reads.append(array(rng, S, [120, 130], adapters=[S[0], edit(rng, S[1], kind, k), S[2]]))
    for pct in (0, DEFAULTS["max_dist_pct"], 30):
        add(f"edits_p{pct}", S, reads, max_dist_pct=pct)
    # piece lengths: two adapters back to back (a piece of length 0), a piece of min_len - 1 and one of min_len; min_len at both ends of its range
    S = random_set(rng, 4, [25])
    reads = [cat(S[0], S[1], rand(rng, 80), S[2]), array(rng, S, [49, 50, 51]), array(rng, S, [50, 49, 50]), cat(S[0], S[1], S[2], S[3]), array(rng, S, [1, 2, 3])]
    add("pieces", S, reads)
    add("pieces_min1", S, reads, min_len=1)
    add("pieces_min65535", S, reads, min_len=65535)
    # order: A0 S A2; A1 S A1; the array reverse complemented; a forward array followed by a reverse one (orient 2); an array twice (complete 0)
    full = array(rng, S, [70, 80, 90])
    reads = [cat(S[0], rand(rng, 70), S[2]), cat(S[1], rand(rng, 70), S[1]), rc(full), cat(full, rand(rng, 9), rc(array(rng, S, [60, 61, 62]))), cat(full, full),
             cat(rc(full), rc(full)), cat(full, rc(full))]
    add("order", S, reads)
    # selection ties.  0: adapters 1 and 2 share their first 22 bases, the read holds adapter 1: both hit the same place, at dist 0 and 2.  1: adapters 3 and 4
    # are u v and v w, the read holds u v w: two hits at dist 0 that overlap, the smaller start wins.  2: adapters 5 and 6 are the same sequence: the smaller
    # search wins.  3: adapter 7 is its own reverse complement: searches 14 and 15 give the same hits.  4: three hits of which the middle one is best and
    # overlaps both others
    S = random_set(rng, 11, [25])
    S[2] = S[1].copy()
    S[2][22] = (S[2][22] + 1) % 4
    S[2][24] = (S[2][24] + 2) % 4
    u, v, w = rand(rng, 10), rand(rng, 15), rand(rng, 10)
    S[3], S[4] = cat(u, v), cat(v, w)
    S[6] = S[5].copy()
    half = rand(rng, 12)
    S[7] = cat(half, rc(half))
    assert np.array_equal(rc(S[7]), S[7])
    p1, x, q, y, r1 = rand(rng, 19), rand(rng, 6), rand(rng, 13), rand(rng, 6), rand(rng, 19)
    S[8], S[9], S[10] = cat(p1, x), cat(x, q, y), cat(y, r1)
    p1e, r1e = p1.copy(), r1.copy()
    p1e[9] = (p1e[9] + 1) % 4
    r1e[9] = (r1e[9] + 1) % 4
    reads = [cat(S[0], rand(rng, 60), S[1], rand(rng, 60), rand(rng, 5)), cat(rand(rng, 40), u, v, w, rand(rng, 40)), cat(S[4], rand(rng, 70), S[5], rand(rng, 70), S[6]),
             cat(S[6], rand(rng, 66), S[7], rand(rng, 77), S[8]), cat(rand(rng, 30), p1e, x, q, y, r1e, rand(rng, 30))]
    add("ties", S, reads)
    # hit counts: exactly 64 hits, 65 hits (overflow), a read made only of copies of one adapter (overflow) and one that is the three adapters and nothing else
    S = random_set(rng, 3, [25])
    gap = codes("ACCA")
    reads = [cat(*([S[0], gap] * 64)), cat(*([S[0], gap] * 65)), cat(*([S[1]] * 100)), cat(S[0], S[1], S[2]), cat(*([S[0], gap] * 63))]
    add("counts", S, reads)
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def _expected(i: int) -> dict:
    _, adapters, opts, reads = limit_cases()[i]
    return segment_reads(adapters, reads, **opts)


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
            bad.append((k, int(z), g[z].tolist()[:6] if k == "pieces" else g[z].tolist(), w[z].tolist()[:6] if k == "pieces" else w[z].tolist()))
    return bad

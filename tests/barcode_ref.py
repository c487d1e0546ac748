"""The barcode rule restated (DESIGN.md §2 "Barcode calls", rule version 1), and the limit set the library and the kernel are checked on.

call_reads() fills the whole edit-distance table of every (barcode, end): row 0 is 0 (a match may start anywhere in the window), column 0 is the row index, unit
costs; E[j] is the last row of the barcode.  brute_end() is the definition itself, without a table shared between substrings: the plain Levenshtein distance of
the barcode to every substring of the window.  Nothing here is bit-parallel, and nothing is shared with barcode_core.h.

limit_cases() lists (name, barcodes, opts, reads): the smallest shapes at which the kernel can still go wrong (see each block); expected() is call_reads() on a
case, computed once per process and shared by the CPU and the GPU tests."""
from __future__ import annotations

import functools

import numpy as np

FIELDS = ("tested", "call", "bq", "idx", "dist", "second", "clip")
DEFAULTS = dict(window=64, max_dist_pct=15, min_margin=1)
K16 = 16 * DEFAULTS["max_dist_pct"] // 100     # the edits at which a 16-mer is still called under the defaults
THREADS = 256          # k_barcode's workgroup: an item is (end, barcode), so 128 barcodes fill one pass over the workgroup and 129 need a second one


def codes(s: str) -> np.ndarray:
    return np.array(["ACGT".index(c) for c in s.upper()], np.uint8)


def rc(c: np.ndarray) -> np.ndarray:
    return (3 - np.asarray(c, np.uint8)[::-1]).astype(np.uint8)


def end_tables(barcodes, s: np.ndarray) -> np.ndarray:
    """E[b, j], 0 <= j <= len(s): the last row of barcode b's table against s, every row of every table filled"""
    nb, W = len(barcodes), len(s)
    lens = np.array([len(p) for p in barcodes])
    P = np.full((nb, int(lens.max())), 255, np.int32)
    for b, p in enumerate(barcodes):
        P[b, : len(p)] = p
    ar = np.arange(W + 1, dtype=np.int32)
    prev = np.zeros((nb, W + 1), np.int32)
    E = np.zeros((nb, W + 1), np.int32)
    for i in range(1, int(lens.max()) + 1):
        t = np.empty((nb, W + 1), np.int32)
        t[:, 0] = i
        if W:
            cost = (P[:, i - 1][:, None] != s[None, :].astype(np.int32)).astype(np.int32)
            t[:, 1:] = np.minimum(prev[:, :-1] + cost, prev[:, 1:] + 1)
        cur = np.minimum.accumulate(t - ar, axis=1) + ar            # ... and the cell to the left + 1
        E[lens == i] = cur[lens == i]
        prev = cur
    return E


def levenshtein(a, b) -> int:
    row = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        new = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            new[j] = min(row[j - 1] + (a[i - 1] != b[j - 1]), row[j] + 1, new[j - 1] + 1)
        row = new
    return row[len(b)]


def brute_end(p, s) -> tuple:
    """(dist, clip) of barcode p in the window s by the definition: every substring s[i:j]"""
    best = (len(p), 0)
    for j in range(len(s) + 1):
        e = min(levenshtein(list(p), list(s[i:j])) for i in range(j + 1))
        if e < best[0]:
            best = (e, j)
    return best


def finish(n, per_end, lens, max_dist_pct, min_margin) -> dict:
    """the report from per_end[z] = None (untested) or [(dist_b array, clip_b array) per end]"""
    out = {k: np.zeros(n, np.int32) for k in ("tested", "call", "bq")}
    out.update({k: np.zeros((n, 2), np.int32) for k in ("idx", "dist", "second", "clip")})
    for z in range(n):
        if per_end[z] is None:
            out["bq"][z] = -1
            out["idx"][z] = -1
            out["dist"][z] = 255
            out["second"][z] = 255
            continue
        out["tested"][z] = 1
        quals = []
        for e, (d, c) in enumerate(per_end[z]):
            b = int(np.argmin(d))                                   # (the first minimum: ties to the smallest index)
            others = np.delete(d, b)
            second = int(others.min()) if len(others) else 255
            m = int(lens[b])
            out["idx"][z, e], out["dist"][z, e], out["second"][z, e], out["clip"][z, e] = b, d[b], second, c[b]
            if d[b] <= m * max_dist_pct // 100 and second - d[b] >= min_margin:
                out["call"][z] |= 1 << e
                quals.append(100 * (m - int(d[b])) // m)
        out["bq"][z] = min(quals) if quals else -1
    return out


def call_reads(barcodes, reads, window=DEFAULTS["window"], max_dist_pct=DEFAULTS["max_dist_pct"], min_margin=DEFAULTS["min_margin"]) -> dict:
    lens = [len(p) for p in barcodes]
    per_end = []
    for c in reads:
        c = np.asarray(c, np.uint8)
        if len(c) == 0:
            per_end.append(None)
            continue
        ends = []
        for s in (c, rc(c)):
            E = end_tables(barcodes, s[: min(len(c), window)])
            ends.append((E.min(axis=1), E.argmin(axis=1)))          # (argmin: the smallest j)
        per_end.append(ends)
    return finish(len(reads), per_end, lens, max_dist_pct, min_margin)


def call_reads_brute(barcodes, reads, window=DEFAULTS["window"], max_dist_pct=DEFAULTS["max_dist_pct"], min_margin=DEFAULTS["min_margin"]) -> dict:
    per_end = []
    for c in reads:
        c = np.asarray(c, np.uint8)
        if len(c) == 0:
            per_end.append(None)
            continue
        ends = []
        for s in (c, rc(c)):
            hits = [brute_end(p, s[: min(len(c), window)]) for p in barcodes]
            ends.append((np.array([h[0] for h in hits]), np.array([h[1] for h in hits])))
        per_end.append(ends)
    return finish(len(reads), per_end, [len(p) for p in barcodes], max_dist_pct, min_margin)


# ---- the limit set
def random_set(rng, n, lens) -> list:
    """n random barcodes, lengths cycling through `lens`"""
    return [rng.integers(0, 4, lens[b % len(lens)]).astype(np.uint8) for b in range(n)]


def edit(rng, p, kind: str, k: int) -> np.ndarray:
    """p with k edits of one kind at distinct interior positions (sub: another base; ins: a base that differs from both neighbours where it can; del)"""
    p = list(int(x) for x in p)
    for pos in sorted(rng.choice(np.arange(1, len(p) - 1), k, replace=False), reverse=True):
        if kind == "sub":
            p[pos] = (p[pos] + 1 + int(rng.integers(0, 3))) % 4
        elif kind == "ins":
            p.insert(pos, int(rng.integers(0, 4)))
        else:
            del p[pos]
    return np.array(p, np.uint8)


def molecule(rng, L, head=None, tail=None, head_at=0, tail_at=0) -> np.ndarray:
    """a random read of L bases with `head` written at head_at and rc(tail) written so that it ends tail_at bases before the read's end; what does not fit
    inside the read is cut off"""
    c = rng.integers(0, 4, L).astype(np.uint8)
    if tail is not None:
        t = rc(tail)
        hi = L - tail_at
        lo = max(0, hi - len(t))
        if hi > lo:
            c[lo:hi] = t[len(t) - (hi - lo):]
    if head is not None:
        n = max(0, min(len(head), L - head_at))
        c[head_at: head_at + n] = head[:n]
    return c


@functools.lru_cache(maxsize=None)
def limit_cases() -> tuple:
    rng = np.random.default_rng(20261020)
    cases = []

    def add(name, barcodes, reads, **opts):
        cases.append((name, tuple(barcodes), {**DEFAULTS, **opts}, tuple(reads)))

    # set sizes: 1 (second = 255), 2, 64 | 65 (one wave of one end | one more), 128 | 129 (2 x 128 = 256 items fill k_barcode's 256 threads in one pass | two
    # more items start a second pass), 384 (three full passes).  The planted barcodes are the first and the last of the set, the places an item count is off by one
    for nb in (1, 2, 64, 65, 128, 129, 384):
        S = random_set(rng, nb, [16])
        reads = [molecule(rng, 200, S[0], S[nb - 1]), molecule(rng, 200, S[nb - 1], S[0]), molecule(rng, 200, S[nb // 2], None), molecule(rng, 200, None, S[nb // 2]), molecule(rng, 200),
                 np.zeros(0, np.uint8), molecule(rng, 40, S[nb - 1], S[nb - 1])]
        add(f"n{nb}", S, reads)
    # lengths 8, 16, 63, 64 (top = 1 << 63) and all four in one set, at windows 8, 64 and 1024; L of 0, m - 1, m, window - 1, window, window + 1, below 2 x window
    # (the two windows overlap) and 3000
    for name, lens in (("m8", [8]), ("m16", [16]), ("m63", [63]), ("m64", [64]), ("mixed", [8, 16, 63, 64])):
        S = random_set(rng, 6, lens)
        for window in (8, 64, 1024):
            reads = []
            for L in sorted({0, min(lens) - 1, min(lens), max(lens) - 1, max(lens), window - 1, window, window + 1, 2 * window - 5, 3000}):
                a, b = S[int(rng.integers(0, 6))], S[int(rng.integers(0, 6))]
                reads += [molecule(rng, L, a, b), molecule(rng, L, a, None, head_at=min(2, L))] if L else [np.zeros(0, np.uint8)]
            add(f"{name}_w{window}", S, reads, window=window)
    S = random_set(rng, 384, [8, 16, 63, 64])
    add("mixed_n384_w256", S, [molecule(rng, 3000, S[383], S[62]), molecule(rng, 300, S[2], S[381])], window=256)
    # placement (16-mers, window 64): flush, shifted 1 .. 5 in, straddling the window's edge (part of it outside), twice in the window (clip is the first)
    S = random_set(rng, 8, [16])
    reads = [molecule(rng, 500, S[1], S[2])]
    reads += [molecule(rng, 500, S[3], S[4], head_at=k, tail_at=k) for k in range(1, 6)]
    reads += [molecule(rng, 500, S[5], S[6], head_at=64 - k, tail_at=64 - k) for k in (15, 12, 8, 4, 1)]
    twice = molecule(rng, 500, S[7], S[0], head_at=3, tail_at=2)
    twice[30:46] = S[7]
    twice[500 - 45: 500 - 29] = rc(S[0])
    add("placement", S, reads + [twice])
    # content: 1, k and k + 1 edits of each kind (k = K16 = 2: floor(16 x 15 / 100)); two identical barcodes (the lower index wins, margin 0); a barcode that is its
    # own reverse complement; the same barcode at both ends; a read made of one base
    S = random_set(rng, 8, [16])
    S[5] = S[2].copy()
    S[6] = codes("ACGTACGTACGTACGT")
    assert np.array_equal(rc(S[6]), S[6])
    reads = []
    for kind in ("sub", "ins", "del"):
        for k in (1, K16, K16 + 1):
            reads.append(molecule(rng, 400, edit(rng, S[0], kind, k), edit(rng, S[1], kind, k)))
    reads += [molecule(rng, 400, S[2], S[5]), molecule(rng, 400, S[5], S[3]), molecule(rng, 400, S[6], S[6]), molecule(rng, 400, S[3], S[3]),
              molecule(rng, 400, S[4], S[7]), np.zeros(300, np.uint8), np.full(20, 3, np.uint8)]
    for pct in (0, DEFAULTS["max_dist_pct"], 30):
        for margin in (0, 1, 5):
            add(f"content_p{pct}_g{margin}", S, reads, max_dist_pct=pct, min_margin=margin)
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def _expected(i: int) -> dict:
    _, barcodes, opts, reads = limit_cases()[i]
    return call_reads(barcodes, reads, **opts)


def expected(i: int) -> dict:
    return _expected(i)


def diff(got, want, n=None) -> list:
    """the fields and reads at which a report (an object with FIELDS as attributes, or a dict) differs from `want`"""
    bad = []
    for k in FIELDS:
        g = np.asarray(got[k] if isinstance(got, dict) else getattr(got, k))
        w = np.asarray(want[k])
        if g.shape != w.shape:
            bad.append((k, "shape", g.shape, w.shape))
            continue
        for z in np.flatnonzero((g != w).reshape(len(w), -1).any(axis=1))[:4]:
            bad.append((k, int(z), g[z].tolist(), w[z].tolist()))
    return bad

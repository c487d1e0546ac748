"""Adapter palindromes (DESIGN.md §2 "Adapter palindromes", rule version 1): the rule restated in numpy, and a brute-force all-pairs reading of it.
tests/test_fold.py checks the restatement against the brute force on the CPU and holds k_fold to the restatement, field for field, on an MI355X."""
import numpy as np

K = 15
NS_MAX = 8192
UNTESTED, NONE, PALINDROME = 0, 1, 2
DEFAULTS = dict(max_occ=8, min_hits=12, min_arm=200, min_span_tenths=8, end_slack=100)


def fmix32(h):
    """murmur3's finaliser on uint32, with wrap-around"""
    h = np.array(h, np.uint32, ndmin=1)
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(16)
    return h


def codes(d):
    """(F, R) of every k-mer position 0 .. L - k: the forward code and the code of the reverse complement"""
    d = np.asarray(d, np.int64) & 3
    n = len(d) - K + 1
    if n <= 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    w = np.lib.stride_tricks.sliding_window_view(d, K)
    pw = 4 ** np.arange(K - 1, -1, -1, dtype=np.int64)
    return w @ pw, (3 - w[:, ::-1]) @ pw


def sampled_positions(d):
    """the sampled positions that enter (the first NS_MAX), in increasing position, with their (F, R)"""
    F, R = codes(d)
    s = np.flatnonzero((fmix32(np.minimum(F, R)) & np.uint32(7)) == 0)[:NS_MAX]
    return s, F[s], R[s]


def kept_positions(d, max_occ):
    """(positions, F, R) of the sampled positions that enter and survive the occurrence cap, in increasing position"""
    s, F, R = sampled_positions(d)
    if len(s) == 0:
        return s, F, R
    _, inv, cnt = np.unique(np.minimum(F, R), return_inverse=True, return_counts=True)
    k = cnt[inv.reshape(-1)] <= max_occ
    return s[k], F[k], R[k]


def hits(d, max_occ):
    """(i, j) of every hit: kept i < j, j >= i + k, F_i == R_j.  Such a pair has one canonical code and opposite orientations, and a kept code has at most
    max_occ positions, so the pairs are found within groups"""
    s, F, R = kept_positions(d, max_occ)
    if len(s) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    C = np.minimum(F, R)
    o = np.lexsort((s, C))
    s, F, R, C = s[o], F[o], R[o], C[o]
    I, J = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for g in range(1, max_occ):
        a = np.arange(len(s) - g)
        m = (C[a] == C[a + g]) & (F[a] == R[a + g]) & (s[a + g] >= s[a] + K)
        I.append(s[a][m]); J.append(s[a + g][m])
    return np.concatenate(I).astype(np.int64), np.concatenate(J).astype(np.int64)


def _verdict(L, h, fold, span, min_i, max_j, o):
    shorter = min(fold, L - fold)
    reach = min_i <= o["end_slack"] if fold <= L - fold else max_j + K >= L - o["end_slack"]
    pal = h >= o["min_hits"] and span >= o["min_arm"] and 10 * span >= o["min_span_tenths"] * shorter and reach
    return (PALINDROME if pal else NONE), fold, h, span


def vote(L, i, j, o):
    """(verdict, fold, hits, span) of a tested draft of length L from its hits"""
    if len(i) == 0:
        return NONE, -1, 0, 0
    D = i + j + K - 1
    b = D >> 6
    nb = ((2 * L - K - 1) >> 6) + 1
    hist = np.bincount(b, minlength=nb + 1)
    H = hist[:nb] + hist[1:nb + 1]
    bs = int(np.argmax(H))                                       # (the first maximum: ties go to the smallest b)
    sel = (b == bs) | (b == bs + 1)
    Ds, Is, Js = D[sel], i[sel], j[sel]
    fold = int(Ds.min() + Ds.max()) // 4
    span = int(min(Is.max() - Is.min(), Js.max() - Js.min())) + K
    return _verdict(L, int(H[bs]), fold, span, int(Is.min()), int(Js.max()), o)


def _opts(o):
    r = dict(DEFAULTS)
    r.update(o or {})
    return r


def fold(d, tested=True, opts=None):
    """the report of one ZMW: (verdict, fold, hits, span); tested = its status after the cascade is SUCCESS"""
    if not tested:
        return UNTESTED, -1, 0, 0
    o = _opts(opts)
    i, j = hits(d, o["max_occ"])
    return vote(len(d), i, j, o)


def fold_bruteforce(d, opts=None):
    """the rule read literally: every pair of positions, every pair of bins, explicit loops for the occurrence cap and the vote"""
    o = _opts(opts)
    L = len(d)
    F, R = codes(d)
    n = len(F)
    if n == 0:
        return NONE, -1, 0, 0
    C = np.minimum(F, R)
    sampled = (fmix32(C) & np.uint32(7)) == 0
    enter = sampled & (np.cumsum(sampled) - 1 < NS_MAX)
    kept = enter.copy()
    for p in np.flatnonzero(enter):
        if int((enter & (C == C[p])).sum()) > o["max_occ"]:
            kept[p] = False
    pos = np.arange(n)
    pair = kept[:, None] & kept[None, :] & (F[:, None] == R[None, :]) & (pos[None, :] >= pos[:, None] + K)
    I, J = np.nonzero(pair)
    if len(I) == 0:
        return NONE, -1, 0, 0
    D = I + J + K - 1
    nb = ((2 * L - K - 1) >> 6) + 1
    best, bs = -1, 0
    for b in range(nb):
        h = int(((D >> 6) == b).sum() + ((D >> 6) == b + 1).sum())
        if h > best:
            best, bs = h, b
    sel = ((D >> 6) == bs) | ((D >> 6) == bs + 1)
    fold_ = (int(D[sel].min()) + int(D[sel].max())) // 4
    span = min(int(I[sel].max() - I[sel].min()), int(J[sel].max() - J[sel].min())) + K
    return _verdict(L, best, fold_, span, int(I[sel].min()), int(J[sel].max()), o)


def revcomp(x):
    return (3 - np.asarray(x, np.uint8)[::-1]).astype(np.uint8)

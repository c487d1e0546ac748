"""Control screen (DESIGN.md §2 "Control screen", rule version 1): the rule restated in numpy, and a brute-force all-pairs reading of it that compares k-mers
as strings (no codes, no hashing).  tests/test_control.py checks the restatement against the brute force on the CPU and holds k_control to the restatement,
field for field, on an MI355X."""
import numpy as np

from fold_ref import codes, revcomp  # noqa: F401  (the same F and R as k_fold's)

K = 15
MIN_LEN, MAX_LEN = 64, 4096
UNTESTED, NONE, FOUND = 0, 1, 2
FIELDS = ("verdict", "strand", "hits", "matched", "ctl_start", "ctl_end", "draft_start", "draft_end")
DEFAULTS = dict(max_occ=4, min_matched=30, min_ctl_tenths=5, min_draft_tenths=8)


def encode(s):
    return np.array(["ACGT".index(c) for c in s.upper()], np.uint8)


def _opts(o):
    r = dict(DEFAULTS)
    r.update(o or {})
    return r


def _report(verdict, strand=-1, hits=0, matched=0, cs=0, ce=0, ds=0, de=0):
    return dict(zip(FIELDS, (int(verdict), int(strand), int(hits), int(matched), int(cs), int(ce), int(ds), int(de))))


def index(C, max_occ):
    """(codes, positions) of the control's index in increasing (code, position): every position 0 .. M - K whose code occurs at most max_occ times in C"""
    F, _ = codes(C)
    if len(F) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    _, inv, cnt = np.unique(F, return_inverse=True, return_counts=True)
    keep = np.flatnonzero(cnt[inv.reshape(-1)] <= max_occ)
    o = np.lexsort((keep, F[keep]))
    return F[keep][o], keep[o].astype(np.int64)


def hits(d, C, max_occ):
    """(o, i, j) of every hit: orientation, draft position, control position"""
    ic, ip = index(C, max_occ)
    F, R = codes(d)
    O, I, J = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    if len(ic) and len(F):
        for o, q in ((0, F), (1, R)):
            lo, hi = np.searchsorted(ic, q, "left"), np.searchsorted(ic, q, "right")
            for g in range(int((hi - lo).max())):
                i = np.flatnonzero(hi - lo > g)
                O.append(np.full(len(i), o, np.int64)); I.append(i.astype(np.int64)); J.append(ip[lo[i] + g])
    return np.concatenate(O), np.concatenate(I), np.concatenate(J)


def _vote(L, M, o, i, j, opts):
    if len(i) == 0:
        return _report(NONE)
    u = np.where(o == 0, i, (L - K) - i)
    dg = u - j + (M - K)
    b = dg >> 6
    nb = ((L - K + M - K) >> 6) + 1
    best, os_, bs = 0, 0, 0
    for oo in (0, 1):                                            # orientation 0 first, then the smallest b: np.argmax takes the first maximum
        hist = np.bincount(b[o == oo], minlength=nb + 1)
        H = hist[:nb] + hist[1:nb + 1]
        if int(H.max()) > best:
            best, os_, bs = int(H.max()), oo, int(np.argmax(H))
    sel = (o == os_) & ((b == bs) | (b == bs + 1))
    Is, Js = i[sel], j[sel]
    matched = len(np.unique(Js))
    cs, ce, ds, de = int(Js.min()), int(Js.max()) + K, int(Is.min()), int(Is.max()) + K
    found = matched >= opts["min_matched"] and 10 * (ce - cs) >= opts["min_ctl_tenths"] * M and 10 * (de - ds) >= opts["min_draft_tenths"] * L
    return _report(FOUND if found else NONE, os_, best, matched, cs, ce, ds, de)


def screen(d, C, opts=None, tested=True):
    """the report of one ZMW as a dict of FIELDS; tested = its status after the cascade is SUCCESS"""
    if not tested:
        return _report(UNTESTED)
    d, C = np.asarray(d, np.uint8), np.asarray(C, np.uint8)
    if len(d) < K:
        return _report(NONE)
    op = _opts(opts)
    o, i, j = hits(d, C, op["max_occ"])
    return _vote(len(d), len(C), o, i, j, op)


def screen_bruteforce(d, C, opts=None, tested=True):
    """the rule read literally: k-mers as strings, every pair of positions, explicit loops for the occurrence cap, the vote and the extents"""
    if not tested:
        return _report(UNTESTED)
    op = _opts(opts)
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    ds_ = "".join("ACGT"[int(x) & 3] for x in d)
    cs_ = "".join("ACGT"[int(x) & 3] for x in C)
    L, M = len(ds_), len(cs_)
    if L < K:
        return _report(NONE)
    ck = [cs_[j:j + K] for j in range(M - K + 1)]
    kept = [j for j in range(M - K + 1) if sum(1 for x in ck if x == ck[j]) <= op["max_occ"]]
    H = []                                                       # (o, i, j, d)
    for i in range(L - K + 1):
        w = ds_[i:i + K]
        r = "".join(comp[c] for c in reversed(w))
        for j in kept:
            if w == ck[j]:
                H.append((0, i, j, i - j + (M - K)))
            if r == ck[j]:
                H.append((1, i, j, (L - K) - i - j + (M - K)))
    if not H:
        return _report(NONE)
    nb = ((L - K + M - K) >> 6) + 1
    best, os_, bs = 0, 0, 0
    for o in (0, 1):
        for b in range(nb):
            h = sum(1 for x in H if x[0] == o and (x[3] >> 6) in (b, b + 1))
            if h > best:
                best, os_, bs = h, o, b
    win = [x for x in H if x[0] == os_ and (x[3] >> 6) in (bs, bs + 1)]
    js, is_ = {x[2] for x in win}, [x[1] for x in win]
    cs, ce, ds, de = min(js), max(js) + K, min(is_), max(is_) + K
    found = len(js) >= op["min_matched"] and 10 * (ce - cs) >= op["min_ctl_tenths"] * M and 10 * (de - ds) >= op["min_draft_tenths"] * L
    return _report(FOUND if found else NONE, os_, best, len(js), cs, ce, ds, de)

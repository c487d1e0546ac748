"""Adapter screen (DESIGN.md §2 "Adapter screen", rule version 1): the rule restated in numpy the plain way (the full (m + 1) x (L + 1) table per search, runs,
starts by a second small table, the union as a boolean array), and a brute-force reading of it for short drafts (the edit distance of the pattern to every
substring).  tests/test_adapters.py checks the restatement against the brute force on the CPU and holds k_adapter to the restatement, field for field, on an
MI355X."""
import numpy as np

MAX_PATTERNS, MAX_LEN, MIN_LEN, MAX_HITS = 8, 64, 16, 16
CONCAT, NEAR_END = 1, 2
DEFAULTS = dict(max_dist_pct=20, min_copies=2, max_insert=100, end_slack=200)
SMRTBELL = "ATCTCTCTCTTTTCCTCCTCCTCCGTTGTTGTTGTTGAGAGAGAT"
FIELDS = ("tested", "verdict", "n_hits", "n_listed", "covered", "max_gap", "first_start", "last_end", "min_dist")


def encode(s):
    return np.array(["ACGT".index(c) for c in s.upper()], np.uint8)


def revcomp(x):
    return (3 - np.asarray(x, np.uint8)[::-1]).astype(np.uint8)


def searches(adapters):
    """search 2a = adapter a as given, 2a + 1 = its reverse complement"""
    out = []
    for a in adapters:
        a = np.asarray(a, np.uint8)
        out += [a, revcomp(a)]
    return out


def _opts(opts):
    o = dict(DEFAULTS)
    o.update(opts or {})
    return o


def _report(tested, L, hits, o):
    """the aggregates, the list and the verdict from every hit (start, end, search, dist) of the ZMW; a dict of FIELDS + hits"""
    if not tested:
        return dict(tested=0, verdict=0, n_hits=0, n_listed=0, covered=0, max_gap=0, first_start=-1, last_end=-1, min_dist=255, hits=[])
    hits = sorted(hits, key=lambda h: (h[1], h[2]))
    union = np.zeros(L, bool)
    for s, e, _, _ in hits:
        union[s:e] = True
    gap = best = 0
    for u in union:
        gap = 0 if u else gap + 1
        best = max(best, gap)
    n = len(hits)
    first = min((h[0] for h in hits), default=-1)
    last = max((h[1] for h in hits), default=-1)
    v = 0
    if n >= o["min_copies"] and best <= o["max_insert"]:
        v |= CONCAT
    if n >= 1 and (first <= o["end_slack"] or last >= L - o["end_slack"]):
        v |= NEAR_END
    return dict(tested=1, verdict=v, n_hits=n, n_listed=min(n, MAX_HITS), covered=int(union.sum()), max_gap=best, first_start=first, last_end=last,
                min_dist=min((h[3] for h in hits), default=255), hits=[tuple(int(x) for x in h) for h in hits[:MAX_HITS]])


# ---------------------------------------------------------------- the restatement
def distance_row(p, d):
    """E[0 .. L]: E[j] = the smallest edit distance of p to a substring of d that ends at j (the last row of the semi-global table)"""
    p, d = np.asarray(p, np.int64), np.asarray(d, np.int64)
    L = len(d)
    jj = np.arange(L + 1)
    row = np.zeros(L + 1, np.int64)
    for i in range(1, len(p) + 1):
        t = np.empty(L + 1, np.int64)
        t[0] = i
        t[1:] = np.minimum(row[1:] + 1, row[:-1] + (d != p[i - 1]))
        row = np.minimum.accumulate(t - jj) + jj                  # row[j] = min over j' <= j of t[j'] + (j - j'): the insertions along the row
    return row


def anchored(p, t):
    """edit(p, t[:x]) for x = 0 .. len(t): the last row of the table that charges the start"""
    p, t = np.asarray(p, np.int64), np.asarray(t, np.int64)
    xx = np.arange(len(t) + 1)
    row = xx.copy()
    for i in range(1, len(p) + 1):
        u = np.empty(len(t) + 1, np.int64)
        u[0] = i
        u[1:] = np.minimum(row[1:] + 1, row[:-1] + (t != p[i - 1]))
        row = np.minimum.accumulate(u - xx) + xx
    return row


def search_hits(p, d, k, s):
    """the hits (start, end, search, dist) of one search; also the smallest E[1 .. L] (len(p) for an empty draft)"""
    E = distance_row(p, d)
    m, L = len(p), len(d)
    out = []
    j = 1
    while j <= L:
        if E[j] > k:
            j += 1
            continue
        r = j
        while r <= L and E[r] <= k:
            r += 1
        end = j + int(np.argmin(E[j:r]))
        dist = int(E[end])
        lo, hi = max(0, m - dist), min(end, m + dist)
        a = anchored(p[::-1], np.asarray(d[end - hi:end])[::-1])
        x = next(x for x in range(lo, hi + 1) if a[x] == dist)
        out.append((end - x, end, s, dist))
        j = r
    return out, int(E[1:].min()) if L else m


def screen(d, adapters, opts=None, tested=True):
    o = _opts(opts)
    hits = []
    if tested:
        for s, p in enumerate(searches(adapters)):
            hits += search_hits(p, d, len(p) * o["max_dist_pct"] // 100, s)[0]
    return _report(tested, len(d), hits, o)


def smallest_distance(d, adapters):
    return min(search_hits(p, d, -1, s)[1] for s, p in enumerate(searches(adapters)))


# ---------------------------------------------------------------- the brute force (short drafts)
def edit_every_substring(p, d):
    """A[i, t] = edit(p, d[i:i + t]) for every start i = 0 .. L and t = 0 .. 2 m (a large number beyond the draft's end): the textbook routine that keeps two
    columns of the table, here for every start at once (one numpy lane per start)"""
    p, d = [int(x) for x in p], np.asarray(d, np.int64)
    m, L = len(p), len(d)
    T = 2 * m
    text = np.concatenate([d, np.full(T, 4, np.int64)])
    ii = np.arange(L + 1)
    A = np.full((L + 1, T + 1), 1 << 20, np.int64)
    A[:, 0] = m
    col = np.tile(np.arange(m + 1, dtype=np.int64), (L + 1, 1))
    for t in range(1, T + 1):
        c = text[ii + t - 1]
        new = np.empty_like(col)
        new[:, 0] = t
        for r in range(1, m + 1):
            new[:, r] = np.minimum(np.minimum(col[:, r] + 1, new[:, r - 1] + 1), col[:, r - 1] + (c != p[r - 1]))
        col = new
        ok = ii + t <= L
        A[ok, t] = col[ok, m]
    return A


def screen_bruteforce(d, adapters, opts=None, tested=True):
    """edit() of the pattern against every substring of at most 2 m bases (a longer one is further from the pattern than the empty one is)"""
    o = _opts(opts)
    L = len(d)
    hits = []
    for s, p in enumerate(searches(adapters) if tested else []):
        m = len(p)
        k = m * o["max_dist_pct"] // 100
        A = edit_every_substring(p, d)
        ed = lambda i, j: int(A[i, j - i])
        E = [min(ed(i, j) for i in range(max(0, j - 2 * m), j + 1)) for j in range(L + 1)]
        j = 1
        while j <= L:
            if E[j] > k:
                j += 1
                continue
            run = []
            while j <= L and E[j] <= k:
                run.append(j)
                j += 1
            dist = min(E[q] for q in run)
            end = min(q for q in run if E[q] == dist)
            x = min(x for x in range(max(0, m - dist), min(end, m + dist) + 1) if ed(end - x, end) == dist)
            hits.append((end - x, end, s, dist))
    return _report(tested, L, hits, o)

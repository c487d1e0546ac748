"""The duplicate rule (DESIGN.md §2 "Duplicate rule") restated in numpy, the limit set of its tests, and a brute force straight from the definition.

The restatement: minimizers from enumerating every k-mer, D from the full (W + 1)^2 table, buckets by key, the sets of a bucket from a plain union over its pairs.
The brute force shares nothing with it but the hash and the packing: D from a second table filled cell by cell, the key clause evaluated per pair, the sets from
a breadth-first search over all n^2 pairs.  tests/test_dup_ref.py holds the one against the other and the library's host calls against the restatement."""
import functools

import numpy as np

UNTESTED, TESTED, OVERFLOW = 0, 1, 2
MAX_BUCKET = 512
FIELDS = ("status", "rep", "set_size", "dup")
SIG_DTYPE = np.dtype([("end", np.uint64, (2, 2)), ("mini", np.uint32, (2,)), ("len", np.int32), ("window", np.int32)])
DEFAULTS = dict(window=32, kmer=12, max_dist_pct=10, max_len_diff_pct=2)
M1, M2, S1, S2, S3 = 0x85EBCA6B, 0xC2B2AE35, 16, 13, 16          # the hash's constants (dup_core.h CCSX_DUP_HASH_*)


def opts(**kw):
    o = dict(DEFAULTS)
    o.update(kw)
    return o


def hash32(x):
    """murmur3's finaliser on uint32 values (an array or one value), in uint64 arithmetic cut to 32 bits"""
    x = np.asarray(x, np.uint64) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(S1); x = (x * np.uint64(M1)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(S2); x = (x * np.uint64(M2)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(S3)
    return x.astype(np.uint32)


def rc(c):
    return (3 - (np.asarray(c, np.uint8) & 3))[::-1].astype(np.uint8)


def ends(read, W):
    """the two end windows of a read of at least W bases: the first W codes of the read and of its reverse complement"""
    c = np.asarray(read, np.uint8) & 3
    return c[:W].copy(), rc(c)[:W].copy()


def kmers(win, k):
    """every k-mer of a window, its first base most significant"""
    v = np.lib.stride_tricks.sliding_window_view(win.astype(np.uint64), k)
    return (v << (2 * np.arange(k - 1, -1, -1, dtype=np.uint64))).sum(axis=1).astype(np.uint32)


def minimizer(win, k):
    return int(hash32(kmers(win, k)).min())


def minimizer_at(win, k):
    """the positions of the k-mers whose hash is the minimizer"""
    h = hash32(kmers(win, k))
    return np.flatnonzero(h == h.min())


def pack(win):
    w = [0, 0]
    for j, b in enumerate(win):
        w[j >> 5] |= int(b) << (2 * (j & 31))
    return w


def sign(reads, o):
    """the signatures of a list of reads"""
    W, k = o["window"], o["kmer"]
    sig = np.zeros(len(reads), SIG_DTYPE)
    for z, r in enumerate(reads):
        sig["len"][z] = len(r)
        if len(r) < W:
            continue
        for e, win in enumerate(ends(r, W)):
            sig["end"][z, e] = pack(win)
            sig["mini"][z, e] = minimizer(win, k)
        sig["window"][z] = W
    return sig


def unpack(words, W):
    return np.array([(int(words[j >> 5]) >> (2 * (j & 31))) & 3 for j in range(W)], np.uint8)


def table(a, b):
    """the full start-anchored unit-cost edit table T[p, q] = ed(a[0, p), b[0, q))"""
    n, m = len(a), len(b)
    T = np.zeros((n + 1, m + 1), np.int64)
    T[0] = np.arange(m + 1)
    ar = np.arange(m + 1)
    for p in range(1, n + 1):
        row = np.empty(m + 1, np.int64)
        row[0] = p
        row[1:] = np.minimum(T[p - 1, 1:] + 1, T[p - 1, :-1] + (b != a[p - 1]))
        T[p] = np.minimum.accumulate(row - ar) + ar               # (the insertions along the row)
    return T


def dist_parts(a, b):
    """(the minimum of the last row, the minimum of the last column) of the table of a against b"""
    T = table(a, b)
    return int(T[-1].min()), int(T[:, -1].min())


def dist(a, b):
    return min(dist_parts(a, b))


def kmax(o):
    return o["window"] * o["max_dist_pct"] // 100


def key(sig, z):
    m = sig["mini"][z]
    return (int(min(m)), int(max(m)))


def may_pair(Li, gi, Lj, gj, o):
    return gi == gj and abs(int(Li) - int(Lj)) * 100 <= o["max_len_diff_pct"] * min(int(Li), int(Lj))


def ends_agree(ei, ej, o, D=dist):
    K = kmax(o)
    return (D(ei[0], ej[0]) <= K and D(ei[1], ej[1]) <= K) or (D(ei[0], ej[1]) <= K and D(ei[1], ej[0]) <= K)


def _report(n):
    return dict(status=np.zeros(n, np.int32), rep=np.arange(n, dtype=np.int32), set_size=np.ones(n, np.int32), dup=np.zeros(n, np.int32))


def _close_sets(rep, members_of, score):
    """the report words of the sets (lists of read indices) in members_of"""
    for members in members_of:
        best = max(score[z] for z in members)
        r = min(z for z in members if score[z] == best)
        for z in members:
            rep["status"][z] = TESTED; rep["rep"][z] = r; rep["set_size"][z] = len(members); rep["dup"][z] = int(r != z)


def cluster(sig, o, group=None, score=None):
    """the report of the signatures: buckets by key, a plain union over the pairs of each bucket"""
    n, W = len(sig), o["window"]
    group = np.zeros(n, np.int64) if group is None else np.asarray(group, np.int64)
    score = np.zeros(n, np.int64) if score is None else np.asarray(score, np.int64)
    rep = _report(n)
    buckets = {}
    for z in range(n):
        if sig["window"][z]:
            buckets.setdefault(key(sig, z), []).append(z)
    memo = {}

    def D(a, b):
        k = (a.tobytes(), b.tobytes())
        if k not in memo:
            memo[k] = memo[k[::-1]] = dist(a, b)
        return memo[k]
    for zs in buckets.values():
        if len(zs) > MAX_BUCKET:
            for z in zs:
                rep["status"][z] = OVERFLOW
            continue
        e = {z: (unpack(sig["end"][z, 0], W), unpack(sig["end"][z, 1], W)) for z in zs}
        label = {z: z for z in zs}
        for a in range(len(zs)):
            for b in range(a + 1, len(zs)):
                i, j = zs[a], zs[b]
                if label[i] != label[j] and may_pair(sig["len"][i], group[i], sig["len"][j], group[j], o) and ends_agree(e[i], e[j], o, D):
                    old, new = label[j], label[i]
                    for z in zs:
                        if label[z] == old:
                            label[z] = new
        _close_sets(rep, [[z for z in zs if label[z] == lab] for lab in set(label.values())], score)
    return rep


def mark(reads, o, group=None, score=None):
    """(signatures, report) of a list of reads"""
    sig = sign(reads, o)
    return sig, cluster(sig, o, group, score)


def diff(got, want):
    """the fields in which a report (attributes or a dict) differs from an expected dict"""
    g = (lambda k: got[k]) if isinstance(got, dict) else (lambda k: getattr(got, k))
    return [(k, np.flatnonzero(np.asarray(g(k)) != want[k])[:8].tolist()) for k in FIELDS if not np.array_equal(np.asarray(g(k)), want[k])]


def partition(rep, order=None):
    """the sets of a report as a set of frozensets of read indices; order[z]: the caller's name of read z"""
    order = np.arange(len(rep["rep"])) if order is None else np.asarray(order)
    sets = {}
    for z, r in enumerate(np.asarray(rep["rep"])):
        sets.setdefault(int(r), []).append(int(order[z]))
    return {frozenset(v) for v in sets.values()}


# ---- the brute force
def _table_cells(a, b):
    n, m = len(a), len(b)
    T = [[0] * (m + 1) for _ in range(n + 1)]
    for q in range(m + 1):
        T[0][q] = q
    for p in range(1, n + 1):
        T[p][0] = p
        for q in range(1, m + 1):
            T[p][q] = min(T[p - 1][q] + 1, T[p][q - 1] + 1, T[p - 1][q - 1] + (a[p - 1] != b[q - 1]))
    return T


@functools.lru_cache(maxsize=None)
def _brute_dist(a: bytes, b: bytes):
    T = _table_cells(a, b)
    return min(min(T[-1]), min(row[-1] for row in T))


def brute(reads, o, group=None, score=None):
    """the report from the definition: every pair of reads is asked every clause, the sets are found by a breadth-first search"""
    n, W, k = len(reads), o["window"], o["kmer"]
    group = [0] * n if group is None else [int(g) for g in group]
    score = [0] * n if score is None else [int(s) for s in score]
    tested = [len(r) >= W for r in reads]
    E = [tuple(bytes(w.tolist()) for w in ends(r, W)) if t else None for r, t in zip(reads, tested)]
    keys = np.full((n, 2), -1, np.int64)
    for z in range(n):
        if tested[z]:
            m = [min(int(hash32(int("".join(str(c) for c in w[j:j + k]), 4))) for j in range(W - k + 1)) for w in (list(E[z][0]), list(E[z][1]))]
            keys[z] = (min(m), max(m))
    same = [np.flatnonzero((keys[:, 0] == keys[z, 0]) & (keys[:, 1] == keys[z, 1])) if tested[z] else np.zeros(0, np.int64) for z in range(n)]
    over = [len(s) > MAX_BUCKET for s in same]
    K = kmax(o)

    def pair(i, j):
        if i == j or not (tested[i] and tested[j]) or over[i] or over[j] or tuple(keys[i]) != tuple(keys[j]) or group[i] != group[j]:
            return False
        Li, Lj = len(reads[i]), len(reads[j])
        if abs(Li - Lj) * 100 > o["max_len_diff_pct"] * min(Li, Lj):
            return False
        D = _brute_dist
        return (D(E[i][0], E[j][0]) <= K and D(E[i][1], E[j][1]) <= K) or (D(E[i][0], E[j][1]) <= K and D(E[i][1], E[j][0]) <= K)
    rep = _report(n)
    seen = [False] * n
    for z in range(n):
        if not tested[z]:
            continue
        if over[z]:
            rep["status"][z] = OVERFLOW
            continue
        if seen[z]:
            continue
        members, queue = [z], [z]
        seen[z] = True
        while queue:
            i = queue.pop(0)
            for j in (int(x) for x in same[i]):                    # (a pair needs the key clause: the other reads are asked it and fail it)
                if not seen[j] and pair(i, j):
                    seen[j] = True
                    members.append(j); queue.append(j)
        _close_sets(rep, [members], score)
    return rep


# ---- the limit set: (name, options, reads, group, score)
def _rand(rng, L):
    return rng.integers(0, 4, L).astype(np.uint8)


def _sub(r, p):
    r = r.copy(); r[p] = (r[p] + 1) & 3
    return r


def _ins(r, p, b=0):
    return np.concatenate([r[:p], np.array([(int(r[p]) + 1 + b) & 3], np.uint8), r[p:]])


def _del(r, p):
    return np.concatenate([r[:p], r[p + 1:]])


EDIT = dict(sub=_sub, ins=_ins)
EDIT["del"] = _del


def edited(rng, r, o, kind, ne, tail=False):
    """r with ne edits of one kind inside its head (tail: its tail) window and outside the minimizer k-mer, such that the edited end keeps its minimizer and
    stands at D = ne exactly from the original one and the other end is unchanged: asserted with the restatement"""
    W, k = o["window"], o["kmer"]
    if tail:
        return rc(edited(rng, rc(r), o, kind, ne))
    win = ends(r, W)[0]
    at = minimizer_at(win, k)
    assert len(at) == 1
    free = [p for p in range(1, W - 1) if not at[0] - 1 <= p <= at[0] + k]
    for _ in range(2000):
        x = r
        for p in sorted(rng.choice(free, ne, replace=False).tolist(), reverse=True):
            x = EDIT[kind](x, p)
        e0, e1 = ends(x, W)
        if minimizer(e0, k) == minimizer(win, k) and dist(win, e0) == ne and np.array_equal(e1, ends(r, W)[1]):
            return x
    raise AssertionError("no placement of the edits keeps the minimizer")


def _dups(rng, n, o):
    """n reads of W .. 2 W bases: about a quarter are copies of earlier ones, as they are, reverse-complemented or with one substitution"""
    W = o["window"]
    reads = []
    for z in range(n):
        if z and rng.random() < 0.25:
            r = reads[int(rng.integers(0, z))]
            how = int(rng.integers(0, 3))
            r = r.copy() if how == 0 else rc(r) if how == 1 else _sub(r, int(rng.integers(0, len(r))))
        else:
            r = _rand(rng, int(rng.integers(W, 2 * W + 1)))
        reads.append(r)
    return reads


@functools.lru_cache(maxsize=None)
def limit_cases():
    rng = np.random.default_rng(20261021)
    cases = []

    def add(name, o, reads, group=None, score=None):
        cases.append((name, o, [np.asarray(r, np.uint8) for r in reads], group, score))
    D = opts()
    W, L = D["window"], 400
    a = _rand(rng, L)
    # read count and length
    add("n0", D, [])
    add("n1", D, [a])
    add("n2", D, [a, _rand(rng, L)])
    add("lengths_W-1_W_W+1", D, [a[:W - 1], a[:W], a[:W + 1], a[:W - 1], a[:W], a[:W + 1]])
    for n in (1, 255, 256, 257, 4097):
        add(f"random_{n}", D, _dups(rng, n, D))
    # windows and k-mers
    for o in (opts(window=16, kmer=16, max_dist_pct=30), opts(window=64, kmer=8), opts(window=32, kmer=12)):
        b = _rand(rng, L)
        reads = [b, b.copy(), rc(b), _rand(rng, L)]
        if o["kmer"] < o["window"]:
            reads += [edited(rng, b, o, "sub", kmax(o)), edited(rng, b, o, "sub", kmax(o) + 1), edited(rng, b, o, "ins", kmax(o), tail=True)]
        else:
            reads += [_sub(b, 3)]                                   # (one k-mer: any edit of the window is an edit of the minimizer)
        add(f"W{o['window']}_k{o['kmer']}", o, reads + _dups(rng, 40, o))
    # edits
    K = kmax(D)
    for kind in ("sub", "ins", "del"):
        for tail in (False, True):
            b = _rand(rng, L)
            reads = [b, edited(rng, b, D, kind, 0, tail), edited(rng, b, D, kind, K, tail)]
            for _ in range(200):                                     # (the read of K + 1 edits is no pair of the read of K edits either: no chain)
                far = edited(rng, b, D, kind, K + 1, tail)
                if mark([reads[2], far], D)[1]["dup"].tolist() == [0, 0]:
                    break
            reads.append(far)
            sig, rep = mark(reads, D)
            assert rep["rep"].tolist() == [0, 0, 0, 3] and len(set(map(tuple, sig["mini"].tolist()))) == 1, (kind, tail, rep)
            add(f"edits_{kind}_{'tail' if tail else 'head'}", D, reads)
    b = _rand(rng, L)
    at = int(minimizer_at(ends(b, W)[0], D["kmer"])[0])
    miss = _sub(b, at + D["kmer"] // 2)
    assert dist(ends(b, W)[0], ends(miss, W)[0]) == 1 and key(sign([b], D), 0) != key(sign([miss], D), 0)
    add("edit_inside_the_minimizer", D, [b, miss])                  # the documented miss: one edit apart and not found
    for kind in ("ins", "del"):
        for p in (0, W - 1):
            for _ in range(2000):                                    # (an edit at the window's edge that keeps the key and costs one edit; at position 0 one
                b = _rand(rng, L)                                    # border of the table decides alone: the other one stands at 2)
                x = EDIT[kind](b, p)
                row, col = dist_parts(ends(b, W)[0], ends(x, W)[0])
                if key(sign([b], D), 0) == key(sign([x], D), 0) and min(row, col) == 1 and (p != 0 or max(row, col) == 2):
                    break
            else:
                raise AssertionError("no such read")
            add(f"{kind}_at_{p}", D, [b, x, x, b])
    # strand and repetition
    b = _rand(rng, L)
    add("opposite_orientation", D, [b, rc(edited(rng, b, D, "sub", 2))])
    half = _rand(rng, L // 2)
    pal = np.concatenate([half, rc(half)])
    assert np.array_equal(pal, rc(pal))
    add("own_reverse_complement", D, [pal, pal.copy(), _rand(rng, L)])
    add("identical_x2", D, [b, b.copy()])
    add("identical_x3", D, [b, _rand(rng, L), b.copy(), b.copy()])
    add("homopolymer", D, [np.zeros(L, np.uint8), np.zeros(L, np.uint8), np.full(L, 3, np.uint8), np.full(L + 1, 2, np.uint8)])
    # length clause and linkage
    mid = lambda r, extra: np.concatenate([r[:200], _rand(rng, extra), r[200:]])
    add("length_at_the_tolerance", D, [b, mid(b, 8)])                # 8 * 100 <= 2 * 400
    add("length_beyond_the_tolerance", D, [b, mid(b, 9)])
    assert mark([b, mid(b, 8)], D)[1]["dup"].tolist() == [0, 1] and mark([b, mid(b, 9)], D)[1]["dup"].tolist() == [0, 0]
    add("chain_by_length", D, [b, mid(b, 8), mid(mid(b, 8), 8)])
    c1 = edited(rng, b, D, "sub", K)
    for _ in range(200):
        c2 = edited(rng, c1, D, "sub", K)
        if dist(ends(b, W)[0], ends(c2, W)[0]) > K:
            break
    assert mark([b, c2], D)[1]["dup"].tolist() == [0, 0] and mark([c2, c1, b], D)[1]["set_size"].tolist() == [3, 3, 3]
    add("chain_by_distance", D, [c2, c1, b, _rand(rng, L)])
    # score and group
    add("score_unique_largest", D, [b, b.copy(), b.copy(), a], None, [5, 9, 7, 1])
    add("score_tied_largest", D, [b, b.copy(), b.copy(), b.copy()], None, [5, 9, 9, -3])
    add("groups_split_equal_reads", D, [b, b.copy(), b.copy(), b.copy(), a], [0, 1, 0, 1, 0], [1, 2, 3, 4, 5])
    # buckets and bytes
    add("bucket_of_512", D, [b] * 512 + [a], None, list(range(513)))
    add("bucket_of_513", D, [a] + [b] * 513, None, list(range(514)))
    mixed = []
    for z, r in enumerate(_dups(rng, 60, D)):
        mixed += [r, r[: z % W]] if z % 3 == 0 else [r]
    add("untested_mixed_in", D, mixed)
    add("high_bits_set", D, [r | np.uint8(0xFC) if z % 2 else r | np.uint8(0x54) for z, r in enumerate(_dups(rng, 30, D))])
    # one component that is a long chain in a bucket of several waves: 300 reads of one pair of ends whose lengths step by 50 from 4000, in shuffled order, so
    # that a read pairs with its few neighbours in length only and the union's trees grow deep before they are flattened
    head, tail = _rand(rng, 64), _rand(rng, 64)
    steps = rng.permutation(300)
    chain = [np.concatenate([head, np.zeros(4000 - 128 + 50 * int(t), np.uint8), tail]) for t in steps]
    assert mark(chain[:40], D)[1]["set_size"].max() < 40
    add("chain_of_300_by_length", D, chain, None, steps.tolist())
    return cases


def with_gaps(reads, rng):
    """(seq, seq_off, seq_len) of the reads with gaps of 1 .. 7 foreign bytes between them, not in order"""
    order = rng.permutation(len(reads))
    seq, off = [], np.zeros(len(reads), np.int64)
    at = 0
    for z in order:
        gap = int(rng.integers(1, 8))
        seq.append(np.full(gap, 0xEE, np.uint8)); at += gap
        off[z] = at
        seq.append(np.asarray(reads[z], np.uint8)); at += len(reads[z])
    seq.append(np.full(3, 0xEE, np.uint8))
    return np.concatenate(seq), off, np.array([len(r) for r in reads], np.int32)


@functools.lru_cache(maxsize=None)
def expected(i):
    """(signatures, report) of limit case i by the restatement; computed once, to be left unchanged"""
    _, o, reads, group, score = limit_cases()[i]
    sig, rep = mark(reads, o, group, score)
    sig.setflags(write=False)
    for v in rep.values():
        v.setflags(write=False)
    return sig, rep

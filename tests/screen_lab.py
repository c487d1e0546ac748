"""The three draft screens' laboratory (DESIGN.md §2 "Adapter palindromes", "Adapter screen", "Control screen"): per screen a limit set of exact drafts that sit
on the boundaries of k_fold, k_adapter and k_control, small functions that say which kernel path a draft takes (so that every case's reason for being in the set
is recomputed, not just named), and a parameterised copy of the rule whose knobs are the slips a kernel could plausibly make (the MUTANTS tables).  With the
default knobs the parameterised copies ARE fold_ref.fold, adapter_ref.screen and control_ref.screen (tests/test_screen_limits.py holds that on random inputs).

A case is (name, draft, request): the request is the key of one entry of the set's `requests` (the options, the adapter set, the control).  The sets are seeded
and built in-process, once per process.  Expectations come from fold_ref / adapter_ref / control_ref alone: the brute force where the draft is short enough
(BRUTE_* below), the restatement otherwise.  A GPU test hands the drafts to the kernels exactly (sdust_lab.batch_from_drafts: identical passes, the POA returns
the template) and runs every request of a batch over every draft of that batch, so a case is also checked under the options of its neighbours.

Every draft has at least opts.min_length = 10 bases and none reaches opts.max_length.  The kernels' guards `nb + 1 > fold_bins`, `words > adapt_words` and
`nb + 1 > ctl_bins` compare a draft against LDS arrays that the launch sizes from the batch's own longest draft, so no draft of a batch can fire them: they are
bounds guards, left as they are, and no case aims at them."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

import adapter_ref as AR
import control_ref as CR
import fold_ref as FR

K = FR.K
NT = 256                            # threads of each of the three kernels
NS_MAX, FOLD_CAP = FR.NS_MAX, 1536  # k_fold: samples that enter; distinct codes and kept positions one table pass holds
CHUNK, BUF, LISTED = 128, 1024, 16  # k_adapter: draft bases per lane, hit keys the LDS buffer holds, listed hits
FILTER_BITS = 32768                 # k_control: bits of the index's prefilter
BRUTE_FOLD, BRUTE_SCREEN = 3000, 600   # the longest drafts the brute forces are asked for


def rc(x):
    return FR.revcomp(x)


@dataclass
class Case:
    name: str               # "<group>/<what>"
    draft: np.ndarray
    request: str            # key of the set's requests
    claim: "object" = None  # () -> bool: the property the name states, recomputed
    batch: str = "short"    # the GPU batch the draft travels in

    def holds(self) -> bool:
        """the claim, recomputed (a claim that was also the construction's retry condition takes the draft)"""
        import inspect
        free = [q for q in inspect.signature(self.claim).parameters.values() if q.default is q.empty]
        return bool(self.claim(self.draft) if free else self.claim())


@dataclass
class LimitSet:
    cases: list
    requests: dict          # key -> the request's arguments (a dict)
    batch_requests: dict = field(default_factory=dict)   # batch -> the request keys run over it (every request of its cases)

    def finish(self):
        names = [c.name for c in self.cases]
        assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
        for c in self.cases:
            c.draft = np.ascontiguousarray(c.draft, np.uint8)
            c.draft.setflags(write=False)
            assert c.request in self.requests, c.name
            self.batch_requests.setdefault(c.batch, [])
            if c.request not in self.batch_requests[c.batch]:
                self.batch_requests[c.batch].append(c.request)
        return self

    def batch(self, b: str) -> list:
        return [c for c in self.cases if c.batch == b]

    def case(self, name: str) -> Case:
        return next(c for c in self.cases if c.name == name)


# ---------------------------------------------------------------- which path a draft takes
def thread_share(count: int, nt: int, tid: int) -> tuple:
    """[p0, p1): thread tid's contiguous share of `count` positions (ccsx_kernels.hip thread_share)"""
    ch = (count + nt - 1) // nt
    p0 = min(tid * ch, count)
    return p0, min(p0 + ch, count)


def share_of(count: int, pos: int) -> int:
    """the thread whose share holds position pos"""
    return pos // ((count + NT - 1) // NT)


def canon(d) -> np.ndarray:
    F, R = FR.codes(d)
    return np.minimum(F, R)


def fold_nparts(ns: int) -> int:
    """the table passes k_fold starts with: the smallest power of two with nparts * CAP >= ns"""
    n = 1
    while n * FOLD_CAP < ns:
        n <<= 1
    return n


def fold_pass(C, nparts: int) -> np.ndarray:
    """the pass of a sample with canonical code C"""
    return ((FR.fmix32(C) >> np.uint32(3)) & np.uint32(nparts - 1)).astype(np.int64)


def fold_schedule(d, max_occ: int) -> list:
    """[(nparts, [(distinct codes, kept positions) per pass])] of every attempt k_fold makes: an attempt with a pass above CAP in either number restarts with
    twice the passes.  (The kernel stops an attempt at its first overflowing pass; the sizes of all its passes are listed.)"""
    s, F, R = FR.sampled_positions(d)
    C = np.minimum(F, R)
    out = []
    nparts = fold_nparts(len(s))
    while True:
        part = fold_pass(C, nparts) if len(s) else np.zeros(0, np.int64)
        sizes = []
        for p in range(nparts):
            u, cnt = np.unique(C[part == p], return_counts=True)
            sizes.append((len(u), int(cnt[cnt <= max_occ].sum())))
        out.append((nparts, sizes))
        if all(c <= FOLD_CAP and k <= FOLD_CAP for c, k in sizes):
            return out
        nparts <<= 1


def n_samples(d) -> int:
    """every sampled position of the draft, those beyond NS_MAX included"""
    return int(((FR.fmix32(canon(d)) & np.uint32(7)) == 0).sum())


def sample_rank(d, pos: int) -> int:
    """position pos is the rank-th sampled position of the draft (1-based); 0 when it is not sampled"""
    smp = np.flatnonzero((FR.fmix32(canon(d)) & np.uint32(7)) == 0)
    r = np.flatnonzero(smp == pos)
    return int(r[0]) + 1 if len(r) else 0


def adapter_chunk(first: int) -> int:
    """the chunk whose lane owns a run with first position `first` (1-based ends): chunk c owns the first positions lo < first <= hi, lo = 128 c"""
    return (first - 1) // CHUNK


def diag_bin(D) -> int:
    return int(D) >> 6


def runs_of(E, k: int) -> list:
    """the maximal runs [a, b] (inclusive ends, 1 <= a) of E[1..L] <= k"""
    ok = np.concatenate([[False], np.asarray(E[1:]) <= k, [False]])
    dd = np.diff(ok.astype(np.int8))
    return list(zip((np.flatnonzero(dd == 1) + 1).tolist(), np.flatnonzero(dd == -1).tolist()))


# ================================================================ k_fold
@dataclass(frozen=True)
class FoldKnobs:
    ns_max: int = 0          # added to NS_MAX
    tie_largest: bool = False  # equal H: the largest b wins
    one_bin: bool = False    # H(b) = hist[b] alone
    j_gt: bool = False       # a hit needs j > i + K
    occ_ge: bool = False     # a code at >= max_occ positions is dropped
    occ_all: bool = False    # the occurrence count is taken over every sampled position, not over the NS_MAX that enter
    span_max: bool = False   # span = max(.., ..) + K
    reach_lt: bool = False   # the shorter arm's side by fold < L - fold


FOLD_DEFAULT = FoldKnobs()
FOLD_MUTANTS = {
    "NS_MAX-1": FoldKnobs(ns_max=-1), "NS_MAX+1": FoldKnobs(ns_max=1), "tie>b": FoldKnobs(tie_largest=True), "one-bin": FoldKnobs(one_bin=True),
    "j>i+K": FoldKnobs(j_gt=True), "occ>=": FoldKnobs(occ_ge=True), "occ-all": FoldKnobs(occ_all=True), "span-max": FoldKnobs(span_max=True),
    "reach<": FoldKnobs(reach_lt=True),
}


def fold_k(d, opts=None, kn: FoldKnobs = FOLD_DEFAULT) -> tuple:
    """fold_ref.fold under the knobs"""
    o = FR._opts(opts)
    L = len(d)
    F, R = FR.codes(d)
    if len(F) == 0:
        return FR.NONE, -1, 0, 0
    C = np.minimum(F, R)
    smp = np.flatnonzero((FR.fmix32(C) & np.uint32(7)) == 0)
    s = smp[:max(0, NS_MAX + kn.ns_max)]
    if len(s) == 0:
        return FR.NONE, -1, 0, 0
    u, cnt = np.unique(C[smp if kn.occ_all else s], return_counts=True)
    c_of = cnt[np.searchsorted(u, C[s])]
    s = s[c_of < o["max_occ"] if kn.occ_ge else c_of <= o["max_occ"]]
    s = s[np.lexsort((s, C[s]))]
    I, J = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for g in range(1, o["max_occ"]):
        a = np.arange(len(s) - g)
        if len(a) == 0:
            break
        lo, hi = s[a], s[a + g]
        m = (C[lo] == C[hi]) & (F[lo] == R[hi]) & ((hi > lo + K) if kn.j_gt else (hi >= lo + K))
        I.append(lo[m]); J.append(hi[m])
    i, j = np.concatenate(I).astype(np.int64), np.concatenate(J).astype(np.int64)
    if len(i) == 0:
        return FR.NONE, -1, 0, 0
    D = i + j + K - 1
    b = D >> 6
    nb = ((2 * L - K - 1) >> 6) + 1
    hist = np.bincount(b, minlength=nb + 1)
    H = hist[:nb].copy() if kn.one_bin else hist[:nb] + hist[1:nb + 1]
    bs = nb - 1 - int(np.argmax(H[::-1])) if kn.tie_largest else int(np.argmax(H))
    sel = (b == bs) if kn.one_bin else (b == bs) | (b == bs + 1)
    Ds, Is, Js = D[sel], i[sel], j[sel]
    fold = int(Ds.min() + Ds.max()) // 4
    ext = (int(Is.max() - Is.min()), int(Js.max() - Js.min()))
    span = (max(ext) if kn.span_max else min(ext)) + K
    shorter = min(fold, L - fold)
    left = fold < L - fold if kn.reach_lt else fold <= L - fold
    reach = int(Is.min()) <= o["end_slack"] if left else int(Js.max()) + K >= L - o["end_slack"]
    pal = int(H[bs]) >= o["min_hits"] and span >= o["min_arm"] and 10 * span >= o["min_span_tenths"] * shorter and reach
    return (FR.PALINDROME if pal else FR.NONE), fold, int(H[bs]), span


def sampled_kmer(rng, avoid=()) -> np.ndarray:
    """a random 15-mer with all four bases whose canonical code is sampled and is not among `avoid`"""
    while True:
        y = rng.integers(0, 4, K).astype(np.uint8)
        c = int(canon(y)[0])
        if (FR.fmix32(c)[0] & 7) == 0 and c not in avoid and len(set(y.tolist())) == 4:
            return y


def quiet(rng, n: int) -> np.ndarray:
    """n random bases without a hit at any max_occ (no sampled canonical code twice)"""
    while True:
        x = rng.integers(0, 4, n).astype(np.uint8)
        if n < K:
            return x
        s, F, R = FR.sampled_positions(x)
        C = np.minimum(F, R)
        if len(np.unique(C)) == len(C):
            return x


def plant(x, pairs) -> np.ndarray:
    """x with y written at i and rc(y) at j for every (i, j, y) of pairs"""
    x = np.array(x, np.uint8)
    for i, j, y in pairs:
        assert j >= i + K or j == i + K - 2
        x[i:i + K] = y
        x[j:j + K] = rc(y)
    return x


def fold_hits(d, max_occ=8) -> list:
    i, j = FR.hits(d, max_occ)
    return sorted(zip(i.tolist(), j.tolist()))


def planted(rng, L: int, ij: list, max_occ: int = 8, tries: int = 400) -> tuple:
    """(draft, kmers): a quiet random draft of L bases whose hits are exactly the pairs ij (each with a sampled 15-mer of its own)"""
    for _ in range(tries):
        ys, seen = [], set()
        for _ in ij:
            y = sampled_kmer(rng, seen)
            seen.add(int(canon(y)[0]))
            ys.append(y)
        d = plant(quiet(rng, L), [(i, j, y) for (i, j), y in zip(ij, ys)])
        if fold_hits(d, max_occ) == sorted(ij):
            return d, ys
    raise AssertionError(("no draft with exactly these hits", L, ij))


ONE = dict(max_occ=8, min_hits=1, min_arm=15, min_span_tenths=0, end_slack=1 << 20)    # a single hit is a palindrome
V_ALL = dict(max_occ=8, min_hits=2, min_arm=60, min_span_tenths=5, end_slack=7)        # what the verdict drafts meet exactly


def _fold_requests() -> dict:
    return {"one": ONE, "one/occ1": dict(ONE, max_occ=1), "one/occ64": dict(ONE, max_occ=64),
            "v/all": V_ALL, "v/hits+1": dict(V_ALL, min_hits=3), "v/arm+1": dict(V_ALL, min_arm=61), "v/slack-1": dict(V_ALL, end_slack=6),
            "v/tenths10": dict(V_ALL, min_span_tenths=10), "v/tenths0": dict(V_ALL, min_span_tenths=0, min_arm=15), "v/slack0": dict(V_ALL, end_slack=0),
            "default": dict(FR.DEFAULTS)}


def _poly_a_case(rng, rank: int, max_occ_copies: int = 0, tail_copy: bool = False):
    """y . A^n . rc(y): every all-A 15-mer is sampled (fmix32(0) = 0), so n sets the rank of rc(y)'s position among the samples; the draft ends with rc(y).
    max_occ_copies > 0: that many positions of y's code in all (copies - 1 of y, one rc(y)); tail_copy: one more y behind a further A-run, beyond the
    NS_MAX-th sample"""
    while True:
        y = sampled_kmer(rng)
        copies = max(1, max_occ_copies - 1)
        head = np.concatenate([np.concatenate([y, quiet(rng, 5)]) for _ in range(copies)])
        for n in range(rank - 60, rank + 20):
            d = np.concatenate([head, np.zeros(n, np.uint8), rc(y)])
            q = len(d) - K
            if sample_rank(d, q) == rank:
                break
        else:
            continue
        if tail_copy:
            fill = NS_MAX - rank + 40
            d = np.concatenate([d, np.zeros(fill, np.uint8), y])
        hs = fold_hits(d, 64)
        if all(jj == q for _, jj in hs) and len(hs) == (copies if rank <= NS_MAX else 0):
            return d, y, q


@functools.lru_cache(maxsize=None)
def fold_cases() -> LimitSet:
    rng = np.random.default_rng(1501)
    cs = []
    add = lambda *a, **k: cs.append(Case(*a, **k))
    # ---- lengths
    add("len/L14_no_position", quiet(rng, 14), "one", lambda: True)
    add("len/L15_one_position", sampled_kmer(rng), "one", lambda: True)
    for npos in (255, 256, 257, 511, 512, 513):
        L = npos + K - 1
        t1 = 3
        t2 = share_of(npos, npos - 1)                                # the last thread that owns anything
        i, j = thread_share(npos, NT, t1)[0], thread_share(npos, NT, t2)[1] - 1
        d, _ = planted(rng, L, [(i, j)])
        add(f"len/npos{npos}_share_first_to_share_last", d, "one",
            lambda d=d, npos=npos, i=i, j=j, t2=t2: len(d) - 14 == npos and j == npos - 1 and thread_share(npos, NT, 3)[0] == i
            and thread_share(npos, NT, t2)[1] - 1 == j and thread_share(npos, NT, t2 + 1) == (npos, npos) and fold_hits(d) == [(i, j)])
    # ---- the sample cap
    for rank in (NS_MAX - 1, NS_MAX, NS_MAX + 1):
        d, y, q = _poly_a_case(rng, rank)
        add(f"ns/later_position_is_sample_{rank}", d, "one",
            lambda d=d, q=q, rank=rank: sample_rank(d, q) == rank == n_samples(d) and (fold_hits(d) == [(0, q)]) == (rank <= NS_MAX)
            and (FR.fold(d, opts=ONE)[0] == FR.PALINDROME) == (rank <= NS_MAX), batch="ns")
    # ---- the table cap: a random draft cut right behind its n-th sample, three planted pairs on one anti-diagonal whose codes fall in different passes
    for n, occ in ((1536, 8), (1537, 8), (3072, 8)):
        for _ in range(200):
            x = rng.integers(0, 4, 9 * n).astype(np.uint8)
            ys = [sampled_kmer(rng) for _ in range(4)]
            c0 = 4000
            x = plant(x, [(c0 - 500 - 40 * q, c0 + 500 + 40 * q, y) for q, y in enumerate(ys)])
            smp = np.flatnonzero((FR.fmix32(canon(x)) & np.uint32(7)) == 0)
            d = x[:int(smp[n - 1]) + K]
            sch = fold_schedule(d, occ)
            parts = {int(fold_pass(canon(y), sch[-1][0])[0]) for y in ys}
            ok = n_samples(d) == n and len(fold_hits(d)) >= 4 and (len(parts) >= 2 or sch[-1][0] == 1)
            if n == 3072:
                ok = ok and [a for a, _ in sch] == [2, 4]
            if ok:
                break
        else:
            raise AssertionError(n)
        want = {1536: [1], 1537: [2], 3072: [2, 4]}[n]
        add(f"cap/{n}_samples", d, "one",
            lambda d=d, n=n, want=want, ys=ys: n_samples(d) == n and [a for a, _ in fold_schedule(d, 8)] == want
            and (n != 1536 or fold_schedule(d, 8)[0][1][0][1] == FOLD_CAP > fold_schedule(d, 8)[0][1][0][0])      # kept positions at CAP, fewer codes
            and (n != 3072 or max(max(s) for s in fold_schedule(d, 8)[0][1]) > FOLD_CAP)                           # the imbalance that restarts the vote
            and (n == 1536 or len({int(fold_pass(canon(y), want[-1])[0]) for y in ys}) >= 2)                       # the planted hits lie in different passes
            and FR.fold(d, opts=ONE)[2] >= 4, batch="cap3072" if n == 3072 else "cap")
    for _ in range(200):                                             # exactly CAP distinct codes in one pass: every sample its own code, so no hit (a hit
        x = rng.integers(0, 4, 9 * 1536).astype(np.uint8)            # needs two samples of one code and ns <= CAP leaves room for CAP - 1 codes then)
        smp = np.flatnonzero((FR.fmix32(canon(x)) & np.uint32(7)) == 0)
        d = x[:int(smp[1535]) + K]
        if fold_schedule(d, 8) == [(1, [(FOLD_CAP, FOLD_CAP)])]:
            break
    add("cap/1536_codes_no_hit", d, "one", lambda d=d: fold_schedule(d, 8) == [(1, [(FOLD_CAP, FOLD_CAP)])] and FR.fold(d, opts=ONE) == (FR.NONE, -1, 0, 0),
        batch="cap")
    # ---- the occurrence cap: a code at exactly max_occ and at max_occ + 1 entering positions (c - 1 copies of y, one rc(y))
    for mo in (1, 8, 64):
        for c in (mo, mo + 1):
            while True:
                y = sampled_kmer(rng)
                d = np.concatenate([quiet(rng, 20)] + [np.concatenate([y, quiet(rng, 2)]) for _ in range(c - 1)] + [quiet(rng, 9), rc(y), quiet(rng, 20)])
                cy = int(canon(y)[0])
                cnt = int((np.minimum(*FR.sampled_positions(d)[1:]) == cy).sum())
                hs = fold_hits(d, max(c, 2))
                if cnt == c and len(hs) == c - 1 and all(canon(d)[i] == cy for i, _ in hs):
                    break
            req = {1: "one/occ1", 8: "one", 64: "one/occ64"}[mo]
            add(f"occ/max_occ{mo}_code_at_{c}", d, req,
                lambda d=d, cy=cy, c=c, mo=mo: int((np.minimum(*FR.sampled_positions(d)[1:]) == cy).sum()) == c
                and len(fold_hits(d, mo)) == (c - 1 if c <= mo else 0) and len(fold_hits(d, mo + 1)) == c - 1)
    d, y, q = _poly_a_case(rng, NS_MAX - 20, max_occ_copies=8, tail_copy=True)
    cy = int(canon(y)[0])
    add("occ/ninth_copy_behind_the_last_sample", d, "one",
        lambda d=d, cy=cy: int((np.minimum(*FR.sampled_positions(d)[1:]) == cy).sum()) == 8 and int((canon(d) == cy).sum()) == 9
        and n_samples(d) > NS_MAX and len(fold_hits(d, 8)) == 7 and FR.fold(d, opts=ONE)[2] >= 1, batch="ns")
    # ---- the vote
    b = 3
    for name, D in (("64b-1", 64 * b - 1), ("64b", 64 * b), ("64b+63", 64 * b + 63)):
        i = 40
        j = D - (K - 1) - i
        d, _ = planted(rng, 260, [(i, j)])
        add(f"vote/D_{name}", d, "one", lambda d=d, D=D, i=i, j=j: fold_hits(d) == [(i, j)] and i + j + 14 == D and diag_bin(D) == (3 if D >= 192 else 2))
    d, _ = planted(rng, 260, [(40, 64 * b - 1 - 14 - 40), (60, 64 * b - 14 - 60)])
    add("vote/pair_across_the_bin_edge", d, "one", lambda d=d: sorted(diag_bin(i + j + 14) for i, j in fold_hits(d)) == [2, 3] and FR.fold(d, opts=ONE)[2] == 2)
    d, _ = planted(rng, 330, [(40, 64 * b + 63 - 14 - 40), (80, 64 * (b + 2) - 14 - 80)])
    add("vote/two_bins_apart_first_wins_with_empty_left_bin", d, "one",
        lambda d=d: sorted(diag_bin(i + j + 14) for i, j in fold_hits(d)) == [3, 5] and FR.fold(d, opts=ONE)[1:3] == ((64 * 3 + 63) * 2 // 4, 1))
    d, _ = planted(rng, 700, [(20, 130), (40, 110), (300, 500), (330, 470)])
    add("vote/equal_H_the_smaller_b_wins", d, "one",
        lambda d=d: sorted(diag_bin(i + j + 14) for i, j in fold_hits(d)) == [2, 2, 12, 12] and FR.fold(d, opts=ONE)[1:] == (82, 2, 35))
    d, _ = planted(rng, 260, [(20, 200), (40, 170)])
    add("vote/span_is_the_smaller_extent", d, "one", lambda d=d: FR.fold(d, opts=ONE) == (FR.PALINDROME, 114, 2, 35))
    L = 256 + 23                                                     # 2 L - 31 and 2 L - 16 share their bin: the latest hit lies in bin nb - 1
    d, _ = planted(rng, L, [(L - 30, L - 15)])
    add("vote/last_bin", d, "one", lambda d=d, L=L: fold_hits(d) == [(L - 30, L - 15)] and diag_bin(2 * L - 31) == ((2 * L - K - 1) >> 6))
    d, _ = planted(rng, 200, [(90, 105)])
    add("vote/j_is_i_plus_15", d, "one", lambda d=d: fold_hits(d) == [(90, 105)] and FR.fold(d, opts=ONE) == (FR.PALINDROME, 104, 1, 15))
    while True:                                                      # j = i + 14 cannot exist (d[i + 14] would be its own complement); j = i + 13 can, and is no hit
        y = sampled_kmer(rng)
        if y[13] == 3 - y[14]:
            d = plant(quiet(rng, 200), [(90, 103, y)])
            F, R = FR.codes(d)
            if F[90] == R[103] and not fold_hits(d):
                break
    add("vote/j_is_i_plus_13_no_hit", d, "one", lambda d=d: FR.codes(d)[0][90] == FR.codes(d)[1][103] and sample_rank(d, 90) > 0 and sample_rank(d, 103) > 0
        and not fold_hits(d))
    # ---- the verdict: two hits on one anti-diagonal, D = 240 (fold 120); V_ALL is met exactly in all four conditions, and missed by one by a neighbour
    d, _ = planted(rng, 300, [(7, 219), (52, 174)])
    add("verdict/left_all_met_exactly", d, "v/all", lambda d=d: FR.fold(d, opts=V_ALL) == (FR.PALINDROME, 120, 2, 60) and fold_hits(d)[0][0] == 7
        and 10 * 60 == 5 * 120 and all(FR.fold(d, opts=o)[0] == FR.NONE for o in (dict(V_ALL, min_hits=3), dict(V_ALL, min_arm=61), dict(V_ALL, end_slack=6))))
    for r in ("v/hits+1", "v/arm+1", "v/slack-1", "v/tenths10", "v/tenths0", "v/slack0", "default"):
        add(f"verdict/left_under_{r[2:] if r != 'default' else r}", d, r, lambda: True)
    d2, _ = planted(rng, 300, [(7, 219), (51, 175)])
    add("verdict/span_one_short_of_5_tenths", d2, "v/tenths0", lambda d=d2: FR.fold(d, opts=dict(V_ALL, min_arm=15)) == (FR.NONE, 120, 2, 59)
        and FR.fold(d, opts=dict(V_ALL, min_arm=15, min_span_tenths=4))[0] == FR.PALINDROME)
    L = 247                                                          # fold 127 > L - fold = 120: the right arm is the shorter one; max_j + K = L - 7
    d3, _ = planted(rng, L, [(15, 225), (60, 180)])
    add("verdict/right_all_met_exactly", d3, "v/all", lambda d=d3, L=L: FR.fold(d, opts=V_ALL) == (FR.PALINDROME, 127, 2, 60) and 127 > L - 127
        and fold_hits(d)[0][1] + K == L - 7 and FR.fold(d, opts=dict(V_ALL, end_slack=6))[0] == FR.NONE)
    L = 240                                                          # fold = L - fold = 120: the left rule applies (min_i = 7), though max_j + K = 234 = L - 6
    d4, _ = planted(rng, L, [(7, 219), (52, 174)])
    add("verdict/fold_equals_L_minus_fold", d4, "v/slack-1", lambda d=d4: FR.fold(d, opts=dict(V_ALL, end_slack=6)) == (FR.NONE, 120, 2, 60)
        and fold_hits(d)[0][1] + K >= 240 - 6)
    L = 239                                                          # fold 120 > L - fold = 119: now the right rule, met at end_slack 6 (max_j + K = 234 >= 233)
    d5, _ = planted(rng, L, [(7, 219), (52, 174)])
    add("verdict/fold_one_above_L_minus_fold", d5, "v/slack-1", lambda d=d5: FR.fold(d, opts=dict(V_ALL, end_slack=6)) == (FR.PALINDROME, 120, 2, 60)
        and FR.fold(d, opts=dict(V_ALL, end_slack=4))[0] == FR.NONE)
    return LimitSet(cs, _fold_requests()).finish()


def fold_expect(d, opts) -> tuple:
    """the expectation: the brute force where it is affordable (asserted equal to the restatement), the restatement otherwise"""
    want = FR.fold(d, opts=opts)
    if len(d) <= BRUTE_FOLD:
        bf = FR.fold_bruteforce(d, opts=opts)
        assert bf == want, (len(d), opts, bf, want)
    return want


# ================================================================ k_control
@dataclass(frozen=True)
class ControlKnobs:
    tie_o1: bool = False        # equal H in both orientations: orientation 1 wins
    tie_largest: bool = False   # equal H within an orientation: the largest b wins
    matched_hits: bool = False  # matched counts hits, not distinct control positions
    cap_draft: bool = False     # the occurrence cap is applied to the draft's codes, not to the control's
    rev_from_i: bool = False    # orientation 1 takes u = i
    ext_no_k: bool = False      # ctl_end and draft_end without + K


CONTROL_DEFAULT = ControlKnobs()
CONTROL_MUTANTS = {"tie-o1": ControlKnobs(tie_o1=True), "tie>b": ControlKnobs(tie_largest=True), "matched=hits": ControlKnobs(matched_hits=True),
                   "cap-on-draft": ControlKnobs(cap_draft=True), "u=i": ControlKnobs(rev_from_i=True), "ends-K": ControlKnobs(ext_no_k=True)}


def control_hits(d, C, max_occ, kn: ControlKnobs = CONTROL_DEFAULT):
    """control_ref.hits under the knobs: (o, i, j)"""
    ic, ip = CR.index(C, 1 << 30 if kn.cap_draft else max_occ)
    F, R = FR.codes(d)
    O, I, J = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    if len(ic) and len(F):
        ok = np.ones(len(F), bool)
        if kn.cap_draft:
            _, inv, cnt = np.unique(F, return_inverse=True, return_counts=True)
            ok = cnt[inv.reshape(-1)] <= max_occ
        for o, q in ((0, F), (1, R)):
            lo, hi = np.searchsorted(ic, q, "left"), np.searchsorted(ic, q, "right")
            for g in range(int((hi - lo).max())):
                i = np.flatnonzero((hi - lo > g) & ok)
                O.append(np.full(len(i), o, np.int64)); I.append(i.astype(np.int64)); J.append(ip[lo[i] + g])
    return np.concatenate(O), np.concatenate(I), np.concatenate(J)


def control_diagonals(d, C, max_occ):
    """(o, i, j, diagonal) of every hit"""
    o, i, j = control_hits(d, C, max_occ)
    return o, i, j, np.where(o == 0, i, (len(d) - K) - i) - j + (len(C) - K)


def control_k(d, C, opts=None, kn: ControlKnobs = CONTROL_DEFAULT) -> dict:
    """control_ref.screen under the knobs"""
    d, C = np.asarray(d, np.uint8), np.asarray(C, np.uint8)
    op = CR._opts(opts)
    L, M = len(d), len(C)
    if L < K:
        return CR._report(CR.NONE)
    o, i, j = control_hits(d, C, op["max_occ"], kn)
    if len(i) == 0:
        return CR._report(CR.NONE)
    u = i if kn.rev_from_i else np.where(o == 0, i, (L - K) - i)
    dg = u - j + (M - K)
    b = dg >> 6
    nb = ((L - K + M - K) >> 6) + 1
    keep = (b >= 0) & (b <= nb)
    best, os_, bs = 0, 0, 0
    for oo in (0, 1):
        hist = np.bincount(b[(o == oo) & keep], minlength=nb + 1)
        H = hist[:nb] + hist[1:nb + 1]
        hb = nb - 1 - int(np.argmax(H[::-1])) if kn.tie_largest else int(np.argmax(H))
        if int(H.max()) > best or (kn.tie_o1 and oo == 1 and int(H.max()) == best and best > 0):
            best, os_, bs = int(H.max()), oo, hb
    if best == 0:
        return CR._report(CR.NONE)
    sel = (o == os_) & ((b == bs) | (b == bs + 1))
    Is, Js = i[sel], j[sel]
    matched = len(Js) if kn.matched_hits else len(np.unique(Js))
    e = 0 if kn.ext_no_k else K
    cs, ce, ds, de = int(Js.min()), int(Js.max()) + e, int(Is.min()), int(Is.max()) + e
    found = matched >= op["min_matched"] and 10 * (ce - cs) >= op["min_ctl_tenths"] * M and 10 * (de - ds) >= op["min_draft_tenths"] * L
    return CR._report(CR.FOUND if found else CR.NONE, os_, best, matched, cs, ce, ds, de)


def filter_bit(code) -> int:
    """the prefilter bit of a code (ccsx_api.cpp builds the bitmap from the index's codes, k_control tests it before the lower bound)"""
    return int(FR.fmix32(code)[0]) & (FILTER_BITS - 1)


def kmer_of(code: int) -> np.ndarray:
    return np.array([(code >> (2 * (K - 1 - t))) & 3 for t in range(K)], np.uint8)


def no_kmer_of(rng, n: int, C, also=()) -> np.ndarray:
    """n random bases that share no 15-mer, in either orientation, with C or with the sequences of `also`"""
    bad = set()
    for x in (C,) + tuple(also):
        F, R = FR.codes(x)
        bad |= set(F.tolist()) | set(R.tolist())
    while True:
        x = rng.integers(0, 4, n).astype(np.uint8)
        if n < K or not (set(FR.codes(x)[0].tolist()) & bad):
            return x


def retry(make, ok, tries: int = 400):
    """the first make() for which ok(it) holds: random flanks now and then extend a planted stretch by a base"""
    for _ in range(tries):
        x = make()
        if ok(x):
            return x
    raise AssertionError("no draft with the property")


C_LOOSE = dict(max_occ=4, min_matched=1, min_ctl_tenths=0, min_draft_tenths=0)
C_V = dict(max_occ=4, min_matched=36, min_ctl_tenths=5, min_draft_tenths=10)
CAP_COUNTS = (1, 2, 4, 5, 64, 65)


@functools.lru_cache(maxsize=None)
def control_cases() -> LimitSet:
    rng = np.random.default_rng(1502)
    rnd = lambda n: rng.integers(0, 4, n).astype(np.uint8)
    while True:
        c64, c100, c4096 = rnd(64), rnd(100), rnd(4096)
        if all(len(np.unique(FR.codes(c)[0])) == len(c) - K + 1 for c in (c64, c100, c4096)):
            break
    units = [sampled_kmer(rng) for _ in CAP_COUNTS]
    ccap = np.concatenate([np.concatenate([np.tile(w, c), no_kmer_of(rng, 20, np.concatenate(units))]) for w, c in zip(units, CAP_COUNTS)])
    req = {"c64": dict(control=c64, opts=C_LOOSE), "c4096": dict(control=c4096, opts=C_LOOSE), "c100": dict(control=c100, opts=C_LOOSE),
           "c100/v": dict(control=c100, opts=C_V), "c100/v_matched+1": dict(control=c100, opts=dict(C_V, min_matched=37)),
           "c100/v_matched-1": dict(control=c100, opts=dict(C_V, min_matched=35)), "c100/v_tenths0": dict(control=c100, opts=dict(C_V, min_ctl_tenths=0, min_draft_tenths=0)),
           "c4096/occ64_tenths10": dict(control=c4096, opts=dict(max_occ=64, min_matched=1, min_ctl_tenths=0, min_draft_tenths=10))}
    for mo in (1, 4, 64):
        req[f"ccap/occ{mo}"] = dict(control=ccap, opts=dict(C_LOOSE, max_occ=mo))
    ref = lambda d, r: CR.screen(d, req[r]["control"], req[r]["opts"])
    cs = []
    add = lambda *a, **k: cs.append(Case(*a, **k))
    jk = lambda n, C: no_kmer_of(rng, n, C)
    # ---- the two ends of the control's length
    add("ctl/M64_has_50_entries", np.concatenate([jk(40, c64), c64, jk(30, c64)]), "c64",
        lambda: len(CR.index(c64, 4)[0]) == 50 and ref(cs[0].draft, "c64") == CR._report(CR.FOUND, 0, 50, 50, 0, 64, 40, 104))
    d = c4096[1000:1400].copy()
    add("ctl/M4096_has_4082_entries", d, "c4096", lambda d=d: len(CR.index(c4096, 4)[0]) == 4082 and ref(d, "c4096")["hits"] == 386 and ref(d, "c4096")["ctl_start"] == 1000)
    # ---- the draft's codes against the sorted index
    ic, ip = CR.index(c64, 4)
    first, last = kmer_of(int(ic[0])), kmer_of(int(ic[-1]))
    d = np.concatenate([np.zeros(30, np.uint8), c64[10:40]])
    add("idx/code_below_every_entry", d, "c64", lambda d=d: 0 < ic[0] and FR.codes(d)[0][0] == 0 and ref(d, "c64")["hits"] == 16)
    d = np.concatenate([np.full(30, 3, np.uint8), c64[10:40]])
    add("idx/code_above_every_entry", d, "c64", lambda d=d: FR.codes(d)[0][0] == 4 ** K - 1 > ic[-1] and ref(d, "c64")["hits"] == 16)
    for nm, w, j in (("first", first, int(ip[0])), ("last", last, int(ip[-1]))):
        ok = lambda d, j=j: ref(d, "c64") == CR._report(CR.FOUND, 0, 1, 1, j, j + K, 20, 35)
        add(f"idx/code_equals_the_{nm}_entry", retry(lambda: np.concatenate([jk(20, c64), w, jk(20, c64)]), ok), "c64", ok)
    bits = {filter_bit(int(c)) for c in ic}
    while True:
        x = rnd(K)
        Fx, Rx = FR.codes(x)
        if int(Fx[0]) not in set(ic.tolist()) and int(Rx[0]) not in set(ic.tolist()) and filter_bit(int(Fx[0])) in bits:
            break
    d = np.concatenate([jk(20, c64), x, jk(5, c64), first, jk(20, c64)])
    add("idx/prefilter_bit_set_code_absent", d, "c64",
        lambda d=d: FR.codes(d)[0][20] not in set(ic.tolist()) and filter_bit(int(FR.codes(d)[0][20])) in bits and ref(d, "c64")["hits"] == 1)
    # ---- the occurrence cap is the control's
    ccodes = FR.codes(ccap)[0]
    for w, c in zip(units, CAP_COUNTS):
        mo = {1: 1, 2: 1, 4: 4, 5: 4, 64: 64, 65: 64}[c]
        ok = lambda d, w=w, c=c, mo=mo: int((ccodes == FR.codes(w)[0][0]).sum()) == c and len(control_hits(d, ccap, 65)[0]) == c \
            and (ref(d, f"ccap/occ{mo}")["hits"] > 0) == (c <= mo)
        add(f"occ/max_occ{mo}_control_code_at_{c}", retry(lambda: np.concatenate([jk(25, ccap), w, jk(25, ccap)]), ok), f"ccap/occ{mo}", ok)
    ok = lambda d: int((FR.codes(d)[0] == FR.codes(units[0])[0][0]).sum()) == 6 == len(control_hits(d, ccap, 1)[0]) and ref(d, "ccap/occ1")["hits"] >= 5
    add("occ/draft_repeats_a_kept_code", retry(lambda: np.concatenate([np.concatenate([units[0], jk(2, ccap)]) for _ in range(6)]), ok), "ccap/occ1", ok)
    # ---- the vote
    d = np.concatenate([jk(43, c100), c100[:50], c100[51:]])         # one control base deleted: diagonals 128 and 127
    add("vote/diagonals_64b_and_64b-1", d, "c100", lambda d=d: sorted(set(control_diagonals(d, c100, 4)[3].tolist())) == [127, 128]
        and ref(d, "c100")["hits"] == ref(d, "c100")["matched"] == len(control_hits(d, c100, 4)[0]) >= 86 - K)
    d = np.concatenate([jk(106, c100), c100[:50], [3 - c100[50]], c100[50:]]).astype(np.uint8)   # one base inserted: diagonals 191 and 192
    add("vote/diagonals_64b+63_and_64b+64", d, "c100", lambda d=d: sorted(set(control_diagonals(d, c100, 4)[3].tolist())) == [191, 192]
        and ref(d, "c100")["hits"] == len(control_hits(d, c100, 4)[0]) >= 86 - K)
    d = np.concatenate([c100[:60], rc(c100[:60])])
    add("vote/orientations_tie_0_wins", d, "c100", lambda d=d: ref(d, "c100") == CR._report(CR.FOUND, 0, 46, 46, 0, 60, 0, 60)
        and control_k(d, c100, C_LOOSE, ControlKnobs(tie_o1=True))["draft_start"] == 60)
    ok = lambda d: ref(d, "c100") == CR._report(CR.FOUND, 0, 26, 26, 0, 40, 0, 40) and sorted(set((control_diagonals(d, c100, 4)[3] >> 6).tolist())) == [1, 5] \
        and len(control_hits(d, c100, 4)[0]) == 52
    add("vote/two_bin_pairs_tie_smaller_b_wins", retry(lambda: np.concatenate([c100[:40], jk(200, c100), c100[:40]]), ok), "c100", ok)
    d = rc(c100)
    add("vote/draft_is_rc_of_control", d, "c100", lambda d=d: ref(d, "c100") == CR._report(CR.FOUND, 1, 86, 86, 0, 100, 0, 100)
        and set(control_diagonals(d, c100, 4)[3].tolist()) == {85})
    add("vote/draft_is_rc_of_control_M64", rc(c64), "c64", lambda: ref(rc(c64), "c64") == CR._report(CR.FOUND, 1, 50, 50, 0, 64, 0, 64))
    # ---- matched counts distinct control positions; the bitmap's words
    d = np.concatenate([c64, c64])
    add("matched/two_copies_of_one_stretch", d, "c64", lambda d=d: ref(d, "c64") == CR._report(CR.FOUND, 0, 100, 50, 0, 64, 0, 128))
    ok = lambda d: sorted(control_diagonals(d, c64, 4)[2].tolist()) == [0, 31, 32, 49] and ref(d, "c64") == CR._report(CR.FOUND, 0, 4, 4, 0, 64, 100, 164)
    add("matched/control_positions_0_31_32_and_last",
        retry(lambda: np.concatenate([jk(100, c64), c64[0:15], jk(16, c64), c64[31:47], jk(2, c64), c64[49:64], jk(20, c64)]), ok), "c64", ok)
    # ---- lengths and shares
    d = jk(14, c64)
    add("len/L14", d, "c64", lambda d=d: ref(d, "c64") == CR._report(CR.NONE))
    d = c64[20:35].copy()
    add("len/L15_one_hit", d, "c64", lambda d=d: ref(d, "c64") == CR._report(CR.FOUND, 0, 1, 1, 20, 35, 0, 15))
    for npos in (255, 256, 257):
        d = c4096[2000:2000 + npos + K - 1].copy()
        add(f"len/npos{npos}_every_position_hits", d, "c4096",
            lambda d=d, npos=npos: ref(d, "c4096") == CR._report(CR.FOUND, 0, npos, npos, 2000, 2000 + npos + 14, 0, npos + 14)
            and thread_share(npos, NT, NT - 1)[1] == npos)
    # ---- FOUND: the three conditions met exactly and missed by one
    d1 = c100[20:70].copy()
    add("found/all_three_met_exactly", d1, "c100/v", lambda: ref(d1, "c100/v") == CR._report(CR.FOUND, 0, 36, 36, 20, 70, 0, 50) and 10 * 50 == 5 * 100)
    add("found/matched_one_short", d1, "c100/v_matched+1", lambda: ref(d1, "c100/v_matched+1")["verdict"] == CR.NONE)
    d2 = c100[20:69].copy()
    add("found/control_extent_one_short", d2, "c100/v_matched-1", lambda: ref(d2, "c100/v_matched-1") == CR._report(CR.NONE, 0, 35, 35, 20, 69, 0, 49))
    d3 = np.concatenate([c100[20:70], [3 - c100[70]]]).astype(np.uint8)
    add("found/draft_extent_one_short_of_10_tenths", d3, "c100/v", lambda: ref(d3, "c100/v") == CR._report(CR.NONE, 0, 36, 36, 20, 70, 0, 50))
    add("found/tenths_0", d3, "c100/v_tenths0", lambda: ref(d3, "c100/v_tenths0")["verdict"] == CR.FOUND)
    d4 = c4096[100:500].copy()
    add("found/draft_tenths_10_max_occ_64", d4, "c4096/occ64_tenths10", lambda: ref(d4, "c4096/occ64_tenths10") == CR._report(CR.FOUND, 0, 386, 386, 100, 500, 0, 400))
    return LimitSet(cs, req).finish()


def control_expect(d, rq) -> dict:
    want = CR.screen(d, rq["control"], rq["opts"])
    if len(d) <= BRUTE_SCREEN and len(rq["control"]) <= 200:
        bf = CR.screen_bruteforce(d, rq["control"], rq["opts"])
        assert bf == want, (len(d), rq["opts"], bf, want)
    return want


# ================================================================ k_adapter
@dataclass(frozen=True)
class AdapterKnobs:
    own_ge: bool = False        # a lane owns the runs whose first position is >= lo: the run that starts at lo is found twice
    warm_m: bool = False        # the fresh start lies m, not m + k, bases before the chunk
    last_min: bool = False      # the run's end is its last minimum
    max_x: bool = False         # the start is the largest x that reaches dist
    k_ceil: bool = False        # k = ceil(m pct / 100)
    by_start: bool = False      # the list is ordered by (start, search)
    overflow_ge: bool = False   # the overflow pass is entered at n_hits >= 1024 (EQUIVALENT, see ADAPTER_EQUIVALENT)
    gap_no_lead: bool = False   # max_gap without the stretch before the first hit
    gap_no_trail: bool = False  # max_gap without the stretch after the last hit


ADAPTER_DEFAULT = AdapterKnobs()
ADAPTER_MUTANTS = {"own>=lo": AdapterKnobs(own_ge=True), "warm-m": AdapterKnobs(warm_m=True), "last-min": AdapterKnobs(last_min=True), "max-x": AdapterKnobs(max_x=True),
                   "k-ceil": AdapterKnobs(k_ceil=True), "by-start": AdapterKnobs(by_start=True), "gap-no-lead": AdapterKnobs(gap_no_lead=True),
                   "gap-no-trail": AdapterKnobs(gap_no_trail=True)}
# Not a mutant of the report: the overflow pass repeats the scan for the hits that end at or before the 16th distinct end and lists the 16 smallest keys among them;
# with exactly 1024 hits the buffer already holds every key, the 16 smallest of all keys end at or before the 16th distinct end, so both ways list the same 16.
# The pass entered one hit early costs time, not a value: no draft kills it, and the 1024 / 1025 cases pin what can be pinned, the report on either side.
ADAPTER_EQUIVALENT = {"overflow>=1024": AdapterKnobs(overflow_ge=True)}


def lane_rows(p, d, starts, W: int) -> np.ndarray:
    """rows[c, t] = E of a fresh start at starts[c] after t draft bases, t = 0 .. W (positions beyond the draft's end read a base that matches nothing)"""
    p, d = np.asarray(p, np.int64), np.asarray(d, np.int64)
    ext = np.concatenate([d, np.full(W, 4, np.int64)])
    seg = ext[np.asarray(starts)[:, None] + np.arange(W)[None, :]]
    tt = np.arange(W + 1)
    row = np.zeros((len(starts), W + 1), np.int64)
    for i in range(1, len(p) + 1):
        t = np.empty_like(row)
        t[:, 0] = i
        t[:, 1:] = np.minimum(row[:, 1:] + 1, row[:, :-1] + (seg != p[i - 1]))
        row = np.minimum.accumulate(t - tt, axis=1) + tt
    return row


def lane_hits(p, d, k: int, s: int, kn: AdapterKnobs = ADAPTER_DEFAULT) -> list:
    """the hits (start, end, search, dist) of one search as k_adapter's lanes find them: lane c of 128-base chunks starts fresh m + k bases before lo = 128 c,
    owns the runs whose first position lies in (lo, hi], and follows an owned run until it closes"""
    m, L = len(p), len(d)
    nch = (L + CHUNK - 1) // CHUNK
    if nch == 0:
        return []
    warm = m + (0 if kn.warm_m else k)
    starts = [max(0, c * CHUNK - warm) for c in range(nch)]
    W = CHUNK + warm + m + k + 8
    while True:
        rows = lane_rows(p, d, starts, W)
        out, short = [], False
        for c in range(nch):
            lo, hi, j0 = c * CHUNK, min(L, (c + 1) * CHUNK), starts[c]
            E = rows[c]
            own, best, end = False, 0, 0
            first = max(lo if kn.own_ge else lo + 1, j0 + 1)
            prev = first - 1 > j0 and E[first - 1 - j0] <= k
            jj = first
            while jj <= L:
                if jj - j0 > W:
                    short = True
                    break
                e = int(E[jj - j0])
                ok = e <= k
                if ok and not prev:
                    own, best, end = True, e, jj
                elif ok and own and (e <= best if kn.last_min else e < best):
                    best, end = e, jj
                elif not ok and prev and own:
                    out.append((end, best))
                    own = False
                if jj >= hi and not own:
                    break
                prev = ok
                jj += 1
            else:
                if own:
                    out.append((end, best))
            if short:
                break
        if not short:
            break
        W *= 2
    hits = []
    for end, dist in out:
        lo_, hi_ = max(0, m - dist), min(end, m + dist)
        a = AR.anchored(np.asarray(p)[::-1], np.asarray(d[end - hi_:end])[::-1])
        xs = [x for x in range(lo_, hi_ + 1) if a[x] == dist]
        x = (xs[-1] if kn.max_x else xs[0]) if xs else hi_
        hits.append((end - x, end, s, dist))
    return hits


def adapter_k(d, adapters, opts=None, kn: AdapterKnobs = ADAPTER_DEFAULT) -> dict:
    """adapter_ref.screen as k_adapter evaluates it, under the knobs"""
    o = AR._opts(opts)
    L = len(d)
    hits = []
    for s, p in enumerate(AR.searches(adapters)):
        k = -(-len(p) * o["max_dist_pct"] // 100) if kn.k_ceil else len(p) * o["max_dist_pct"] // 100
        hits += lane_hits(p, d, k, s, kn)
    every = sorted(hits, key=lambda h: (h[1], h[2]))
    union = np.zeros(L, bool)
    for st, e, _, _ in every:
        union[st:e] = True
    cov = np.flatnonzero(union)
    gaps = np.diff(np.concatenate([[-1], cov, [L]])) - 1             # the stretches before, between and behind the covered bases
    if len(cov) and kn.gap_no_lead:
        gaps = gaps[1:]
    if len(cov) and kn.gap_no_trail:
        gaps = gaps[:-1]
    best = int(gaps.max()) if len(gaps) else 0
    n = len(every)
    first = min((h[0] for h in every), default=-1)
    last = max((h[1] for h in every), default=-1)
    v = 0
    if n >= o["min_copies"] and best <= o["max_insert"]:
        v |= AR.CONCAT
    if n >= 1 and (first <= o["end_slack"] or last >= L - o["end_slack"]):
        v |= AR.NEAR_END
    listed = every
    if n > BUF or (kn.overflow_ge and n >= BUF):                     # the overflow pass: the keys of the hits up to the 16th distinct end
        ends = sorted({h[1] for h in every})
        bound = ends[LISTED - 1] if len(ends) >= LISTED else L
        listed = [h for h in every if h[1] <= bound]
    if kn.by_start:
        listed = sorted(listed, key=lambda h: (h[0], h[2]))
    return dict(tested=1, verdict=v, n_hits=n, n_listed=min(n, LISTED), covered=int(union.sum()), max_gap=best, first_start=first, last_end=last,
                min_dist=min((h[3] for h in every), default=255), hits=[tuple(int(x) for x in h) for h in listed[:LISTED]])


def every_hit(d, adapters, opts) -> list:
    """every hit of the restatement in (end, search) order, the unlisted ones included"""
    o = AR._opts(opts)
    out = []
    for s, p in enumerate(AR.searches(adapters)):
        out += AR.search_hits(p, d, len(p) * o["max_dist_pct"] // 100, s)[0]
    return sorted(out, key=lambda h: (h[1], h[2]))


def first_positions(d, p, k) -> list:
    """the first position of every run of one search"""
    return [a for a, _ in runs_of(AR.distance_row(p, d), k)]


A_OPTS = dict(max_dist_pct=0, min_copies=2, max_insert=30, end_slack=7)


def far_from(rng, n: int, pats, k_of) -> np.ndarray:
    """n random bases without a hit of any of the patterns (both orientations) at the distances k_of(m)"""
    while True:
        x = rng.integers(0, 4, n).astype(np.uint8)
        if all(AR.distance_row(p, x)[1:].min(initial=99) > k_of(len(p)) + 1 for p in AR.searches(pats)):
            return x


@functools.lru_cache(maxsize=None)
def adapter_cases() -> LimitSet:
    rng = np.random.default_rng(1503)
    rnd = lambda n: rng.integers(0, 4, n).astype(np.uint8)
    a16, a64 = rnd(16), rnd(64)
    p16 = np.tile(np.array([0, 1], np.uint8), 8)
    h = rnd(16)
    s32 = np.concatenate([h, rc(h)])                                # its own reverse complement
    eight = [a16, a64, p16, s32, rnd(20), a64[10:34].copy(), rnd(40), rnd(48)]      # (the sixth lies inside the second: hits whose end and start orders differ)
    U = rnd(80)
    U[32:64] = s32
    unit_set = [np.tile(U, 2)[10 * q + 66:10 * q + 82] for q in range(7)] + [s32]      # seven 16-base windows of the unit and the 32-base palindrome in it
    req = {"a16/k0": dict(adapters=[a16], opts=A_OPTS), "a16/k0/copies+1": dict(adapters=[a16], opts=dict(A_OPTS, min_copies=3)),
           "a16/k0/insert-1": dict(adapters=[a16], opts=dict(A_OPTS, max_insert=29)), "a16/k0/slack-1": dict(adapters=[a16], opts=dict(A_OPTS, end_slack=6)),
           "a16/k3": dict(adapters=[a16], opts=dict(A_OPTS, max_dist_pct=20)), "a64/k0": dict(adapters=[a64], opts=A_OPTS),
           "a64/k19": dict(adapters=[a64], opts=dict(A_OPTS, max_dist_pct=30)), "eight/k0": dict(adapters=eight, opts=A_OPTS),
           "eight/pct20": dict(adapters=eight, opts=dict(A_OPTS, max_dist_pct=20)), "p16/k1": dict(adapters=[p16], opts=dict(A_OPTS, max_dist_pct=10)),
           "unit/k1": dict(adapters=unit_set, opts=dict(A_OPTS, max_dist_pct=10))}
    ref = lambda d, r: AR.screen(d, req[r]["adapters"], req[r]["opts"])
    allh = lambda d, r: every_hit(d, req[r]["adapters"], req[r]["opts"])
    jk = lambda n: far_from(rng, n, [a16, a64], lambda m: m * 30 // 100)
    cs = []
    add = lambda *a, **k: cs.append(Case(*a, **k))

    def exact(r, want, make):
        """a draft whose hits under request r are exactly `want`"""
        ok = lambda d: allh(d, r) == want
        return retry(make, ok), ok

    # ---- draft and pattern sizes
    d = jk(10)
    add("size/L_is_min_length", d, "a16/k3", lambda d=d: len(d) == 10 and ref(d, "a16/k3")["n_hits"] == 0 and ref(d, "a16/k3")["max_gap"] == 10)
    d = a64[:40].copy()
    add("size/L_below_m", d, "a64/k19", lambda d=d: len(d) < 64 and ref(d, "a64/k19")["n_hits"] == 0)
    add("size/L_is_m", a64.copy(), "a64/k19", lambda: allh(a64, "a64/k19") == [(0, 64, 0, 0)] and ref(a64, "a64/k19")["max_gap"] == 0)
    for L in (127, 128, 129):
        d, ok = exact("a16/k0", [(L - 16, L, 0, 0)], lambda L=L: np.concatenate([jk(L - 16), a16]))
        add(f"size/L{L}_hit_ends_at_L", d, "a16/k0", ok)
    # ---- the warm-up: k inserted bases, distance k exactly over m + k draft bases, the hit ending at lo and at lo + 1
    def inserted(p, k):
        at = np.sort(rng.choice(np.arange(2, len(p) - 1), k, replace=False))
        out = []
        for q, b in enumerate(p):
            if q in at:
                out.append(3 - int(p[q]) if p[q] != p[q - 1] else (int(p[q]) + 1) & 3)
            out.append(int(b))
        return np.array(out, np.uint8)
    for nm, r, p, k in (("m16_k3", "a16/k3", a16, 3), ("m64_k19", "a64/k19", a64, 19)):
        for end in (128, 129):
            w = len(p) + k
            d, ok = exact(r, [(end - w, end, 0, k)], lambda p=p, k=k, end=end, w=w: np.concatenate([jk(end - w), inserted(p, k), jk(60)]))
            add(f"warm/{nm}_spans_m_plus_k_ends_at_{end}", d, r, ok)
    d = cs[-1].draft[129 - 83:129].copy()
    add("size/L_is_m_plus_k", d, "a64/k19", lambda d=d: len(d) == 64 + 19 and allh(d, "a64/k19") == [(0, 83, 0, 19)])
    # ---- k = 0 and the top bit of a 64-base pattern
    d, ok = exact("a64/k0", [(30, 94, 0, 0), (100, 164, 1, 0)], lambda: np.concatenate([jk(30), a64, jk(6), rc(a64), jk(20)]))
    add("pat/m64_k0_both_orientations_three_words", d, "a64/k0", ok)
    # ---- ownership at the chunk edge lo = 128 (k = 3: an exact copy that ends at e gives the run [e - 3, e + 3])
    for nm, e, first in (("run_starts_at_lo", 131, 128), ("run_starts_at_lo_plus_1", 132, 129), ("run_starts_in_chunk_0_minimum_in_chunk_1", 130, 127)):
        d, ok = exact("a16/k3", [(e - 16, e, 0, 0)], lambda e=e: np.concatenate([jk(e - 16), a16, jk(40)]))
        add(f"own/{nm}", d, "a16/k3", lambda d, ok=ok, e=e, first=first: ok(d) and first_positions(d, a16, 3) == [first] and adapter_chunk(first) == (first - 1) // 128
            and adapter_chunk(e) == 1)
    d, ok = exact("a16/k0", [(112, 128, 0, 0)], lambda: np.concatenate([jk(112), a16, jk(40)]))
    add("own/k0_run_is_position_lo", d, "a16/k0", lambda d, ok=ok: ok(d) and adapter_chunk(128) == 0 and adapter_chunk(129) == 1)
    d, ok = exact("a16/k0", [(113, 129, 0, 0)], lambda: np.concatenate([jk(113), a16, jk(40)]))
    add("own/k0_run_is_position_lo_plus_1", d, "a16/k0", ok)
    d, ok = exact("a16/k0", [(0, 16, 0, 0)], lambda: np.concatenate([a16, jk(40)]))
    add("own/hit_starts_at_base_0", d, "a16/k0", ok)
    d = np.concatenate([jk(100), np.tile(np.array([0, 1], np.uint8), 150), jk(60)])
    add("own/run_spans_whole_chunks", d, "p16/k1",
        lambda d=d: [(a, b) for a, b in runs_of(AR.distance_row(p16, d), 1) if b - a > 256] and len(runs_of(AR.distance_row(p16, d), 1)) == 1
        and adapter_chunk(runs_of(AR.distance_row(p16, d), 1)[0][0]) == 0 and adapter_chunk(runs_of(AR.distance_row(p16, d), 1)[0][1]) == 3)
    d = np.concatenate([jk(150), a16[:15]])
    add("own/run_open_at_the_drafts_end", d, "a16/k3", lambda d=d: runs_of(AR.distance_row(a16, d), 3)[-1][1] == len(d) and ref(d, "a16/k3")["last_end"] == len(d))
    # ---- runs, ends and starts
    d = np.concatenate([jk(40), np.tile(np.array([0, 1], np.uint8), 9), jk(40)])
    add("run/two_runs_one_position_apart", d, "eight/k0", lambda d=d: [h[:2] for h in allh(d, "eight/k0") if h[2] == 4] == [(40, 56), (42, 58)])
    sub = a16.copy()
    sub[0] = 3 - sub[0]
    sub[15] = 3 - sub[15]                                            # first and last base substituted: starts 15 and 16 back tie, ends e - 1 and e tie
    ok = lambda d: allh(d, "a16/k3") == [(51, 65, 0, 2)] and AR.distance_row(a16, d)[65] == AR.distance_row(a16, d)[66] == 2 \
        and adapter_k(d, [a16], req["a16/k3"]["opts"], AdapterKnobs(last_min=True))["hits"][0][1] == 66 \
        and adapter_k(d, [a16], req["a16/k3"]["opts"], AdapterKnobs(max_x=True))["hits"][0][0] == 50
    add("run/two_ends_and_two_starts_tie", retry(lambda: np.concatenate([jk(50), sub, jk(50)]), ok), "a16/k3", ok)
    # ---- eight adapters; one is its own reverse complement: both searches hit the same span
    d, ok = exact("eight/k0", [(30, 62, 6, 0), (30, 62, 7, 0)], lambda: np.concatenate([jk(30), s32, jk(30)]))
    add("set/palindromic_adapter_two_hits_one_span", d, "eight/k0", ok)
    d = np.concatenate([jk(12)] + [np.concatenate([x, jk(9)]) for x in eight] + [rc(eight[7]), jk(15)])
    add("set/every_adapter_once", d, "eight/pct20", lambda d=d: sorted({h[2] for h in allh(d, "eight/pct20")}) == [0, 2, 4, 6, 7, 8, 10, 12, 14, 15]
        and ref(d, "eight/pct20")["min_dist"] == 0)
    d, ok = exact("eight/k0", [(30, 54, 10, 0), (20, 84, 2, 0)], lambda: np.concatenate([jk(20), a64, jk(20)]))
    add("list/ordered_by_end_not_by_start", d, "eight/k0", ok)
    far = a16.copy()
    far[[2, 6, 10, 13]] = 3 - far[[2, 6, 10, 13]]                     # four substitutions: k = floor(16 * 20 / 100) = 3 leaves no hit, a k of 4 would
    d = retry(lambda: np.concatenate([jk(30), far, jk(30)]), lambda d: AR.distance_row(a16, d)[1:].min() == 4)
    add("pat/k_is_rounded_down", d, "a16/k3", lambda d=d: AR.distance_row(a16, d)[1:].min() == 4 and 16 * 20 // 100 == 3 and ref(d, "a16/k3")["n_hits"] == 0)
    # ---- the list: 16 and 17 hits
    for n in (16, 17):
        want = [(5 + 22 * q, 21 + 22 * q, 0, 0) for q in range(n)]
        d, ok = exact("a16/k0", want, lambda n=n: np.concatenate([jk(5)] + [np.concatenate([a16, jk(6)]) for _ in range(n)]))
        add(f"list/{n}_hits", d, "a16/k0", lambda d, ok=ok, n=n: ok(d) and ref(d, "a16/k0")["n_listed"] == 16 and ref(d, "a16/k0")["n_hits"] == n)
    # ---- the union's words and max_gap's places
    d, ok = exact("eight/k0", [(32, 64, 6, 0), (32, 64, 7, 0)], lambda: np.concatenate([jk(32), s32, jk(40)]))
    add("union/exactly_one_word", d, "eight/k0", ok)
    d, ok = exact("a16/k0", [(16, 32, 0, 0)], lambda: np.concatenate([jk(16), a16, jk(300)]))
    add("union/ends_on_bit_31_gap_at_the_end_over_many_shares", d, "a16/k0",
        lambda d, ok=ok: ok(d) and ref(d, "a16/k0")["max_gap"] == 300 and len(d) == 332 and thread_share(332, NT, 16) == (32, 34))
    d, ok = exact("a16/k0", [(300, 316, 0, 0)], lambda: np.concatenate([jk(300), a16]))
    add("gap/at_the_start", d, "a16/k0", lambda d, ok=ok: ok(d) and ref(d, "a16/k0")["max_gap"] == 300)
    d, ok = exact("a16/k0", [(40, 56, 0, 0), (96, 112, 0, 0)], lambda: np.concatenate([jk(40), a16, jk(40), a16, jk(30)]))
    add("gap/L_below_256_empty_shares", d, "a16/k0", lambda d, ok=ok: ok(d) and len(d) == 142 and thread_share(142, NT, 200) == (142, 142) and ref(d, "a16/k0")["max_gap"] == 40)
    d = np.tile(a16, 9)
    add("gap/draft_covered_entirely", d, "a16/k0", lambda d=d: ref(d, "a16/k0")["max_gap"] == 0 and ref(d, "a16/k0")["covered"] == 144 and ref(d, "a16/k0")["n_hits"] == 9)
    # ---- the verdict: A_OPTS is met exactly in min_copies, max_insert and end_slack, at the near end and at the far end
    dn, ok = exact("a16/k0", [(7, 23, 0, 0), (53, 69, 0, 0)], lambda: np.concatenate([jk(7), a16, jk(30), a16, jk(12)]))
    add("verdict/near_end_all_met_exactly", dn, "a16/k0", lambda d, ok=ok: ok(d) and ref(d, "a16/k0")["verdict"] == 3 and ref(d, "a16/k0")["max_gap"] == 30
        and ref(d, "a16/k0/copies+1")["verdict"] == 2 and ref(d, "a16/k0/insert-1")["verdict"] == 2 and ref(d, "a16/k0/slack-1")["verdict"] == 1)
    for r in ("a16/k0/copies+1", "a16/k0/insert-1", "a16/k0/slack-1"):
        add(f"verdict/near_end_under_{r[7:]}", dn, r, lambda: True)
    df, ok = exact("a16/k0", [(12, 28, 0, 0), (58, 74, 0, 0)], lambda: np.concatenate([jk(12), a16, jk(30), a16, jk(7)]))
    add("verdict/far_end_met_exactly", df, "a16/k0", lambda d, ok=ok: ok(d) and ref(d, "a16/k0")["verdict"] == 3 and ref(d, "a16/k0/slack-1")["verdict"] == 1
        and ref(d, "a16/k0")["last_end"] == len(d) - 7)
    # ---- exactly 1024 and 1025 hits: copies of the 80-base unit, a fixed number of hits a copy (the windows, the palindrome twice), a partial copy, one more window
    nh = lambda d: AR.screen(d, unit_set, req["unit/k1"]["opts"])["n_hits"]
    body = lambda off, n, cut: np.concatenate([U[off:], np.tile(U, n), U[:cut]])
    shared16 = lambda hs: len({x[1] for x in hs}) >= LISTED and sum(1 for x in hs if x[1] == sorted({y[1] for y in hs})[LISTED - 1]) >= 2
    off = next(f for f in range(80) if shared16(allh(body(f, 3, 0), "unit/k1")))      # the draft starts inside a copy so that the 16th end is the palindrome's
    small, three = nh(body(off, 2, 0)), nh(body(off, 3, 0))                         # (every further copy adds three - small hits)
    n = 2 + (BUF - small) // (three - small)
    base = nh(body(off, n, 0))
    by_count = {}
    for c in range(80):                                              # (the hits of the partial copy, counted on a short draft; the full draft is checked below)
        by_count.setdefault(base + nh(body(off, 2, c)) - small, c)
    for want, nm in ((BUF, "list/1024_hits"), (BUF + 1, "list/1025_hits_16th_end_shared")):
        d = body(off, n, by_count[want])
        add(nm, d, "unit/k1", lambda d=d, want=want: ref(d, "unit/k1")["n_hits"] == want and shared16(allh(d, "unit/k1")), batch="long")
    return LimitSet(cs, req).finish()


def adapter_expect(d, rq) -> dict:
    want = AR.screen(d, rq["adapters"], rq["opts"])
    if len(d) <= BRUTE_SCREEN and len(d) * sum(len(a) ** 2 for a in rq["adapters"]) <= 600 * 64 * 64:
        bf = AR.screen_bruteforce(d, rq["adapters"], rq["opts"])
        assert bf == want, (len(d), rq["opts"], bf, want)
    return want

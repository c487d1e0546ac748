"""The representative rule restated in numpy (DESIGN.md §2 "Representative rule"): class, pass and every written byte, from the section's words alone — the
median is a sort of (length, index) tuples, not the library's rank count.  Plus what the tests share: batches built pass by pass, poisoned result planes, a
plane-for-plane comparison, and the limit set."""
from __future__ import annotations

import copy

import numpy as np

from ccs_amd import api

POLISHED, NONE, DRAFT, SUBREAD = 0, 1, 2, 3
QV = 10
MAX_PASSES = 255
SUCCESS, TOO_FEW_PASSES, DRAFT_FAILURE, TOO_MANY_UNUSABLE, NON_CONVERGENT, TOO_SHORT, TOO_LONG, LOW_RQ, EMPTY_WINDOW, CAPACITY, HETERODUPLEX = range(11)
PARTIAL, REVERSE = 2, 1
POISON = 0xA5
ZMW_FIELDS = ("status", "seq_len", "rq", "np_", "ec", "iters", "n_windows", "fn", "rn")
PLANE_FIELDS = ("seq", "qual", "raw_qv", "kin")
LENGTHS = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 3001)


def make_batch(zmws, seed=0, high_bits=False) -> api.Batch:
    """zmws: per ZMW a list of (bases, flag).  pw 1 .. 3 and ipd 1 .. 60 are random; high_bits: the base bytes carry random bits above the low two"""
    rng = np.random.default_rng(seed)
    read_off, base_off, flags, bases = [0], [0], [], [np.zeros(0, np.uint8)]
    for passes in zmws:
        for b, f in passes:
            b = np.asarray(b, np.uint8)
            bases.append(b | (rng.integers(0, 64, len(b)).astype(np.uint8) << 2) if high_bits else b)
            flags.append(f); base_off.append(base_off[-1] + len(b))
        read_off.append(read_off[-1] + len(passes))
    n, nb = len(zmws), base_off[-1]
    return api.Batch(np.arange(n, dtype=np.int32), np.ascontiguousarray(np.tile(np.array([9.0, 16.0, 8.0, 13.0], np.float32), (n, 1))),
                     np.array(read_off, np.int32), np.array(base_off, np.int64), np.ascontiguousarray(np.concatenate(bases), np.uint8),
                     rng.integers(1, 4, nb).astype(np.uint8), rng.integers(1, 61, nb).astype(np.uint8), np.array(flags, np.uint8).reshape(len(flags)))


def nall_of(n_passes: int, top_passes: int) -> int:
    return min(n_passes, MAX_PASSES if top_passes <= 0 or top_passes > MAX_PASSES else top_passes)


def classify(st: int, nall: int, Ld: int, slot: int, fallback: bool) -> int:
    if st in (SUCCESS, LOW_RQ):
        return POLISHED
    if nall == 0 or st in (TOO_SHORT, TOO_LONG):
        return NONE
    if Ld > 0 and st != TOO_FEW_PASSES and not fallback:
        return DRAFT if Ld <= slot else NONE
    return SUBREAD


def median_pass(lens, flags) -> int:
    """the pass of rank |C| // 2 among C in (length, index) order: a sort of tuples"""
    full = [(int(l), q) for q, (l, f) in enumerate(zip(lens, flags)) if not f & PARTIAL]
    C = full if full else [(int(l), q) for q, l in enumerate(lens)]
    return sorted(C)[len(C) // 2][1]


def apply(batch: api.Batch, top_passes: int, status, drafts, res: api.Results, fallback=False, kinetics=False):
    """the rule applied in place to res; returns (cls [n], pass [n])"""
    n = batch.n_zmw
    cls, pas = np.zeros(n, np.int32), np.full(n, -1, np.int32)
    for z in range(n):
        r0 = int(batch.read_off[z])
        nall = nall_of(int(batch.read_off[z + 1]) - r0, top_passes)
        so, slot = int(res.seq_off[z]), int(res.seq_off[z + 1] - res.seq_off[z])
        c = cls[z] = classify(int(status[z]), nall, len(drafts[z]), slot, fallback)
        if c in (POLISHED, NONE):
            continue
        if c == DRAFT:
            src = np.asarray(drafts[z], np.uint8) & 3
        else:
            lens = [int(batch.base_off[r0 + q + 1] - batch.base_off[r0 + q]) for q in range(nall)]
            p = pas[z] = median_pass(lens, batch.flags[r0:r0 + nall])
            b0 = int(batch.base_off[r0 + p])
            src = batch.bases[b0:b0 + lens[p]] & 3
            if kinetics and res.kin is not None:
                res.kin[0, so:so + lens[p]] = batch.ipd[b0:b0 + lens[p]]
                res.kin[1, so:so + lens[p]] = batch.pw[b0:b0 + lens[p]]
        L = len(src)
        res.seq[so:so + L] = src
        res.qual[so:so + L] = QV
        if res.raw_qv is not None:
            res.raw_qv[so:so + L] = float(QV)
        res.seq_len[z], res.rq[z], res.ec[z] = L, -1.0, 0.0
    return cls, pas


def poisoned_results(batch: api.Batch, kinetics=False, raw=True) -> api.Results:
    """Results on the batch's capacity layout whose every output byte is POISON (seq_off is the layout)"""
    res = api.Results.allocate(batch, kinetics=kinetics, raw=raw)
    for f in ZMW_FIELDS + PLANE_FIELDS:
        a = getattr(res, f)
        if a is not None:
            a.view(np.uint8)[...] = POISON
    return res


def clone(res: api.Results) -> api.Results:
    return copy.deepcopy(res)


def diff(a: api.Results, b: api.Results) -> list:
    """the arrays of a and b that differ in some byte, whole planes (so that a byte written where none should be shows)"""
    out = []
    for f in ("seq_off",) + ZMW_FIELDS + PLANE_FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        if (x is None) != (y is None) or (x is not None and x.tobytes() != y.tobytes()):
            out.append(f)
    return out


def diff_zmw(a: api.Results, b: api.Results, z: int) -> list:
    """the fields of ZMW z that differ: its per-ZMW words and its whole slot in every plane"""
    out = [f for f in ZMW_FIELDS if getattr(a, f)[z].tobytes() != getattr(b, f)[z].tobytes()]
    lo, hi = int(a.seq_off[z]), int(a.seq_off[z + 1])
    for f in PLANE_FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        if x is not None and y is not None and x[..., lo:hi].tobytes() != y[..., lo:hi].tobytes():
            out.append(f)
    return out


def limit_cases(seed=11) -> list:
    """(name, zmws, top_passes, status [n], drafts [n]): every case a small batch of its own"""
    rng = np.random.default_rng(seed)
    rnd = lambda L: rng.integers(0, 4, int(L)).astype(np.uint8)
    full = lambda L, rev=0: (rnd(L), rev)
    part = lambda L, rev=0: (rnd(L), PARTIAL | rev)
    cases = []
    # every status, on a ZMW of two full-length passes and a partial one with a draft of 40 bases, and again without a draft
    z3 = lambda: [full(37), full(41, 1), part(20)]
    cases.append(("statuses", [z3() for _ in range(22)], 0, list(range(11)) * 2, [rnd(40)] * 11 + [rnd(0)] * 11))
    # nall 0 / 1 / 2 / 255 / 260 (the cut to 255: the 256th and later passes are the longest and the only full-length ones, they must not count)
    many = lambda k: [part(5 + (q * 7) % 23, q & 1) for q in range(k)]
    cut = many(255) + [full(90) for _ in range(5)]
    cases.append(("nall", [[], [full(30)], [full(30), full(29, 1)], many(255), cut, [p for p in many(255)[:-1]] + [full(12, 1)]], 0,
                  [TOO_FEW_PASSES] * 5 + [DRAFT_FAILURE], [rnd(0)] * 6))
    cases.append(("top_passes_2", [[full(50), full(40), full(30), full(20), full(10)], [part(9), part(8), full(7)]], 2, [TOO_MANY_UNUSABLE, TOO_FEW_PASSES],
                  [rnd(0), rnd(0)]))
    # nfull 0 / 1 / 2 with 0 .. 4 partial passes
    zs = [[full(30 + q, q & 1) for q in range(nf)] + [part(60 + 3 * q, q & 1) for q in range(npart)] for nf in (0, 1, 2) for npart in range(5)]
    cases.append(("nfull", zs, 0, [TOO_FEW_PASSES] * len(zs), [rnd(0)] * len(zs)))
    # ties at the median: the earlier and the later index of two equal lengths, all equal, |C| even and odd, the representative on the reverse strand
    tie = [[full(5), full(7), full(7, 1)], [full(7), full(7, 1), full(9)], [full(7)] * 4, [full(7, 1)] * 5, [full(9), full(7), full(7), full(5, 1)],
           [full(8), full(6, 1), full(7), full(6, 1), full(9), full(6)], [part(7, 1), part(7), part(7, 1)]]
    tie = [[(rnd(len(b)), f) for b, f in z] for z in tie]
    cases.append(("ties", tie, 0, [DRAFT_FAILURE] * len(tie), [rnd(0)] * len(tie)))
    # draft and pass lengths around the 16-byte words of the copy, and one of a few thousand; the slot offsets move the alignment of source and destination
    zs, dr, st = [], [], []
    for k, L in enumerate(LENGTHS):
        zs.append([full(L, k & 1)] + [part(3 + k)] * (k % 3)); dr.append(rnd(0)); st.append(TOO_FEW_PASSES)         # SUBREAD of L bases
        zs.append([full(L), full(max(1, L - 1), 1)]); dr.append(rnd(L + (L >> 2) + 64 if k & 1 else L)); st.append(TOO_MANY_UNUSABLE)   # DRAFT of L or of its whole slot
    cases.append(("lengths", zs, 0, st, dr))
    # a draft one base longer than its slot: NONE, never truncated; with the fallback: a subread
    cases.append(("draft_beyond_slot", [[full(10), full(8)], [full(10), full(8)]], 0, [TOO_MANY_UNUSABLE, NON_CONVERGENT], [rnd(10 + 2 + 64 + 1), rnd(10 + 2 + 64)]))
    return cases

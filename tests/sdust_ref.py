"""Restatement of the tandem-repeat rule (DESIGN.md §2 "Tandem repeats", rule version 1) for parity tests of k_sdust.

Symmetric DUST (Morgulis et al. 2006) over the triplets of a draft (codes 0..3):
  * triplet j = 16 s[j] + 4 s[j+1] + s[j+2], j = 0 .. L - 3;
  * an interval of l >= 2 triplets has S = sum_t c_t (c_t - 1) / 2 pairs of equal triplets and score S / (l - 1);
  * it lies in a window when it spans at most W = 64 bases, i.e. l <= W - 2;
  * it is a perfect interval when its score exceeds T / 10 = 2.0 (S * 10 > T * (l - 1)) and no sub-interval scores higher;
  * a base is masked when it lies in a perfect interval (triplet i covers bases i .. i + 2);
  * tandem_len = the longest run of masked bases (0 for L < 3).

`masked_incremental` follows k_sdust operation for operation (sequentially, one lane); `masked_bruteforce` applies the written
definition to every sub-interval of every window.  tests/test_tandem.py holds them equal and the GPU to them.
"""
from __future__ import annotations

import numpy as np

W = 64                 # window in bases
T = 20                 # threshold in tenths: score > 2.0
KMAX = W - 3           # most triplets - 1 of an interval inside a window


def triplets(seq) -> np.ndarray:
    s = np.asarray(seq, np.int64) & 3
    if len(s) < 3:
        return np.zeros(0, np.int64)
    return 16 * s[:-2] + 4 * s[1:-1] + s[2:]


def masked_incremental(seq, lo: int = 0, e0: int | None = None, e1: int | None = None, mask: np.ndarray | None = None) -> np.ndarray:
    """the kernel's loop for the ends [e0, e1) of one lane whose warm-up starts at triplet lo (defaults: the whole draft).  Returns the mask
    (bool per base); `mask` is ORed into when given."""
    seq = np.asarray(seq, np.int64) & 3
    Ld = len(seq)
    if mask is None:
        mask = np.zeros(Ld, bool)
    tri = triplets(seq)
    nt = len(tri)
    if e0 is None:
        e0, e1 = 1, nt
    best = [0] * 64                 # best perfect interval per start (ring slot start & 63): S << 8 | k, 0 = none
    win = {int(tri[lo]): 1} if nt > lo else {}      # triplet counts of the window [ilo, e]
    Sw = 0                          # its pairs of equal triplets
    for e in range(lo + 1, e1):
        if e - (W - 2) >= lo:       # triplet e - 62 leaves the window
            to = int(tri[e - (W - 2)])
            win[to] -= 1
            Sw -= win[to]
        tn = int(tri[e])
        Sw += win.get(tn, 0)
        win[tn] = win.get(tn, 0) + 1
        best[e & 63] = 0
        cnt = {int(tri[e]): 1}
        ilo = max(lo, e - KMAX)
        ilo = max(ilo, e - ((Sw - 1) >> 1 if Sw > 0 else 0))   # exact gate: a suffix has at most Sw pairs and needs S > 2k
        S = M = 0
        imn = -1
        for i in range(e - 1, ilo - 1, -1):
            k = e - i
            t = int(tri[i])
            c = cnt.get(t, 0)
            S += c
            cnt[t] = c + 1
            b = best[i & 63]
            if b and (not M or (b >> 8) * (M & 255) > (M >> 8) * (b & 255)):
                M = b
            if S * 10 > T * k and (not M or S * (M & 255) >= (M >> 8) * k):
                M = (S << 8) | k
                best[i & 63] = M
                imn = i
        if e >= e0 and imn >= 0:
            mask[imn:e + 3] = True
    return mask


def masked_lanes(seq, lanes: int = 64) -> np.ndarray:
    """the kernel's split: lane l owns ends [1 + l ch, 1 + (l + 1) ch) and warms up over the W - 3 ends before them"""
    seq = np.asarray(seq, np.int64) & 3
    mask = np.zeros(len(seq), bool)
    nt = len(seq) - 2
    if nt < 2:
        return mask
    ch = (nt - 1 + lanes - 1) // lanes
    for lane in range(lanes):
        e0 = 1 + lane * ch
        e1 = min(e0 + ch, nt)
        if e0 < e1:
            masked_incremental(seq, max(0, e0 - KMAX), e0, e1, mask)
    return mask


def pair_table(seq) -> tuple[np.ndarray, np.ndarray]:
    """S[i, k] = pairs of equal triplets in the interval of triplets [i, i + k] (counted directly), valid where i + k < nt"""
    tri = triplets(seq)
    nt = len(tri)
    S = np.full((max(nt, 1), KMAX + 1), -1, np.int64)
    for i in range(nt):
        for k in range(0, min(KMAX, nt - 1 - i) + 1):
            _, c = np.unique(tri[i:i + k + 1], return_counts=True)
            S[i, k] = int((c * (c - 1) // 2).sum())
    return S, tri


def perfect_intervals_bruteforce(seq) -> set:
    """every perfect interval (i, e) of triplets, from the definition: for every window of W bases and every interval inside it with
    l >= 2 triplets, score > T / 10 and no sub-interval (l >= 2) with a higher score"""
    S, tri = pair_table(seq)
    nt = len(tri)
    L = len(seq)
    out, seen = set(), set()
    for ws in range(0, max(1, L - W + 1)):           # window of bases [ws, ws + W): triplets [ws, min(ws + W, L) - 3]
        last = min(ws + W, L) - 3
        for i in range(ws, last + 1):
            for e in range(i + 1, last + 1):
                if (i, e) in seen:
                    continue
                seen.add((i, e))
                k = e - i
                s = S[i, k]
                if not s * 10 > T * k:
                    continue
                # every sub-interval [a, b] with b > a: S[a, b - a] / (b - a) <= s / k
                ok = True
                for a in range(i, e):
                    kk = np.arange(1, e - a + 1)
                    if np.any(S[a, kk] * k > s * kk):
                        ok = False
                        break
                if ok:
                    out.add((i, e))
    del nt
    return out


def masked_bruteforce(seq) -> np.ndarray:
    mask = np.zeros(len(seq), bool)
    for i, e in perfect_intervals_bruteforce(seq):
        mask[i:e + 3] = True
    return mask


def longest_run(mask) -> int:
    best = cur = 0
    for v in np.asarray(mask, bool):
        cur = cur + 1 if v else 0
        best = max(best, cur)
    return best


def tandem_len(seq) -> int:
    """the rule's tandem_len of one draft"""
    return longest_run(masked_incremental(seq)) if len(seq) >= 3 else 0


def revcomp(seq) -> np.ndarray:
    return (3 - (np.asarray(seq, np.int64) & 3))[::-1].astype(np.uint8)

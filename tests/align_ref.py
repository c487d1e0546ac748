"""The plain reference of the subread-to-draft alignment: UNBANDED global alignment scores in int64 numpy, nothing else.  It knows the SPEC's four scores (DESIGN.md §2:
match +3, mismatch -5, insertion -4, deletion -4) and what "entering a column" and "a clean position" mean; it knows no band, no band placement, no tie-break, no move
word and no window.  What it can say about the engine's (and the CPU restatement's) banded result is therefore independent of how either walks its band:

  F[i][j]   best score of read[:i] against draft[:j] (F[i][0] = -4 i: leading insertions), B[i][j] the same for read[i:] against draft[j:], OPT = F[I][Ld] = B[0][0]
  entry     "the path enters column j at row i" is optimal iff the best NON-insertion arrival at (i, j) plus B[i][j] is OPT — whichever optimal path was taken
  clean     position p can be clean (passed by a diagonal step with equal bases) on an optimal path only if some row i matches it there: F[i-1][p] + 3 + B[i][p+1] = OPT
"""
import numpy as np

MATCH, MISMATCH, INS, DEL = 3, -5, -4, -4
NEG = -(1 << 40)


def forward(read, draft):
    """F [I + 1, Ld + 1] int64, one column at a time: diagonal and deletion from the column before, then the insertion chain F[i][j] = max_k<=i (c_k - 4 (i - k)) as a running
    maximum of c_i + 4 i"""
    r, d = np.asarray(read, np.int64), np.asarray(draft, np.int64)
    I, L = len(r), len(d)
    i4 = -INS * np.arange(I + 1, dtype=np.int64)
    F = np.empty((I + 1, L + 1), np.int64)
    F[:, 0] = -i4
    for j in range(1, L + 1):
        prev = F[:, j - 1]
        c = prev + DEL
        c[1:] = np.maximum(c[1:], prev[:-1] + np.where(r == d[j - 1], MATCH, MISMATCH))
        F[:, j] = np.maximum.accumulate(c + i4) - i4
    return F


def backward(read, draft):
    """B [I + 1, Ld + 1]: the forward table of the reversed sequences, turned round"""
    return np.ascontiguousarray(forward(np.asarray(read)[::-1], np.asarray(draft)[::-1])[::-1, ::-1])


def entry_is_optimal(F, B, r, d, j, i):
    """some optimal alignment ENTERS column j (j draft bases consumed) at row i (i read bases consumed): arrives there by a diagonal or a deletion step — read bases inserted
    while the path waits in column j come after the entry.  Column 0 is entered at row 0."""
    I, L = len(r), len(d)
    if not (0 <= i <= I and 0 <= j <= L): return False
    if j == 0: return i == 0
    E = F[i][j - 1] + DEL
    if i >= 1: E = max(E, F[i - 1][j - 1] + (MATCH if r[i - 1] == d[j - 1] else MISMATCH))
    return bool(E + B[i][j] == F[I][L])


def clean_is_possible(F, B, r, d, p):
    """draft position p may be reported clean only if some read base equal to it is matched to it on an optimal alignment"""
    I, L = len(r), len(d)
    return any(r[i - 1] == d[p] and F[i - 1][p] + MATCH + B[i][p + 1] == F[I][L] for i in range(1, I + 1))


class Ref:
    """What the checks need of one pass's F and B, kept instead of the tables (a 2300 x 2300 pass has two 42 MB tables): OPT; per window-edge column the rows at which an optimal
    path can enter it; per draft position whether it can be clean; and the unbanded bounds of the split forms over the edge columns `need` —
      split    max over edge columns s and rows i1 <= i2 of F[i1][s] + B[i2][s] (a prefix, one block of read bases left out, a suffix)
      split2   the same with the prefix ending at edge s1 and the suffix starting at a later edge s2
      prefix / suffix (partial passes)  max over edge columns s >= 1 of max_i F[i][s] / over s < Ld of max_i B[i][s]"""

    def __init__(self, read, draft, need):
        r, d = np.asarray(read, np.int64), np.asarray(draft, np.int64)
        F, B = forward(r, d), backward(r, d)
        I, L = len(r), len(d)
        self.I, self.L, self.opt = I, L, int(F[I, L])
        assert self.opt == int(B[0, 0])
        self.need = [int(c) for c in need]
        self.entry_ok = {}
        for j in self.need:
            if j == 0:
                ok = np.zeros(I + 1, bool); ok[0] = True
            else:
                E = F[:, j - 1] + DEL
                E[1:] = np.maximum(E[1:], F[:-1, j - 1] + np.where(r == d[j - 1], MATCH, MISMATCH))
                ok = (E + B[:, j]) == self.opt
            self.entry_ok[j] = ok
        self.clean_ok = (((F[:-1, :-1] + MATCH + B[1:, 1:]) == self.opt) & (r[:, None] == d[None, :])).any(axis=0) if I and L else np.zeros(L, bool)
        pre = {s: np.maximum.accumulate(F[:, s]) for s in self.need}                  # best prefix score that ends at or above row i
        self.bound_split = max(int((pre[s] + B[:, s]).max()) for s in self.need)
        self.bound_split2, g = NEG, None
        for s in self.need:
            if g is not None: self.bound_split2 = max(self.bound_split2, int((g + B[:, s]).max()))
            g = pre[s] if g is None else np.maximum(g, pre[s])
        self.bound_prefix = max([int(F[:, s].max()) for s in self.need if s >= 1] or [NEG])
        self.bound_suffix = max([int(B[:, s].max()) for s in self.need if s < L] or [NEG])

    def bound(self, route):
        return {"split": self.bound_split, "split_s0": self.bound_split, "split_sLd": self.bound_split, "split2": self.bound_split2}.get(route, self.opt)


def check_pass(ref, route, valid, score, rs, dirty, suboptimal, partial=None, tag=""):
    """The independent properties of one pass's stage result (the engine's or the restatement's) against its Ref; `suboptimal`: the pass is on the lab's planted list, the
    only excuse from score == OPT.  Raises AssertionError naming the pass (tag) and the column."""
    if not valid: return
    covered = [j for j in ref.need if 0 <= int(rs[j]) <= ref.I]
    ent = [int(rs[j]) for j in covered]
    assert all(a <= b for a, b in zip(ent, ent[1:])), f"{tag}: entry rows decrease over the covered edges {list(zip(covered, ent))}"
    if route == "partial":
        b = ref.bound_suffix if partial else ref.bound_prefix
        assert score <= b, f"{tag}: partial score {score} above the unbanded bound {b}"
        return
    assert score <= ref.bound(route), f"{tag}: {route} score {score} above the unbanded bound {ref.bound(route)}"
    if route not in ("narrow", "wide_invalid", "wide_saturated", "wide") or suboptimal: return
    assert score == ref.opt, f"{tag}: {route} score {score}, unbanded optimum {ref.opt}"
    for j in ref.need:
        i = int(rs[j])
        assert 0 <= i <= ref.I and ref.entry_ok[j][i], f"{tag}: column {j}: no optimal alignment enters it at row {i}"
    for p in np.flatnonzero(np.asarray(dirty) == 0):
        assert ref.clean_ok[p], f"{tag}: position {int(p)} reported clean, but no optimal alignment matches it"

"""The plain unbanded reference of the alignment stage (tests/align_ref.py) against a brute force, and the CPU restatement's alignment cascade against the reference on the
alignment lab (tests/align_lab.py) — everything here runs without a GPU.  All integer, all exact: the only passes excused from score == OPT are the two the lab plants at
the 16-row band's deletion limit and lists by (zmw, pass), and each of them must really fall short."""
import functools

import numpy as np
import pytest

import align_lab as G
import align_ref as A
import oracle_lib as O


def _brute(r, d):
    """best global score of r against d, by recursion on the last step"""
    @functools.lru_cache(maxsize=None)
    def f(i, j):
        if i == 0 or j == 0: return -4 * (i + j)
        return max(f(i - 1, j - 1) + (3 if r[i - 1] == d[j - 1] else -5), f(i - 1, j) - 4, f(i, j - 1) - 4)
    return f


def test_tables_against_brute_force():
    rng = np.random.default_rng(4)
    for _ in range(80):
        r = tuple(int(b) for b in rng.integers(0, 3, rng.integers(0, 8)))
        d = tuple(int(b) for b in rng.integers(0, 3, rng.integers(1, 8)))
        F, B = A.forward(r, d), A.backward(r, d)
        f, g = _brute(r, d), _brute(r[::-1], d[::-1])
        for i in range(len(r) + 1):
            for j in range(len(d) + 1):
                assert F[i][j] == f(i, j) and B[i][j] == g(len(r) - i, len(d) - j), (r, d, i, j)
        assert F[len(r)][len(d)] == B[0][0]
        # the vectorised forms kept by Ref say what the two plain predicates say, and every column is entered somewhere, a fully matching pass is clean everywhere
        ref = A.Ref(r, d, range(len(d) + 1))
        for j in range(len(d) + 1):
            got = [A.entry_is_optimal(F, B, r, d, j, i) for i in range(len(r) + 1)]
            assert got == ref.entry_ok[j].tolist() and any(got), (r, d, j)
        assert [A.clean_is_possible(F, B, r, d, p) for p in range(len(d))] == ref.clean_ok.tolist()


def test_known_answers():
    rng = np.random.default_rng(8)
    t = rng.integers(0, 4, 60).astype(np.uint8)
    opt = lambda r: int(A.forward(r, t)[len(r)][len(t)])
    assert opt(t) == 180 and opt(t[:0]) == -240
    assert opt(G.edited(t, [G._mm(t, 30)])) == 180 - 8                       # one mismatch: a match lost, -5
    assert opt(G.edited(t, [(30, 1, [])])) == 177 - 4 and opt(G.edited(t, [(30, 0, [G._other(t[29], t[30])])])) == 180 - 4
    assert opt(G.edited(t, [(20, 7, []), (40, 0, [0] * 9)])) == 3 * 53 - 28 - 36
    r = G.edited(t, [(30, 0, [G._other(t[29], t[30])] * 3)])
    F, B = A.forward(r, t), A.backward(r, t)
    # column 30 is entered at row 30, BEFORE the three inserted bases (they are emitted while the path waits there), and at no other row; column 31 at row 34
    assert [i for i in range(len(r) + 1) if A.entry_is_optimal(F, B, r, t, 30, i)] == [30] and A.entry_is_optimal(F, B, r, t, 31, 34) and not A.entry_is_optimal(F, B, r, t, 31, 31)
    assert all(A.clean_is_possible(F, B, r, t, p) for p in range(60))       # (necessary, not sufficient: the neighbours of an insertion are dirty by the SPEC's rule)
    rm = G.edited(t, [G._mm(t, 30)])
    assert [p for p in range(60) if not A.clean_is_possible(A.forward(rm, t), A.backward(rm, t), rm, t, p)] == [30]
    # the restatement's global band on an easy pair equals the unbanded optimum
    rs, v, sc, dirty = O.align_ev_w(rm, t, O.need_cols(t))
    assert (v, sc) == (1, 172) and np.flatnonzero(dirty).tolist() == [30]


def test_lab_drafts_are_the_templates(built):
    L = G.lab(); batch = L.batch()
    for z, (name, t, _) in enumerate(L.zmws):
        assert np.array_equal(O.poa_draft(batch, z), t), f"zmw {z} ({name}): the POA draft is not the planted template"
    assert 14 <= batch.n_zmw <= 18 and 95 <= len(batch.flags) <= 120


@pytest.mark.parametrize("wide", [0, 1])
def test_restatement_against_the_plain_reference(built, wide):
    """every pass of the lab through the restatement's cascade (wide = 1: opts.disable_heuristics): score == OPT, every window-edge entry optimal, every clean position possibly
    clean for the routes narrow / wide_*; score <= the unbanded bound of its route and non-decreasing entries for every valid pass.  Zero exceptions beyond the planted list."""
    G.check_all(G.routes(wide), wide)
    if wide: assert all(r[0] in ("wide", "lost", "partial") or r[0].startswith("split") for r in G.routes(1).values())


def test_planted_edits_dirty_the_positions_the_spec_names(built):
    """DESIGN.md §2 "Pile-up evidence": a mismatch or a deletion marks its position, an inserted base both neighbours, leading insertions position 0 (and trailing ones the
    last) — single edits planted where they have one placement, on and off the window-edge columns"""
    L = G.lab()
    for wide in (0, 1):
        for key, want in L.expect_dirty.items():
            name, rs, v, sc, dirty = G.routes(wide)[key]
            assert v and name in ("narrow", "wide") and set(np.flatnonzero(dirty).tolist()) == want, (key, name, sorted(set(np.flatnonzero(dirty).tolist()) ^ want))


def test_lab_contains_the_planted_shapes(built):
    E = G.evidence(G.routes(0))
    print("\n[align lab, CPU restatement] evidence", E)
    G.assert_evidence(E)

"""The tandem-repeat detector at its kernel's limits (DESIGN.md §2 "Tandem repeats").  tests/golden/sdust_limits.npz holds drafts that place a masked run
against every boundary of k_sdust — a lane's range of ends (ch = ceil((nt - 1) / 64)), its 61-end warm-up, the 32-bit words of the LDS mask, the
cb = ceil(Ld / 64) chunks of the longest-run scan — and drafts on which a kernel with one plausible slip (tests/sdust_lab.py MUTANTS) reports another
tandem_len.  On the CPU every claim of the file is recomputed, the expectation from the written definition; on an MI355X k_sdust is handed exactly these drafts
(identical passes: the POA returns the template) and must report exactly these values, in any ZMW order, synchronously or through a ticket.  Further on the
GPU: the mask at opts.max_length, the deciding draft of DESIGN.md §2 through the draft cascade (k_sdust(pass > 0) and its early return), and the flag's >=.

(a) of the limit set: a draft "killed by warm-1 and by no single-lane mutant" does not exist.  warm-1 differs from the rule only at a lane's first end e0, where
the suffix of 62 triplets starts before the shortened warm-up; kmax-1 loses exactly the intervals of 62 triplets, at every end, and nothing else (such an interval
is the last one scored at its end and its ring slot is cleared before its start is read again).  So mask(kmax-1) is inside mask(warm-1) is inside the mask, the
longest run is monotone in the mask, and every warm-1 kill is a kmax-1 kill.  The set holds, and the test asserts, the nearest thing that exists: drafts on which a
warm-1 kernel reports a value that no single-lane mutant reports.
(b) of the limit set: the request for this set named 8 triplets with counts (6, 1, 1) as the smallest shape with S = 2 k + 1.  No draft has it as its only
interval above the threshold: six equal triplets among eight are adjacent somewhere, so they are a homopolymer's, a non-homopolymer base spoils two triplets only
next to the draft's end, and the six then form a run whose own score is 15 / 5.  The shortest such draft the generator finds has 17 triplets with S = 33.
(d): a masked run has at least 7 bases (5 equal triplets: 10 pairs over 4; 4 triplets give 6 / 3 = 2.0, which is not above the threshold), so a longest run
cannot lie inside one scan chunk of cb = 1 or 2 bases, nor strictly inside a chunk of the cb <= 7 that drafts of at most 400 bases have; what the file holds
for cb >= 4 is a run that touches one chunk only."""
import os

import numpy as np
import pytest

from ccs_amd import api
import sdust_lab as LAB
import sdust_ref as R

REQUIRED_LENGTHS = sorted(set(range(10, 71)) | {32 * k + d for k in (2, 3, 4) for d in (-1, 0, 1)} | {67, 68, 131, 132})   # (Ld - 3 = 64, 65, 128, 129: ch steps)
MASK_PROPERTIES = (["run/starts_at_0", "run/ends_at_last", "word/begins_at_bit0", "word/ends_at_bit31", "word/three_whole_words", "word/inside_one_word",
                    "gap/one_unmasked_base"]
                   + [f"scan/cb{c}/{p}" for c in ("1", "2", "4+") for p in ("inside_one_chunk", "whole_chunk_between_partial", "longer_first", "longer_second")])
# what no draft can have (the module's docstring): a run of at least 7 bases inside a chunk of 1 or 2
UNREALISABLE = {"scan/cb1/inside_one_chunk", "scan/cb2/inside_one_chunk"}


@pytest.fixture(scope="module")
def lim():
    L = LAB.load()
    for d in L.drafts:
        d.setflags(write=False)
    return L


@pytest.fixture(scope="module")
def masks(lim):
    """the expected mask of every draft of the set, from the written definition; the incremental form and the 64-lane split agree with it"""
    out = []
    for n, d in zip(lim.names, lim.drafts):
        m = R.masked_bruteforce(d)
        assert np.array_equal(m, R.masked_incremental(d)) and np.array_equal(m, R.masked_lanes(d)), n
        m.setflags(write=False)
        out.append(m)
    return out


@pytest.fixture(scope="module")
def kill_table(lim):
    """[draft, mutant]: tandem_len changes under the mutant — recomputed, not read from the file"""
    return np.array([[m in kl for m in LAB.MUTANTS] for kl in map(LAB.kills, lim.drafts)], bool)


# ---------------------------------------------------------------- CPU: the parameterised rule
@pytest.mark.parametrize("seed", range(6))
def test_default_knobs_are_the_restatement(seed):
    rng = np.random.default_rng(100 + seed)
    L = int(rng.integers(3, 420))
    x = rng.integers(0, 4, L).astype(np.uint8)
    for _ in range(int(rng.integers(0, 4))):
        u = rng.integers(0, 4, int(rng.integers(1, 13))).astype(np.uint8)
        n = int(rng.integers(8, 100))
        p = int(rng.integers(0, max(1, L - 8)))
        rep = np.tile(u, n // len(u) + 1)[:min(n, L - p)]
        err = rng.random(len(rep)) < 0.04
        rep[err] = rng.integers(0, 4, int(err.sum()))
        x[p:p + len(rep)] = rep
    assert np.array_equal(LAB.masked_incremental(x), R.masked_incremental(x))
    assert np.array_equal(LAB.masked_lanes(x), R.masked_lanes(x))
    assert np.array_equal(LAB.masked_lanes(x, lanes=7), R.masked_lanes(x, lanes=7))
    assert LAB.tandem_len(x) == R.tandem_len(x)


def test_mutant_table():
    assert list(LAB.MUTANTS) == ["warm-1", "leave-1", "gate-1", "kmax-1", "tie>", "ring61", "thr>="]
    assert all(k != LAB.DEFAULT for k in LAB.MUTANTS.values())
    # leave+1 is equivalent: the window's pairs only bound a suffix's pairs from above
    for k in range(12):
        x = np.random.default_rng(k).integers(0, 2 + k % 3, 60 + 20 * k).astype(np.uint8)
        assert np.array_equal(LAB.masked_lanes(x, LAB.Knobs(leave=1)), R.masked_lanes(x))


# ---------------------------------------------------------------- CPU: the limit set's claims, recomputed
def test_limit_set_is_small_and_in_range(lim):
    assert os.path.getsize(LAB.GOLDEN) < 64 << 10
    assert len(lim.drafts) == len(lim.names) == len(lim.expect) == len(lim.kills) <= 300 and len(set(lim.names)) == len(lim.names)
    assert all(10 <= len(d) <= 400 and d.max() <= 3 for d in lim.drafts)
    assert lim.mutants == list(LAB.MUTANTS)
    assert len(lim.too_short) == 9 and len(set(lim.too_short.tolist())) == 1            # a homopolymer below opts.min_length = 10
    assert api.default_opts().min_length == 10


def test_expected_values_are_the_definitions(lim, masks):
    for n, m, want in zip(lim.names, masks, lim.expect):
        assert R.longest_run(m) == want, n


def test_a_every_mutant_is_killed_three_times(lim, kill_table):
    assert np.array_equal(kill_table, lim.kills)
    for j, m in enumerate(LAB.MUTANTS):
        assert kill_table[:, j].sum() >= 3, m
    warm = [k for k in range(len(lim.drafts)) if kill_table[k, 0]]
    chs = {min(LAB.ch_of(len(lim.drafts[k])), 3) for k in warm}
    assert chs == {1, 2, 3}, chs                                   # Ld - 3 in 1..64, 65..128, above 128
    # The lane split itself is pinned, not the longest suffix.  No draft is killed by warm-1 and by no single-lane mutant (the module's docstring): warm-1 loses
    # some of the perfect intervals of 62 triplets, kmax-1 all of them and nothing else, so their masks nest and every warm-1 kill is a kmax-1 kill.  What the set
    # holds instead: drafts on which the value a warm-1 kernel reports is that of NO single-lane mutant, so the failure names the split
    kmax = list(LAB.MUTANTS).index("kmax-1")
    told = 0
    for k in warm:
        d = lim.drafts[k]
        assert kill_table[k, kmax]
        mw, mk = LAB.masked_lanes(d, LAB.MUTANTS["warm-1"]), LAB.masked_lanes(d, LAB.MUTANTS["kmax-1"])
        assert not (mk & ~mw).any() and not (mw & ~R.masked_lanes(d)).any()
        told += LAB.tandem_len(d, LAB.MUTANTS["warm-1"]) not in {LAB.tandem_len(d, LAB.MUTANTS[m]) for m in LAB.SINGLE_LANE}
    assert told >= 1


def test_b_the_gate_admits_its_smallest_score(lim):
    d = lim.drafts[lim.index("gate/limit")]
    over = [(i, e, S, k) for i, e, S, k in LAB.interval_scores(d) if S * 10 > LAB.T * k]
    assert len(over) == 1
    i, e, S, k = over[0]
    assert S == 2 * k + 1
    assert lim.expect[lim.index("gate/limit")] == e + 3 - i > 0
    assert LAB.kills(d, ["gate-1"]) == {"gate-1": 0}


def test_c_a_tie_with_a_perfect_interval_inside(lim):
    z = lim.index("tie/nested_equal_score")
    d = lim.drafts[z]
    S, _ = R.pair_table(d)
    per = sorted(R.perfect_intervals_bruteforce(d))
    ties = [((i, e), (a, b)) for i, e in per for a, b in per if (a, b) != (i, e) and i <= a and b <= e and S[a, b - a] * (e - i) == S[i, e - i] * (b - a)]
    assert ties
    assert LAB.tandem_len(d, LAB.MUTANTS["tie>"]) != lim.expect[z]


def _unique_longest(m):
    rr = LAB.runs(m)
    lens = sorted(b - a + 1 for a, b in rr)
    assert len(lens) == 1 or lens[-1] > lens[-2]
    return LAB.longest(m)


def test_d_mask_words_and_scan_chunks(lim, masks):
    assert set(lim.unrealised) == UNREALISABLE
    assert sorted(lim.unrealised + [n for n in lim.names if n in MASK_PROPERTIES]) == sorted(MASK_PROPERTIES)
    for Ld in (10, 64, 65, 200):
        z = lim.index(f"full/{Ld}")
        assert len(lim.drafts[z]) == Ld and masks[z].all() and lim.expect[z] == Ld
    for name in MASK_PROPERTIES:
        if name in lim.unrealised:
            continue
        z = lim.index(name)
        m, L = masks[z], len(lim.drafts[z])
        if name == "gap/one_unmasked_base":
            rr = LAB.runs(m)
            assert any(c - b == 2 for (a, b), (c, d) in zip(rr, rr[1:]))
            continue
        what = name.split("/")[-1]
        if what in ("longer_first", "longer_second"):
            rr = LAB.runs(m)
            assert len(rr) == 2
            (a, b), (c, d) = rr
            assert (b - a > d - c) if what == "longer_first" else (d - c > b - a), name
        else:
            a, b = _unique_longest(m)
            assert b - a + 1 == lim.expect[z]
        if name.startswith("scan/"):
            cb = LAB.cb_of(L)
            assert {"cb1": cb == 1, "cb2": cb == 2, "cb4+": cb >= 4}[name.split("/")[1]], (name, L)
            if what == "inside_one_chunk":
                assert a // cb == b // cb
            elif what == "whole_chunk_between_partial" and cb == 1:
                assert 0 < a and b < L - 1                                       # (a chunk of one base is never partial)
            elif what == "whole_chunk_between_partial":
                assert a % cb != 0 and (b + 1) % cb != 0 and (b + 1) // cb - (a + cb - 1) // cb >= 1
        elif name == "run/starts_at_0":
            assert a == 0 and not m.all()
        elif name == "run/ends_at_last":
            assert b == L - 1 and not m.all()
        elif name == "word/begins_at_bit0":
            assert a > 0 and a % 32 == 0
        elif name == "word/ends_at_bit31":
            assert b < L - 1 and b % 32 == 31
        elif name == "word/three_whole_words":
            assert (b + 1) // 32 - (a + 31) // 32 >= 3
        elif name == "word/inside_one_word":
            assert a // 32 == b // 32


def test_e_every_length_at_which_the_launch_changes_shape(lim):
    have = {}
    for k in lim.group("len/"):
        assert len(lim.drafts[k]) == int(lim.names[k].split("/")[1])
        have[len(lim.drafts[k])] = int(lim.expect[k])
    assert sorted(have) == REQUIRED_LENGTHS
    assert {LAB.ch_of(67), LAB.ch_of(68), LAB.ch_of(131), LAB.ch_of(132)} == {1, 2, 3}
    assert 2 * sum(v > 0 for v in have.values()) >= len(have)
    assert R.tandem_len(lim.too_short) == 9                        # (masked by the rule; the kernel never sees it: status TOO_SHORT)


def test_the_oracle_hands_every_draft_back(lim, built):
    """three identical passes on alternating strands: the draft generator returns the template itself, for every draft of the set"""
    import oracle_lib as O
    b = LAB.batch_from_drafts(lim.drafts)
    for z, d in enumerate(lim.drafts):
        reads, flags = LAB.passes_of(b, z)
        assert flags == [0, 1, 0] and np.array_equal(reads[1], R.revcomp(d))
        got, _ = O.poa_generator(reads, flags, 5)
        assert got is not None and np.array_equal(got, d), lim.names[z]


# ---------------------------------------------------------------- GPU
import test_tandem as TT  # noqa: E402  (its _opts, _same and the per-ZMW _invariant)

TOO_SHORT, TOO_LONG, DRAFT_FAILURE = 5, 6, 2


@pytest.mark.gpu
def test_limit_set_on_the_gpu(lim, built):
    """one handle, default options, the cascade on: k_sdust sees exactly the set's drafts and reports the definition's tandem_len for every one"""
    assert api.STATUS_NAMES[TOO_SHORT] == "TOO_SHORT"
    drafts = list(lim.drafts) + [lim.too_short]
    want = np.concatenate([lim.expect, [0]]).astype(np.int32)
    n = len(drafts)
    b = LAB.batch_from_drafts(drafts)
    h = api.Handle(0)
    res, tl, _ = h.consensus_extras(b, tandem=True)
    for z in range(n - 1):
        assert np.array_equal(h.stage_draft(z), drafts[z]), lim.names[z]
    bad = [(lim.names[z] if z < n - 1 else "too_short", int(tl[z]), int(want[z])) for z in range(n) if tl[z] != want[z]]
    assert not bad, bad
    assert res.status[n - 1] == TOO_SHORT
    # the ZMW order reversed: the same values (k_sdust takes the ZMWs longest first, whatever their order)
    _, tlr, _ = h.consensus_extras(LAB.batch_from_drafts(drafts[::-1], seed=1), tandem=True)
    assert np.array_equal(tlr[::-1], want)
    # through a ticket
    rs = api.Results.allocate(b, pinned=True)
    tls = api.tandem_buffer(n, pinned=True)
    h.wait(h.submit(b, rs, tandem=tls))
    assert np.array_equal(tls, want)
    h.close()


@pytest.mark.gpu
def test_mask_at_max_length(built):
    """the LDS mask is sized for opts.max_length: drafts masked over their whole length at max_length - 1 and max_length, and one base beyond"""
    drafts = [np.tile(np.array(u, np.uint8), L // len(u) + 1)[:L] for L, u in ((199, [0, 2, 2, 2, 2, 3]), (200, [1, 3]), (201, [0, 1, 2]))]
    assert [R.tandem_len(d) for d in drafts] == [199, 200, 201]
    b = LAB.batch_from_drafts(drafts)
    h = api.Handle(0, opts=TT._opts(max_length=200))
    res, tl, _ = h.consensus_extras(b, tandem=True)
    for z in range(2):
        assert np.array_equal(h.stage_draft(z), drafts[z])
    assert tl.tolist() == [199, 200, 0]
    assert res.status[2] == TOO_LONG and api.STATUS_NAMES[TOO_LONG] == "TOO_LONG"
    h.close()


@pytest.mark.gpu
def test_the_deciding_draft_is_the_first_one_the_cascade_aligns_to(built):
    """decided once, on the first draft with status SUCCESS after its generator — pass 0's even when the cascade then drops it, the fallback's
    when pass 0 gives none — and kept for the rest of the call"""
    cases = LAB.cascade_cases()
    b = LAB.batch_from_passes([c.passes for c in cases])
    h1 = api.Handle(0, opts=TT._opts(no_fallback_draft=1))
    r1 = h1.consensus(b)
    first = [h1.stage_draft(z) for z in range(b.n_zmw)]
    h1.close()
    h = api.Handle(0)
    res, tl, _ = h.consensus_extras(b, tandem=True)
    final = [h.stage_draft(z) for z in range(b.n_zmw)]
    h.close()
    for z, c in enumerate(cases):
        if c.first is None:
            assert r1.status[z] == DRAFT_FAILURE, c.name               # no first draft: decided in pass 1
        else:
            assert np.array_equal(first[z], c.first), c.name           # the junk pass 0 is its generator's draft
            assert r1.status[z] != 0, c.name                           # ... and without the cascade the ZMW is lost
            assert not np.array_equal(final[z], first[z]), c.name      # the fallback (or the last resort) replaced it
        assert res.status[z] not in (1, 2, 3), (c.name, int(res.status[z]))   # the final draft is one the passes align to
        assert R.tandem_len(final[z]) == c.final_len and c.first_len == (R.tandem_len(first[z]) if c.first is not None else 0), c.name
        assert tl[z] == c.expect, (c.name, int(tl[z]), c.expect, c.final_len)
    assert [c.expect == c.final_len for c in cases] == [False, False, True, False]
    for z, c in enumerate(cases):
        one = b.slice(z, z + 1)
        _, tlz, flagged, _, _ = TT._invariant(one, c.threshold)
        assert tlz[0] == c.expect and bool(flagged[0]) == (c.expect >= c.threshold), c.name
    assert [c.expect >= c.threshold for c in cases] == [True, False, True, True]


@pytest.mark.gpu
def test_the_flag_is_set_at_tandem_len_exactly(built):
    """flag = tandem_len >= min_tandem_repeat_length: at a ZMW's own tandem_len it runs with the heuristics off, one above with them on"""
    import tandem_synth
    b, _ = tandem_synth.make(48, (6, 12), (2500, 5000), seed=21, frac=0.5, tract=(400, 2000))
    hd, hx = api.Handle(0), api.Handle(0, opts=TT._opts(disable_heuristics=1))
    ref_d, ref_x = hd.consensus(b), hx.consensus(b)
    _, tl, _ = hd.consensus_extras(b, tandem=True)
    differ = [z for z in range(b.n_zmw) if tl[z] > 0 and (ref_d.status[z] != ref_x.status[z] or not np.array_equal(ref_d.sequence(z), ref_x.sequence(z))
                                                           or not np.array_equal(ref_d.quals(z), ref_x.quals(z)))]
    assert differ
    z = differ[0]
    for thr, ref in ((int(tl[z]), ref_x), (int(tl[z]) + 1, ref_d)):
        res, tl2, _ = hd.consensus_extras(b, tandem=True, min_tandem_repeat_length=thr)
        assert np.array_equal(tl2, tl)
        TT._same(res, ref, z)
        for y in range(b.n_zmw):                                       # (and every other ZMW by the same rule)
            TT._same(res, ref_x if tl[y] >= thr else ref_d, y)
    hd.close(); hx.close()

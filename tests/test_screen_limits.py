"""The three draft screens at their kernels' limits, the CPU half (DESIGN.md §2 "Adapter palindromes", "Adapter screen", "Control screen"; tests/screen_lab.py
holds the limit sets).  Every property a case is named for is recomputed by the lab's path functions (thread shares, table passes, chunk owners, bins, the
counts 8192, 1536 and 1024); the expectation of every case is fold_ref's, adapter_ref's or control_ref's, brute force and restatement agreeing wherever the brute
force is affordable; every mutant of the lab's parameterised rules changes the report of at least one case, while the default knobs are the restatements; and
the draft generator hands every draft of the sets back unchanged from three identical passes, which is what lets tests/test_screen_limits_gpu.py give the
kernels these exact bytes."""
import numpy as np
import pytest

from ccs_amd import api
import adapter_ref as AR
import control_ref as CR
import fold_ref as FR
import screen_lab as LAB
import sdust_lab

SCREENS = {
    "fold": (LAB.fold_cases, LAB.FOLD_MUTANTS, LAB.FOLD_DEFAULT, lambda d, rq: LAB.fold_expect(d, rq), lambda d, rq, kn: LAB.fold_k(d, rq, kn)),
    "adapter": (LAB.adapter_cases, LAB.ADAPTER_MUTANTS, LAB.ADAPTER_DEFAULT, lambda d, rq: LAB.adapter_expect(d, rq), lambda d, rq, kn: LAB.adapter_k(d, rq["adapters"], rq["opts"], kn)),
    "control": (LAB.control_cases, LAB.CONTROL_MUTANTS, LAB.CONTROL_DEFAULT, lambda d, rq: LAB.control_expect(d, rq), lambda d, rq, kn: LAB.control_k(d, rq["control"], rq["opts"], kn)),
}
# the long drafts (the caps) are tried against the mutants that can tell them apart only: the adapter lanes of a 7 kb draft cost a second per mutant
LONG_MUTANTS = {"adapter": ()}


def unique_drafts(cases) -> list:
    """the distinct drafts of the cases, in order of first appearance, with the names that share each"""
    out, seen = [], {}
    for c in cases:
        k = c.draft.tobytes()
        if k not in seen:
            seen[k] = len(out)
            out.append((c.draft, [c.name]))
        else:
            out[seen[k]][1].append(c.name)
    return out


# ---------------------------------------------------------------- the parameterised rules
@pytest.mark.parametrize("seed", range(4))
def test_default_knobs_are_the_restatements(seed):
    rng = np.random.default_rng(700 + seed)
    rnd = lambda n: rng.integers(0, 4, int(n)).astype(np.uint8)
    # fold: random drafts with planted pairs, repeated sampled 15-mers, a homopolymer stretch
    y = LAB.sampled_kmer(rng)
    t = rnd(rng.integers(300, 2500))
    for p in rng.choice(np.arange(0, len(t) - 20, 40), int(rng.integers(2, 7)), replace=False):
        t[p:p + LAB.K] = y if rng.random() < 0.5 else LAB.rc(y)
    x = rnd(rng.integers(100, 600))
    for d in (rnd(rng.integers(0, 40)), t, np.concatenate([x, rnd(30), LAB.rc(x)]), np.concatenate([rnd(200), np.zeros(300, np.uint8), rnd(200)])):
        for o in (None, LAB.ONE, dict(LAB.ONE, max_occ=2), dict(LAB.V_ALL, min_arm=20)):
            assert LAB.fold_k(d, o) == FR.fold(d, opts=o), (len(d), o)
    # control
    c = rnd(rng.integers(64, 300))
    unit = np.tile(rnd(20), 8)
    for d, ctl in ((rnd(rng.integers(0, 40)), c), (np.concatenate([rnd(50), c[10:], rnd(30), LAB.rc(c), rnd(20)]), c), (np.concatenate([c, c]), c),
                   (np.concatenate([rnd(30), unit[7:120], rnd(20)]), unit), (rnd(400), c)):
        for o in (None, LAB.C_LOOSE, dict(LAB.C_LOOSE, max_occ=1), dict(LAB.C_LOOSE, max_occ=64)):
            assert LAB.control_k(d, ctl, o) == CR.screen(d, ctl, o), (len(d), o)
    # adapter: the lanes of 128 bases against the full table, drafts of several chunks, runs of every length
    a, b = rnd(rng.integers(16, 30)), rnd(rng.integers(30, 65))
    ac = np.tile(np.array([0, 1], np.uint8), 10)
    noisy = lambda p: np.delete(p, int(rng.integers(1, len(p) - 1))) if rng.random() < 0.5 else p
    parts = []
    for _ in range(int(rng.integers(3, 9))):
        parts += [rnd(rng.integers(0, 120)), noisy([a, b, LAB.rc(a), LAB.rc(b)][int(rng.integers(0, 4))])]
    for d, ads in ((np.concatenate(parts), [a, b]), (np.concatenate([rnd(90), np.tile(np.array([0, 1], np.uint8), 170), rnd(50)]), [ac, a]), (rnd(20), [a]),
                   (np.zeros(0, np.uint8), [a])):
        for o in (None, dict(max_dist_pct=0, min_copies=1, max_insert=0, end_slack=0), dict(max_dist_pct=30, min_copies=3, max_insert=40, end_slack=60)):
            assert LAB.adapter_k(d, ads, o) == AR.screen(d, ads, o), (len(d), o)


def test_mutant_tables():
    assert list(LAB.FOLD_MUTANTS) == ["NS_MAX-1", "NS_MAX+1", "tie>b", "one-bin", "j>i+K", "occ>=", "occ-all", "span-max", "reach<"]
    assert list(LAB.ADAPTER_MUTANTS) == ["own>=lo", "warm-m", "last-min", "max-x", "k-ceil", "by-start", "gap-no-lead", "gap-no-trail"]
    assert list(LAB.CONTROL_MUTANTS) == ["tie-o1", "tie>b", "matched=hits", "cap-on-draft", "u=i", "ends-K"]
    for table, default in ((LAB.FOLD_MUTANTS, LAB.FOLD_DEFAULT), (LAB.ADAPTER_MUTANTS, LAB.ADAPTER_DEFAULT), (LAB.CONTROL_MUTANTS, LAB.CONTROL_DEFAULT),
                           (LAB.ADAPTER_EQUIVALENT, LAB.ADAPTER_DEFAULT)):
        assert all(k != default for k in table.values()) and len(set(table.values())) == len(table)


def test_the_overflow_pass_one_hit_early_is_equivalent():
    """ADAPTER_EQUIVALENT: entering the overflow pass at 1024 hits lists the same 16 hits (the argument is in the lab); held on both sides of the boundary"""
    S = LAB.adapter_cases()
    for name in ("list/1024_hits", "list/1025_hits_16th_end_shared"):
        c = S.case(name)
        rq = S.requests[c.request]
        want = AR.screen(c.draft, rq["adapters"], rq["opts"])
        assert LAB.adapter_k(c.draft, rq["adapters"], rq["opts"]) == want == LAB.adapter_k(c.draft, rq["adapters"], rq["opts"], LAB.ADAPTER_EQUIVALENT["overflow>=1024"])


# ---------------------------------------------------------------- the limit sets
def test_the_path_functions():
    assert [LAB.thread_share(257, 256, t) for t in (0, 127, 128, 129, 255)] == [(0, 2), (254, 256), (256, 257), (257, 257), (257, 257)]
    assert LAB.thread_share(255, 256, 254) == (254, 255) and LAB.thread_share(255, 256, 255) == (255, 255) and LAB.thread_share(512, 256, 255) == (510, 512)
    assert [LAB.fold_nparts(n) for n in (0, 1536, 1537, 3072, 3073, 8192)] == [1, 1, 2, 2, 4, 8]
    assert int(FR.fmix32(0)[0]) == 0 and LAB.fold_pass(np.array([0]), 4)[0] == 0                  # every all-A 15-mer is sampled, pass 0
    assert [LAB.adapter_chunk(j) for j in (1, 128, 129, 256, 257)] == [0, 0, 1, 1, 2]
    assert [LAB.diag_bin(D) for D in (63, 64, 127, 128)] == [0, 1, 1, 2]
    assert LAB.runs_of(np.array([9, 0, 1, 5, 1, 1]), 1) == [(1, 2), (4, 5)]


@pytest.mark.parametrize("screen", list(SCREENS))
def test_limit_set(screen, capsys):
    """every claim recomputed, brute force == restatement == the default knobs on every case, and the mutant kill table"""
    cases_of, mutants, default, expect, under = SCREENS[screen]
    S = cases_of()
    opts = api.default_opts()
    kills = {m: [] for m in mutants}
    for c in S.cases:
        assert opts.min_length <= len(c.draft) < opts.max_length and c.draft.max() <= 3, c.name
        assert c.holds(), c.name
        rq = S.requests[c.request]
        want = expect(c.draft, rq)                                   # (asserts brute force == restatement where the brute force applies)
        assert under(c.draft, rq, default) == want, c.name
        for m, kn in mutants.items():
            if c.batch != "short" and screen in LONG_MUTANTS and m not in LONG_MUTANTS[screen]:
                continue
            if under(c.draft, rq, kn) != want:
                kills[m].append(c.name)
    with capsys.disabled():
        print(f"\n{screen}: {len(S.cases)} cases on {len(unique_drafts(S.cases))} drafts, {len(S.requests)} requests; batches "
              + ", ".join(f"{b} ({len(unique_drafts(S.batch(b)))} drafts x {len(r)} requests)" for b, r in S.batch_requests.items()))
        for m, ks in kills.items():
            print(f"  {m:14s} killed by {len(ks):2d}: {', '.join(ks[:3])}{' ...' if len(ks) > 3 else ''}")
    assert all(kills.values()), [m for m, ks in kills.items() if not ks]


def test_what_the_sets_reach():
    """the places the generated batches cannot aim at, each reached exactly"""
    F, A = LAB.fold_cases(), LAB.adapter_cases()
    assert [LAB.n_samples(F.case(f"ns/later_position_is_sample_{r}").draft) for r in (8191, 8192, 8193)] == [8191, 8192, 8193]
    assert [[p for p, _ in LAB.fold_schedule(F.case(f"cap/{n}_samples").draft, 8)] for n in (1536, 1537, 3072)] == [[1], [2], [2, 4]]
    two = LAB.fold_schedule(F.case("cap/3072_samples").draft, 8)[0][1]
    assert sum(k for _, k in two) == 3072 and max(k for _, k in two) > LAB.FOLD_CAP
    rq = A.requests["unit/k1"]
    assert [AR.screen(A.case(n).draft, rq["adapters"], rq["opts"])["n_hits"] for n in ("list/1024_hits", "list/1025_hits_16th_end_shared")] == [1024, 1025]
    assert max(len(c.draft) for S in (F, A, LAB.control_cases()) for c in S.cases) < 26000
    assert all(len(c.draft) <= 1200 for S in (F, A, LAB.control_cases()) for c in S.cases if c.batch == "short")


def test_the_oracle_hands_every_draft_back(built):
    """three identical passes on alternating strands: the draft generator returns the template itself, for every draft of the three sets"""
    import oracle_lib as O
    for cases_of in (LAB.fold_cases, LAB.adapter_cases, LAB.control_cases):
        drafts = unique_drafts(cases_of().cases)
        b = sdust_lab.batch_from_drafts([d for d, _ in drafts])
        for z, (d, names) in enumerate(drafts):
            reads, flags = sdust_lab.passes_of(b, z)
            assert flags == [0, 1, 0] and np.array_equal(reads[1], LAB.rc(d))
            got, _ = O.poa_generator(reads, flags, 5)
            assert got is not None and np.array_equal(got, d), names

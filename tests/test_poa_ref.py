"""The POA draft pinned on the CPU (no GPU needed): the plain reference of tests/poa_ref.py is held to brute force and to known answers, and the CPU
restatement's POA (oracle/ccs_oracle.c, through its per-pass record hook) is held to the reference — on the planted lab (tests/poa_lab.py) and on a seeded fuzz.

A pass that went through the 32-row band must score what the unbanded int64 DP over the whole graph scores (OPT).  The passes allowed to fall short are the
explicit list `excused` of the lab's entries; each must really fall short (a stale excuse fails), and no fuzz ZMW may be excused."""
from functools import lru_cache

import numpy as np
import pytest

from ccs_amd import api
import lowcx
import oracle_lib as O
import poa_lab as L
import poa_ref as R


def zmw_reads(batch, z):
    r0, r1 = int(batch.read_off[z]), int(batch.read_off[z + 1])
    return [np.asarray(batch.bases[int(batch.base_off[r]):int(batch.base_off[r + 1])]) for r in range(r0, r1)], [int(f) for f in batch.flags[r0:r1]]


def logs(recs): return np.array([q.log() for q in recs], np.int32).reshape(-1, 5)


def same_draft(a, b): return (a is None and b is None) or (a is not None and b is not None and np.array_equal(a, b))


def compare(name, reads, flags, cov, bb=0):
    """oracle against poa_spec(band=32) for one generator: the draft and every per-pass record, exactly.  Returns the reference's (draft, records)"""
    d, recs = R.poa_spec(reads, flags, cov, bb, snapshots=True)
    od, orec = O.poa_generator(reads, flags, cov, bb)
    mine = logs(recs)
    assert len(mine) == len(orec), f"{name} (cov {cov}, backbone {bb}): the oracle logs {len(orec)} passes, the reference {len(mine)}"
    for k in range(len(mine)):
        for f, fld in enumerate(("I", "end score", "end position", "threaded", "vertices")):
            assert mine[k, f] == orec[k, f], f"{name} (cov {cov}, backbone {bb}) pass {k + 1} {fld}: oracle {orec[k, f]}, reference {mine[k, f]}"
    assert same_draft(d, od), f"{name} (cov {cov}, backbone {bb}): the oracle's draft differs from the reference's"
    return d, recs


def check_opt(name, reads, flags, recs, backbone, excused=()):
    """score <= OPT on the graph before the pass, with equality except for the excused passes — which must really fall short"""
    rev0 = flags[backbone] & 1
    for q in recs:
        o = R.opt_unbanded(q.dag, R.orient(reads[q.read], (flags[q.read] & 1) != rev0))
        assert q.score <= o.opt, f"{name} pass {q.rr}: the banded score {q.score} exceeds the unbanded optimum {o.opt}"
        if q.rr in excused:
            assert q.score < o.opt, f"{name} pass {q.rr}: excused, but it reaches the optimum {o.opt} — a stale excuse"
            continue
        assert q.score == o.opt, f"{name} pass {q.rr}: score {q.score}, the unbanded optimum is {o.opt}"
        if q.threaded:                              # the path the pass was threaded along: every matched vertex lies on some optimal alignment at its row
            off = [(i, k) for i, k in enumerate(q.path_pos) if k >= 0 and not o.on_optimal(k, i + 1)]
            assert not off, f"{name} pass {q.rr}: read base / vertex position {off[:4]} of its path lie on no optimal alignment"


# ---- the reference itself
def test_opt_unbanded_against_brute_force():
    rng = np.random.default_rng(11)
    seen_multi = 0
    for it in range(400):
        n = int(rng.integers(1, 7))
        preds = [[u for u in range(k) if rng.random() < 0.45] for k in range(n)]
        dag = R.Dag(rng.integers(0, 4, n), preds)
        read = [int(x) for x in rng.integers(0, 4, int(rng.integers(0, 6)))]
        o = R.opt_unbanded(dag, read)
        best, cells = R.brute_force(dag, read)
        assert o.opt == best, (it, dag.base, dag.preds, read, o.opt, best)
        mine = {(k, i) for k in range(n) for i in range(len(read) + 1) if o.on_optimal(k, i)}
        assert mine == cells, (it, dag.base, dag.preds, read, sorted(mine ^ cells))
        seen_multi += any(len(p) > 1 for p in preds)
    assert seen_multi > 150                          # graphs with a vertex of several in-edges


def test_poa_spec_known_answers_unbanded():
    """the known answers of test_oracle_draft.test_poa_known_answers, with full columns"""
    rng = np.random.default_rng(0)
    t = rng.integers(0, 4, 300).astype(np.uint8)
    draft = lambda reads, flags=None, cov=5: R.poa_spec(reads, flags or [0] * len(reads), cov, band=None)[0]
    assert np.array_equal(draft([t, t, t]), t)
    s = t.copy(); s[100] = (s[100] + 1) & 3
    assert np.array_equal(draft([s, t, t]), t)
    assert np.array_equal(draft([t, s, s]), s)
    ins = np.insert(t, 150, (t[150] + 2) & 3)
    dele = np.delete(t, 200)
    assert np.array_equal(draft([ins, t, t]), t)
    assert np.array_equal(draft([t, dele, t, t]), t)
    rc = (3 - t[::-1]).astype(np.uint8)
    assert np.array_equal(draft([t, rc, t], [0, 1, 0]), t)
    assert np.array_equal(draft([rc, t, rc], [1, 0, 1]), rc)
    assert np.array_equal(draft([s, t, t], cov=1), s)
    assert R.poa_spec([np.zeros(0, np.uint8), t], [0, 0], 5)[0] is None          # an empty backbone: DRAFT_FAILURE


# ---- the lab: every class occurs, oracle = reference, banded = unbanded optimum, planted drafts
@lru_cache(maxsize=None)
def lab_spec(k):
    z = L.lab()[k]
    return compare(z.name, z.reads, z.flags, L.COV)


def test_lab_shape():
    Z = L.lab()
    assert len({z.name for z in Z}) == len(Z) and 30 <= len(Z) <= 64
    assert max(len(z.reads) for z in Z) <= 14 and min(len(z.reads) for z in Z) >= 3          # (fewer than opts.min_passes = 3 passes: the engine drafts nothing)
    want = {"ring boundary", "far edge slot", "in-edge count", "record blocks", "trace-back block", "short reads", "chunk reload", "gate", "ties", "strands",
            "coverage option", "fallback", "overflow", "band limit"}
    assert {z.cls for z in Z} == want


@pytest.mark.parametrize("k", range(len(L.lab())), ids=[z.name for z in L.lab()])
def test_lab_entry(built, k):
    z = L.lab()[k]
    d, recs = lab_spec(k)
    assert z.checks or z.excused, f"{z.name} ({z.cls}): nothing says that the class occurs"
    for what, fn in z.checks: assert fn(recs), f"{z.name} ({z.cls}): the class does not occur — {what}: {recs}"
    g = np.concatenate([np.arange(1, len(recs) + 1, dtype=np.int32)[:, None], logs(recs)], 1)
    for what, fn in z.log_checks: assert fn(g), f"{z.name} ({z.cls}): not visible in the log words — {what}: {g.tolist()}"
    assert (d is None) == z.fails, f"{z.name}: DRAFT_FAILURE of the first generator expected {z.fails}"
    check_opt(z.name, z.reads, z.flags, recs, 0, z.excused)
    if z.fallback is None:
        if z.planted is not None: assert same_draft(d, z.planted), f"{z.name} ({z.cls}): the planted draft is not the reference's draft"
    else:
        assert R.fallback_backbone(z.reads, z.flags) == z.fallback, f"{z.name}: the fallback's backbone"
        d2, recs2 = compare(z.name, z.reads, z.flags, 2 * L.COV, z.fallback)
        check_opt(z.name + " (fallback)", z.reads, z.flags, recs2, z.fallback, z.excused2)
        assert [q.read for q in recs2] == [(z.fallback + rr) % len(z.reads) for rr in range(1, len(z.reads))], f"{z.name}: the passes do not wrap around the backbone"
        if z.planted is not None: assert same_draft(d2, z.planted), f"{z.name} ({z.cls}): the planted draft is not the fallback generator's draft"


@pytest.mark.parametrize("cov", [1, 2, 5])
def test_lab_coverage_option(built, cov):
    """max_poa_cov below the passes of most ZMWs: min(full passes, cov) - 1 records, partial passes never among them"""
    for z in L.lab():
        if len(z.reads[0]) > 500: continue
        d, recs = compare(z.name, z.reads, z.flags, cov)
        nfull = sum(1 for f in z.flags if not f & 2)
        assert len(recs) == min(nfull, cov) - 1, f"{z.name}: {len(recs)} passes in the POA at max_poa_cov {cov}"
        if cov == 1: assert same_draft(d, R.orient(z.reads[0], 0)), f"{z.name}: one pass is its own draft"
    z = next(z for z in L.lab() if z.name == "fallback_middle")
    for bb in (0, 2, 4): compare(z.name, z.reads, z.flags, cov, bb)          # backbones at the first, a middle and the last pass


# ---- fuzz: small ZMWs of the library's generator and of the low-complexity one; no pass may fall short of OPT
FUZZ = [("synth", lambda: api.synth(110, (3, 8), (40, 400), seed=41)), ("lowcx", lambda: lowcx.make(*L.LOWCX_FUZZ[:-1], tpl=L.LOWCX_FUZZ[-1])),
        ("channel x 1.5", lambda: lowcx.make(40, (3, 8), (40, 400), 47, channel=1.5))]


@pytest.mark.parametrize("name,make", FUZZ, ids=[f[0] for f in FUZZ])
def test_fuzz_oracle_equals_reference_and_reaches_opt(built, name, make):
    b = make()
    threaded = 0
    for z in range(b.n_zmw):
        if name == "lowcx" and z in L.LOWCX_SHORT: continue       # (a lab entry of its own, with its excuses named: test_lab_entry[lowcx_<z>])
        reads, flags = zmw_reads(b, z)
        d, recs = compare(f"{name} zmw {z}", reads, flags, 5)
        check_opt(f"{name} zmw {z}", reads, flags, recs, 0)
        threaded += sum(q.threaded for q in recs)
    assert threaded > b.n_zmw

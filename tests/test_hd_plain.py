"""The heteroduplex rule on the CPU, three ways: the exact Fisher test of tests/hd_plain.py against the restatement's log-factorial one, hd_plain against
tests/hd_ref.py on hand-made records, and every planted batch of tests/hd_lab.py on the oracle's stages: the census must show the limit the batch is named
for, with no borderline case.  tests/test_hd_limits_gpu.py repeats the last part on the engine's stages and holds the kernels to both."""
import numpy as np
import pytest

import hd_lab
import hd_plain
import hd_ref



def _fisher_tables():
    for nf in range(13):
        for nr in range(13):
            for a in range(nf + 1):
                for c in range(nr + 1):
                    yield a, nf, c, nr
    rng = np.random.default_rng(7)
    for _ in range(3000):
        nf, nr = (int(v) for v in rng.integers(0, 256, 2))
        yield int(rng.integers(0, nf + 1)), nf, int(rng.integers(0, nr + 1)), nr
    yield from [(0, 255, 255, 255), (255, 255, 0, 255), (128, 255, 127, 255), (127, 255, 128, 255), (0, 0, 0, 0), (0, 0, 5, 9), (3, 3, 0, 0), (0, 255, 0, 255),
                (255, 255, 255, 255), (3, 3, 0, 3), (0, 3, 3, 3), (2, 3, 1, 3), (1, 254, 1, 1), (0, 252, 3, 3), (100, 100, 0, 155), (0, 100, 155, 155)]


def test_exact_fisher_against_the_restatement():
    worst, near = 0.0, 0
    for (a, nf, c, nr) in _fisher_tables():
        p, tie = hd_plain.fisher_exact(a, nf, c, nr)
        near += int(tie)
        if tie:
            continue                                   # (a table at the tie rule may fall either way in floating point: counted, none occurs)
        q = hd_ref.fisher(a, nf, c, nr)
        dev = abs(q - float(p)) / float(p)
        worst = max(worst, dev)
        assert dev <= 1e-9, (a, nf, c, nr, q, float(p))
    print(f"largest relative deviation {worst:.3e}, near-tie tables {near}")       # (measured: 3.26e-12 over these 11297 tables; DESIGN.md §2 quotes it)
    assert near == 0


def test_exact_fisher_properties():
    assert hd_plain.fisher_exact(3, 3, 0, 3) == (hd_plain.Fraction(1, 10), False)
    assert hd_plain.fisher_exact(0, 8, 8, 8)[0] == hd_plain.Fraction(2, 12870)          # the mirror image has exactly the observed probability
    assert hd_plain.fisher_exact(5, 10, 5, 10)[0] == 1 and hd_plain.fisher_exact(0, 0, 0, 0)[0] == 1
    assert hd_plain.fisher_exact(0, 100, 155, 155)[0] == hd_plain.Fraction(1, hd_plain.comb(255, 100))


def test_edit_walk_tie_order():
    t = [1, 2, 0, 0, 0, 0, 3, 1]
    out = hd_plain.edit_walk([1, 2, 0, 0, 0, 3, 1], t)
    assert out[2] == 4 and [out[c] for c in (3, 4, 5)] == [0, 0, 0]                     # a deletion in a run lands on the run's first column
    assert hd_plain.edit_walk([], [1, 2]) == {0: 4, 1: 4} and hd_plain.edit_walk([1, 2, 3], []) == {}
    assert hd_plain.edit_walk([0, 1, 3, 3], [0, 1, 2, 3]) == {0: 0, 1: 1, 2: 3, 3: 3}


def _random_record(rng):
    """a Zmw with arbitrary entry rows: edited copies of a draft, rows from each copy's column map, then jitter, gaps and invalid passes"""
    nw = int(rng.integers(1, 9))
    wb = np.concatenate([[0], np.cumsum(rng.integers(19, 26, nw))]).astype(np.int32)
    Ld = int(wb[-1])
    draft = rng.integers(0, 4, Ld, dtype=np.uint8)
    cols = hd_ref.need_cols(wb, Ld)
    n = int(rng.integers(2, 24))
    strands = rng.integers(0, 2, n)
    hetero = [("sub", int(c), int(rng.integers(0, 4))) for c in rng.integers(0, Ld, int(rng.integers(0, 5)))]
    if rng.random() < 0.5 and Ld > 60:
        hetero.append(("ins", int(rng.integers(5, Ld - 5)), rng.integers(0, 4, int(rng.integers(15, 30)))) if rng.random() < 0.5
                      else ("del", int(rng.integers(5, Ld - 40)), int(rng.integers(15, 30))))
    reads = []
    for q in range(n):
        edits = list(hetero) if strands[q] else []
        edits += [("sub", int(c), int(rng.integers(0, 4))) for c in rng.integers(0, Ld, int(rng.integers(0, 4)))]
        if rng.random() < 0.3:
            edits.append(("ins", int(rng.integers(1, Ld)), rng.integers(0, 4, int(rng.integers(1, 4)))))
        if rng.random() < 0.3:
            edits.append(("del", int(rng.integers(1, Ld - 3)), int(rng.integers(1, 3))))
        seq = hd_lab.edited(draft, edits)
        shift = np.zeros(Ld + 1, np.int64)                       # row of every column: the column plus the net length of the edits before it
        for kind, col, x in edits:
            if kind == "ins":
                shift[col + 1:] += len(x)
            elif kind == "del":
                shift[col + 1: col + x] -= np.arange(1, x); shift[col + x:] -= x
        ent = np.array([c + shift[c] for c in cols], np.int64)
        if rng.random() < 0.15:
            ent[int(rng.integers(0, len(ent)))] += int(rng.integers(-30, 31))       # rows that make a segment negative, too long or out of the pass
        if rng.random() < 0.1:
            ent[int(rng.integers(0, len(ent))):] = -1
        fl = int(strands[q]) | (2 if q >= n - 2 and rng.random() < 0.3 else 0)
        native = (3 - seq[::-1]).astype(np.uint8) if strands[q] else seq
        reads.append((native, fl, bool(rng.random() < 0.9), ent))
    return hd_ref.Zmw(draft, wb, 0 if rng.random() < 0.95 else 3, int(rng.integers(0, min(n, 3))), reads)


def test_plain_against_the_restatement_on_hand_made_records():
    rng = np.random.default_rng(11)
    zmws = [_random_record(rng) for _ in range(60)]
    sets = [dict(), dict(hd_lab.EVERY_CANDIDATE), dict(min_indel=10, max_pvalue=0.01), dict(min_indel=1), dict(min_strand_passes=1, max_pvalue=0.01),
            dict(max_pvalue=1.0, min_alt_frac=0.3), dict(max_pvalue=1.0, min_alt_frac=0.25), dict(min_sites=3), dict(max_pvalue=0.0), dict(max_pvalue=0.1),
            dict(max_pvalue=1.0, min_strand_passes=2)]
    seen = dict(sub=0, indel=0, hd=0, ds=0, untested=0)
    for kw in sets:
        o = hd_lab.ref_opts(kw)
        plain, cens = hd_plain.hd_zmws(zmws, o)
        keep = [z for z, c in enumerate(cens) if not hd_plain.borderline(c)]
        ref = hd_ref.hd_zmws(zmws, o)
        assert len(keep) >= len(zmws) - 2
        assert hd_lab.differences([plain[z] for z in keep], [ref[z] for z in keep]) == [], kw
        for r in plain:
            seen["sub"] += r["n_sub"]; seen["indel"] += r["n_indel"]
            seen[("untested", "ds", "hd")[r["verdict"]]] += 1
    assert all(v > 20 for v in seen.values()), seen


@pytest.fixture(scope="module")
def oracle_runs():
    """every batch once: (lab, censuses, reports of hd_plain, reports of hd_ref) per option set, on the oracle's stages"""
    cache = {}

    def run(name):
        if name not in cache:
            lab = hd_lab.BATCHES[name]()
            stage = hd_lab.oracle_stage(lab)
            recs = hd_lab.used_records(stage)
            both = [hd_plain.hd_zmws(stage, hd_lab.ref_opts(kw)) for kw in lab.opt_sets]
            cache[name] = (lab, [c for _, c in both], [r for r, _ in both], [hd_ref.hd_zmws(recs, hd_lab.ref_opts(kw)) for kw in lab.opt_sets])
        return cache[name]
    return run


@pytest.mark.parametrize("name", list(hd_lab.BATCHES))
def test_batch_reaches_its_limit_on_the_oracle_stages(oracle_runs, name):
    lab, cens, plain, ref = oracle_runs(name)
    hd_lab.check_census(name, lab, cens, plain)
    for k, kw in enumerate(lab.opt_sets):
        keep = [z for z in range(lab.batch.n_zmw) if not hd_plain.borderline(cens[k][z])]       # (noisy_small only: check_census caps them at 1 of 64)
        assert hd_lab.differences([plain[k][z] for z in keep], [ref[k][z] for z in keep]) == [], (name, kw)

#!/usr/bin/env python3
"""The study behind the default max_dist_pct of the segmentation (DESIGN.md §2 "Segment rule"), on the CPU: arrays A0 S1 A1 .. S8 A8 of nine random 25-mers and
segments of 300-600 bases, on either strand, are sequenced into 3, 6 and 10 passes (tools/lowcx.py, the numpy channel), the oracle makes their consensus, and
the rule's restatement (tests/segment_ref.py) finds the hits.  Over a grid of max_dist_pct, per pass count: the planted adapters that have no hit (missed), the
hits that are no planted adapter, the arrays the rule calls complete; and on the consensus of molecules without adapters the false hits per Mb.
    python tools/segment_study.py [--out profiles/segment_study.txt]"""
import argparse
import os
import sys

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tools"))
sys.path.insert(0, os.path.join(R, "tests"))
from ccs_amd import api  # noqa: E402
import adapter_synth  # noqa: E402
import segment_ref as REF  # noqa: E402
import oracle_lib  # noqa: E402

N_SET, M, SEED = 9, 25, 6200
N_ARRAYS, N_BARE, SEGMENT, BARE = 32, 64, (300, 601), (4000, 6000)
GRID = (5, 10, 15, 20, 25, 30)


def molecules(rng, S, n, planted):
    tpls = []
    for z in range(n):
        if planted:
            t = REF.array(rng, S, [int(rng.integers(*SEGMENT)) for _ in range(N_SET - 1)])
            tpls.append(REF.rc(t) if z & 1 else t)
        else:
            tpls.append(REF.rand(rng, int(rng.integers(*BARE))))
    return tpls


def consensus(tpls, passes, rng):
    b = adapter_synth.from_templates(tpls, [passes] * len(tpls), rng)
    res = api.Results.allocate(b)
    oracle_lib.consensus_batch(api.default_model(), api.default_opts(), b, res, nthreads=min(16, os.cpu_count() or 1))
    return [res.sequence(z).copy() for z in range(b.n_zmw) if res.seq_len[z] > 0]


def hits_of(S, c, pct):
    """(dist, start, search, end) of every hit of every search"""
    out = []
    for s in range(2 * len(S)):
        p = REF.search_pattern(S, s)
        out += [(d, s0, s, e0) for s0, e0, d in REF.table_hits(p, c, len(p) * pct // 100)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(R, "profiles", "segment_study.txt"))
    a = ap.parse_args()
    rng = np.random.default_rng(SEED)
    S = REF.random_set(rng, N_SET, [M])
    pats = S + [REF.rc(x) for x in S]
    pair = min(REF.levenshtein(list(pats[i]), list(pats[j])) for i in range(len(pats)) for j in range(i))
    o = api.segment_opts_default()
    lines = [f"segmentation: {N_SET} random {M}-mers (smallest edit distance between two of them or their reverse complements {pair}); per pass count {N_ARRAYS} arrays of "
             f"{N_SET - 1} segments of {SEGMENT[0]}-{SEGMENT[1] - 1} bases, every second one reverse complemented, and {N_BARE} molecules of {BARE[0]}-{BARE[1] - 1} bases "
             f"without adapters; tools/lowcx.py channel, oracle consensus; seed {SEED}",
             f"shipped defaults: max_dist_pct {o.max_dist_pct} (k = {M * o.max_dist_pct // 100} of {M}), min_len {o.min_len}", "",
             "passes  max_dist_pct   k   arrays with a consensus   planted adapters   missed   hits that are no planted adapter   complete arrays     "
             "adapter-free: reads      bases   false hits   per Mb"]
    total = {pct: [0, 0, 0, 0, 0, 0] for pct in GRID}            # planted, missed, extra, complete, bare bases, bare hits
    n_arrays = 0
    for passes in (3, 6, 10):
        arrays = consensus(molecules(rng, S, N_ARRAYS, True), passes, rng)
        bare = consensus(molecules(rng, S, N_BARE, False), passes, rng)
        n_arrays += len(arrays)
        for pct in GRID:
            missed = extra = 0
            per_read = []
            for c in arrays:
                hits = hits_of(S, c, pct)
                per_read.append((len(c), hits))
                fwd, rev = {h[2] >> 1 for h in hits if not h[2] & 1}, {h[2] >> 1 for h in hits if h[2] & 1}
                found = max(len(fwd), len(rev))                      # (the strand the molecule is on: the one with more adapters found)
                missed += N_SET - found
                extra += len(hits) - found
            rep = REF.finish(len(arrays), per_read, N_SET, o.min_len)
            complete = int(rep["complete"].sum())
            false = sum(len(hits_of(S, c, pct)) for c in bare)
            bases = sum(len(c) for c in bare)
            planted = N_SET * len(arrays)
            for k, v in enumerate((planted, missed, extra, complete, bases, false)):
                total[pct][k] += v
            lines.append(f"{passes:6d}  {pct:12d}  {M * pct // 100:2d}   {len(arrays):10d}/{N_ARRAYS:<13d} {planted:16d} {missed:8d} {extra:34d} {complete:17d}     "
                         f"{len(bare):19d} {bases:10d} {false:12d} {1e6 * false / bases:8.2f}" + ("   <- shipped" if pct == o.max_dist_pct else ""))
        lines.append("")
    lines.append("all pass counts together: max_dist_pct -> missed of planted, hits that are no planted adapter, complete arrays, false hits per Mb of adapter-free consensus")
    for pct in GRID:
        p, m, e, c, b, f = total[pct]
        lines.append(f"  max_dist_pct {pct:2d}: {m:4d} of {p} missed, {e:4d} other hits, {c:3d} of {n_arrays} arrays complete, {f:4d} false hits in {b} bases = {1e6 * f / b:.2f} per Mb"
                     + ("   <- shipped" if pct == o.max_dist_pct else ""))
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()

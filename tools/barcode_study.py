#!/usr/bin/env python3
"""The study behind the defaults of the barcode calls (DESIGN.md §2 "Barcode calls"), on the CPU: molecules barcode_a · insert · rc(barcode_b) from a set of 96
random 16-mers are sequenced into 3, 6 and 10 passes (tools/lowcx.py, the numpy channel), the oracle makes their consensus, and the rule's restatement
(tests/barcode_ref.py) gives the distance of every barcode at every end.  Per pass count: the distance of the planted barcode, the margin from it to the best
barcode that was not planted, and how many ends the shipped options call, call wrong or leave uncalled; on molecules without barcodes the smallest distance of
any barcode and the ends the options call.  Then the same distances under a grid of options.
    python tools/barcode_study.py [--out profiles/barcode_study.txt]"""
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
import barcode_ref as REF  # noqa: E402
import oracle_lib  # noqa: E402

N_SET, M, SEED = 96, 16, 5100
N_PLANTED, N_BARE, INSERT = 192, 96, (800, 1500)
GRID = [(p, g) for p in (10, 15, 20, 25, 30) for g in (0, 1, 2, 3)]


def molecules(rng, S, n, planted):
    tpls, truth = [], []
    for _ in range(n):
        a, b = (int(rng.integers(0, N_SET)), int(rng.integers(0, N_SET))) if planted else (-1, -1)
        ins = rng.integers(0, 4, int(rng.integers(*INSERT))).astype(np.uint8)
        tpls.append(np.concatenate([S[a], ins, REF.rc(S[b])]).astype(np.uint8) if planted else ins)
        truth.append((a, b))
    return tpls, truth


def distances(S, reads, window):
    """[(dist of every barcode at end 0, at end 1)] per read with a consensus"""
    out = []
    for c in reads:
        out.append(None if len(c) == 0 else tuple(REF.end_tables(S, s[: min(len(c), window)]).min(axis=1) for s in (c, REF.rc(c))))
    return out


def judge(dist, truth, pct, margin):
    """(ends called right, called wrong, not called) under max_dist_pct / min_margin; truth -1: any call is wrong"""
    right = wrong = none = 0
    for d, t in zip(dist, truth):
        if d is None:
            continue
        for e in range(2):
            b = int(np.argmin(d[e]))
            second = int(np.delete(d[e], b).min())
            if d[e][b] <= M * pct // 100 and second - d[e][b] >= margin:
                right, wrong = right + (b == t[e]), wrong + (b != t[e])
            else:
                none += 1
    return right, wrong, none


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(R, "profiles", "barcode_study.txt"))
    a = ap.parse_args()
    rng = np.random.default_rng(SEED)
    S = REF.random_set(rng, N_SET, [M])
    pair = min(REF.levenshtein(list(S[i]), list(S[j])) for i in range(N_SET) for j in range(i))
    o = api.barcode_opts_default()
    lines = [f"barcode calls: {N_SET} random {M}-mers (smallest pairwise edit distance {pair}); per pass count {N_PLANTED} molecules barcode_a . insert . rc(barcode_b) and "
             f"{N_BARE} without barcodes, inserts of {INSERT[0]}-{INSERT[1]} bases, tools/lowcx.py channel, oracle consensus; seed {SEED}",
             f"shipped defaults: window {o.window}, max_dist_pct {o.max_dist_pct} (k = {M * o.max_dist_pct // 100} of {M}), min_margin {o.min_margin}", "",
             "passes  consensus/molecules   planted: dist  0     1     2     3    >3   max     margin to the best other: min  med  max     ends right wrong uncalled"
             "     bare: consensus  smallest dist min  med  max   ends called"]
    kept = []
    for passes in (3, 6, 10):
        row = f"{passes:6d}"
        for planted in (True, False):
            tpls, truth = molecules(rng, S, N_PLANTED if planted else N_BARE, planted)
            b = adapter_synth.from_templates(tpls, [passes] * len(tpls), rng)
            res = api.Results.allocate(b)
            oracle_lib.consensus_batch(api.default_model(), api.default_opts(), b, res, nthreads=min(16, os.cpu_count() or 1))
            reads = [res.sequence(z).copy() if res.seq_len[z] > 0 else np.zeros(0, np.uint8) for z in range(b.n_zmw)]
            dist = distances(S, reads, o.window)
            have = [(d, t) for d, t in zip(dist, truth) if d is not None]
            kept.append((passes, planted, dist, truth))
            if planted:
                dp = np.array([d[e][t[e]] for d, t in have for e in range(2)])
                mg = np.array([int(np.delete(d[e], t[e]).min()) - int(d[e][t[e]]) for d, t in have for e in range(2)])
                right, wrong, none = judge(dist, truth, o.max_dist_pct, o.min_margin)
                row += (f"   {len(have):9d}/{len(tpls):<9d}          " + "".join(f"{int((dp == k).sum()):6d}" for k in range(4)) + f"{int((dp > 3).sum()):6d}{int(dp.max()):6d}"
                        f"                         {int(mg.min()):5d}{int(np.median(mg)):5d}{int(mg.max()):5d}     {right:10d}{wrong:6d}{none:9d}")
            else:
                sm = np.array([int(d[e].min()) for d, _ in have for e in range(2)])
                _, wrong, _ = judge(dist, truth, o.max_dist_pct, o.min_margin)
                row += f"     {len(have):9d}/{len(tpls):<4d}           {int(sm.min()):5d}{int(np.median(sm)):5d}{int(sm.max()):5d}   {wrong:11d}"
        lines.append(row)
    lines += ["", "the same distances under other options (all pass counts together): max_dist_pct min_margin -> planted ends right / wrong / uncalled, bare ends called"]
    bad_default = None
    for pct, g in GRID:
        r = w = n = bw = 0
        for passes, planted, dist, truth in kept:
            a3 = judge(dist, truth, pct, g)
            if planted:
                r, w, n = r + a3[0], w + a3[1], n + a3[2]
            else:
                bw += a3[1]
        shipped = (pct, g) == (o.max_dist_pct, o.min_margin)
        if shipped:
            bad_default = (w, bw, 2 * sum(sum(d is not None for d in dist) for _, planted, dist, _ in kept if not planted))
        lines.append(f"  max_dist_pct {pct:2d} min_margin {g}: {r:5d} right {w:4d} wrong {n:5d} uncalled, {bw:4d} bare ends called" + ("   <- shipped" if shipped else ""))
    lines += ["", f"with the shipped defaults {bad_default[0]} planted ends are called wrong and {bad_default[1]} of {bad_default[2]} bare ends are called"]
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()

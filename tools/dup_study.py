#!/usr/bin/env python3
"""The study behind the distance and length defaults of the duplicate rule (DESIGN.md §2 "Duplicate rule"), on the CPU: random inserts are sequenced as two or
three ZMWs each (every second copy reverse complemented) into 3, 6 and 10 passes (tools/lowcx.py, the numpy channel), beside unrelated inserts and pairs of
inserts that share their first 100 bases only; the oracle makes every ZMW's consensus and the rule's restatement (tests/dup_ref.py) is applied to the reads.
Per pass count, over a grid of max_dist_pct x max_len_diff_pct at the shipped window and k: the planted pairs that are missed, by cause — the two reads have
different keys (an edit inside a minimizer k-mer, or another k-mer made the minimum: no option of the grid brings them back), their ends stand too far apart, or
their lengths do — and the pairs of reads of different inserts that are called (false pairs).  A pair is what the predicate says of two reads; the sets
(single linkage) can only join more.
    python tools/dup_study.py [--out profiles/dup_study.txt]"""
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
import dup_ref as REF  # noqa: E402
import oracle_lib  # noqa: E402

SEED = 8100
N_TWICE, N_THRICE, N_ALONE, N_SHARED, INSERT, SHARED = 24, 12, 24, 12, (600, 1001), 100
DIST, LEN = (0, 5, 10, 15, 20, 30), (0, 1, 2, 5, 10)


def molecules(rng):
    """(templates, the insert of each): inserts twice and three times over, alone, and pairs that share one end only (two inserts, one molecule each)"""
    tpls, ins = [], []
    k = 0
    for copies, count in ((2, N_TWICE), (3, N_THRICE), (1, N_ALONE)):
        for _ in range(count):
            t = rng.integers(0, 4, int(rng.integers(*INSERT))).astype(np.uint8)
            for c in range(copies):
                tpls.append(REF.rc(t) if c & 1 else t.copy()); ins.append(k)
            k += 1
    for _ in range(N_SHARED):
        head = rng.integers(0, 4, SHARED).astype(np.uint8)
        for _ in range(2):
            tpls.append(np.concatenate([head, rng.integers(0, 4, int(rng.integers(*INSERT)) - SHARED).astype(np.uint8)])); ins.append(k)
            k += 1
    return tpls, ins


def consensus(tpls, passes, rng):
    b = adapter_synth.from_templates(tpls, [passes] * len(tpls), rng)
    res = api.Results.allocate(b)
    oracle_lib.consensus_batch(api.default_model(), api.default_opts(), b, res, nthreads=min(16, os.cpu_count() or 1))
    return [res.sequence(z).copy() if res.seq_len[z] > 0 else None for z in range(b.n_zmw)]


def pair_figures(reads, sig, i, j, W):
    """(keys equal, the smallest kmax that admits the ends, |Li - Lj| * 100 / min(Li, Lj) rounded up)"""
    ei, ej = REF.ends(reads[i], W), REF.ends(reads[j], W)
    same = max(REF.dist(ei[0], ej[0]), REF.dist(ei[1], ej[1]))
    opp = max(REF.dist(ei[0], ej[1]), REF.dist(ei[1], ej[0]))
    Li, Lj = len(reads[i]), len(reads[j])
    return REF.key(sig, i) == REF.key(sig, j), min(same, opp), -(-abs(Li - Lj) * 100 // min(Li, Lj))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(R, "profiles", "dup_study.txt"))
    a = ap.parse_args()
    rng = np.random.default_rng(SEED)
    d = api.dup_opts_default()
    o = REF.opts(window=d.window, kmer=d.kmer)
    W = d.window
    lines = [f"duplicate rule: per pass count {N_TWICE} inserts as two ZMWs, {N_THRICE} as three (every second copy reverse complemented), {N_ALONE} alone and "
             f"{N_SHARED} pairs of inserts that share their first {SHARED} bases only; inserts of {INSERT[0]}-{INSERT[1] - 1} bases; tools/lowcx.py channel, oracle "
             f"consensus; window {d.window}, kmer {d.kmer}; seed {SEED}",
             f"shipped defaults: max_dist_pct {d.max_dist_pct}, max_len_diff_pct {d.max_len_diff_pct}", "",
             "passes  max_dist_pct (kmax)  max_len_diff_pct   planted pairs   missed: keys differ   ends too far   lengths too far   found   pairs of different inserts   called (false)"]
    total = {(dp, lp): [0, 0, 0, 0, 0, 0] for dp in DIST for lp in LEN}
    for passes in (3, 6, 10):
        tpls, ins = molecules(rng)
        cons = consensus(tpls, passes, rng)
        have = [z for z, c in enumerate(cons) if c is not None and len(c) >= W]
        reads = [cons[z] for z in have]
        sig = REF.sign(reads, o)
        n = len(reads)
        planted, other = [], []
        for x in range(n):
            for y in range(x + 1, n):
                f = pair_figures(reads, sig, x, y, W)
                if ins[have[x]] == ins[have[y]]:
                    planted.append(f)
                elif f[0]:                                           # (a pair of different inserts with different keys is never asked)
                    other.append(f)
        n_other = n * (n - 1) // 2 - len(planted)
        lines.append(f"# {passes} passes: {len(have)} of {len(tpls)} ZMWs with a consensus; ends of the planted pairs with equal keys stand at kmax "
                     + ", ".join(f"{k}: {sum(1 for f in planted if f[0] and f[1] == k)}" for k in sorted({f[1] for f in planted if f[0]}))
                     + "; their lengths differ by (percent, rounded up) " + ", ".join(f"{k}: {sum(1 for f in planted if f[0] and f[2] == k)}" for k in sorted({f[2] for f in planted if f[0]})))
        for dp in DIST:
            for lp in LEN:
                K = W * dp // 100
                keys = sum(1 for f in planted if not f[0])
                far = sum(1 for f in planted if f[0] and f[1] > K)
                length = sum(1 for f in planted if f[0] and f[1] <= K and f[2] > lp)
                found = len(planted) - keys - far - length
                false = sum(1 for f in other if f[1] <= K and f[2] <= lp)
                mark = "  <- shipped" if (dp, lp) == (d.max_dist_pct, d.max_len_diff_pct) else ""
                lines.append(f"{passes:6d}  {dp:12d} ({K:2d})  {lp:16d}  {len(planted):14d}  {keys:20d}  {far:13d}  {length:16d}  {found:6d}  {n_other:26d}  {false:14d}{mark}")
                for k, v in enumerate((len(planted), keys, far, length, found, false)):
                    total[(dp, lp)][k] += v
    lines += ["", "all pass counts:"]
    for (dp, lp), t in total.items():
        mark = "  <- shipped" if (dp, lp) == (d.max_dist_pct, d.max_len_diff_pct) else ""
        lines.append(f"   all  {dp:12d} ({W * dp // 100:2d})  {lp:16d}  {t[0]:14d}  {t[1]:20d}  {t[2]:13d}  {t[3]:16d}  {t[4]:6d}  {'':26s}  {t[5]:14d}{mark}")
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()

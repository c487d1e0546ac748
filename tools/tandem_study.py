#!/usr/bin/env python3
"""Does the per-ZMW heuristics switch (DESIGN.md §2 "Tandem repeats") buy the low-complexity yield of --disable-heuristics at near-default cost?
Random templates with one planted 1-2 kb tract (AGGGGT x n, or a 2-4-mer unit: tools/tandem_synth.py) beside random controls, through three
configurations on the same batch: default heuristics, global disable_heuristics, and the per-ZMW switch at a few thresholds.  Per configuration:
status counts, errors against the truth (edit distance per kb of the successful ZMWs, tract ZMWs and controls apart), k_polish ms (the polish
stage from the handle's events, median of --reps) and the flagged fraction.  The output is committed under profiles/ (tandem_study.txt)."""
import argparse
import os
import sys

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [R, os.path.join(R, "tools"), os.path.join(R, "tests")]
from ccs_amd import api  # noqa: E402
import oracle_lib as O  # noqa: E402
import tandem_synth  # noqa: E402


def errors(res, b, zs):
    e = n = 0
    for z in zs:
        t = b.tpl[b.tpl_off[z]:b.tpl_off[z + 1]]
        s = res.sequence(z)
        e += min(O.edit_distance(s, t), O.edit_distance(s, (3 - t[::-1]).astype(np.uint8)))
        n += len(t)
    return e, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--zmws", type=int, default=512)
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--length", type=int, default=5000)
    ap.add_argument("--frac", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--thresholds", default="250,500,1000")
    a = ap.parse_args()
    b, tracts = tandem_synth.make(a.zmws, a.passes, (a.length, a.length), a.seed, frac=a.frac, tract=(1000, 2000))
    tr = tracts > 0
    print(f"# tools/tandem_study.py --zmws {a.zmws} --passes {a.passes} --length {a.length} --frac {a.frac} --seed {a.seed}: "
          f"{int(tr.sum())} ZMWs with a planted 1-2 kb tract, {int((~tr).sum())} random controls")
    print(f"{'config':<18} {'ok tract':>9} {'ok ctrl':>8} {'fail':>5}  {'err/kb tract':>12} {'err/kb ctrl':>11}  {'polish ms':>9} {'total ms':>9}  "
          f"{'flagged':>7} {'flag tract':>10} {'flag ctrl':>9}  failures")
    configs = [("default", 0, 0), ("disable_heuristics", 1, 0)] + [(f"switch >= {t}", 0, int(t)) for t in a.thresholds.split(",")]
    for name, dis, thr in configs:
        o = api.default_opts(); o.disable_heuristics = dis
        h = api.Handle(0, opts=o)
        pol, tot = [], []
        for _ in range(a.reps):
            if thr:
                res, tl, _ = h.consensus_extras(b, tandem=True, min_tandem_repeat_length=thr)
            else:
                res = h.consensus(b); tl = None
            t = h.timings(); pol.append(t.polish_ms); tot.append(t.total_ms)
        h.close()
        ok = res.status == 0
        et, nt = errors(res, b, np.flatnonzero(ok & tr))
        ec, nc = errors(res, b, np.flatnonzero(ok & ~tr))
        fl = (tl >= thr) if tl is not None else np.zeros(b.n_zmw, bool)
        st, cnt = np.unique(res.status[~ok], return_counts=True)
        fails = " ".join(f"{int(s)}:{int(c)}" for s, c in zip(st, cnt)) or "-"
        print(f"{name:<18} {int((ok & tr).sum()):>9} {int((ok & ~tr).sum()):>8} {int((~ok).sum()):>5}  {1e3 * et / max(nt, 1):>12.2f} "
              f"{1e3 * ec / max(nc, 1):>11.2f}  {np.median(pol):>9.1f} {np.median(tot):>9.1f}  {fl.mean():>7.3f} {int((fl & tr).sum()):>10} "
              f"{int((fl & ~tr).sum()):>9}  {fails}")
    print("# failures: status code:count (include/ccsx.h enum ccsx_status)")


if __name__ == "__main__":
    main()

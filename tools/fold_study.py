#!/usr/bin/env python3
"""The study behind the adapter-palindrome thresholds (DESIGN.md §2 "Adapter palindromes"): tools/fold_synth.py data through the engine with a
ccsx_fold_request.  Per class: the ZMWs, those tested (status SUCCESS after the cascade), those flagged at the default thresholds, the consensus reads the
engine would write without the detector (status SUCCESS, rq >= 0.99), and the range of hits, span and span / shorter arm in tenths over the tested ZMWs.
    python tools/fold_study.py [--out profiles/fold_study.txt]"""
import argparse
import os
import sys

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tools"))
from ccs_amd import api  # noqa: E402
import fold_synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--per-class", type=int, default=128)
    ap.add_argument("--passes", default="6,12")
    ap.add_argument("--length", default="1000,10000")
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    plo, phi = (int(x) for x in a.passes.split(","))
    llo, lhi = (int(x) for x in a.length.split(","))
    n = a.per_class * len(fold_synth.CLASSES)
    b, kinds, _ = fold_synth.make(n, (plo, phi), (llo, lhi), seed=a.seed)
    h = api.Handle(0)
    d = h.draft(b)
    res, rep = h.consensus_fold(b)
    o = api.fold_opts_default()
    lines = [f"adapter palindromes: {n} ZMWs ({a.per_class} per class), {plo}-{phi} passes, templates of {llo}-{lhi} bases, seed {a.seed}",
             f"defaults: max_occ {o.max_occ}, min_hits {o.min_hits}, min_arm {o.min_arm}, min_span_tenths {o.min_span_tenths}, end_slack {o.end_slack}", "",
             f"{'class':12s} {'ZMWs':>5s} {'tested':>6s} {'flagged':>7s} {'HiFi w/o':>8s}   {'hits min-max':>13s} {'span min-max':>13s} {'tenths min-max':>14s}"]
    for k, name in enumerate(fold_synth.CLASSES):
        m = kinds == k
        t = m & (rep.verdict != api.FOLD_UNTESTED)
        fl = m & (rep.verdict == api.FOLD_PALINDROME)
        hifi = m & (res.status == 0) & (res.rq >= 0.99)
        L = np.array([len(d.draft(z)) for z in range(b.n_zmw)])
        shorter = np.maximum(1, np.minimum(rep.fold, L - rep.fold))
        tenths = np.where(rep.fold >= 0, 10 * rep.span // shorter, 0)
        rng_ = lambda v: f"{int(v[t].min()) if t.any() else 0}-{int(v[t].max()) if t.any() else 0}"
        lines.append(f"{name:12s} {int(m.sum()):5d} {int(t.sum()):6d} {int(fl.sum()):7d} {int(hifi.sum()):8d}   {rng_(rep.hits):>13s} {rng_(rep.span):>13s} {rng_(tenths):>14s}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)
    h.close()


if __name__ == "__main__":
    main()

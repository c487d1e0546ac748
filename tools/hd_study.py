#!/usr/bin/env python3
"""The study behind the heteroduplex finder's defaults (DESIGN.md §2 "Heteroduplex rule"; output: profiles/hd_study.txt).

False-positive rate on homoduplex controls (random and low-complexity templates) and recall on planted heteroduplexes, against passes per strand,
number of planted substitutions and indel length.  Default: ccsx_hd_batch on the GPU.  --oracle: the CPU restatement (tests/hd_ref.py) on the
oracle's stages (oracle_lib.poa_draft / windows / align), no GPU needed (slow: use small --scale)."""
import argparse
import os
import sys

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (R, os.path.join(R, "tests"), os.path.join(R, "tools")):
    sys.path.insert(0, p)
from ccs_amd import api  # noqa: E402
import hd_ref  # noqa: E402
import hd_synth  # noqa: E402


def oracle_verdicts(batch, opts):
    import oracle_lib
    zs = []
    for z in range(batch.n_zmw):
        d = oracle_lib.poa_draft(batch, z)
        wb = oracle_lib.windows(d)
        cols = hd_ref.need_cols(wb, len(d))
        reads = []
        for r in range(int(batch.read_off[z]), int(batch.read_off[z + 1])):
            bases, fl = batch.read(r)[0], int(batch.flags[r])
            rs, v, _ = oracle_lib.align(oracle_lib.orient(bases, fl & 1), d)
            reads.append((bases, fl, bool(v), np.array([rs[c] for c in cols], np.int64)))
        zs.append(hd_ref.Zmw(d, wb, 0 if len(d) else 2, 0, reads))
    return np.array([r["verdict"] for r in hd_ref.hd_zmws(zs, opts)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--oracle", action="store_true")
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies every set's ZMW count")
    ap.add_argument("--length", type=int, default=5000)
    a = ap.parse_args()
    o = api.hd_opts_default() if not a.oracle else None
    ro = hd_ref.Opts()
    h = None if a.oracle else api.Handle(0)
    n = lambda k: max(4, int(k * a.scale))

    def flagged(batch):
        if a.oracle:
            v = oracle_verdicts(batch, ro)
        else:
            v = h.hd(batch, h.draft(batch), o).verdict
        return int((v == api.HD_HETERODUPLEX).sum()), int((v == api.HD_DOUBLE_STRAND).sum()), batch.n_zmw

    print(f"# heteroduplex finder study, rule version 1, options {ro}, {a.length}-bp templates, {'oracle stages + restatement' if a.oracle else 'ccsx_hd_batch'}")
    print("# set                      passes/strand  flagged / ZMWs   (DOUBLE_STRAND)")
    seed = 1000
    for pps in (10, 5, 3):
        for tpl in ("random", "lowcx"):
            seed += 1
            f, ds, m = flagged(hd_synth.make(n(2048 if pps == 10 and tpl == "random" else 512), pps, a.length, seed, tpl=tpl, control=True)[0])
            print(f"control {tpl:<18} {pps:>6}        {f:>5} / {m:<6} ({ds})  false-positive rate {f / m:.4f}")
    for pps in (10, 5, 3):
        for k in (1, 2, 4):
            seed += 1
            f, ds, m = flagged(hd_synth.make(n(128), pps, a.length, seed, k_sub=k)[0])
            print(f"substitutions k={k:<10} {pps:>6}        {f:>5} / {m:<6} ({ds})  recall {f / m:.3f}")
        for ln in (21, 30, 50, -30):
            seed += 1
            f, ds, m = flagged(hd_synth.make(n(128), pps, a.length, seed, indel=ln)[0])
            print(f"{'insertion' if ln > 0 else 'deletion'} {abs(ln):>3} bp          {pps:>6}        {f:>5} / {m:<6} ({ds})  recall {f / m:.3f}")
    if h:
        h.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What the pileup summary costs on one batch (default 16384 ZMWs x 10 passes x 10 kb, the bench.py workload), for a kernel trace:
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/pileup_bench.py
Four modes, `--reps` synchronous calls each: plain consensus, pileup alone (ccsx_consensus_pileup), kinetics alone (a handle with hifi_kinetics) and both.
One JSON line: per mode the polish stage (k_polish + the kinetics / pileup kernel) and the stitch (k_stitch + k_pile_stitch) in ms, from the handle's
events, median over the calls.  The per-kernel split comes from the trace (k_kinetics_t<KIN, PILE>)."""
import argparse
import json
import os
import sys

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
from ccs_amd import api  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--zmws", type=int, default=16384)
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--length", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    b = api.synth(a.zmws, a.passes, a.length, seed=1)
    out = dict(zmws=a.zmws, passes=a.passes, length=a.length)
    for name, kin, pile in (("plain", 0, False), ("pileup", 0, True), ("kinetics", 1, False), ("both", 1, True)):
        opts = api.default_opts(); opts.hifi_kinetics = kin
        h = api.Handle(0, opts=opts)
        pol, sti = [], []
        for _ in range(a.reps):
            if pile:
                h.consensus_pileup(b)
            else:
                h.consensus(b)
            t = h.timings()
            pol.append(t.polish_ms); sti.append(t.stitch_ms)
        out[name] = dict(polish_ms=round(float(np.median(pol)), 2), stitch_ms=round(float(np.median(sti)), 2))
        h.close()
    for name in ("pileup", "kinetics", "both"):
        out[name]["adds_ms"] = round(out[name]["polish_ms"] + out[name]["stitch_ms"] - out["plain"]["polish_ms"] - out["plain"]["stitch_ms"], 2)
    out["both_over_kinetics_ms"] = round(out["both"]["adds_ms"] - out["kinetics"]["adds_ms"], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

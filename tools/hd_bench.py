#!/usr/bin/env python3
"""Drives ccsx_hd_batch on one batch (default 16384 ZMWs x 10 passes x 10 kb, the bench.py workload) for a kernel trace of the heteroduplex finder:
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/hd_bench.py
The draft stage runs first (ccsx_draft_batch), then ccsx_hd_batch `--reps` times; one JSON line with the wall time of each call and the verdict counts."""
import argparse
import json
import os
import sys
import time

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
    h = api.Handle(0)
    d = h.draft(b)
    wall = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        rep = h.hd(b, d)
        wall.append((time.perf_counter() - t0) * 1e3)
    t = h.timings()
    v = np.bincount(rep.verdict, minlength=3)
    print(json.dumps(dict(zmws=a.zmws, passes=a.passes, length=a.length, hd_call_ms=[round(x, 1) for x in wall],
                          align_ms=round(t.align_ms, 2), hd_kernels_ms=round(t.polish_ms + t.stitch_ms, 2),
                          verdicts={api.HD_VERDICT_NAMES[k]: int(v[k]) for k in range(3)})))
    h.close()


if __name__ == "__main__":
    main()

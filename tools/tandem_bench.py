#!/usr/bin/env python3
"""What tandem-repeat detection costs on one batch (default 16384 ZMWs x 10 passes x 10 kb, the bench.py workload), for a kernel trace:
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/tandem_bench.py
Three modes, `--reps` synchronous calls each: plain consensus, detection only (tandem_len, threshold 0) and the per-ZMW switch at --min-len.
One JSON line: per mode the draft stage (POA + k_sdust) and the whole step in ms from the handle's events, median over the calls, and the
ZMWs flagged.  k_sdust's own time comes from the trace."""
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
    ap.add_argument("--min-len", type=int, default=1000)
    a = ap.parse_args()
    b = api.synth(a.zmws, a.passes, a.length, seed=1)
    out = dict(zmws=a.zmws, passes=a.passes, length=a.length)
    h = api.Handle(0)
    for name, tandem, thr in (("plain", False, 0), ("detect", True, 0), ("switch", True, a.min_len)):
        dr, tot, flagged = [], [], 0
        for _ in range(a.reps):
            if tandem:
                _, tl, _ = h.consensus_extras(b, tandem=True, min_tandem_repeat_length=thr)
                flagged = int((tl >= thr).sum()) if thr > 0 else 0
                out.setdefault("tandem_len_max", int(tl.max()))
            else:
                h.consensus(b)
            t = h.timings()
            dr.append(t.draft_ms); tot.append(t.total_ms)
        out[name] = dict(draft_ms=round(float(np.median(dr)), 2), total_ms=round(float(np.median(tot)), 2), flagged=flagged)
    h.close()
    for name in ("detect", "switch"):
        out[name]["adds_ms"] = round(out[name]["total_ms"] - out["plain"]["total_ms"], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

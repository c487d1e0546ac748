#!/usr/bin/env python3
"""What adapter-palindrome detection costs in the fused, ticketed path (default 16384 ZMWs x 10 passes x 10 kb, the bench.py workload).  For a kernel trace:
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/fold_bench.py
The batch goes through `--steps` tickets (three in flight, after `--warmup` tickets) without and with a ccsx_fold_request, alternating `--rounds` times; one
JSON line gives per configuration the best round's ZMWs/s and step time, the mean per-ticket stage times, and the verdicts of the last ticket."""
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
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    a = ap.parse_args()
    b = api.synth(a.zmws, a.passes, a.length, seed=1).pinned()
    h = api.Handle(0)
    res = [api.Results.allocate(b, pinned=True, raw=False) for _ in range(3)]
    reps = [api.FoldReport.allocate(b.n_zmw, pinned=True) for _ in range(3)]
    out = dict(zmws=a.zmws, passes=a.passes, length=a.length, steps=a.steps, warmup=a.warmup, rounds=a.rounds)

    def run(k, fold):
        ts = [h.submit(b, res[i % 3], fold=reps[i % 3] if fold else None) for i in range(k)]   # (a submit that reuses a slot retires its ticket)
        for t in ts[-3:]:
            h.wait(t)
        tm = [h.ticket_timings(t) for t in ts[-3:]]
        for t in ts:
            h.release(t)
        return tm

    for _ in range(a.rounds):
        for name, fold in (("no_fold", False), ("fold", True)):
            run(a.warmup, fold)
            t0 = time.perf_counter()
            tm = run(a.steps, fold)
            wall = time.perf_counter() - t0
            r = dict(zmws_per_s=round(a.steps * a.zmws / wall, 1), step_ms=round(wall * 1e3 / a.steps, 1))
            for f in ("draft_ms", "align_ms", "polish_ms", "total_ms"):
                r[f] = round(float(np.mean([getattr(x, f) for x in tm])), 2)
            if fold:
                v = np.bincount(reps[(a.steps - 1) % 3].verdict, minlength=3)
                r["verdicts"] = dict(untested=int(v[0]), none=int(v[1]), palindrome=int(v[2]))
            if name not in out or r["zmws_per_s"] > out[name]["zmws_per_s"]:
                out[name] = r
    out["fold_adds_pct"] = round(100.0 * (out["fold"]["step_ms"] / out["no_fold"]["step_ms"] - 1.0), 2)
    print(json.dumps(out))
    h.close()


if __name__ == "__main__":
    main()

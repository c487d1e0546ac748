#!/usr/bin/env python3
"""Drives ccsx_hd_batch on one batch (default 16384 ZMWs x 10 passes x 10 kb, the bench.py workload) for a kernel trace of the heteroduplex finder:
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/hd_bench.py
The draft stage runs first (ccsx_draft_batch), then ccsx_hd_batch `--reps` times; one JSON line with the wall time of each call and the verdict counts.

--fused: the finder in the fused, ticketed path instead (ccsx_submit_hd).  The batch goes through `--steps` tickets (three in flight, after `--warmup`
tickets) in each of three configurations — no request, a request with split = 0, a request with split = 1 — and one JSON line gives ZMWs/s and the
mean per-ticket stage times of each."""
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
    ap.add_argument("--fused", action="store_true", help="the finder on tickets of the fused path: no HD / HD split 0 / HD split 1")
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    b = api.synth(a.zmws, a.passes, a.length, seed=1)
    if a.fused:
        return fused(a, b)
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


def fused(a, b):
    b = b.pinned()
    h = api.Handle(0)
    res = [api.Results.allocate(b, pinned=True, raw=False) for _ in range(3)]
    reps = [api.HdReport.allocate(b.n_zmw, pinned=True) for _ in range(3)]
    out = dict(zmws=a.zmws, passes=a.passes, length=a.length, steps=a.steps, warmup=a.warmup)
    for name, hd, split in (("no_hd", False, False), ("hd_split0", True, False), ("hd_split1", True, True)):
        def run(k):
            ts = []
            for i in range(k):                 # (a submit that reuses a slot retires its ticket: three in flight)
                ts.append(h.submit(b, res[i % 3], hd=reps[i % 3] if hd else None, hd_split=split))
            for t in ts[-3:]:
                h.wait(t)
            tm = [h.ticket_timings(t) for t in ts[-3:]]
            for t in ts:
                h.release(t)
            return tm
        run(a.warmup)
        t0 = time.perf_counter()
        tm = run(a.steps)
        wall = time.perf_counter() - t0
        r = dict(zmws_per_s=round(a.steps * a.zmws / wall, 1), step_ms=round(wall * 1e3 / a.steps, 1))
        for f in ("draft_ms", "align_ms", "polish_ms", "total_ms"):
            r[f] = round(float(np.mean([getattr(x, f) for x in tm])), 2)
        last = (a.steps - 1) % 3
        if hd:
            v = np.bincount(reps[last].verdict, minlength=3)
            r["verdicts"] = {api.HD_VERDICT_NAMES[k]: int(v[k]) for k in range(3)}
        r["statuses"] = {api.STATUS_NAMES[int(k)]: int(c) for k, c in zip(*np.unique(res[last].status, return_counts=True))}
        out[name] = r
    print(json.dumps(out))
    h.close()


if __name__ == "__main__":
    main()

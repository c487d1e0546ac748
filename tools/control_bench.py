#!/usr/bin/env python3
"""What the control screen costs in the fused, ticketed path (default 16384 ZMWs x 10 passes x 10 kb, the bench.py workload, against a 2000-base control).  For a
kernel trace:
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/control_bench.py --rounds 1 --steps 3 --warmup 1
The batch goes through `--steps` tickets (three in flight, after `--warmup` tickets) without and with a ccsx_control_request, alternating `--rounds` times in the
same process; one JSON line gives per configuration the best round's ZMWs/s and step time, every round's step time of the no-request configuration and their
spread, the mean per-ticket stage times, and the screen's counts on the last ticket.  The number to hold is the step time with the request against the step time
without it in the same run, next to that spread."""
import argparse
import json
import os
import sys
import time

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tools"))
from ccs_amd import api  # noqa: E402
import control_synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--zmws", type=int, default=16384)
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--length", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    b = api.synth(a.zmws, a.passes, a.length, seed=1).pinned()
    h = api.Handle(0)
    res = [api.Results.allocate(b, pinned=True, raw=False) for _ in range(3)]
    reps = [api.ControlReport.allocate(b.n_zmw, pinned=True) for _ in range(3)]
    seq = api.ControlSeq.from_string(control_synth.TEST_CONTROL)
    out = dict(zmws=a.zmws, passes=a.passes, length=a.length, steps=a.steps, warmup=a.warmup, rounds=a.rounds, control_bases=seq.len)

    def run(k, screen):
        ts = [h.submit(b, res[i % 3], control=reps[i % 3] if screen else None, control_seq=seq) for i in range(k)]   # (a submit that reuses a slot retires its ticket)
        for t in ts[-3:]:
            h.wait(t)
        tm = [h.ticket_timings(t) for t in ts[-3:]]
        for t in ts:
            h.release(t)
        return tm

    every = dict(no_control=[], control=[])
    for _ in range(a.rounds):
        for name, screen in (("no_control", False), ("control", True)):
            run(a.warmup, screen)
            t0 = time.perf_counter()
            tm = run(a.steps, screen)
            wall = time.perf_counter() - t0
            r = dict(zmws_per_s=round(a.steps * a.zmws / wall, 1), step_ms=round(wall * 1e3 / a.steps, 2))
            every[name].append(r["step_ms"])
            for f in ("draft_ms", "align_ms", "polish_ms", "total_ms"):
                r[f] = round(float(np.mean([getattr(x, f) for x in tm])), 2)
            if screen:
                rep = reps[(a.steps - 1) % 3]
                r["screen"] = dict(tested=int((rep.verdict != 0).sum()), with_hits=int((rep.hits > 0).sum()), found=int((rep.verdict == 2).sum()))
            if name not in out or r["zmws_per_s"] > out[name]["zmws_per_s"]:
                out[name] = r
    out["step_ms_by_round"] = every
    nc = every["no_control"]
    out["no_control_spread_pct"] = round(100.0 * (max(nc) - min(nc)) / min(nc), 2)
    out["control_adds_pct"] = round(100.0 * (out["control"]["step_ms"] / out["no_control"]["step_ms"] - 1.0), 2)
    print(json.dumps(out))
    h.close()


if __name__ == "__main__":
    main()

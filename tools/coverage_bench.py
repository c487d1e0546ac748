#!/usr/bin/env python3
"""What the coverage screen costs in the fused, ticketed path (default 16384 ZMWs x 10 passes x 10 kb, the bench.py workload).  For a kernel trace:
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/coverage_bench.py --rounds 1 --steps 3 --warmup 1
The batch goes through `--steps` tickets (three in flight, after `--warmup` tickets) without a ccsx_coverage_request, with one at gate 0 (detection only) and
with one at every gate bit, alternating `--rounds` times in the same process; one JSON line gives per configuration the best round's ZMWs/s and step time, every
round's step time and the spread of the no-request configuration, the mean per-ticket stage times, and the screen's counts on the last ticket.  The number to
hold is the step time with the request against the step time without it in the same run, next to that spread.  --out FILE: the lines of
profiles/coverage_bench.txt, every one written here."""
import argparse
import json
import os
import sys
import time

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
from ccs_amd import api  # noqa: E402

CONFIGS = (("no_request", None), ("gate_0", 0), ("gate_all", api.COVERAGE_GATE_ALL))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--zmws", type=int, default=16384)
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--length", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    b = api.synth(a.zmws, a.passes, a.length, seed=1).pinned()
    h = api.Handle(0)
    res = [api.Results.allocate(b, pinned=True, raw=False) for _ in range(3)]
    reps = [api.CoverageReport.allocate(b.n_zmw, pinned=True) for _ in range(3)]
    out = dict(zmws=a.zmws, passes=a.passes, length=a.length, steps=a.steps, warmup=a.warmup, rounds=a.rounds)

    def run(k, gate):
        ts = [h.submit(b, res[i % 3], coverage=reps[i % 3] if gate is not None else None, coverage_gate=gate or 0) for i in range(k)]   # (a submit that reuses a slot retires its ticket)
        for t in ts[-3:]:
            h.wait(t)
        tm = [h.ticket_timings(t) for t in ts[-3:]]
        for t in ts:
            h.release(t)
        return tm

    every = {name: [] for name, _ in CONFIGS}
    for _ in range(a.rounds):
        for name, gate in CONFIGS:
            run(a.warmup, gate)
            t0 = time.perf_counter()
            tm = run(a.steps, gate)
            wall = time.perf_counter() - t0
            r = dict(zmws_per_s=round(a.steps * a.zmws / wall, 1), step_ms=round(wall * 1e3 / a.steps, 2))
            every[name].append(r["step_ms"])
            for f in ("draft_ms", "align_ms", "polish_ms", "total_ms"):
                r[f] = round(float(np.mean([getattr(x, f) for x in tm])), 2)
            if gate is not None:
                rep = reps[(a.steps - 1) % 3]
                r["screen"] = dict(tested=int((rep.verdict != 0).sum()), **{api.STATUS_NAMES[9 + v].lower(): int((rep.verdict == v).sum()) for v in range(2, 6)},
                                   lost_segments=int((rep.reach_sum - rep.used_sum)[rep.used_sum > 0].sum()), reach_segments=int(rep.reach_sum[rep.used_sum > 0].sum()),
                                   gated=int((res[(a.steps - 1) % 3].status >= 11).sum()))
            if name not in out or r["zmws_per_s"] > out[name]["zmws_per_s"]:
                out[name] = r
    out["step_ms_by_round"] = every
    nr = every["no_request"]
    out["no_request_spread_pct"] = round(100.0 * (max(nr) - min(nr)) / min(nr), 2)
    for name in ("gate_0", "gate_all"):
        out[name + "_adds_pct"] = round(100.0 * (out[name]["step_ms"] / out["no_request"]["step_ms"] - 1.0), 2)
        out[name + "_adds_pct_mean"] = round(100.0 * (float(np.mean(every[name])) / float(np.mean(nr)) - 1.0), 2)
    line = json.dumps(out)
    print(line)
    if a.out:
        fmt = lambda v: " ".join(f"{x:.2f}" for x in v)
        s = out["gate_all"]["screen"]
        with open(a.out, "w") as f:
            f.write(f"python tools/coverage_bench.py   (MI355X; {a.zmws} ZMWs x {a.passes} passes x {a.length} bases, {a.steps} tickets with three in flight after {a.warmup} "
                    f"warm-up\ntickets, without a ccsx_coverage_request, with one at gate 0 and with one at every gate bit, alternating {a.rounds} rounds in one process)\n\n")
            f.write(line + "\n\n")
            f.write(f"ms per step by round: without the request {fmt(nr)} (spread {out['no_request_spread_pct']:.2f} %), gate 0 {fmt(every['gate_0'])}, "
                    f"every gate bit {fmt(every['gate_all'])}.\n")
            f.write(f"Best round against best round: gate 0 {out['gate_0_adds_pct']:+.2f} %, every gate bit {out['gate_all_adds_pct']:+.2f} %; mean against mean "
                    f"{out['gate_0_adds_pct_mean']:+.2f} % and {out['gate_all_adds_pct_mean']:+.2f} %.\n")
            f.write(f"The screen on the last ticket with every gate bit: {s['tested']} of {a.zmws} ZMWs tested, {s['gated']} gated "
                    f"({s['draft_too_different']} draft too different, {s['insufficient_spans']} insufficient spans, {s['coverage_drops']} coverage drops, "
                    f"{s['reads_failed_polishing']} reads failed polishing); the polish used all but {s['lost_segments']} of the {s['reach_segments']} reaching segments of the ZMWs it ran on.\n")
    h.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What the pass orientation costs in the fused, ticketed path (default 16384 ZMWs x 10 passes x 10 kb, the bench.py workload).  For a kernel trace:
    rocprofv3 --kernel-trace --stats -d OUT -o trace -- python tools/orient_bench.py --rounds 1 --steps 3 --warmup 1
    python tools/orient_bench.py --trace-summary OUT --out profiles/orient_rocprofv3_summary.txt
The batch goes through `--steps` tickets (three in flight, after `--warmup` tickets) with no pass flagged and with every pass flagged CCSX_PASS_STRAND_UNKNOWN
(its true bit as the prior), alternating `--rounds` times in the same process; one JSON line gives per configuration the best round's ZMWs/s and step time, every
round's step time and the spread of the no-flag configuration, the mean per-ticket stage times, and the calls of the last flagged ticket's batch (the seam, once,
outside the timed part).  The number to hold is the step time with every pass flagged against the step time with none in the same run, best against best, next to
that spread.  --out FILE: the lines of profiles/orient_bench.txt, every one written here."""
import argparse
import glob
import json
import os
import sqlite3
import sys
import time

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
from ccs_amd import api  # noqa: E402

CONFIGS = ("no_flag", "all_flagged")


def trace_summary(root, out):
    """per-kernel durations of a rocprofv3 --kernel-trace run (its rocpd database under `root`), and k_orient's ms per step"""
    dbs = sorted(glob.glob(os.path.join(root, "**", "*_results.db"), recursive=True))
    if not dbs:
        sys.exit(f"no *_results.db under {root}")
    rows = sqlite3.connect(dbs[0]).execute("select name, count(*), sum(end-start), avg(end-start), min(end-start), max(end-start) from kernels group by name order by 3 desc").fetchall()
    tot = sum(r[2] for r in rows) or 1
    lines = ["pass orientation in the fused, ticketed path: rocprofv3 --kernel-trace --stats -- python tools/orient_bench.py --rounds 1 --steps 3 --warmup 1",
             "(16384 ZMWs x 10 passes x 10 kb; 4 tickets with no pass flagged, then 4 with every pass flagged: k_orient runs in 4 of the 8 steps, and once more in the",
             "seam call that counts the calls; no counters in this run)", "",
             f"{'kernel':40s} {'calls':>6s} {'total_ms':>12s} {'avg_ms':>12s} {'min_ms':>12s} {'max_ms':>12s} {'pct':>7s}"]
    for n, k, s, a, mn, mx in rows:
        lines.append(f"{n[:40]:40s} {k:6d} {s / 1e6:12.3f} {a / 1e6:12.3f} {mn / 1e6:12.3f} {mx / 1e6:12.3f} {100 * s / tot:7.2f}")
    ko = [r for r in rows if r[0].startswith("k_orient")]
    lines += ["", f"k_orient: {ko[0][3] / 1e6:.3f} ms per step (one launch per batch that carries the bit, {ko[0][1]} launches)" if ko else "k_orient: not in the trace"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        with open(out, "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--zmws", type=int, default=16384)
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--length", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-summary", default=None)
    a = ap.parse_args()
    if a.trace_summary:
        return trace_summary(a.trace_summary, a.out)
    plain = api.synth(a.zmws, a.passes, a.length, seed=1).pinned()
    batches = dict(no_flag=plain, all_flagged=plain.with_unknown_strands())
    h = api.Handle(0)
    res = [api.Results.allocate(plain, pinned=True, raw=False) for _ in range(3)]
    out = dict(zmws=a.zmws, passes=a.passes, length=a.length, steps=a.steps, warmup=a.warmup, rounds=a.rounds)

    def run(k, b):
        ts = [h.submit(b, res[i % 3]) for i in range(k)]              # (a submit that reuses a slot retires its ticket)
        for t in ts[-3:]:
            h.wait(t)
        tm = [h.ticket_timings(t) for t in ts[-3:]]
        for t in ts:
            h.release(t)
        return tm

    every = {name: [] for name in CONFIGS}
    status = {}
    for _ in range(a.rounds):
        for name in CONFIGS:
            run(a.warmup, batches[name])
            t0 = time.perf_counter()
            tm = run(a.steps, batches[name])
            wall = time.perf_counter() - t0
            r = dict(zmws_per_s=round(a.steps * a.zmws / wall, 1), step_ms=round(wall * 1e3 / a.steps, 2))
            every[name].append(r["step_ms"])
            for f in ("draft_ms", "align_ms", "polish_ms", "total_ms"):
                r[f] = round(float(np.mean([getattr(x, f) for x in tm])), 2)
            status[name] = res[(a.steps - 1) % 3].status.copy(), res[(a.steps - 1) % 3].seq_len.copy()
            if name not in out or r["zmws_per_s"] > out[name]["zmws_per_s"]:
                out[name] = r
    rep = h.orient(batches["all_flagged"])
    out["calls"] = {api.ORIENT_CALL_NAMES[c].lower(): int((rep.call == c).sum()) for c in range(6)}
    out["same_results"] = bool(np.array_equal(status["no_flag"][0], status["all_flagged"][0]) and np.array_equal(status["no_flag"][1], status["all_flagged"][1]))
    out["step_ms_by_round"] = every
    nf = every["no_flag"]
    out["no_flag_spread_pct"] = round(100.0 * (max(nf) - min(nf)) / min(nf), 2)
    out["all_flagged_adds_pct"] = round(100.0 * (out["all_flagged"]["step_ms"] / out["no_flag"]["step_ms"] - 1.0), 2)
    out["all_flagged_adds_pct_mean"] = round(100.0 * (float(np.mean(every["all_flagged"])) / float(np.mean(nf)) - 1.0), 2)
    line = json.dumps(out)
    print(line)
    if a.out:
        fmt = lambda v: " ".join(f"{x:.2f}" for x in v)
        c = out["calls"]
        with open(a.out, "w") as f:
            f.write(f"python tools/orient_bench.py   (MI355X; {a.zmws} ZMWs x {a.passes} passes x {a.length} bases, {a.steps} tickets with three in flight after {a.warmup} "
                    f"warm-up\ntickets, with no pass flagged and with every pass flagged CCSX_PASS_STRAND_UNKNOWN, alternating {a.rounds} rounds in one process)\n\n")
            f.write(line + "\n\n")
            f.write(f"ms per step by round: no pass flagged {fmt(nf)} (spread {out['no_flag_spread_pct']:.2f} %), every pass flagged {fmt(every['all_flagged'])}.\n")
            f.write(f"Best round against best round: every pass flagged {out['all_flagged_adds_pct']:+.2f} %; mean against mean {out['all_flagged_adds_pct_mean']:+.2f} %.\n")
            f.write(f"Draft stage (draft_ms + align_ms of a ticket, k_orient included): {out['no_flag']['draft_ms'] + out['no_flag']['align_ms']:.2f} ms with no pass flagged, "
                    f"{out['all_flagged']['draft_ms'] + out['all_flagged']['align_ms']:.2f} ms with every pass flagged; polish stage {out['no_flag']['polish_ms']:.2f} / "
                    f"{out['all_flagged']['polish_ms']:.2f} ms.\n")
            f.write(f"The calls on the flagged batch: {c['anchor']} anchors, {c['same']} same, {c['opposite']} opposite, {c['undetermined']} undetermined of "
                    f"{a.zmws * a.passes} passes; statuses and lengths of the last flagged ticket equal the unflagged one's: {out['same_results']}.\n")
    h.close()


if __name__ == "__main__":
    main()

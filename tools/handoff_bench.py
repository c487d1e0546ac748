#!/usr/bin/env python3
"""What the polisher hand-off costs in the fused, ticketed path (default 16384 ZMWs x 10 passes x 10 kb, the bench.py workload).  For a kernel trace:
    rocprofv3 --kernel-trace --stats -d OUT -o trace -- python tools/handoff_bench.py --rounds 1 --steps 3 --warmup 1
    python tools/handoff_bench.py --trace-summary OUT --out profiles/handoff_rocprofv3_summary.txt
The batch goes through `--steps` tickets (three in flight, after `--warmup` tickets) without the request, with it at the default options into torch tensors on
the GPU, and with it into page-locked host memory, alternating `--rounds` times in the same process; one JSON line gives per configuration the best round's
ZMWs/s and step time, every round's step time, the spread of the no-request configuration, counts and the bytes the request moves.  The numbers to hold are
the step times with the request against the step time without it in the same run, best against best and mean against mean, next to that spread.
--out FILE: the lines of profiles/handoff_bench.txt, every one written here."""
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

CONFIGS = ("no_request", "device", "pinned_host")
KERNELS = ("k_tile_select", "k_tile_scan", "k_tile_rows")


def trace_summary(root, out):
    """per-kernel durations of a rocprofv3 --kernel-trace run (its rocpd database under `root`), and the three hand-off kernels' ms per step"""
    dbs = sorted(glob.glob(os.path.join(root, "**", "*_results.db"), recursive=True))
    if not dbs:
        sys.exit(f"no *_results.db under {root}")
    rows = sqlite3.connect(dbs[0]).execute("select name, count(*), sum(end-start), avg(end-start), min(end-start), max(end-start) from kernels group by name order by 3 desc").fetchall()
    tot = sum(r[2] for r in rows) or 1
    steps = max([r[1] for r in rows if r[0].startswith("k_stitch")] or [0])
    asked = max([r[1] for r in rows if r[0].startswith(KERNELS)] or [0])
    lines = ["the polisher hand-off in the fused, ticketed path: a rocprofv3 --kernel-trace --stats run of tools/handoff_bench.py (no counters in this run)",
             f"{steps} tickets in the trace, warm-up tickets and the max_tiles probe included; {asked} of them carried the hand-off request", "",
             f"{'kernel':40s} {'calls':>6s} {'total_ms':>12s} {'avg_ms':>12s} {'min_ms':>12s} {'max_ms':>12s} {'pct':>7s}"]
    for n, k, s, a, mn, mx in rows:
        lines.append(f"{n[:40]:40s} {k:6d} {s / 1e6:12.3f} {a / 1e6:12.3f} {mn / 1e6:12.3f} {mx / 1e6:12.3f} {100 * s / tot:7.2f}")
    lines.append("")
    for kn in KERNELS:
        kr = [r for r in rows if r[0].startswith(kn)]
        lines.append(f"{kn}: {kr[0][3] / 1e6:.3f} ms per launch ({kr[0][1]} launches)" if kr else f"{kn}: not in the trace")
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
    ap.add_argument("--max-tiles", type=int, default=0, help="capacity of the hand-off arrays in tiles (0: a first run's count of selected tiles, rounded up)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-summary", default=None)
    a = ap.parse_args()
    if a.trace_summary:
        return trace_summary(a.trace_summary, a.out)
    import torch                                               # BEFORE the first call into libccsx.so: the two share one HIP runtime only in this order
    torch.cuda.init()
    from ccs_amd import api
    plain = api.synth(a.zmws, a.passes, a.length, seed=1).pinned()
    h = api.Handle(0)
    res = [api.Results.allocate(plain, pinned=True, raw=False) for _ in range(3)]
    o = api.handoff_opts_default()
    out = dict(zmws=a.zmws, passes=a.passes, length=a.length, steps=a.steps, warmup=a.warmup, rounds=a.rounds, tile_len=o.tile_len, max_rows=o.max_rows,
               skip_above=o.skip_above)
    if a.max_tiles <= 0:                                       # the capacity an integrator would give it: what the batch selects, with a little room
        probe = api.Handoff.allocate(plain, 1, o)
        t = h.submit(plain, res[0], handoff=probe)
        h.wait(t)
        h.release(t)
        a.max_tiles = min(max(64, int(probe.counts[1]) * 9 // 8), 1 << 17)   # (at most 1 GB per destination at the defaults; counts shows a truncation)
    dests = dict(no_request=[None] * 3, device=[api.Handoff.allocate(plain, a.max_tiles, o, device=0) for _ in range(3)],
                 pinned_host=[api.Handoff.allocate(plain, a.max_tiles, o, pinned=True) for _ in range(3)])
    out["max_tiles"] = a.max_tiles
    out["bytes_per_ticket"] = int(sum(np.prod(sh) * np.dtype(dt).itemsize for sh, dt in api.Handoff.shapes(a.max_tiles, o).values()))

    def run(k, ho):
        ts = [h.submit(plain, res[i % 3], handoff=ho[i % 3]) for i in range(k)]      # (a submit that reuses a slot retires its ticket)
        for t in ts[-3:]:
            h.wait(t)
        tm = [h.ticket_timings(t) for t in ts[-3:]]
        for t in ts:
            h.release(t)
        return tm

    every = {name: [] for name in CONFIGS}
    keep = {}
    for _ in range(a.rounds):
        for name in CONFIGS:
            run(a.warmup, dests[name])
            t0 = time.perf_counter()
            tm = run(a.steps, dests[name])
            wall = time.perf_counter() - t0
            r = dict(zmws_per_s=round(a.steps * a.zmws / wall, 1), step_ms=round(wall * 1e3 / a.steps, 2))
            every[name].append(r["step_ms"])
            for f in ("polish_ms", "stitch_ms", "total_ms"):
                r[f] = round(float(np.mean([getattr(x, f) for x in tm])), 2)
            last = (a.steps - 1) % 3
            keep[name] = (res[last].status.copy(), res[last].seq_len.copy(), None if dests[name][last] is None else dests[name][last].host())
            if name not in out or r["zmws_per_s"] > out[name]["zmws_per_s"]:
                out[name] = r
    dv, ph = keep["device"][2], keep["pinned_host"][2]
    out["counts"] = [int(x) for x in ph.counts]
    n = ph.n_tiles
    out["device_equals_host"] = bool(dv.counts.tolist() == ph.counts.tolist() and all(np.array_equal(getattr(dv, k)[:n], getattr(ph, k)[:n]) for k in ph.FIELDS[1:]))
    out["same_results"] = bool(all(np.array_equal(keep["no_request"][i], keep[c][i]) for c in CONFIGS[1:] for i in (0, 1)))
    out["step_ms_by_round"] = every
    nr = every["no_request"]
    out["no_request_spread_pct"] = round(100.0 * (max(nr) - min(nr)) / min(nr), 2)
    for c in CONFIGS[1:]:
        out[c + "_adds_pct"] = round(100.0 * (out[c]["step_ms"] / out["no_request"]["step_ms"] - 1.0), 2)
        out[c + "_adds_pct_mean"] = round(100.0 * (float(np.mean(every[c])) / float(np.mean(nr)) - 1.0), 2)
    line = json.dumps(out)
    print(line)
    if a.out:
        fmt = lambda v: " ".join(f"{x:.2f}" for x in v)
        with open(a.out, "w") as f:
            f.write(f"python tools/handoff_bench.py   (MI355X; {a.zmws} ZMWs x {a.passes} passes x {a.length} bases, {a.steps} tickets with three in flight after {a.warmup} "
                    f"warm-up\ntickets, without the hand-off request, with it at the default options (tile_len {o.tile_len}, max_rows {o.max_rows}, skip_above {o.skip_above}) "
                    f"into torch tensors on the GPU and\ninto page-locked host memory, max_tiles {a.max_tiles}, alternating {a.rounds} rounds in one process)\n\n")
            f.write(line + "\n\n")
            f.write(f"ms per step by round: no request {fmt(nr)} (spread {out['no_request_spread_pct']:.2f} %), device destination {fmt(every['device'])}, "
                    f"page-locked host {fmt(every['pinned_host'])}.\n")
            for c, what in (("device", "device destination"), ("pinned_host", "page-locked host destination")):
                f.write(f"Best round against best round: {what} {out[c + '_adds_pct']:+.2f} %; mean against mean {out[c + '_adds_pct_mean']:+.2f} %.\n")
            f.write(f"counts: {out['counts'][0]} tiles, {out['counts'][1]} selected; the ticketed form copies the whole capacity: {out['bytes_per_ticket']} bytes per ticket.\n")
            f.write(f"Stitch stage of a ticket (k_stitch and the three hand-off kernels): {out['no_request']['stitch_ms']:.2f} ms without the request, "
                    f"{out['device']['stitch_ms']:.2f} / {out['pinned_host']['stitch_ms']:.2f} ms with it.\n")
            f.write(f"The device destination's bytes equal the host destination's: {out['device_equals_host']}; statuses and lengths with the request equal those without: "
                    f"{out['same_results']}.\n")
    h.close()


if __name__ == "__main__":
    main()

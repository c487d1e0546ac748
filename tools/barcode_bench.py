#!/usr/bin/env python3
"""What the barcode calls cost.  Two parts, every line of profiles/barcode_bench.txt written here:
  1. k_barcode alone on resident reads (tools/barcode_bench/kernel_bench.hip, built here with hipcc): 16384 reads, 96 and 384 barcodes, windows 64 and 256.
  2. the two-stage step of 16384 ZMWs x 10 passes x 10 kb (the bench.py workload) through tickets, three in flight: without the request, with it (96 16-mers,
     default options), and — given --parent ROOT, a built checkout of the parent commit — the parent's library, each in a process of its own, alternating
     `--rounds` times.  Median and min-max of the ms per step; "off" and "parent" must lie inside each other's spread.
For the kernel's time per ticket, a kernel trace in a run of its own:
    rocprofv3 --kernel-trace --stats -d OUT -o trace -- python tools/barcode_bench.py --child on --steps 3 --warmup 1
    python tools/barcode_bench.py --trace-summary OUT --out profiles/barcode_rocprofv3_summary.txt
--build-only: compile kernel_bench and stop (no GPU needed).  The build, the ticket loop and the rounds are tools/reads_bench.py's, shared with the other two."""
import argparse
import glob
import os
import sqlite3
import subprocess
import sys

import numpy as np

import reads_bench as RB

DEPS = ("ccsx_barcode.hip", "ccsx_barcode_api.cpp", "barcode_core.h", "wave_ops.h")


def child(a):
    """one configuration in this process (tools/reads_bench.py timed_tickets); one JSON line"""
    sys.path.insert(0, a.root or RB.R)
    from ccs_amd import api
    b = api.synth(a.zmws, a.passes, a.length, seed=1).pinned()

    def request(api, n):
        if a.child != "on":
            return None
        rng = np.random.default_rng(11)
        return dict(barcodes=api.BarcodeReport.allocate(n, pinned=True), barcode_set=api.BarcodeSet.from_codes([rng.integers(0, 4, 16).astype(np.uint8) for _ in range(96)]))

    def summary(kw):
        rep = kw["barcodes"]
        return dict(tested=int(rep.tested.sum()), called_ends=int((rep.call & 1).sum() + (rep.call >> 1).sum()))
    RB.timed_tickets(a, b, request, summary if a.child == "on" else None)


def trace_summary(root, out):
    dbs = sorted(glob.glob(os.path.join(root, "**", "*_results.db"), recursive=True))
    if not dbs:
        sys.exit(f"no *_results.db under {root}")
    rows = sqlite3.connect(dbs[0]).execute("select name, count(*), sum(end-start), avg(end-start), min(end-start), max(end-start) from kernels group by name order by 3 desc").fetchall()
    tot = sum(r[2] for r in rows) or 1
    lines = ["barcode calls in the fused, ticketed path: a rocprofv3 --kernel-trace --stats run of tools/barcode_bench.py --child on (no counters in this run)", "",
             f"{'kernel':40s} {'calls':>6s} {'total_ms':>12s} {'avg_ms':>12s} {'min_ms':>12s} {'max_ms':>12s} {'pct':>7s}"]
    for n, k, s, av, mn, mx in rows:
        lines.append(f"{n[:40]:40s} {k:6d} {s / 1e6:12.3f} {av / 1e6:12.3f} {mn / 1e6:12.3f} {mx / 1e6:12.3f} {100 * s / tot:7.2f}")
    kb = [r for r in rows if "k_barcode" in r[0]]
    kp = [r for r in rows if "k_polish" in r[0]]
    lines += ["", f"k_barcode: {kb[0][3] / 1e6:.3f} ms per ticket ({kb[0][1]} tickets)" + (f", {100 * kb[0][3] / kp[0][3]:.3f} % of k_polish's {kp[0][3] / 1e6:.1f} ms" if kp else "")
              if kb else "k_barcode: not in the trace"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        with open(out, "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser()
    RB.add_step_arguments(ap)
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--build-only", action="store_true")
    ap.add_argument("--trace-summary", default=None)
    a = ap.parse_args()
    if a.trace_summary:
        return trace_summary(a.trace_summary, a.out)
    if a.build_only:
        return RB.build_kernel_bench("barcode", DEPS)
    if a.child:
        return child(a)
    lines = ["python tools/barcode_bench.py   (MI355X)", ""]
    if not a.skip_kernel:
        exe = RB.build_kernel_bench("barcode", DEPS)
        lines += subprocess.run([exe, str(a.zmws), str(a.length)], check=True, capture_output=True, text=True, timeout=600).stdout.splitlines() + [""]
    configs = ["off", "on"] + (["parent"] if a.parent else [])
    every, last = RB.alternate(__file__, configs, a, lambda c: "off" if c == "parent" else c)
    rows, med = RB.round_lines(configs, every)
    lines.append(f"the two-stage step: {a.zmws} ZMWs x {a.passes} passes x {a.length} bases, {a.steps} tickets with three in flight after {a.warmup} warm-up tickets, one process per "
                 f"configuration, alternating {a.rounds} rounds; request on: 96 16-mers at the default options")
    lines += rows
    lines.append(f"  request on against off, median against median: {100 * (med['on'] / med['off'] - 1):+.2f} %")
    if a.parent:
        lines.append(RB.parent_line(every, med))
    lines.append(f"  request on: {last['on']['tested']} reads tested, {last['on']['called_ends']} ends called; SUCCESS ZMWs on / off: {last['on']['success']} / {last['off']['success']}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What the barcode calls cost.  Two parts, every line of profiles/barcode_bench.txt written here:
  1. k_barcode alone on resident reads (tools/barcode_bench/kernel_bench.hip, built here with hipcc): 16384 reads, 96 and 384 barcodes, windows 64 and 256.
  2. the two-stage step of 16384 ZMWs x 10 passes x 10 kb (the bench.py workload) through tickets, three in flight: without the request, with it (96 16-mers,
     default options), and — given --parent ROOT, a built checkout of the parent commit — the parent's library, each in a process of its own, alternating
     `--rounds` times.  Median and min-max of the ms per step; "off" and "parent" must lie inside each other's spread.
For the kernel's time per ticket, a kernel trace in a run of its own:
    rocprofv3 --kernel-trace --stats -d OUT -o trace -- python tools/barcode_bench.py --child on --steps 3 --warmup 1
    python tools/barcode_bench.py --trace-summary OUT --out profiles/barcode_rocprofv3_summary.txt
--build-only: compile kernel_bench and stop (no GPU needed)."""
import argparse
import glob
import json
import os
import sqlite3
import subprocess
import sys
import time

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(R, "tools", "barcode_bench", "kernel_bench")
SRC = os.path.join(R, "tools", "barcode_bench", "kernel_bench.hip")


def build_kernel_bench():
    deps = [SRC] + [os.path.join(R, "ccs_amd", "csrc", f) for f in ("ccsx_barcode.hip", "ccsx_barcode_api.cpp", "barcode_core.h", "wave_ops.h")]
    if os.path.exists(EXE) and all(os.path.getmtime(d) <= os.path.getmtime(EXE) for d in deps):
        return
    subprocess.check_call([os.environ.get("HIPCC", "hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(R, "include"),
                           "-I" + os.path.join(R, "ccs_amd", "csrc"), SRC, "-o", EXE])


def child(a):
    """one configuration in this process: a.steps tickets after a.warmup, three in flight; one JSON line"""
    sys.path.insert(0, a.root or R)
    from ccs_amd import api
    b = api.synth(a.zmws, a.passes, a.length, seed=1).pinned()
    h = api.Handle(0)
    res = [api.Results.allocate(b, pinned=True, raw=False) for _ in range(3)]
    kw = [{}] * 3
    if a.child == "on":
        rng = np.random.default_rng(11)
        bset = api.BarcodeSet.from_codes([rng.integers(0, 4, 16).astype(np.uint8) for _ in range(96)])
        kw = [dict(barcodes=api.BarcodeReport.allocate(b.n_zmw, pinned=True), barcode_set=bset) for _ in range(3)]

    def run(k):
        ts = [h.submit(b, res[i % 3], **kw[i % 3]) for i in range(k)]
        for t in ts[-3:]:
            h.wait(t)
        for t in ts:
            h.release(t)
    run(a.warmup)
    t0 = time.perf_counter()
    run(a.steps)
    wall = time.perf_counter() - t0
    out = dict(config=a.child, step_ms=round(wall * 1e3 / a.steps, 2), zmws_per_s=round(a.steps * a.zmws / wall, 1), success=int((res[(a.steps - 1) % 3].status == 0).sum()))
    if a.child == "on":
        rep = kw[(a.steps - 1) % 3]["barcodes"]
        out["tested"] = int(rep.tested.sum())
        out["called_ends"] = int((rep.call & 1).sum() + (rep.call >> 1).sum())
    h.close()
    print("RESULT " + json.dumps(out))


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
    ap.add_argument("--zmws", type=int, default=16384)
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--length", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (its ccs_amd/libccsx.so is what its process loads)")
    ap.add_argument("--child", choices=("off", "on", "parent"), default=None)
    ap.add_argument("--root", default=None)
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--build-only", action="store_true")
    ap.add_argument("--trace-summary", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.trace_summary:
        return trace_summary(a.trace_summary, a.out)
    if a.build_only:
        return build_kernel_bench()
    if a.child:
        return child(a)
    lines = [f"python tools/barcode_bench.py   (MI355X)", ""]
    if not a.skip_kernel:
        build_kernel_bench()
        lines += subprocess.run([EXE, str(a.zmws), str(a.length)], check=True, capture_output=True, text=True, timeout=600).stdout.splitlines() + [""]
    configs = ["off", "on"] + (["parent"] if a.parent else [])
    every = {c: [] for c in configs}
    last = {}
    for _ in range(a.rounds):
        for c in configs:
            root = os.path.abspath(a.parent) if c == "parent" else R
            env = {k: v for k, v in os.environ.items() if k != "CCSX_LIB"}
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", c, "--root", root, "--zmws", str(a.zmws), "--passes", str(a.passes),
                                "--length", str(a.length), "--steps", str(a.steps), "--warmup", str(a.warmup)], capture_output=True, text=True, timeout=900, cwd=root, env=env)
            got = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not got:
                sys.exit(f"configuration {c} failed (exit {p.returncode}):\n{p.stdout}\n{p.stderr}")   # (nothing more is started)
            last[c] = json.loads(got[-1][7:])
            every[c].append(last[c]["step_ms"])
            print(got[-1], flush=True)
    med = {c: float(np.median(v)) for c, v in every.items()}
    lines.append(f"the two-stage step: {a.zmws} ZMWs x {a.passes} passes x {a.length} bases, {a.steps} tickets with three in flight after {a.warmup} warm-up tickets, one process per "
                 f"configuration, alternating {a.rounds} rounds; request on: 96 16-mers at the default options")
    for c in configs:
        lines.append(f"  {c:7s} ms per step by round: " + " ".join(f"{x:.2f}" for x in every[c]) + f"   median {med[c]:.2f} (min {min(every[c]):.2f}, max {max(every[c]):.2f})")
    lines.append(f"  request on against off, median against median: {100 * (med['on'] / med['off'] - 1):+.2f} %")
    if a.parent:
        inside = min(every["off"]) <= max(every["parent"]) and min(every["parent"]) <= max(every["off"])
        lines.append(f"  off against the parent commit's library, median against median: {100 * (med['off'] / med['parent'] - 1):+.2f} %; the two spreads "
                     f"{'overlap' if inside else 'DO NOT overlap'}")
    lines.append(f"  request on: {last['on']['tested']} reads tested, {last['on']['called_ends']} ends called; SUCCESS ZMWs on / off: {last['on']['success']} / {last['off']['success']}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

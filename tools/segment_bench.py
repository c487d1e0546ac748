#!/usr/bin/env python3
"""What the segmentation costs.  Two parts, every line of profiles/segment_bench.txt written here:
  1. k_segment alone on resident reads (tools/segment_bench/kernel_bench.hip, built here with hipcc): 16384 reads of 10 kb, 9 and 17 adapters of 25 bases;
     median, min and max of 7 launches; the first 512 reads of each configuration are compared with the host rule.
  2. the two-stage step of 16384 ZMWs x 10 passes x 10 kb (the bench.py workload) through tickets, three in flight: without the request, with it (17 25-mers,
     default options), and — given --parent ROOT, a built checkout of the parent commit — the parent's library, each in a process of its own, alternating
     `--rounds` times.  Median and min-max of the ms per step; "off" and "parent" must lie inside each other's spread.
--build-only: compile kernel_bench and stop (no GPU needed)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(R, "tools", "segment_bench", "kernel_bench")
SRC = os.path.join(R, "tools", "segment_bench", "kernel_bench.hip")


def build_kernel_bench():
    deps = [SRC] + [os.path.join(R, "ccs_amd", "csrc", f) for f in ("ccsx_segment.hip", "ccsx_segment_api.cpp", "ccsx_barcode_api.cpp", "segment_core.h", "barcode_core.h")]
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
        sset = api.SegmentSet.from_codes([rng.integers(0, 4, 25).astype(np.uint8) for _ in range(17)])
        kw = [dict(segments=api.SegmentReport.allocate(b.n_zmw, pinned=True), segment_set=sset) for _ in range(3)]

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
        rep = kw[(a.steps - 1) % 3]["segments"]
        out["tested"] = int(rep.tested.sum())
        out["hits"] = int(rep.n_hits.sum())
    h.close()
    print("RESULT " + json.dumps(out))


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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.build_only:
        return build_kernel_bench()
    if a.child:
        return child(a)
    lines = ["python tools/segment_bench.py   (MI355X)", ""]
    if not a.skip_kernel:
        build_kernel_bench()
        lines += subprocess.run([EXE, str(a.zmws), str(a.length)], check=True, capture_output=True, text=True, timeout=600).stdout.splitlines() + [""]
        print("\n".join(lines), flush=True)
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
                 f"configuration, alternating {a.rounds} rounds; request on: 17 25-mers at the default options")
    for c in configs:
        lines.append(f"  {c:7s} ms per step by round: " + " ".join(f"{x:.2f}" for x in every[c]) + f"   median {med[c]:.2f} (min {min(every[c]):.2f}, max {max(every[c]):.2f})")
    lines.append(f"  request on against off, median against median: {100 * (med['on'] / med['off'] - 1):+.2f} %")
    if a.parent:
        inside = min(every["off"]) <= max(every["parent"]) and min(every["parent"]) <= max(every["off"])
        lines.append(f"  off against the parent commit's library, median against median: {100 * (med['off'] / med['parent'] - 1):+.2f} %; the two spreads "
                     f"{'overlap' if inside else 'DO NOT overlap'}")
    lines.append(f"  request on: {last['on']['tested']} reads tested, {last['on']['hits']} hits; SUCCESS ZMWs on / off: {last['on']['success']} / {last['off']['success']}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

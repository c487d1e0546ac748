"""What the benchmarks of the analyses on final reads share (tools/segment_bench.py, tools/cdna_bench.py): the stand-alone kernel_bench program's build, the
ticket loop of one configuration's process, and the alternating rounds of off / on / parent processes with their report lines."""
import json
import os
import subprocess
import sys
import time

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(R, "ccs_amd", "csrc")


def build_kernel_bench(name: str, deps) -> str:
    """tools/<name>_bench/kernel_bench from kernel_bench.hip, rebuilt when it or one of `deps` (files of ccs_amd/csrc) is newer; the program's path"""
    src, exe = os.path.join(R, "tools", name + "_bench", "kernel_bench.hip"), os.path.join(R, "tools", name + "_bench", "kernel_bench")
    files = [src] + [os.path.join(CSRC, f) for f in deps]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in files):
        subprocess.check_call([os.environ.get("HIPCC", "hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(R, "include"), "-I" + CSRC, src, "-o", exe])
    return exe


def add_step_arguments(ap) -> None:
    ap.add_argument("--zmws", type=int, default=16384)
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--length", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="seconds one configuration's process may take")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (its ccs_amd/libccsx.so is what its process loads)")
    ap.add_argument("--child", default=None)
    ap.add_argument("--root", default=None)
    ap.add_argument("--out", default=None)


def timed_tickets(a, b, request, summary=None) -> None:
    """one configuration in this process: a.steps tickets of the pinned batch b after a.warmup, three in flight; prints one RESULT line.  request(api, n): None, or
    the keyword arguments of Handle.submit for one ticket; summary(kw of the last ticket) -> further fields of the line"""
    from ccs_amd import api
    h = api.Handle(0)
    res = [api.Results.allocate(b, pinned=True, raw=False) for _ in range(3)]
    kw = [request(api, b.n_zmw) or {} for _ in range(3)]

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
    if summary is not None:
        out.update(summary(kw[(a.steps - 1) % 3]))
    h.close()
    print("RESULT " + json.dumps(out))


def alternate(script: str, configs, a, child_of=lambda c: c) -> tuple:
    """a.rounds rounds of one process per configuration, each under its own time limit; "parent" runs in a.parent with that checkout's library.  The first
    process that fails ends the run.  (ms per step by configuration, the last RESULT of each)"""
    every, last = {c: [] for c in configs}, {}
    for _ in range(a.rounds):
        for c in configs:
            root = os.path.abspath(a.parent) if c == "parent" else R
            env = {k: v for k, v in os.environ.items() if k != "CCSX_LIB"}
            p = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(script), "--child", child_of(c), "--root", root, "--zmws", str(a.zmws),
                                "--passes", str(a.passes), "--length", str(a.length), "--steps", str(a.steps), "--warmup", str(a.warmup)],
                               capture_output=True, text=True, cwd=root, env=env)
            got = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not got:
                sys.exit(f"configuration {c} failed (exit {p.returncode}):\n{p.stdout}\n{p.stderr}")   # (nothing more is started)
            last[c] = json.loads(got[-1][7:])
            every[c].append(last[c]["step_ms"])
            print(c, got[-1], flush=True)
    return every, last


def round_lines(configs, every) -> tuple:
    """(one line per configuration, the medians)"""
    med = {c: float(np.median(v)) for c, v in every.items()}
    return [f"  {c:7s} ms per step by round: " + " ".join(f"{x:.2f}" for x in every[c]) + f"   median {med[c]:.2f} (min {min(every[c]):.2f}, max {max(every[c]):.2f})"
            for c in configs], med


def parent_line(every, med) -> str:
    inside = min(every["off"]) <= max(every["parent"]) and min(every["parent"]) <= max(every["off"])
    return (f"  off against the parent commit's library, median against median: {100 * (med['off'] / med['parent'] - 1):+.2f} %; the two spreads "
            f"{'overlap' if inside else 'DO NOT overlap'}")

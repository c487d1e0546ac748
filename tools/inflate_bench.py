#!/usr/bin/env python3
"""The numbers of DESIGN.md §7 "GPU inflate" -> profiles/inflate_bench.txt.

  tools/inflate_bench.py --build                      compile tools/inflate_bench/kernel_bench (hipcc, gfx950); needs no GPU
  tools/inflate_bench.py --run [--zmws N] [--rounds R] [--parent-ccs PATH] [--out FILE]
      1. writes a synthetic 10 x 10 kb subreads.bam of N ZMWs (default 32768) to a temporary directory
      2. k_inflate alone on ~1 GB of its blocks resident in HBM (kernel_bench)
      3. `ccs` BAM -> BAM with 16 host threads on one card, --gpu-inflate off and on alternating, R rounds each (default 3), with --log-level INFO: wall
         time of the process, and of each arm's last round the driver's own lines: its ZMWs/s, the reader's and the GPU worker's accounting, and the engine's
         device times from the ticket timings ("ccs: engine (ticket timings ...)"); CCSX_INFLATE_PRIO=high is a third arm
      4. with --parent-ccs: a `ccs` built from the parent commit, flag off, once per round (the flag-off path must be unchanged; that binary logs no ticket
         timings)
  --build also records k_inflate's resources (hipcc -Rpass-analysis=kernel-resource-usage) in tools/inflate_bench/build/resources.txt; --run copies them into
  the report, so every line of profiles/inflate_bench.txt is written by this tool.
"""
import argparse
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KB_DIR = os.path.join(ROOT, "tools", "inflate_bench", "build")
KB = os.path.join(KB_DIR, "kernel_bench")
CCS = os.path.join(ROOT, "ccs_amd", "bin", "ccs")


def build():
    os.makedirs(KB_DIR, exist_ok=True)
    p = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize",
                        "-falign-loops=64", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ccs_amd", "csrc"), "-Rpass-analysis=kernel-resource-usage",
                        "-c", os.path.join(ROOT, "ccs_amd", "csrc", "ccsx_inflate.hip"), "-o", os.path.join(KB_DIR, "ccsx_inflate.o")], capture_output=True, text=True, check=True)
    keep = [l.split("remark:", 1)[1].replace(" [-Rpass-analysis=kernel-resource-usage]", "").strip() for l in p.stderr.splitlines() if "remark" in l]
    with open(os.path.join(KB_DIR, "resources.txt"), "w") as f:
        f.write("k_inflate resources (the library's flags, gfx950): " + "; ".join(" ".join(k.split()) for k in keep if not k.startswith("Function Name")) +
                " -> LDS admits two workgroups of one wave64 per CU, 512 streams resident on the card; the spilled SGPRs live in VGPR lanes, not in memory\n")
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "ccs_amd", "csrc"), os.path.join(ROOT, "tools", "inflate_bench", "kernel_bench.hip"), "-o", KB, "-lz"])


def ccs_run(exe, bam, out, extra, env=None, log=None):
    t0 = time.time()
    p = subprocess.run([exe, bam, out, "-j", "16", "--log-level", "INFO", "--suppress-reports", *extra], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, **(env or {})))
    dt = time.time() - t0
    if p.returncode != 0:
        raise RuntimeError(f"{exe} {extra}: exit {p.returncode}: {p.stderr[-2000:]}")
    lines = [l for l in p.stderr.splitlines() if re.search(r"GPU workers|ZMWs/s|reader thread|engine \(ticket", l)]
    if log is not None:
        log.extend("      " + l for l in lines[-8:])
    return dt


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", action="store_true")
    ap.add_argument("--run", action="store_true")
    ap.add_argument("--zmws", type=int, default=32768)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-ccs", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inflate_bench.txt"))
    a = ap.parse_args()
    if a.build:
        build()
    if not a.run:
        return 0
    work = tempfile.mkdtemp(prefix="inflate_bench_")
    rep = []
    try:
        bam = os.path.join(work, "s.subreads.bam")
        subprocess.check_call([CCS, "--write-synthetic", f"{a.zmws},10,10000,1", bam, "-j", "16"], timeout=1500)
        rep.append(f"tools/inflate_bench.py --run --zmws {a.zmws} --rounds {a.rounds}" + (" --parent-ccs ..." if a.parent_ccs else "") + "   (one MI355X, 16 host threads; DESIGN.md §7 \"GPU inflate\")")
        res = os.path.join(KB_DIR, "resources.txt")
        rep.append(open(res).read().strip() if os.path.exists(res) else "k_inflate resources: not recorded (run --build first)")
        rep.append("scale: one host core inflates ~0.59 GB/s (libdeflate); the engine at 38.8 k ZMWs/s consumes ~5.3 GB/s of inflated input (derived, DESIGN.md §7)")
        rep.append(f"input: {a.zmws} ZMWs x 10 passes x 10 kb, {os.path.getsize(bam) / 1e9:.2f} GB of BGZF")
        p = subprocess.run([KB, bam], capture_output=True, text=True, timeout=300)
        rep.append(p.stdout.strip() or ("kernel_bench failed: " + p.stderr.strip()[-500:]))
        if p.returncode != 0:
            raise RuntimeError(rep[-1])
        print("\n".join(rep), flush=True)
        arms = [("off", CCS, [], {}), ("on (low priority, the default)", CCS, ["--gpu-inflate"], {}), ("on, CCSX_INFLATE_PRIO=high", CCS, ["--gpu-inflate"], {"CCSX_INFLATE_PRIO": "high"})]
        if a.parent_ccs:
            arms.insert(1, ("parent commit's binary, off", a.parent_ccs, [], {}))
        times = {n: [] for n, *_ in arms}
        detail = {}
        out = os.path.join(work, "o.bam")
        for r in range(a.rounds):
            for name, exe, extra, env in arms:
                log = []
                times[name].append(ccs_run(exe, bam, out, extra, env, log))
                detail[name] = log
                print(f"round {r} {name}: {times[name][-1]:.2f} s = {a.zmws / times[name][-1]:.0f} ZMWs/s", flush=True)
        rep.append(f"end to end: ccs BAM -> BAM, -j 16, one card, {a.rounds} alternating rounds (wall seconds of the whole process; ZMWs/s = {a.zmws} / wall)")
        for name, *_ in arms:
            t = times[name]
            rep.append(f"  {name:34s} median {statistics.median(t):6.2f} s  min {min(t):6.2f}  max {max(t):6.2f}   = {a.zmws / statistics.median(t):7.0f} ZMWs/s   rounds: " + " ".join(f"{x:.2f}" for x in t))
            rep.extend(detail[name])
    finally:
        shutil.rmtree(work, ignore_errors=True)
        with open(a.out, "w") as f:
            f.write("\n".join(rep) + "\n")
    print("\n".join(rep))
    return 0


if __name__ == "__main__":
    sys.exit(main())

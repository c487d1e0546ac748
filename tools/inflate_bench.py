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
import shutil
import subprocess
import sys
import tempfile

import codec_bench as B
from codec_bench import CCS, ROOT

KB = os.path.join(B.kb_dir("inflate"), "kernel_bench")
LINES = r"GPU workers|ZMWs/s|reader thread|engine \(ticket"


def build():
    B.build("inflate", "LDS admits two workgroups of one wave64 per CU, 512 streams resident on the card; the spilled SGPRs live in VGPR lanes, not in memory")


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
        input_line = B.write_synthetic(a.zmws, bam)
        rep.append(f"tools/inflate_bench.py --run --zmws {a.zmws} --rounds {a.rounds}" + (" --parent-ccs ..." if a.parent_ccs else "") + "   (one MI355X, 16 host threads; DESIGN.md §7 \"GPU inflate\")")
        rep.append(B.resources("inflate"))
        rep.append("scale: one host core inflates ~0.59 GB/s (libdeflate); the engine at 38.8 k ZMWs/s consumes ~5.3 GB/s of inflated input (derived, DESIGN.md §7)")
        rep.append(input_line)
        p = subprocess.run([KB, bam], capture_output=True, text=True, timeout=300)
        rep.append(p.stdout.strip() or ("kernel_bench failed: " + p.stderr.strip()[-500:]))
        if p.returncode != 0:
            raise RuntimeError(rep[-1])
        print("\n".join(rep), flush=True)
        arms = [("off", CCS, [], {}), ("on (low priority, the default)", CCS, ["--gpu-inflate"], {}), ("on, CCSX_INFLATE_PRIO=high", CCS, ["--gpu-inflate"], {"CCSX_INFLATE_PRIO": "high"})]
        if a.parent_ccs:
            arms.insert(1, ("parent commit's binary, off", a.parent_ccs, [], {}))
        out = os.path.join(work, "o.bam")
        times, detail = B.alternate(arms, a.rounds, a.zmws, lambda arm, log: B.ccs_run(arm[1], bam, out, arm[2], LINES, arm[3], log))
        rep.append(f"end to end: ccs BAM -> BAM, -j 16, one card, {a.rounds} alternating rounds (wall seconds of the whole process; ZMWs/s = {a.zmws} / wall)")
        for name, *_ in arms:
            rep.append(f"  {name:34s} {B.spread(times[name], a.zmws)}   {B.rounds_of(times[name])}")
            rep.extend(detail[name])
    finally:
        shutil.rmtree(work, ignore_errors=True)
        with open(a.out, "w") as f:
            f.write("\n".join(rep) + "\n")
    print("\n".join(rep))
    return 0


if __name__ == "__main__":
    sys.exit(main())

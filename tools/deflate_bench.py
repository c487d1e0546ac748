#!/usr/bin/env python3
"""The numbers of DESIGN.md §7 "GPU deflate" -> profiles/deflate_bench.txt.

  tools/deflate_bench.py --build                      compile tools/deflate_bench/kernel_bench (hipcc, gfx950); needs no GPU
  tools/deflate_bench.py --ratio                      the compression table alone (CPU, host path of the rule): prints it, writes nothing
  tools/deflate_bench.py --run [--zmws N] [--rounds R] [--parent-ccs PATH] [--out FILE]
      1. the compression table: the two corpora of tests/deflate_ref.py through api.deflate_host against zlib level 1 and level 4 on the same 0xff00-byte spans
      2. writes a synthetic 10 x 10 kb subreads.bam of N ZMWs (default 16384) to a temporary directory
      3. per workload (plain, --hifi-kinetics): `ccs` BAM -> BAM with 16 host threads on one card, --gpu-deflate off, on and (with --parent-ccs) a `ccs` built
         from the parent commit, alternating, R rounds each (default 3), with --log-level INFO: wall time of the process, and of each arm's last round the
         driver's own lines (its ZMWs/s, the GPU worker's accounting, the engine's ticket timings, the deflater's accounting)
      4. per workload: k_deflate alone on ~0.2 GB of the flag-off output's inflated blocks resident in HBM (kernel_bench), with the compressed size against zlib
  --build also records k_deflate's resources (hipcc -Rpass-analysis=kernel-resource-usage) in tools/deflate_bench/build/resources.txt; --run copies them into
  the report, so every line of profiles/deflate_bench.txt is written by this tool.
"""
import argparse
import os
import shutil
import subprocess
import sys
import tempfile
import zlib

import codec_bench as B
from codec_bench import CCS, ROOT

KB = os.path.join(B.kb_dir("deflate"), "kernel_bench")
LINES = r"GPU workers|ZMWs/s|engine \(ticket|--gpu-deflate: \d"


def build():
    B.build("deflate", "LDS admits one workgroup of four wave64 per CU, 256 spans resident on the card")


def ratio_table():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import deflate_ref as R
    from ccs_amd import api
    lines = ["compression (CPU, the rule's host path; spans of 0xff00 bytes as the BAM writer cuts them; yardstick zlib level 1, the driver's own level 4 beside it):"]
    for name, kin in (("hifi", False), ("hifi-kinetics", True)):
        spans = R.spans_of(R.hifi_corpus(kin))
        ours = stored = 0
        for at in range(0, len(spans), 16):
            streams, status, call = api.deflate_host(spans[at:at + 16])
            assert not status.any()
            ours += sum(len(s) for s in streams)
            stored += sum(1 for i, s in enumerate(streams) if len(s) == api.deflate_bound(len(spans[at + i])))
        z = {}
        for level in (1, 4):
            z[level] = 0
            for s in spans:
                c = zlib.compressobj(level, zlib.DEFLATED, -15)
                z[level] += len(c.compress(s) + c.flush())
        raw = sum(len(s) for s in spans)
        excess = 100.0 * (ours - z[1]) / z[1]
        margin = 5 * -(-excess // 5)
        lines.append(f"  {name:14s} {raw} bytes in {len(spans)} spans: rule {ours} ({stored} spans stored), zlib-1 {z[1]}, zlib-4 {z[4]}; excess over zlib-1 {excess:+.2f} % "
                     f"-> the test's margin {margin:+.0f} % (ceiling 25 %)")
    return lines


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", action="store_true")
    ap.add_argument("--ratio", action="store_true")
    ap.add_argument("--run", action="store_true")
    ap.add_argument("--zmws", type=int, default=16384)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-ccs", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deflate_bench.txt"))
    a = ap.parse_args()
    if a.build:
        build()
    if a.ratio:
        print("\n".join(ratio_table()))
    if not a.run:
        return 0
    work = tempfile.mkdtemp(prefix="deflate_bench_")
    rep = []
    try:
        rep.append(f"tools/deflate_bench.py --run --zmws {a.zmws} --rounds {a.rounds}" + (" --parent-ccs ..." if a.parent_ccs else "") + "   (one MI355X, 16 host threads; DESIGN.md §7 \"GPU deflate\")")
        rep.append(B.resources("deflate"))
        rep.extend(ratio_table())
        print("\n".join(rep), flush=True)
        bam = os.path.join(work, "s.subreads.bam")
        rep.append(B.write_synthetic(a.zmws, bam))
        for wname, wextra in (("plain", []), ("--hifi-kinetics", ["--hifi-kinetics"])):
            arms = [("off", CCS, []), ("on", CCS, ["--gpu-deflate"])]
            if a.parent_ccs:
                arms.insert(1, ("parent commit's binary, off", a.parent_ccs, []))
            out = {n: os.path.join(work, f"o{k}.bam") for k, (n, *_) in enumerate(arms)}
            times, detail = B.alternate(arms, a.rounds, a.zmws, lambda arm, log: B.ccs_run(arm[1], bam, out[arm[0]], wextra + arm[2], LINES, None, log), wname + " ")
            size = {n: os.path.getsize(out[n]) for n, *_ in arms}
            rep.append(f"end to end, {wname}: ccs BAM -> BAM, -j 16, one card, {a.rounds} alternating rounds (wall seconds of the whole process; ZMWs/s = {a.zmws} / wall)")
            for name, *_ in arms:
                rep.append(f"  {name:28s} {B.spread(times[name], a.zmws)}   OUT.bam {size[name] / 1e6:.1f} MB   {B.rounds_of(times[name])}")
                rep.extend(detail[name])
            p = subprocess.run([KB, out["off"], "2e8"], capture_output=True, text=True, timeout=600)
            rep.append(f"{wname}: " + (p.stdout.strip() or ("kernel_bench failed: " + p.stderr.strip()[-500:])))
            if p.returncode != 0:
                raise RuntimeError(rep[-1])
            print(rep[-1], flush=True)
    finally:
        shutil.rmtree(work, ignore_errors=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(rep) + "\n")
    print("\n".join(rep))
    return 0


if __name__ == "__main__":
    sys.exit(main())

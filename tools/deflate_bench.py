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
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KB_DIR = os.path.join(ROOT, "tools", "deflate_bench", "build")
KB = os.path.join(KB_DIR, "kernel_bench")
CCS = os.path.join(ROOT, "ccs_amd", "bin", "ccs")


def build():
    os.makedirs(KB_DIR, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ccs_amd", "csrc")]
    p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize", "-falign-loops=64", *inc,
                        "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(ROOT, "ccs_amd", "csrc", "ccsx_deflate.hip"), "-o", os.path.join(KB_DIR, "ccsx_deflate.o")],
                       capture_output=True, text=True, check=True)
    keep = [l.split("remark:", 1)[1].replace(" [-Rpass-analysis=kernel-resource-usage]", "").strip() for l in p.stderr.splitlines() if "remark" in l]
    with open(os.path.join(KB_DIR, "resources.txt"), "w") as f:
        f.write("k_deflate resources (the library's flags, gfx950): " + "; ".join(" ".join(k.split()) for k in keep if not k.startswith("Function Name")) +
                " -> LDS admits one workgroup of four wave64 per CU, 256 spans resident on the card\n")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", *inc, os.path.join(ROOT, "tools", "deflate_bench", "kernel_bench.hip"), "-o", KB, "-lz"])


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


def ccs_run(exe, bam, out, extra, log=None):
    t0 = time.time()
    p = subprocess.run([exe, bam, out, "-j", "16", "--log-level", "INFO", "--suppress-reports", *extra], capture_output=True, text=True, timeout=900)
    dt = time.time() - t0
    if p.returncode != 0:
        raise RuntimeError(f"{exe} {extra}: exit {p.returncode}: {p.stderr[-2000:]}")
    lines = [l for l in p.stderr.splitlines() if re.search(r"GPU workers|ZMWs/s|engine \(ticket|--gpu-deflate: \d", l)]
    if log is not None:
        log.extend("      " + l for l in lines[-8:])
    return dt


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
        res = os.path.join(KB_DIR, "resources.txt")
        rep.append(open(res).read().strip() if os.path.exists(res) else "k_deflate resources: not recorded (run --build first)")
        rep.extend(ratio_table())
        print("\n".join(rep), flush=True)
        bam = os.path.join(work, "s.subreads.bam")
        subprocess.check_call([CCS, "--write-synthetic", f"{a.zmws},10,10000,1", bam, "-j", "16"], timeout=1500)
        rep.append(f"input: {a.zmws} ZMWs x 10 passes x 10 kb, {os.path.getsize(bam) / 1e9:.2f} GB of BGZF")
        for wname, wextra in (("plain", []), ("--hifi-kinetics", ["--hifi-kinetics"])):
            arms = [("off", CCS, []), ("on", CCS, ["--gpu-deflate"])]
            if a.parent_ccs:
                arms.insert(1, ("parent commit's binary, off", a.parent_ccs, []))
            times = {n: [] for n, *_ in arms}
            detail, size = {}, {}
            out = {n: os.path.join(work, f"o{k}.bam") for k, (n, *_) in enumerate(arms)}
            for r in range(a.rounds):
                for name, exe, extra in arms:
                    log = []
                    times[name].append(ccs_run(exe, bam, out[name], wextra + extra, log))
                    detail[name] = log
                    size[name] = os.path.getsize(out[name])
                    print(f"{wname} round {r} {name}: {times[name][-1]:.2f} s = {a.zmws / times[name][-1]:.0f} ZMWs/s", flush=True)
            rep.append(f"end to end, {wname}: ccs BAM -> BAM, -j 16, one card, {a.rounds} alternating rounds (wall seconds of the whole process; ZMWs/s = {a.zmws} / wall)")
            for name, *_ in arms:
                t = times[name]
                rep.append(f"  {name:28s} median {statistics.median(t):6.2f} s  min {min(t):6.2f}  max {max(t):6.2f}   = {a.zmws / statistics.median(t):7.0f} ZMWs/s   "
                           f"OUT.bam {size[name] / 1e6:.1f} MB   rounds: " + " ".join(f"{x:.2f}" for x in t))
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

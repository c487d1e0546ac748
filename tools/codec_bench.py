"""What tools/inflate_bench.py and tools/deflate_bench.py share: the build of a codec's kernel_bench with the kernel's resource usage, the synthetic subreads
BAM, one timed `ccs` run with the driver's log lines, the alternating rounds over the arms, and the median / min / max of an arm."""
import os
import re
import statistics
import subprocess
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CCS = os.path.join(ROOT, "ccs_amd", "bin", "ccs")


def kb_dir(codec: str) -> str:
    return os.path.join(ROOT, "tools", codec + "_bench", "build")


def build(codec: str, occupancy: str) -> None:
    """tools/<codec>_bench/build/kernel_bench, and in resources.txt beside it what hipcc says k_<codec> uses under the library's flags, with `occupancy` behind it"""
    os.makedirs(kb_dir(codec), exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ccs_amd", "csrc")]
    p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize", "-falign-loops=64", *inc,
                        "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(ROOT, "ccs_amd", "csrc", f"ccsx_{codec}.hip"), "-o", os.path.join(kb_dir(codec), f"ccsx_{codec}.o")],
                       capture_output=True, text=True, check=True)
    keep = [l.split("remark:", 1)[1].replace(" [-Rpass-analysis=kernel-resource-usage]", "").strip() for l in p.stderr.splitlines() if "remark" in l]
    with open(os.path.join(kb_dir(codec), "resources.txt"), "w") as f:
        f.write(f"k_{codec} resources (the library's flags, gfx950): " + "; ".join(" ".join(k.split()) for k in keep if not k.startswith("Function Name")) + " -> " + occupancy + "\n")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", *inc, os.path.join(ROOT, "tools", codec + "_bench", "kernel_bench.hip"), "-o",
                           os.path.join(kb_dir(codec), "kernel_bench"), "-lz"])


def resources(codec: str) -> str:
    res = os.path.join(kb_dir(codec), "resources.txt")
    return open(res).read().strip() if os.path.exists(res) else f"k_{codec} resources: not recorded (run --build first)"


def write_synthetic(zmws: int, bam: str) -> str:
    """a synthetic 10 x 10 kb subreads.bam of `zmws` ZMWs; returns the report's line about it"""
    subprocess.check_call([CCS, "--write-synthetic", f"{zmws},10,10000,1", bam, "-j", "16"], timeout=1500)
    return f"input: {zmws} ZMWs x 10 passes x 10 kb, {os.path.getsize(bam) / 1e9:.2f} GB of BGZF"


def ccs_run(exe, bam, out, extra, lines_re, env=None, log=None) -> float:
    """one `ccs` BAM -> BAM run; returns its wall seconds and appends the last of the driver's log lines that match lines_re to log"""
    t0 = time.time()
    p = subprocess.run([exe, bam, out, "-j", "16", "--log-level", "INFO", "--suppress-reports", *extra], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, **(env or {})))
    dt = time.time() - t0
    if p.returncode != 0:
        raise RuntimeError(f"{exe} {extra}: exit {p.returncode}: {p.stderr[-2000:]}")
    lines = [l for l in p.stderr.splitlines() if re.search(lines_re, l)]
    if log is not None:
        log.extend("      " + l for l in lines[-8:])
    return dt


def alternate(arms, rounds: int, zmws: int, run, label: str = ""):
    """rounds times over the arms in turn: arms are tuples whose first element is the arm's name, run(arm, log) its wall seconds.  Returns ({name: the times},
    {name: the log lines of its last round})"""
    times = {arm[0]: [] for arm in arms}
    detail = {}
    for r in range(rounds):
        for arm in arms:
            log = []
            times[arm[0]].append(run(arm, log))
            detail[arm[0]] = log
            print(f"{label}round {r} {arm[0]}: {times[arm[0]][-1]:.2f} s = {zmws / times[arm[0]][-1]:.0f} ZMWs/s", flush=True)
    return times, detail


def spread(t, zmws: int) -> str:
    return f"median {statistics.median(t):6.2f} s  min {min(t):6.2f}  max {max(t):6.2f}   = {zmws / statistics.median(t):7.0f} ZMWs/s"


def rounds_of(t) -> str:
    return "rounds: " + " ".join(f"{x:.2f}" for x in t)

#!/usr/bin/env python3
"""What the segmentation costs.  Two parts, every line of profiles/segment_bench.txt written here:
  1. k_segment alone on resident reads (tools/segment_bench/kernel_bench.hip, built here with hipcc): 16384 reads of 10 kb, 9 and 17 adapters of 25 bases;
     median, min and max of 7 launches; the first 512 reads of each configuration are compared with the host rule.
  2. the two-stage step of 16384 ZMWs x 10 passes x 10 kb (the bench.py workload) through tickets, three in flight: without the request, with it (17 25-mers,
     default options), and — given --parent ROOT, a built checkout of the parent commit — the parent's library, each in a process of its own, alternating
     `--rounds` times.  Median and min-max of the ms per step; "off" and "parent" must lie inside each other's spread.
--build-only: compile kernel_bench and stop (no GPU needed).  The build, the ticket loop and the rounds are tools/reads_bench.py's, shared with tools/barcode_bench.py and tools/cdna_bench.py."""
import argparse
import subprocess
import sys

import numpy as np

import reads_bench as RB

DEPS = ("ccsx_segment.hip", "ccsx_segment_api.cpp", "ccsx_barcode_api.cpp", "segment_core.h", "barcode_core.h")


def child(a):
    """one configuration in this process (tools/reads_bench.py timed_tickets); one JSON line"""
    sys.path.insert(0, a.root or RB.R)
    from ccs_amd import api
    b = api.synth(a.zmws, a.passes, a.length, seed=1).pinned()

    def request(api, n):
        if a.child != "on":
            return None
        rng = np.random.default_rng(11)
        return dict(segments=api.SegmentReport.allocate(n, pinned=True), segment_set=api.SegmentSet.from_codes([rng.integers(0, 4, 25).astype(np.uint8) for _ in range(17)]))
    RB.timed_tickets(a, b, request, (lambda kw: dict(tested=int(kw["segments"].tested.sum()), hits=int(kw["segments"].n_hits.sum()))) if a.child == "on" else None)


def main():
    ap = argparse.ArgumentParser()
    RB.add_step_arguments(ap)
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--build-only", action="store_true")
    a = ap.parse_args()
    if a.build_only:
        return RB.build_kernel_bench("segment", DEPS)
    if a.child:
        return child(a)
    lines = ["python tools/segment_bench.py   (MI355X)", ""]
    if not a.skip_kernel:
        exe = RB.build_kernel_bench("segment", DEPS)
        lines += subprocess.run([exe, str(a.zmws), str(a.length)], check=True, capture_output=True, text=True, timeout=600).stdout.splitlines() + [""]
        print("\n".join(lines), flush=True)
    configs = ["off", "on"] + (["parent"] if a.parent else [])
    every, last = RB.alternate(__file__, configs, a, lambda c: "off" if c == "parent" else c)
    rows, med = RB.round_lines(configs, every)
    lines.append(f"the two-stage step: {a.zmws} ZMWs x {a.passes} passes x {a.length} bases, {a.steps} tickets with three in flight after {a.warmup} warm-up tickets, one process per "
                 f"configuration, alternating {a.rounds} rounds; request on: 17 25-mers at the default options")
    lines += rows
    lines.append(f"  request on against off, median against median: {100 * (med['on'] / med['off'] - 1):+.2f} %")
    if a.parent:
        lines.append(RB.parent_line(every, med))
    lines.append(f"  request on: {last['on']['tested']} reads tested, {last['on']['hits']} hits; SUCCESS ZMWs on / off: {last['on']['success']} / {last['off']['success']}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What the cDNA analysis costs.  Two parts, every line of profiles/cdna_bench.txt written here (the shared machinery: tools/reads_bench.py):
  1. k_cdna alone on resident reads (tools/cdna_bench/kernel_bench.hip, built here with hipcc): 16384 full-length reads of 10 kb with tails of 30 bases, 2 and 16
     primers of 25 bases; median, min and max of 7 launches; the first 512 reads of each configuration are compared with the host rule.
  2. the two-stage step of 16384 ZMWs x 10 passes x 10 kb (the bench.py workload) through tickets, three in flight: without the request, with it (2 and 16
     25-mers, default options), and — given --parent ROOT, a built checkout of the parent commit — the parent's library, each in a process of its own under its
     own time limit, alternating `--rounds` times.  Every configuration runs on the same passes: the ends of 5p . insert . A x 30 . rc(3p) are
     planted into every pass (the first 25 and the last 57 bases of a forward pass, their reverse complement in a reverse pass), so the consensus reaches step 4
     of the rule and the request's configurations time the poly(A) scan and the walk over the whole read, not the ends alone.  Median and min-max of the ms per
     step; "off" and "parent" must lie inside each other's spread.
--build-only: compile kernel_bench and stop (no GPU needed)."""
import argparse
import os
import subprocess
import sys

import numpy as np

import reads_bench as RB

M, TAIL = 25, 30


def planted_batch(api, a):
    """api.synth's batch with a cDNA molecule's ends written into every pass; (batch, the 16 primers, of which 0 and 1 are planted)"""
    rng = np.random.default_rng(11)
    primers = [rng.integers(0, 4, M).astype(np.uint8) for _ in range(16)]
    head = primers[0]
    tail = np.concatenate([np.array([2, 1], np.uint8), np.zeros(TAIL, np.uint8), (3 - primers[1][::-1]).astype(np.uint8)])   # G C . A x 30 . rc(3p)
    rc = lambda x: (3 - x[::-1]).astype(np.uint8)                     # noqa: E731
    b = api.synth(a.zmws, a.passes, a.length, seed=1)
    for r in range(len(b.flags)):
        lo, hi = int(b.base_off[r]), int(b.base_off[r + 1])
        first, last = (rc(tail), rc(head)) if b.flags[r] & 1 else (head, tail)
        b.bases[lo:lo + len(first)] = first
        b.bases[hi - len(last):hi] = last
    return b, primers


def child(a):
    sys.path.insert(0, a.root or RB.R)
    from ccs_amd import api
    b, primers = planted_batch(api, a)
    P = int(a.child[2:]) if a.child.startswith("on") else 0

    def request(api, n):
        if not P:
            return None
        return dict(cdna=api.CdnaReport.allocate(n, pinned=True), cdna_primers=api.CdnaPrimers.from_codes(primers[:P], [k & 1 for k in range(P)]))

    def summary(kw):
        rep = kw["cdna"]
        return dict(tested=int(rep.tested.sum()), classes=np.bincount(rep.cls[rep.tested == 1], minlength=7).tolist(),
                    tails=np.bincount(rep.polya_len[rep.cls == 6], minlength=TAIL + 3)[TAIL - 2:TAIL + 3].tolist())
    RB.timed_tickets(a, b.pinned(), request, summary if P else None)


def main():
    ap = argparse.ArgumentParser()
    RB.add_step_arguments(ap)
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--build-only", action="store_true")
    a = ap.parse_args()
    deps = ("ccsx_cdna.hip", "ccsx_cdna_api.cpp", "ccsx_barcode_api.cpp", "cdna_core.h", "segment_core.h", "barcode_core.h", "wave_ops.h")
    if a.build_only:
        return RB.build_kernel_bench("cdna", deps)
    if a.child:
        return child(a)
    lines = ["python tools/cdna_bench.py   (MI355X)", ""]
    if not a.skip_kernel:
        exe = RB.build_kernel_bench("cdna", deps)
        lines += subprocess.run(["timeout", "-k", "10", str(a.limit), exe, str(a.zmws), str(a.length)], check=True, capture_output=True, text=True).stdout.splitlines() + [""]
        print("\n".join(lines), flush=True)
    configs = ["off", "on2", "on16"] + (["parent"] if a.parent else [])
    every, last = RB.alternate(__file__, configs, a, lambda c: "off" if c == "parent" else c)
    rows, med = RB.round_lines(configs, every)
    lines.append(f"the two-stage step: {a.zmws} ZMWs x {a.passes} passes x {a.length} bases, every pass with a planted 5' primer, A x {TAIL} tail and 3' primer, {a.steps} tickets "
                 f"with three in flight after {a.warmup} warm-up tickets, one process per configuration, alternating {a.rounds} rounds; request on: the planted pair alone, and "
                 f"with 14 more random 25-mers, roles alternating, at the default options")
    lines += rows
    for c in ("on2", "on16"):
        lines.append(f"  request {c} against off, median against median: {100 * (med[c] / med['off'] - 1):+.2f} % = {med[c] - med['off']:+.2f} ms; {last[c]['tested']} reads tested, "
                     f"per class {last[c]['classes']}, full-length reads with polya_len {TAIL - 2} .. {TAIL + 2}: {last[c]['tails']}")
    if a.parent:
        lines.append(RB.parent_line(every, med))
    lines.append(f"  SUCCESS ZMWs on2 / on16 / off: {last['on2']['success']} / {last['on16']['success']} / {last['off']['success']}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

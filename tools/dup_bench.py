#!/usr/bin/env python3
"""What duplicate marking costs.  Two parts, every line of profiles/dup_bench.txt written here:
  1. the kernels alone on resident reads (tools/dup_bench/kernel_bench.hip, built here with hipcc): about a million reads of 10 kb of which about a tenth are
     planted duplicates in sets of 2 - 4; k_dup_sign, k_dup_keys, the sort, k_dup_buckets and k_dup_verify each as the median (min - max) of 7 launches, the first
     512 reads checked against the host rule; k_dup_verify on one full bucket of 512; the two host calls on one thread, for scale.
  2. ccs --mark-duplicates end to end on a BAM of --reads HiFi-like reads of 10 kb (written here: random reads, one in ten a copy of an earlier one; qualities
     0xff), `--rounds` times, with the phases the driver logs at --log-level INFO: pass 2 is inflate, copy and deflate alone, pass 1 outside
     ccsx_dup_sign_reads is inflate, parsing and base decoding.  A new mode: no parent commit has it to compare with.
Each GPU process runs under its own time limit and the first that fails ends the run.  --build-only: compile kernel_bench and stop (no GPU needed)."""
import argparse
import os
import re
import struct
import subprocess
import sys
import time
import zlib

import numpy as np

import reads_bench as RB

DEPS = ("ccsx_dup.hip", "ccsx_dup_api.cpp", "ccsx_barcode_api.cpp", "dup_core.h", "barcode_core.h", "wave_ops.h")


def write_bam(path, n, length, seed=5):
    """n unaligned records of `length` +- 20 random bases (one in ten a copy of an earlier read, half of those reverse complemented), rq tags; BGZF at level 1"""
    rng = np.random.default_rng(seed)
    nib = np.array([1, 2, 4, 8], np.uint8)
    reads, raw = [], [b"BAM\x01" + struct.pack("<i", 0) + struct.pack("<i", 0)]
    for z in range(n):
        if z and rng.random() < 0.1:
            c = reads[int(rng.integers(max(0, len(reads) - 64), len(reads)))]
            c = (3 - c[::-1]).astype(np.uint8) if rng.random() < 0.5 else c
        else:
            c = rng.integers(0, 4, length - 20 + int(rng.integers(0, 41)), dtype=np.uint8)
        reads.append(c)
        reads = reads[-64:]
        L = len(c)
        v = nib[np.concatenate([c, np.zeros(L & 1, np.uint8)])]
        name = f"m1/{z}/ccs".encode()
        body = struct.pack("<iiBBHHHiiii", -1, -1, len(name) + 1, 255, 4680, 0, 4, L, -1, -1, 0) + name + b"\0" + ((v[0::2] << 4) | v[1::2]).tobytes() + b"\xff" * L
        body += b"rqf" + struct.pack("<f", float(rng.uniform(0.99, 1.0))) + b"zmi" + struct.pack("<i", z)
        raw.append(struct.pack("<i", len(body)) + body)
    data = b"".join(raw)
    with open(path, "wb") as f:
        for a in range(0, len(data), 0xff00):
            blk = data[a:a + 0xff00]
            co = zlib.compressobj(1, zlib.DEFLATED, -15)
            comp = co.compress(blk) + co.flush()
            f.write(b"\x1f\x8b\x08\x04" + b"\0" * 4 + b"\0\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, len(comp) + 25) + comp
                    + struct.pack("<II", zlib.crc32(blk) & 0xFFFFFFFF, len(blk)))
        f.write(bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0]))
    return os.path.getsize(path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-reads", type=int, default=1 << 20)
    ap.add_argument("--length", type=int, default=10000)
    ap.add_argument("--reads", type=int, default=32768, help="reads of the end-to-end BAM")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="seconds one GPU process may take")
    ap.add_argument("--work", default="/tmp/dup_bench")
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-cli", action="store_true")
    ap.add_argument("--build-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.build_only:
        return RB.build_kernel_bench("dup", DEPS)
    lines = ["python tools/dup_bench.py   (MI355X)", ""]
    if not a.skip_kernel:
        exe = RB.build_kernel_bench("dup", DEPS)
        lines += subprocess.run(["timeout", "-k", "10", str(a.limit), exe, str(a.kernel_reads), str(a.length)], check=True, capture_output=True, text=True).stdout.splitlines() + [""]
        print("\n".join(lines), flush=True)
    if not a.skip_cli:
        os.makedirs(a.work, exist_ok=True)
        bam, out = os.path.join(a.work, "in.bam"), os.path.join(a.work, "out.bam")
        size = write_bam(bam, a.reads, a.length)
        ccs = os.path.join(RB.R, "ccs_amd", "bin", "ccs")
        rows = []
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            p = subprocess.run(["timeout", "-k", "10", str(a.limit), ccs, "--mark-duplicates", bam, out, "--log-level", "INFO", "-j", "16"],
                               capture_output=True, text=True)
            if p.returncode != 0:
                sys.exit(f"ccs --mark-duplicates failed (exit {p.returncode}):\n{p.stderr}")      # (nothing more is started)
            m = re.search(r"(\d+) reads, (\d+) sets, (\d+) duplicates marked; pass 1 ([\d.]+) s \(of which ccsx_dup_sign_reads ([\d.]+) s.*ccsx_dup_cluster ([\d.]+) s, pass 2 ([\d.]+) s", p.stderr)
            wall = time.perf_counter() - t0
            rows.append((wall,) + tuple(float(x) for x in m.groups()[3:]) + tuple(int(x) for x in m.groups()[:3]))
            print(rows[-1], flush=True)
        med = lambda k: float(np.median([r[k] for r in rows]))      # noqa: E731
        span = lambda k: f"{med(k):.3f} ({min(r[k] for r in rows):.3f} - {max(r[k] for r in rows):.3f})"      # noqa: E731
        io = med(1) - med(2) + med(4)
        lines += [f"ccs --mark-duplicates end to end: a BAM of {a.reads} reads of {a.length} +- 20 bases ({size / 1e6:.0f} MB, BGZF level 1), one read in ten a copy of an "
                  f"earlier one; {rows[-1][5]} reads, {rows[-1][6]} sets, {rows[-1][7]} duplicates; -j 16; median (min - max) of {a.rounds} runs, seconds",
                  f"  whole process {span(0)}   (with the handle's creation and the process start)",
                  f"  pass 1 {span(1)}, of which ccsx_dup_sign_reads with its copies {span(2)}",
                  f"  ccsx_dup_cluster with its copies {span(3)}",
                  f"  pass 2 {span(4)}",
                  f"  inflate, parsing and decoding in pass 1 and inflate, copy and deflate in pass 2: {io:.3f} s = {100 * io / (med(1) + med(3) + med(4)):.0f} % of the three phases",
                  "  a new mode: no parent commit has it to compare with"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What the cell-tag analysis costs.  Two parts, every line of profiles/cell_bench.txt written here (the shared machinery: tools/reads_bench.py):
  1. k_cell alone on resident reads (tools/cell_bench/kernel_bench.hip with cdna_unit.hip, built here with hipcc): 16384 reads of 10 kb with the two fields
     planted, whitelists of 4096 and 2^23 barcodes; median, min and max of 7 launches, beside k_cdna at 2 primers on the same reads in the same process; the
     first 512 reads of each configuration are compared with the host rule.
  2. ccs --cell-reads end to end on a BAM of --e2e-reads such reads written here, with the phases its INFO line gives, `--rounds` times.
Each GPU step runs under its own time limit, and the first that fails ends the run.  --build-only: compile kernel_bench and stop (no GPU needed)."""
import argparse
import os
import re
import struct
import subprocess
import sys
import tempfile
import zlib

import numpy as np

import reads_bench as RB

DEPS = ("ccsx_cell.hip", "ccsx_cdna.hip", "ccsx_cell_api.cpp", "ccsx_cdna_api.cpp", "ccsx_barcode_api.cpp", "cell_core.h", "cdna_core.h", "dup_core.h", "segment_core.h",
        "barcode_core.h", "wave_ops.h")
M, TAIL, B, U = 25, 30, 16, 12


def build() -> str:
    d = os.path.join(RB.R, "tools", "cell_bench")
    srcs, exe = [os.path.join(d, "kernel_bench.hip"), os.path.join(d, "cdna_unit.hip")], os.path.join(d, "kernel_bench")
    files = srcs + [os.path.join(RB.CSRC, f) for f in DEPS]
    if not os.path.exists(exe) or any(os.path.getmtime(f) > os.path.getmtime(exe) for f in files):
        subprocess.check_call([os.environ.get("HIPCC", "hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(RB.R, "include"), "-I" + RB.CSRC, *srcs, "-o", exe])
    return exe


def write_inputs(d: str, n: int, L: int, nw: int) -> None:
    """in.bam (n reads of L bases shaped like kernel_bench's, BGZF at level 1), primers.fasta and wl.txt (nw barcodes) in d"""
    rng = np.random.default_rng(3)
    text = lambda c: "".join("ACGT"[int(x)] for x in c)              # noqa: E731
    rc = lambda x: (3 - x[::-1]).astype(np.uint8)                     # noqa: E731
    p5, p3 = rng.integers(0, 4, M).astype(np.uint8), rng.integers(0, 4, M).astype(np.uint8)
    wl = np.unique(rng.integers(0, 1 << 32, nw + nw // 8, dtype=np.uint64))[:nw]
    rng.shuffle(wl)
    codes = ((wl[:, None] >> (2 * (B - 1 - np.arange(B, dtype=np.uint64)))[None, :]) & np.uint64(3)).astype(np.uint8)
    with open(os.path.join(d, "primers.fasta"), "w") as f:
        f.write(f">five_5p\n{text(p5)}\n>three_3p\n{text(p3)}\n")
    with open(os.path.join(d, "wl.txt"), "w") as f:
        f.write("\n".join(text(c) for c in codes) + "\n")
    hdr = "@HD\tVN:1.6\tSO:unknown\tpb:5.0.0\n@RG\tID:ab12cd34\tPL:PACBIO\tDS:READTYPE=CCS\tPU:m1\n"
    nib = np.array([1, 2, 4, 8], np.uint8)
    data = bytearray(b"BAM\x01" + struct.pack("<i", len(hdr)) + hdr.encode() + struct.pack("<i", 0))
    with open(os.path.join(d, "in.bam"), "wb") as f:
        def flush(everything=False):
            while len(data) >= 0xff00 or (everything and data):
                payload = bytes(data[:0xff00])
                del data[:0xff00]
                co = zlib.compressobj(1, zlib.DEFLATED, -15)
                comp = co.compress(payload) + co.flush()
                f.write(b"\x1f\x8b\x08\x04" + b"\0" * 4 + b"\0\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, 25 + len(comp)) + comp +
                        struct.pack("<II", zlib.crc32(payload) & 0xFFFFFFFF, len(payload)))
        for z in range(n):
            bc = codes[rng.integers(0, nw)].copy()
            if z % 4 == 3:
                bc[rng.integers(0, B)] ^= 2
            fields = np.concatenate([bc, rng.integers(0, 4, U).astype(np.uint8)])
            c = np.concatenate([p5, rng.integers(0, 4, L - 2 * M - TAIL - B - U - 2).astype(np.uint8), np.array([2, 1], np.uint8), np.zeros(TAIL, np.uint8), rc(fields), rc(p3)])
            if z & 1:
                c = rc(c)
            name = f"m1/{z}/ccs".encode() + b"\0"
            v = nib[c]
            data += struct.pack("<iiiBBHHHiiii", 32 + len(name) + L // 2 + L + 7, -1, -1, len(name), 255, 4680, 0, 4, L, -1, -1, 0) + name + ((v[0::2] << 4) | v[1::2]).tobytes() + \
                b"\x28" * L + b"zmi" + struct.pack("<i", z)
            flush()
        flush(True)
        f.write(bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=16384)
    ap.add_argument("--length", type=int, default=10000)
    ap.add_argument("--e2e-reads", type=int, default=4096)
    ap.add_argument("--e2e-whitelist", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds one GPU step may take")
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--build-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.length % 2 == 0
    exe = build()
    if a.build_only:
        return
    lines = ["python tools/cell_bench.py   (MI355X)", ""]
    if not a.skip_kernel:
        lines += subprocess.run(["timeout", "-k", "10", str(a.limit), exe, str(a.reads), str(a.length)], check=True, capture_output=True, text=True).stdout.splitlines() + [""]
        print("\n".join(lines), flush=True)
    with tempfile.TemporaryDirectory(prefix="cell_bench_") as d:
        write_inputs(d, a.e2e_reads, a.length, a.e2e_whitelist)
        ccs = os.path.join(RB.R, "ccs_amd", "bin", "ccs")
        lines.append(f"ccs --cell-reads end to end: {a.e2e_reads} reads of {a.length} bases in a BAM of {os.path.getsize(os.path.join(d, 'in.bam')) / 1e6:.1f} MB, design T-12U-16B, "
                     f"a whitelist of {a.e2e_whitelist} barcodes, every fourth barcode with a substitution; {a.rounds} runs, one process each")
        for r in range(a.rounds):
            p = subprocess.run(["timeout", "-k", "10", str(a.limit), ccs, "--cell-reads", os.path.join(d, "in.bam"), os.path.join(d, "out.bam"), "--cdna-primers",
                                os.path.join(d, "primers.fasta"), "--cell-design", "T-12U-16B", "--cell-whitelist", os.path.join(d, "wl.txt"), "--log-level", "INFO"],
                               capture_output=True, text=True)
            got = [ln for ln in p.stderr.splitlines() if ln.startswith("ccs: --cell-reads:")]
            if p.returncode != 0 or not got:
                sys.exit(f"run {r} failed (exit {p.returncode}):\n{p.stderr}")   # (nothing more is started)
            lines.append("  " + re.sub(r"^ccs: --cell-reads: ", "", got[-1]))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

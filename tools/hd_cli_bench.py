#!/usr/bin/env python3
"""What `ccs --heteroduplexes` costs a run of the driver.  Every line of profiles/hd_cli_bench.txt is written here.
BAM -> BAM: 16384 ZMWs x 10 passes x 10 kb, every 20th ZMW a planted heteroduplex (tools/hd_synth.py: four substitutions on the reverse strand), -j 16.  A
planted ZMW has --het-passes passes, 10 + 10 by default: at 5 + 5 the rule's Fisher test cannot reach max_pvalue 1e-3 (its smallest p is 7.9e-3),
so a 10-pass heteroduplex is never called and the run would hold no strand ticket.  One process per configuration, alternating `--rounds` times after one uncounted run: the option
off, `split`, `drop`, and — given --parent-ccs, the driver of a built checkout of the parent commit — that binary.  Per configuration the wall time of the whole process and the ticket timings the driver prints at --log-level INFO.  "off" and
"parent" must lie inside each other's spread; `split` and `drop` are reported against "off" with its spread, and the ticket timings say which share of the
difference is the finder in the draft stage and which the single-strand tickets.
The input is written here, by --jobs processes (each its own run of BGZF blocks; BGZF blocks concatenate), into --dir and kept there for a second call."""
import argparse
import os
import re
import struct
import subprocess
import sys
import time
import zlib
from concurrent.futures import ProcessPoolExecutor

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [R, os.path.join(R, "tools"), os.path.join(R, "tests")]
CCS = os.path.join(R, "ccs_amd", "bin", "ccs")
HDR = ("@HD\tVN:1.6\tSO:unknown\tpb:5.0.0\n@RG\tID:x\tPL:PACBIO\tDS:READTYPE=SUBREAD;Ipd:CodecV1=ip;PulseWidth:CodecV1=pw;"
       "BINDINGKIT=101-789-500;SEQUENCINGKIT=101-826-100;BASECALLERVERSION=5.0.0;FRAMERATEHZ=100.000000\tPU:m1\tPM:SEQUELII\n")
NIB = np.array([1, 2, 4, 8], np.uint8)


def bgzf(payload: bytes) -> bytes:
    co = zlib.compressobj(1, zlib.DEFLATED, -15)
    comp = co.compress(payload) + co.flush()
    return (b"\x1f\x8b\x08\x04" + b"\0" * 4 + b"\0\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, 12 + 6 + len(comp) + 8 - 1) + comp +
            struct.pack("<II", zlib.crc32(payload) & 0xFFFFFFFF, len(payload)))


def record(name: bytes, bases, pw, ipd, zm, snr, cx) -> bytes:
    n = len(bases)
    nib = NIB[bases]
    if n & 1:
        nib = np.append(nib, np.uint8(0))
    packed = (nib[0::2] << 4 | nib[1::2]).astype(np.uint8).tobytes()
    body = (struct.pack("<iiBBHHHiiii", -1, -1, len(name) + 1, 255, 4680, 0, 4, n, -1, -1, 0) + name + b"\0" + packed + b"\xff" * n +
            b"zmi" + struct.pack("<i", zm) + b"snBf" + struct.pack("<i", 4) + np.asarray(snr, "<f4").tobytes() +
            b"pwBC" + struct.pack("<i", n) + pw.tobytes() + b"ipBC" + struct.pack("<i", n) + ipd.tobytes() + b"cxi" + struct.pack("<i", cx))
    return struct.pack("<i", len(body)) + body


def write_part(job):
    """ZMWs [z0, z1) as BGZF blocks in `path`: every `every`-th ZMW (hole number divisible by it) a planted heteroduplex"""
    import hd_synth
    path, z0, z1, passes, length, every, seed, het_passes = job
    buf, n_het = bytearray(), 0
    with open(path, "wb") as f:
        for z in range(z0, z1):
            het = every > 0 and z % every == 0
            b, _ = hd_synth.make(1, (het_passes if het else passes) // 2, length, seed=seed * 1000003 + z, k_sub=4 if het else 0, control=not het)
            n_het += het
            q = 0
            for r in range(int(b.read_off[1])):
                o, e = int(b.base_off[r]), int(b.base_off[r + 1])
                buf += record(b"m1/%d/%d_%d" % (z, q, q + e - o), b.bases[o:e], b.pw[o:e], b.ipd[o:e], z, b.snr[0], 3 | (32 if b.flags[r] & 1 else 16))
                q += e - o + 45
            while len(buf) >= 0xff00:
                f.write(bgzf(bytes(buf[:0xff00]))); del buf[:0xff00]
        # (a part ends on a block boundary: a record may span blocks, not parts)
        while buf:
            f.write(bgzf(bytes(buf[:0xff00]))); del buf[:0xff00]
    return n_het


def write_input(a, path):
    t0 = time.time()
    step = (a.zmws + a.jobs - 1) // a.jobs
    jobs = [(f"{path}.part{k}", z0, min(a.zmws, z0 + step), a.passes, a.length, a.het_every, a.seed, a.het_passes) for k, z0 in enumerate(range(0, a.zmws, step))]
    with ProcessPoolExecutor(a.jobs) as ex:
        n_het = sum(ex.map(write_part, jobs))
    with open(path, "wb") as f:
        f.write(bgzf(b"BAM\x01" + struct.pack("<i", len(HDR)) + HDR.encode() + struct.pack("<i", 0)))
        for j in jobs:
            with open(j[0], "rb") as g:
                while True:
                    chunk = g.read(1 << 24)
                    if not chunk:
                        break
                    f.write(chunk)
            os.remove(j[0])
        f.write(bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0]))
    return n_het, time.time() - t0


def run(ccs, a, inp, out, extra):
    """one process of the driver: wall seconds of the whole process and what its INFO lines say"""
    t0 = time.perf_counter()
    p = subprocess.run([ccs, inp, out, "-j", str(a.threads), "--log-level", "INFO", "--refresh-rate", "1e9", *extra], capture_output=True, text=True, timeout=a.timeout)
    wall = time.perf_counter() - t0
    if p.returncode != 0:
        sys.exit(f"{ccs} {' '.join(extra)} failed (exit {p.returncode}):\n{p.stderr[-3000:]}")                 # (nothing more is started)
    got = dict(wall=wall)
    m = re.search(r"engine \(ticket timings, (\d+) tickets, (\d+) ZMWs\): first kernel to last ([\d.]+) ms.*draft \+ align ([\d.]+) ms, polish ([\d.]+) ms, "
                  r"between the stages ([\d.]+) ms, ticket start to end ([\d.]+) ms", p.stderr)
    if m:
        got.update(tickets=int(m.group(1)), span_ms=float(m.group(3)), draft=float(m.group(4)), polish=float(m.group(5)), total=float(m.group(7)))
    m = re.search(r"single-strand tickets, (\d+) tickets, (\d+) strands\): on the device ([\d.]+) ms in all", p.stderr)
    if m:
        got.update(ss_tickets=int(m.group(1)), strands=int(m.group(2)), ss_ms=float(m.group(3)))
    m = re.search(r"(\d+) ZMWs in, (\d+) HiFi reads out.*?(\d+) heteroduplex ZMWs", p.stderr)
    if m:
        got.update(zmws=int(m.group(1)), reads=int(m.group(2)), het=int(m.group(3)))
    else:
        m = re.search(r"(\d+) ZMWs in, (\d+) HiFi reads out", p.stderr)
        got.update(zmws=int(m.group(1)), reads=int(m.group(2)))
    return got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--zmws", type=int, default=16384)
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--length", type=int, default=10000)
    ap.add_argument("--het-every", type=int, default=20)
    ap.add_argument("--het-passes", type=int, default=20, help="passes of a planted ZMW (half per strand)")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--jobs", type=int, default=16, help="processes that write the input")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=600, help="seconds a run of the driver may take")
    ap.add_argument("--parent-ccs", default=None, help="the ccs binary of a built checkout of the parent commit")
    ap.add_argument("--dir", default="/tmp/hd_cli_bench")
    ap.add_argument("--input-only", action="store_true")
    ap.add_argument("--out", default=None, help="the text is appended to this file")
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    inp = os.path.join(a.dir, f"in.{a.zmws}x{a.passes}x{a.length}.every{a.het_every}x{a.het_passes}.seed{a.seed}.subreads.bam")
    lines = ["python tools/hd_cli_bench.py   (MI355X)", ""]
    if not os.path.exists(inp):
        n_het, secs = write_input(a, inp)
        lines.append(f"input: {a.zmws} ZMWs x {a.passes} passes x {a.length} bases, {n_het} planted heteroduplexes (every {a.het_every}th ZMW: four substitutions on the "
                     f"reverse strand, {a.het_passes} passes), {os.path.getsize(inp) / 1e9:.2f} GB, written in {secs:.0f} s by {a.jobs} processes")
    else:
        lines.append(open(inp + ".txt").read().strip() if os.path.exists(inp + ".txt") else f"input: {inp} (kept from an earlier call), {os.path.getsize(inp) / 1e9:.2f} GB")
    print(lines[-1], flush=True)
    with open(inp + ".txt", "w") as f:
        f.write(lines[-1] + "\n")
    if a.input_only:
        return
    configs = [("off", CCS, []), ("split", CCS, ["--heteroduplexes", "split"]), ("drop", CCS, ["--heteroduplexes", "drop"])]
    if a.parent_ccs:
        configs.append(("parent", os.path.abspath(a.parent_ccs), []))
    every = {c: [] for c, _, _ in configs}
    got = run(CCS, a, inp, os.path.join(a.dir, "out.warm.bam"), [])       # one run that is not counted: the input in the page cache, the device awake
    print(f"warm-up (off, not counted): wall={got['wall']:.2f}", flush=True)
    for rnd in range(a.rounds):
        for c, ccs, extra in configs:
            got = run(ccs, a, inp, os.path.join(a.dir, f"out.{c}.bam"), extra)
            every[c].append(got)
            print(f"round {rnd} {c}: " + " ".join(f"{k}={v:.2f}" if isinstance(v, float) else f"{k}={v}" for k, v in got.items()), flush=True)
    med = lambda c, k: float(np.median([g[k] for g in every[c] if k in g])) if any(k in g for g in every[c]) else float("nan")
    lines.append(f"ccs IN.bam OUT.bam -j {a.threads} --log-level INFO, one process per configuration, alternating {a.rounds} rounds after one run that is not counted; wall: the whole process; the device "
                 "figures are the driver's ticket timings (HIP events), per 1000 ZMWs")
    for c, _, _ in configs:
        w = [g["wall"] for g in every[c]]
        g = every[c][-1]
        lines.append(f"  {c:6s} wall s by round: " + " ".join(f"{x:.2f}" for x in w) + f"   median {np.median(w):.2f} (min {min(w):.2f}, max {max(w):.2f}); "
                     f"{g.get('zmws')} ZMWs in, {g.get('reads')} reads in OUT" + (f", {g['het']} heteroduplex ZMWs" if "het" in g else ""))
        lines.append(f"         tickets {g.get('tickets')}: first kernel to last {med(c, 'span_ms'):.0f} ms; draft + align {med(c, 'draft'):.2f} ms, polish {med(c, 'polish'):.2f} ms, "
                     f"ticket start to end {med(c, 'total'):.2f} ms per 1000 ZMWs" +
                     (f"; single-strand tickets {g['ss_tickets']} with {g['strands']} strands, {med(c, 'ss_ms'):.0f} ms on the device in all" if "ss_tickets" in g else ""))
    off = [g["wall"] for g in every["off"]]
    for c in ("split", "drop"):
        lines.append(f"  {c} against off, median against median: wall {100 * (med(c, 'wall') / med('off', 'wall') - 1):+.2f} % (off spreads {100 * (min(off) / np.median(off) - 1):+.2f} "
                     f".. {100 * (max(off) / np.median(off) - 1):+.2f} %); first kernel to last {100 * (med(c, 'span_ms') / med('off', 'span_ms') - 1):+.2f} %; "
                     f"draft + align per 1000 ZMWs {100 * (med(c, 'draft') / med('off', 'draft') - 1):+.2f} %, polish {100 * (med(c, 'polish') / med('off', 'polish') - 1):+.2f} %")
    if a.parent_ccs:
        par = [g["wall"] for g in every["parent"]]
        inside = min(off) <= max(par) and min(par) <= max(off)
        lines.append(f"  off against the parent commit's driver, median against median: {100 * (np.median(off) / np.median(par) - 1):+.2f} %; the two spreads "
                     f"{'overlap' if inside else 'DO NOT overlap'}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()

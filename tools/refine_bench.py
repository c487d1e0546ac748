#!/usr/bin/env python3
"""What the polisher hand-back costs in the ticketed path (default 16384 ZMWs x 10 passes x 10 kb, the bench.py workload).  For a kernel trace:
    rocprofv3 --kernel-trace --stats -d OUT -o trace -- python tools/refine_bench.py --rounds 1 --steps 3 --warmup 1
    python tools/refine_bench.py --trace-summary OUT --out profiles/refine_rocprofv3_summary.txt
Every second 100-base tile of every consensus is replaced (docs/faq/revio.md:40: 30-70 % of the windows go through the second polisher): the replacement is the
tile's own bases with the last one dropped, kept or doubled in turn, so the spliced sequences stay as good as the base.  The batch goes through `--steps` tickets
(three in flight, after `--warmup` tickets) of ccsx_submit_polish(QV_ONLY) on the sequences spliced beforehand on the host — the existing seam, the baseline —,
of ccsx_submit_refine with the tiles in torch tensors on the GPU, and of ccsx_submit_refine with the tiles in page-locked host memory, alternating `--rounds`
times in the same process; one JSON line gives per configuration the best round's step time, every round's step time and the spread of the baseline.
--out FILE: the lines of profiles/refine_bench.txt, every one written here."""
import argparse
import ctypes as C
import glob
import json
import os
import sqlite3
import sys
import time

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)

CONFIGS = ("polish_seam", "device", "pinned_host")
KERNELS = ("k_refine_check", "k_refine_plan", "k_refine_splice")


def trace_summary(root, out):
    """per-kernel durations of a rocprofv3 --kernel-trace run (its rocpd database under `root`), and the three hand-back kernels' ms per launch"""
    dbs = sorted(glob.glob(os.path.join(root, "**", "*_results.db"), recursive=True))
    if not dbs:
        sys.exit(f"no *_results.db under {root}")
    rows = sqlite3.connect(dbs[0]).execute("select name, count(*), sum(end-start), avg(end-start), min(end-start), max(end-start) from kernels group by name order by 3 desc").fetchall()
    tot = sum(r[2] for r in rows) or 1
    short = lambda n: n.replace("(anonymous namespace)::", "").split("(")[0].split("::")[-1]
    steps = max([r[1] for r in rows if short(r[0]).startswith("k_stitch")] or [0])
    asked = max([r[1] for r in rows if short(r[0]).startswith(KERNELS)] or [0])
    lines = ["the polisher hand-back in the ticketed path: a rocprofv3 --kernel-trace --stats run of tools/refine_bench.py (no counters in this run)",
             f"{steps} tickets in the trace, the base consensus, the draft run and warm-up tickets included; {asked} of them were hand-backs", "",
             f"{'kernel':40s} {'calls':>6s} {'total_ms':>12s} {'avg_ms':>12s} {'min_ms':>12s} {'max_ms':>12s} {'pct':>7s}"]
    for n, k, s, a, mn, mx in rows:
        lines.append(f"{short(n)[:40]:40s} {k:6d} {s / 1e6:12.3f} {a / 1e6:12.3f} {mn / 1e6:12.3f} {mx / 1e6:12.3f} {100 * s / tot:7.2f}")
    lines.append("")
    for kn in KERNELS:
        kr = [r for r in rows if short(r[0]).startswith(kn)]
        lines.append(f"{kn}: {kr[0][3] / 1e6:.3f} ms per launch ({kr[0][1]} launches)" if kr else f"{kn}: not in the trace")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        with open(out, "w") as f:
            f.write(text)


def half_the_tiles(base, T=100, U=128):
    """every second T-base tile of every consensus: (tile_zmw, tile_start, tile_len, new_len, new_seq, new_qual) and the per-position repeat counts that give the
    same splice on the host (np.repeat): the last base of a replaced tile is dropped, kept or doubled in turn"""
    L = base.seq_len.astype(np.int64)
    nt = (L + T - 1) // T
    z = np.repeat(np.arange(len(L)), nt)
    t = np.arange(int(nt.sum())) - np.repeat(np.cumsum(nt) - nt, nt)
    sel = (t % 2) == 0
    z, t = z[sel], t[sel]
    start = t * T
    ln = np.minimum(T, L[z] - start)
    d = (np.arange(len(z)) % 3) - 1
    d[ln + d < 1] = 0
    nl = ln + d
    m = len(z)
    seq, qual = np.zeros((m, U), np.uint8), np.zeros((m, U), np.uint8)
    o = base.seq_off[z] + start
    for a in range(0, m, 1 << 16):
        b = min(m, a + (1 << 16))
        idx = o[a:b, None] + np.minimum(np.arange(U)[None, :], ln[a:b, None] - 1)
        live = np.arange(U)[None, :] < nl[a:b, None]
        seq[a:b], qual[a:b] = np.where(live, base.seq[idx], 0), np.where(live, base.qual[idx], 0)
    rep = np.ones(len(base.seq), np.int8)
    rep[o + ln - 1] = 1 + d
    return (z.astype(np.int32), start.astype(np.int32), ln.astype(np.int32), nl.astype(np.int32), seq, qual), rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--zmws", type=int, default=16384)
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--length", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-summary", default=None)
    a = ap.parse_args()
    if a.trace_summary:
        return trace_summary(a.trace_summary, a.out)
    import torch                                               # BEFORE the first call into libccsx.so: the two share one HIP runtime only in this order
    torch.cuda.init()
    from ccs_amd import api
    L_ = api.lib()
    plain = api.synth(a.zmws, a.passes, a.length, seed=1).pinned()
    h = api.Handle(0)
    base = api.Results.allocate(plain, pinned=True, raw=False)
    t = h.submit(plain, base)
    h.wait(t)
    h.release(t)
    dr = h.draft(plain)
    backbone = dr.backbone.copy()
    arrays, rep = half_the_tiles(base)
    n_tiles = len(arrays[0])
    # the baseline's drafts: the same splice on the host
    drafts = api.Drafts.allocate(plain, pinned=True)
    for z in range(plain.n_zmw):
        o, k = int(base.seq_off[z]), int(base.seq_len[z])
        d = np.repeat(base.seq[o:o + k], rep[o:o + k])
        drafts.seq[o:o + len(d)] = d
        drafts.len[z], drafts.backbone[z] = len(d), backbone[z]
    res = [api.Results.allocate(plain, pinned=True, raw=False) for _ in range(3)]
    reps = [api.RefineReport.allocate(plain, pinned=True) for _ in range(3)]
    tiles = dict(device=api.RefineTiles.from_arrays(*arrays, device=0), pinned_host=api.RefineTiles.from_arrays(*arrays, pinned=True))
    cb, cd = plain.c_struct(), drafts.c_struct()
    out = dict(zmws=a.zmws, passes=a.passes, length=a.length, steps=a.steps, warmup=a.warmup, rounds=a.rounds, tile_len=100, stride=128, n_tiles=n_tiles,
               tiles_per_zmw=round(n_tiles / a.zmws, 1), tile_bytes_per_ticket=int(sum(x.nbytes for x in arrays)))

    def submit(name, i):
        if name == "polish_seam":
            tk = C.c_int64()
            cr = res[i % 3].c_struct()
            h._check(L_.ccsx_submit_polish(h._h, C.byref(cb), C.byref(cd), C.byref(cr), api.QV_ONLY, C.byref(tk)), "ccsx_submit_polish")
            return tk.value, cr
        return h.submit_refine(plain, base, tiles[name], backbone, res[i % 3], reps[i % 3]), None

    def run(k, name):
        ts = [submit(name, i) for i in range(k)]               # (a submit that reuses a slot retires its ticket)
        for tk, _ in ts[-3:]:
            h._check(L_.ccsx_wait(h._h, tk), "ccsx_wait")
        tm = [h.ticket_timings(tk) for tk, _ in ts[-3:]]
        for tk, _ in ts:
            h.release(tk)
        return tm

    every = {name: [] for name in CONFIGS}
    keep = {}
    for _ in range(a.rounds):
        for name in CONFIGS:
            run(a.warmup, name)
            t0 = time.perf_counter()
            tm = run(a.steps, name)
            wall = time.perf_counter() - t0
            r = dict(zmws_per_s=round(a.steps * a.zmws / wall, 1), step_ms=round(wall * 1e3 / a.steps, 2))
            every[name].append(r["step_ms"])
            for f in ("setup_ms", "polish_ms", "total_ms"):
                r[f] = round(float(np.mean([getattr(x, f) for x in tm])), 2)
            last = (a.steps - 1) % 3
            keep[name] = (res[last].status.copy(), res[last].seq_len.copy(), res[last].qual.copy(), res[last].rq.copy())
            if name not in out or r["step_ms"] < out[name]["step_ms"]:
                out[name] = r
    last = (a.steps - 1) % 3
    out["counts"] = [int(x) for x in reps[last].counts]
    out["codes"] = {api.REFINE_CODE_NAMES[int(c)]: int(k) for c, k in zip(*np.unique(reps[last].code, return_counts=True))}
    out["same_results"] = bool(all(np.array_equal(keep["polish_seam"][i], keep[c][i]) for c in CONFIGS[1:] for i in range(4)))
    out["step_ms_by_round"] = every
    nr = every["polish_seam"]
    out["polish_seam_spread_pct"] = round(100.0 * (max(nr) - min(nr)) / min(nr), 2)
    for c in CONFIGS[1:]:
        out[c + "_adds_pct"] = round(100.0 * (out[c]["step_ms"] / out["polish_seam"]["step_ms"] - 1.0), 2)
        out[c + "_adds_pct_mean"] = round(100.0 * (float(np.mean(every[c])) / float(np.mean(nr)) - 1.0), 2)
    line = json.dumps(out)
    print(line)
    if a.out:
        fmt = lambda v: " ".join(f"{x:.2f}" for x in v)
        with open(a.out, "w") as f:
            f.write(f"python tools/refine_bench.py   (MI355X; {a.zmws} ZMWs x {a.passes} passes x {a.length} bases, {a.steps} tickets with three in flight after {a.warmup} "
                    f"warm-up\ntickets: ccsx_submit_polish(QV_ONLY) on the sequences spliced beforehand on the host, ccsx_submit_refine with the tiles in torch tensors on the "
                    f"GPU and\nwith the tiles in page-locked host memory; every second 100-base tile of every consensus replaced, {n_tiles} tiles, stride 128, the merged quals "
                    f"downloaded;\nalternating {a.rounds} rounds in one process)\n\n")
            f.write(line + "\n\n")
            f.write(f"ms per step by round: polish seam on host-spliced drafts {fmt(nr)} (spread {out['polish_seam_spread_pct']:.2f} %), hand-back with device tiles "
                    f"{fmt(every['device'])}, with page-locked host tiles {fmt(every['pinned_host'])}.\n")
            for c, what in (("device", "device tiles"), ("pinned_host", "page-locked host tiles")):
                f.write(f"Best round against best round: {what} {out[c + '_adds_pct']:+.2f} %; mean against mean {out[c + '_adds_pct_mean']:+.2f} %.\n")
            f.write(f"counts: {out['counts'][0]} ZMWs refined, {out['counts'][1]} tiles applied, {out['counts'][2]} list-order violations; codes {out['codes']}; the tile list "
                    f"is {out['tile_bytes_per_ticket']} bytes per ticket.\n")
            f.write(f"Statuses, lengths, quals and rq of the hand-back equal those of the polish seam on the host-spliced drafts: {out['same_results']}.\n")
    h.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The study behind the poly(A) defaults of the cDNA rule (DESIGN.md §2 "cDNA rule"), on the CPU: molecules 5p . insert . A x t . rc(3p) with tails of 15-150
bases, half of them with an A-rich stretch (70 % A over 30 bases, ending in a base other than A) just upstream of the tail, molecules without a tail (half of
them with the same A-rich stretch before the 3' primer) and concatemers of two molecules, on either strand, are sequenced into 3, 6 and 10 passes
(tools/lowcx.py, the numpy channel), the oracle makes their consensus, and the rule's restatement (tests/cdna_ref.py) is applied.  Over a grid of
polya_mismatch x polya_xdrop x polya_max, per pass count: the error of polya_len against the planted length (plain and A-rich inserts apart), the tails of at
least min_polya planted bases that come out shorter than min_polya (missed), and the bare inserts given a tail of min_polya or more.  The concatemers missed and
invented do not depend on the scan and are given once per pass count.
    python tools/cdna_study.py [--out profiles/cdna_study.txt]"""
import argparse
import os
import sys

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tools"))
sys.path.insert(0, os.path.join(R, "tests"))
from ccs_amd import api  # noqa: E402
import adapter_synth  # noqa: E402
import cdna_ref as REF  # noqa: E402
import oracle_lib  # noqa: E402

M, SEED = 25, 7300
N_TAILED, N_BARE, N_CONCAT, INSERT, TAILS = 64, 32, 16, (500, 901), (15, 151)
GRID = [(mm, xd, pm) for pm in (128, 512) for mm in (1, 2, 3, 4) for xd in (3, 6, 10, 16)]


def insert(rng, rich: bool) -> np.ndarray:
    b = REF.body(rng, int(rng.integers(*INSERT)))
    if rich:
        b[-30:-1] = np.where(rng.random(29) < 0.7, REF.A, b[-30:-1])
    return b


def molecules(rng, p5, p3):
    """(templates, kind, planted tail, A-rich) per molecule; every second template reverse complemented"""
    tpls, meta = [], []
    for z in range(N_TAILED + N_BARE + N_CONCAT):
        rich = bool(z & 2)
        if z < N_TAILED:
            t = int(rng.integers(*TAILS))
            tpl, kind = REF.mol(p5, p3, insert(rng, rich), t), "tailed"
        elif z < N_TAILED + N_BARE:
            t, tpl, kind = 0, REF.mol(p5, p3, insert(rng, rich), 0), "bare"
        else:
            t = 30
            tpl, kind = REF.cat(REF.mol(p5, p3, insert(rng, False), 30), REF.mol(p5, p3, insert(rng, rich), t)), "concat"
        tpls.append(REF.rc(tpl) if z & 1 else tpl)
        meta.append((kind, t, rich))
    return tpls, meta


def consensus(tpls, passes, rng):
    b = adapter_synth.from_templates(tpls, [passes] * len(tpls), rng)
    res = api.Results.allocate(b)
    oracle_lib.consensus_batch(api.default_model(), api.default_opts(), b, res, nthreads=min(16, os.cpu_count() or 1))
    return [res.sequence(z).copy() if res.seq_len[z] > 0 else None for z in range(b.n_zmw)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(R, "profiles", "cdna_study.txt"))
    a = ap.parse_args()
    rng = np.random.default_rng(SEED)
    p5, p3 = REF.random_set(rng, 2, [M])
    o = api.cdna_opts_default()
    shipped = (o.polya_mismatch, o.polya_xdrop, o.polya_max)
    lines = [f"cDNA poly(A) scan: two random {M}-mers as 5' and 3' primer; per pass count {N_TAILED} molecules with a tail of {TAILS[0]}-{TAILS[1] - 1} A, {N_BARE} without a "
             f"tail and {N_CONCAT} concatemers of two molecules, inserts of {INSERT[0]}-{INSERT[1] - 1} bases, every second insert A-rich before the tail (70 % A over 30 "
             f"bases), every second molecule reverse complemented; tools/lowcx.py channel, oracle consensus; seed {SEED}",
             f"shipped defaults: polya_mismatch {o.polya_mismatch}, polya_xdrop {o.polya_xdrop}, polya_max {o.polya_max}, min_polya {o.min_polya}", "",
             "passes  mismatch  xdrop  polya_max   tailed reads   mean |err| plain   A-rich   max |err|   tails >= min_polya missed   bare reads   given a tail"]
    total = {g: [0, 0.0, 0, 0, 0, 0] for g in GRID}              # tailed reads, sum |err|, max |err|, missed, bare reads, bare given a tail
    for passes in (3, 6, 10):
        tpls, meta = molecules(rng, p5, p3)
        reads = consensus(tpls, passes, rng)
        have = [z for z, c in enumerate(reads) if c is not None]
        base = REF.cdna_reads([p5, p3], [0, 1], [reads[z] for z in have], min_polya=0, min_len=1)        # ends, strand and internal hits: not the scan's
        ok = {z: i for i, z in enumerate(have) if base["strand"][i] >= 0 and base["cls"][i] != REF.SHORT}
        wrong = sum(1 for i, z in enumerate(have) if base["strand"][i] >= 0 and base["strand"][i] != (z & 1))
        cm = sum(1 for z, i in ok.items() if meta[z][0] == "concat" and base["n_internal"][i] == 0)
        ci = sum(1 for z, i in ok.items() if meta[z][0] != "concat" and base["n_internal"][i] > 0)
        nc = sum(1 for z in ok if meta[z][0] == "concat")
        lines.append(f"{passes:6d}  {len(have)} of {len(reads)} molecules reach a consensus, {len(ok)} with both primers called ({wrong} on the wrong strand); concatemers missed "
                     f"{cm} of {nc}, invented {ci} of {len(ok) - nc}")
        xs = {}
        for z, i in ok.items():
            c, L = reads[z], len(reads[z])
            c0, c1 = int(base["clip"][i][0]), int(base["clip"][i][1])
            xs[z] = REF.polya_x(c, int(base["strand"][i]), c0, c1, min(512, L - c0 - c1))
        for g in GRID:
            mm, xd, pm = g
            err = {False: [], True: []}
            missed = bare = given = 0
            for z, x in xs.items():
                kind, t, rich = meta[z]
                got = REF.polya_scan(x[:pm], mm, xd)
                if kind == "tailed":
                    err[rich].append(abs(got - t))
                    missed += t >= o.min_polya and got < o.min_polya
                elif kind == "bare":
                    bare += 1
                    given += got >= o.min_polya
            both = err[False] + err[True]
            for k, v in enumerate((len(both), float(sum(both)), 0, missed, bare, given)):
                total[g][k] += v
            total[g][2] = max(total[g][2], max(both))
            lines.append(f"{passes:6d}  {mm:8d}  {xd:5d}  {pm:9d}   {len(both):12d}   {np.mean(err[False]):17.2f}   {np.mean(err[True]):6.2f}   {max(both):9d}   {missed:25d}   "
                         f"{bare:10d}   {given:12d}" + ("   <- shipped" if g == shipped else ""))
        lines.append("")
    lines.append("all pass counts together: (mismatch, xdrop, polya_max) -> mean and largest |polya_len - planted|, tails missed at min_polya, bare inserts given a tail")
    for g in GRID:
        n, s, mx, missed, bare, given = total[g]
        lines.append(f"  mismatch {g[0]} xdrop {g[1]:2d} polya_max {g[2]:3d}: mean {s / n:6.2f}, largest {mx:3d}, {missed:3d} of {n} tails missed, {given:3d} of {bare} bare inserts given a tail"
                     + ("   <- shipped" if g == shipped else ""))
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()

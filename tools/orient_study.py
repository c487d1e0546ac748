#!/usr/bin/env python3
"""The study behind the defaults of the pass orientation (DESIGN.md §2 "Pass orientation"), on the CPU: the rule's restatement (tests/orient_ref.py) on the
project's synthetic generator (api.synth) and on tools/lowcx.py data (low-complexity templates, the numpy channel).  Per generator, insert length and pass count
every pass is submitted strand-unknown with a random bit; behind the full-length passes of every ZMW come partial passes (a piece of 50-500 bases of a pass,
either strand) and junk passes (random bases, as long as a pass).  Against the generator's truth: wrong calls (SAME / OPPOSITE against the true relative strand of
the anchor; any call of a junk pass), the share UNDETERMINED, and the distributions (min / median / max) of v_same and v_opp for true-same, true-opposite and junk
passes.  Then the same votes under a grid of options: the shipped defaults must show zero wrong calls.
    python tools/orient_study.py [--out profiles/orient_study.txt]"""
import argparse
import os
import sys

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tools"))
sys.path.insert(0, os.path.join(R, "tests"))
from ccs_amd import api  # noqa: E402
import lowcx  # noqa: E402
import orient_lab  # noqa: E402
import orient_ref as REF  # noqa: E402

U = REF.UNKNOWN
ZMWS = {200: 24, 1000: 16, 10000: 6, 20000: 4}
GRID = [(m, r) for m in (4, 6, 8, 12, 16, 20, 24, 32) for r in (2, 3, 4, 8)]


def zmw_passes(rng, gen, passes, length, seed):
    """[(bases, true strand)] of one ZMW's full-length passes"""
    if gen == "synth":
        b = api.synth(1, passes, length, seed=seed)
        return [(b.read(r)[0].copy(), int(b.flags[r]) & 1) for r in range(passes)]
    t = lowcx.lowcx_template(rng, length)
    out = []
    for k in range(passes):
        s, _ = lowcx.sequence_read(rng, t)
        out.append((REF.revcomp(s) if k & 1 else s.astype(np.uint8), k & 1))
    return out


def one_set(rng, gen, passes, length, seed):
    """(batch, truth per pass: relative strand class 0 same-as-stored / 1 = the stored strand bit, kind per pass: 'full' 'partial' 'junk')"""
    Z, truth, kind = [], [], []
    for z in range(ZMWS[length]):
        full = zmw_passes(rng, gen, passes, length, seed + z)
        ps = [(b, U | int(rng.integers(0, 2))) for b, _ in full]
        truth += [s for _, s in full]; kind += ["full"] * len(full)
        for _ in range(2):                                              # partial passes: a piece of a pass, at either end's adapter
            b, s = full[int(rng.integers(0, len(full)))]
            n = int(min(len(b), rng.integers(50, 501)))
            a = int(rng.integers(0, len(b) - n + 1))
            ps.append((b[a:a + n].copy(), U | 2 | (4 * int(rng.integers(0, 2))) | int(rng.integers(0, 2)))); truth.append(s); kind.append("partial")
        for _ in range(2):                                              # junk passes: unrelated bases
            ps.append((rng.integers(0, 4, len(full[0][0])).astype(np.uint8), U | 2 | int(rng.integers(0, 2)))); truth.append(-1); kind.append("junk")
        Z.append(ps)
    return orient_lab.make_batch(Z), np.array(truth), np.array(kind)


def judge(batch, rep, truth, kind, opts):
    """(wrong calls, undetermined, decided) over the passes that are not anchors"""
    wrong = und = n = 0
    for z in range(batch.n_zmw):
        r0, r1 = int(batch.read_off[z]), int(batch.read_off[z + 1])
        a = r0 + int(rep["anchor"][z])
        for r in range(r0, r1):
            if r == a:
                continue
            n += 1
            c = REF.call(int(rep["votes_same"][r]), int(rep["votes_opp"][r]), opts)
            if c == REF.UNDETERMINED:
                und += 1
            elif truth[r] < 0 or (c == REF.SAME) != (truth[r] == truth[a]):
                wrong += 1
    return wrong, und, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=4100)
    ap.add_argument("--passes", default="3,10,30")
    ap.add_argument("--lengths", default="200,1000,10000,20000")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    D = REF.DEFAULTS
    rng = np.random.default_rng(a.seed)
    f = lambda x: " ".join(f"{int(v):6d}" for v in (x.min(), np.median(x), x.max())) if len(x) else "-"
    lines = [f"pass orientation: per generator, insert length and pass count {ZMWS} ZMWs (by length); every pass strand-unknown with a random bit; per ZMW two partial",
             f"passes of 50-500 bases and two junk passes behind the full-length ones; seed {a.seed}", "shipped defaults: " + ", ".join(f"{k} {v}" for k, v in D.items()), "",
             f"{'generator':9s} {'length':>6s} {'passes':>6s} {'judged':>6s} {'wrong':>5s} {'full undet %':>12s} {'partial undet %':>15s} {'junk undet %':>12s}   "
             f"{'true-same: v_same min med max':>30s} {'v_opp':>20s}   {'true-opposite: v_same':>22s} {'v_opp':>20s}   {'junk: v_same':>20s} {'v_opp':>20s}"]
    grid = {g: [0, 0, 0, 0, 0] for g in GRID}
    total_wrong = 0
    for gen in ("synth", "lowcx"):
        for length in (int(x) for x in a.lengths.split(",")):
            for passes in (int(x) for x in a.passes.split(",")):
                b, truth, kind = one_set(rng, gen, passes, length, a.seed + 1000 * passes + length)
                rep = REF.orient(b)
                w, u, n = judge(b, rep, truth, kind, D)
                total_wrong += w
                for g in GRID:
                    x = judge(b, rep, truth, kind, dict(min_votes=g[0], ratio=g[1]))
                    for i in range(3):
                        grid[g][i] += x[i]
                    real = kind != "junk"
                    c = np.array([REF.call(int(vs_), int(vo_), dict(min_votes=g[0], ratio=g[1])) for vs_, vo_ in zip(rep["votes_same"], rep["votes_opp"])])
                    anc = np.zeros(len(truth), bool); anc[b.read_off[:-1] + rep["anchor"]] = True
                    grid[g][3] += int((real & ~anc & (c == REF.UNDETERMINED)).sum()); grid[g][4] += int((real & ~anc).sum())
                anchors = np.zeros(len(truth), bool)
                anchors[b.read_off[:-1] + rep["anchor"]] = True
                ta = np.repeat(truth[b.read_off[:-1] + rep["anchor"]], np.diff(b.read_off))
                und = rep["call"] == REF.UNDETERMINED
                share = lambda m: f"{100.0 * und[m].sum() / max(1, m.sum()):.1f}"
                same, opp, junk = ~anchors & (truth >= 0) & (truth == ta), ~anchors & (truth >= 0) & (truth != ta), kind == "junk"
                vs, vo = rep["votes_same"], rep["votes_opp"]
                lines.append(f"{gen:9s} {length:6d} {passes:6d} {n:6d} {w:5d} {share(~anchors & (kind == 'full')):>12s} {share(kind == 'partial'):>15s} {share(junk):>12s}   "
                             f"{f(vs[same]):>30s} {f(vo[same]):>20s}   {f(vs[opp]):>22s} {f(vo[opp]):>20s}   {f(vs[junk]):>20s} {f(vo[junk]):>20s}")
    lines += ["", "the same votes under other options (all sets together): min_votes ratio -> wrong calls, undetermined % of the passes of the molecule (full and partial)"]
    for g in GRID:
        w, u, n, ur, nr = grid[g]
        lines.append(f"  min_votes {g[0]:2d} ratio {g[1]}: {w:4d} wrong, {100.0 * ur / nr:5.1f} % undetermined of {nr}" + ("   <- shipped" if g == (D["min_votes"], D["ratio"]) else ""))
    lines += ["", "with the shipped defaults no pass is called wrong" if total_wrong == 0 else f"the shipped defaults call {total_wrong} passes WRONG"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()

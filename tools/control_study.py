#!/usr/bin/env python3
"""The study behind the control screen's defaults (DESIGN.md §2 "Control screen"), on the CPU: tools/control_synth.py data through the oracle
(tests/oracle_lib.py) and the rule's restatement (tests/control_ref.py).  Per kind and pass count: the ZMWs whose draft cascade ends in SUCCESS (the oracle's final
status is not a draft-stage failure: those are the tested ones), how many of them the shipped defaults flag, and the distributions (min / median / max) of
`matched`, of the control span in tenths of M and of the draft span in tenths of L on the pass-0 POA draft.
    python tools/control_study.py [--out profiles/control_study.txt]"""
import argparse
import os
import sys

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tools"))
sys.path.insert(0, os.path.join(R, "tests"))
from ccs_amd import api  # noqa: E402
import control_ref  # noqa: E402
import control_synth as S  # noqa: E402
import oracle_lib  # noqa: E402

DRAFT_FAILURES = (1, 2, 3, 5, 6)      # TOO_FEW_PASSES, DRAFT_FAILURE, TOO_MANY_UNUSABLE, TOO_SHORT, TOO_LONG


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--per-kind", type=int, default=44)             # x 6 kinds = 264 ZMWs per set
    ap.add_argument("--length", default="300,6000")
    ap.add_argument("--passes", default="3,5,10,30")
    ap.add_argument("--seed", type=int, default=2040)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    llo, lhi = (int(x) for x in a.length.split(","))
    C = S.encode(S.TEST_CONTROL)
    M = len(C)
    D = control_ref.DEFAULTS
    lines = [f"control screen: {a.per_kind} ZMWs per kind and pass count ({a.per_kind * len(S.KINDS)} per set), random parts of {llo}-{lhi} bases, the 2000-base "
             f"test control, seed {a.seed}",
             "shipped defaults: " + ", ".join(f"{k} {v}" for k, v in D.items()), "",
             f"{'kind':11s} {'passes':>6s} {'ZMWs':>5s} {'tested':>6s} {'flagged':>7s}   {'matched: min med max':>22s}   {'ctl span, tenths of M':>22s}   {'draft span, tenths of L':>23s}"]
    wrong = []
    for passes in (int(x) for x in a.passes.split(",")):
        n = a.per_kind * len(S.KINDS)
        b, kinds = S.make(n, passes, (llo, lhi), seed=a.seed + passes)
        res = api.Results.allocate(b)
        oracle_lib.consensus_batch(api.default_model(), api.default_opts(), b, res, nthreads=a.threads)
        tested = ~np.isin(res.status, DRAFT_FAILURES)
        for k, name in enumerate(S.KINDS):
            zs = np.flatnonzero(kinds == k)
            m, cs, ds, flagged = [], [], [], 0
            for z in zs:
                if not tested[z]:
                    continue
                d = oracle_lib.poa_draft(b, int(z))
                r = control_ref.screen(d, C)
                flagged += r["verdict"] == control_ref.FOUND
                m.append(r["matched"]); cs.append(10.0 * (r["ctl_end"] - r["ctl_start"]) / M); ds.append(10.0 * (r["draft_end"] - r["draft_start"]) / max(1, len(d)))
            nt = int(tested[zs].sum())
            want = nt if name in ("control", "control_rc") else 0 if name in ("partial", "random", "lowcx") else None
            if want is not None and flagged != want:
                wrong.append(f"{name} at {passes} passes: {flagged} flagged of {nt} tested, expected {want}")
            f = lambda x, fmt: " ".join(format(v, fmt) for v in (min(x), float(np.median(x)), max(x))) if x else "-"
            lines.append(f"{name:11s} {passes:6d} {len(zs):5d} {nt:6d} {flagged:7d}   {f(m, '6.0f'):>22s}   {f(cs, '6.2f'):>22s}   {f(ds, '6.2f'):>23s}")
    lines += ["", "with the shipped defaults every tested control / control_rc ZMW is flagged and no partial / random / lowcx ZMW" if not wrong else
              "the shipped defaults do NOT separate the kinds: " + "; ".join(wrong)]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()

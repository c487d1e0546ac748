#!/usr/bin/env python3
"""The study behind the adapter screen's defaults (DESIGN.md §2 "Adapter screen"), on the CPU: tools/adapter_synth.py data through the oracle
(tests/oracle_lib.py) and the rule's restatement (tests/adapter_ref.py).  Per kind and pass count: the ZMWs whose draft cascade ends in SUCCESS (the oracle's final
status is not a draft-stage failure: those are the tested ones), the distribution of a hit's `dist` on the pass-0 POA draft and on a last-resort draft (a raw
pass; the oracle has no seam that returns a fallback draft, so that class is not reported), the verdicts on the POA draft, and over the controls the smallest
E anywhere.
    python tools/adapter_study.py [--out profiles/adapter_study.txt]"""
import argparse
import os
import sys

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tools"))
sys.path.insert(0, os.path.join(R, "tests"))
from ccs_amd import api  # noqa: E402
import adapter_ref  # noqa: E402
import adapter_synth as S  # noqa: E402
import oracle_lib  # noqa: E402

DRAFT_FAILURES = (1, 2, 3, 5, 6)      # TOO_FEW_PASSES, DRAFT_FAILURE, TOO_MANY_UNUSABLE, TOO_SHORT, TOO_LONG


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--per-kind", type=int, default=24)
    ap.add_argument("--length", default="500,8000")
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    llo, lhi = (int(x) for x in a.length.split(","))
    A = [adapter_ref.encode(S.SMRTBELL)]
    o = api.adapter_opts_default()
    lines = [f"adapter screen: {a.per_kind} ZMWs per kind and pass count, templates of {llo}-{lhi} bases (dimers: 4-40 copies), the built-in adapter, seed {a.seed}",
             f"defaults: max_dist_pct {o.max_dist_pct} (k = 9), min_copies {o.min_copies}, max_insert {o.max_insert}, end_slack {o.end_slack}", "",
             f"{'kind':11s} {'passes':>6s} {'ZMWs':>5s} {'tested':>6s} {'hits/ZMW':>8s} {'CONCAT':>6s} {'NEAR':>5s} {'both':>5s} {'none':>5s}   "
             f"{'dist on POA drafts: mean max':>28s}   {'on raw passes: mean max found/planted':>38s}"]
    smallest = {}
    for passes in (3, 6, 10):
        n = a.per_kind * len(S.KINDS)
        b, kinds = S.make(n, passes, (llo, lhi), seed=a.seed + passes)
        res = api.Results.allocate(b)
        oracle_lib.consensus_batch(api.default_model(), api.default_opts(), b, res, nthreads=a.threads)
        tested = ~np.isin(res.status, DRAFT_FAILURES)
        for k, name in enumerate(S.KINDS):
            zs = np.flatnonzero(kinds == k)
            v = np.zeros(4, int)
            dist, rdist, nh, planted, found = [], [], 0, 0, 0
            for z in zs:
                if not tested[z]:
                    continue
                d = oracle_lib.poa_draft(b, int(z))
                r = adapter_ref.screen(d, A)
                v[r["verdict"]] += 1
                nh += r["n_hits"]
                for s, p in enumerate(adapter_ref.searches(A)):
                    dist += [h[3] for h in adapter_ref.search_hits(p, d, 9, s)[0]]
                r0 = int(b.read_off[z])
                raw = b.bases[int(b.base_off[r0]):int(b.base_off[r0 + 1])]
                t = b.tpl[int(b.tpl_off[z]):int(b.tpl_off[z + 1])]
                if name in ("dimer", "near_end", "interior", "palindrome"):
                    planted += adapter_ref.screen(t, A)["n_hits"]
                    for s, p in enumerate(adapter_ref.searches(A)):
                        hs = adapter_ref.search_hits(p, raw, 9, s)[0]
                        rdist += [h[3] for h in hs]
                        found += len(hs)
                else:
                    smallest[name] = min(smallest.get(name, 99), adapter_ref.smallest_distance(d, A), adapter_ref.smallest_distance(raw, A))
            nt = int(tested[zs].sum())
            f = lambda x: f"{np.mean(x):.2f} {max(x):3d}" if x else "   -   -"
            lines.append(f"{name:11s} {passes:6d} {len(zs):5d} {nt:6d} {nh / max(1, nt):8.2f} {v[1]:6d} {v[2]:5d} {v[3]:5d} {v[0]:5d}   {f(dist):>28s}   "
                         f"{f(rdist):>24s} {found:6d}/{planted:<6d}")
    lines += ["", "smallest E of either search anywhere on a control's POA draft or raw pass (k = 9): " + ", ".join(f"{k} {v}" for k, v in sorted(smallest.items()))]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()

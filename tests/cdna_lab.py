"""The synthetic molecules of the cDNA tests: templates 5p . transcript . poly(A) . rc(3p) of two 25-base primers and transcripts of 500 .. 900 bases, sequenced
into passes (tools/adapter_synth.py from_templates), as an api.Batch for the library's tests."""
from __future__ import annotations

import numpy as np

import adapter_synth
import cdna_ref as R

SEED = 5
TAIL = 30
# the kinds take turns.  sense / antisense: a full-length molecule with an A x 30 tail, as it reads / reverse complemented; notail: no poly(A); concatemer: two
# molecules in one; oneprimer: the 3' primer is not there; fivefive: the 5' primer at both ends; none: no primer at all; fail: two passes, below
# opts.min_passes, no consensus (the last two ZMWs)
KINDS = ("sense", "antisense", "notail", "concatemer", "oneprimer", "fivefive", "none")


def primers(seed=SEED) -> tuple:
    """(primers as code arrays, roles)"""
    return R.random_set(np.random.default_rng(seed + 1000), 2, [25]), [0, 1]


def templates(n=14, seed=SEED) -> tuple:
    """(templates, passes per ZMW, kind per ZMW)"""
    rng = np.random.default_rng(seed)
    (p5, p3), _ = primers(seed)
    tpls, npass, kinds = [], [], []
    for z in range(n):
        kind = "fail" if z >= n - 2 else KINDS[z % len(KINDS)]
        t = R.body(rng, int(rng.integers(500, 901)))
        full = R.mol(p5, p3, t, TAIL)
        tpls.append({"antisense": R.rc(full), "notail": R.mol(p5, p3, t, 0), "concatemer": R.cat(full, R.mol(p5, p3, R.body(rng, 400), TAIL)),
                     "oneprimer": R.cat(p5, t, np.full(TAIL, R.A, np.uint8)), "fivefive": R.cat(p5, t, R.rc(p5)), "none": t}.get(kind, full))
        npass.append(2 if kind == "fail" else 8)
        kinds.append(kind)
    return tpls, npass, kinds


def batch(n=14, seed=SEED):
    """(api.Batch, kinds, primers as code arrays, roles)"""
    tpls, npass, kinds = templates(n, seed)
    return (adapter_synth.from_templates(tpls, npass, np.random.default_rng(seed + 1)), kinds) + primers(seed)

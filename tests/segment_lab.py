"""The synthetic molecules of the segment tests: templates A0 S1 A1 .. SK AK of five 25-base adapters and segments of 300 .. 600 bases, sequenced into passes
(tools/adapter_synth.py from_templates), as an api.Batch for the library's tests."""
from __future__ import annotations

import numpy as np

import adapter_synth
import segment_ref as R

SEED = 11
N_ADAPTERS = 5
# the kinds take turns.  forward / reverse: the whole array of four segments, as the set reads / reverse complemented; partial: its first three segments only;
# missing: the middle adapter is not there, segments 2 and 3 are one piece; none: no adapter at all; fail: two passes, below opts.min_passes, no consensus
KINDS = ("forward", "reverse", "partial", "missing", "none", "fail")


def adapter_set(seed=SEED) -> list:
    return R.random_set(np.random.default_rng(seed + 1000), N_ADAPTERS, [25])


def templates(n=12, seed=SEED) -> tuple:
    """(templates, passes per ZMW, kind per ZMW)"""
    rng = np.random.default_rng(seed)
    S = adapter_set(seed)
    tpls, npass, kinds = [], [], []
    for z in range(n):
        kind = KINDS[z % len(KINDS)]
        segs = [R.rand(rng, int(rng.integers(300, 601))) for _ in range(N_ADAPTERS - 1)]
        if kind == "none":
            t = R.cat(*segs[:3])
        elif kind == "partial":
            t = R.cat(S[0], segs[0], S[1], segs[1], S[2], segs[2], S[3])
        elif kind == "missing":
            t = R.cat(S[0], segs[0], S[1], segs[1], segs[2], S[3], segs[3], S[4])
        else:
            t = R.cat(S[0], segs[0], S[1], segs[1], S[2], segs[2], S[3], segs[3], S[4])
        tpls.append(R.rc(t) if kind == "reverse" else t)
        npass.append(2 if kind == "fail" else 8)
        kinds.append(kind)
    return tpls, npass, kinds


def batch(n=12, seed=SEED):
    """(api.Batch, kinds, adapter set as code arrays)"""
    tpls, npass, kinds = templates(n, seed)
    return adapter_synth.from_templates(tpls, npass, np.random.default_rng(seed + 1)), kinds, adapter_set(seed)

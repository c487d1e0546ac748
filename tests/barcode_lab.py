"""The synthetic molecules of the barcode tests: templates barcode_a · insert · rc(barcode_b) sequenced into passes (tools/adapter_synth.py from_templates), as an
api.Batch for the library's tests and as (zm, kind, passes) for the driver's."""
from __future__ import annotations

import numpy as np

import adapter_synth
import barcode_ref as R

SEED = 7
N_BARCODES = 12
KINDS = ("both", "both", "head", "tail", "none", "fail")        # the kinds take turns; fail: two passes, below opts.min_passes, no consensus


def barcode_set(seed=SEED) -> list:
    """12 random 16-mers; the last one is 20 bases long, so that the set has two lengths"""
    rng = np.random.default_rng(seed + 1000)
    S = R.random_set(rng, N_BARCODES, [16])
    S[-1] = rng.integers(0, 4, 20).astype(np.uint8)
    return S


def templates(n=24, seed=SEED) -> tuple:
    """(templates, passes per ZMW, kind per ZMW, (a, b) planted per ZMW or -1)"""
    rng = np.random.default_rng(seed)
    S = barcode_set(seed)
    tpls, npass, kinds, planted = [], [], [], []
    for z in range(n):
        kind = KINDS[z % len(KINDS)]
        a, b = int(rng.integers(0, N_BARCODES)), int(rng.integers(0, N_BARCODES))
        if kind in ("tail", "none"):
            a = -1
        if kind in ("head", "none"):
            b = -1
        insert = rng.integers(0, 4, int(rng.integers(2000, 3000))).astype(np.uint8)
        tpls.append(np.concatenate([S[a] if a >= 0 else insert[:0], insert, R.rc(S[b]) if b >= 0 else insert[:0]]).astype(np.uint8))
        npass.append(2 if kind == "fail" else 8)
        kinds.append(kind)
        planted.append((a, b))
    return tpls, npass, kinds, planted


def batch(n=24, seed=SEED):
    """(api.Batch, kinds, planted, barcode set as code arrays)"""
    tpls, npass, kinds, planted = templates(n, seed)
    return adapter_synth.from_templates(tpls, npass, np.random.default_rng(seed + 1)), kinds, planted, barcode_set(seed)

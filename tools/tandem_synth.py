#!/usr/bin/env python3
"""Synthetic ZMWs for tandem-repeat detection (DESIGN.md §2 "Tandem repeats"): random templates, some with ONE planted tract of
`tract` bases (the `AGGGGT` x n of docs/faq/low-complexity.md:11-12, or a random 2-4-mer unit), the rest random controls.  Reads go
through the off-model channel of tools/lowcx.py.  Pure numpy, independent of the library's generator."""
from __future__ import annotations

import os
import sys

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tools"))
from ccs_amd import api  # noqa: E402
import lowcx  # noqa: E402

AGGGGT = np.array([0, 2, 2, 2, 2, 3], np.uint8)


def tract_template(rng, L, tract_len, kind):
    """random template of L bases with one tract of tract_len bases at a random place; kind 'aggggt' or 'kmer' (unit of 2-4 bases)"""
    t = rng.integers(0, 4, L, dtype=np.uint8)
    if tract_len <= 0:
        return t
    if kind == "aggggt":
        unit = AGGGGT
    else:
        u = int(rng.integers(2, 5))
        unit = rng.integers(0, 4, u, dtype=np.uint8)
        while len(set(unit.tolist())) == 1:
            unit = rng.integers(0, 4, u, dtype=np.uint8)
    n = min(tract_len, L)
    p = int(rng.integers(0, L - n + 1))
    t[p:p + n] = np.tile(unit, n // len(unit) + 1)[:n]
    return t


def make(n, passes, length, seed, frac=0.5, tract=(1000, 2000), channel=1.0):
    """(api.Batch, tract lengths [n] with 0 = control).  passes / length / tract: int or (lo, hi)"""
    rng = np.random.default_rng(seed)
    plo, phi = (passes, passes) if isinstance(passes, int) else passes
    llo, lhi = (length, length) if isinstance(length, int) else length
    tlo, thi = (tract, tract) if isinstance(tract, int) else tract
    zmw_id, snr, read_off, base_off, flags, tpls, tpl_off, tracts = [], [], [0], [0], [], [], [0], []
    bases, pws = [], []
    for z in range(n):
        P = int(rng.integers(plo, phi + 1))
        L = int(rng.integers(llo, lhi + 1))
        tl = int(rng.integers(tlo, thi + 1)) if rng.random() < frac else 0
        t = tract_template(rng, L, tl, "aggggt" if rng.random() < 0.5 else "kmer")
        tracts.append(min(tl, L))
        tpls.append(t); tpl_off.append(tpl_off[-1] + L)
        zmw_id.append(z)
        snr.append(np.maximum(4.0, np.array([9.0, 16.0, 8.0, 13.0]) * (1 + 0.1 * rng.standard_normal(4))))
        for k in range(P):
            b, p = lowcx.sequence_read(rng, t, channel)
            if k & 1:
                b, p = (3 - b[::-1]).astype(np.uint8), p[::-1]
            bases.append(b); pws.append(p); flags.append(k & 1)
            base_off.append(base_off[-1] + len(b))
        read_off.append(read_off[-1] + P)
    nb = base_off[-1]
    batch = api.Batch(np.array(zmw_id, np.int32), np.ascontiguousarray(np.array(snr, np.float32)), np.array(read_off, np.int32),
                      np.array(base_off, np.int64), np.ascontiguousarray(np.concatenate(bases), np.uint8),
                      np.ascontiguousarray(np.concatenate(pws), np.uint8), rng.integers(1, 61, nb).astype(np.uint8),
                      np.array(flags, np.uint8), tpl_off=np.array(tpl_off, np.int64), tpl=np.concatenate(tpls).astype(np.uint8))
    return batch, np.array(tracts, np.int32)

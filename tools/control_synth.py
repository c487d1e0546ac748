#!/usr/bin/env python3
"""Synthetic ZMWs for the control screen (DESIGN.md §2 "Control screen"): molecules that are the spike-in control, and molecules that are not.  control: the
control C as given; control_rc: its reverse complement; partial: a random template with a stretch of 30-45 % of C inside; concat: C · spacer · C (spacer of
0-200 random bases); random and lowcx (tools/lowcx.py) templates without any of it.  Reads go through the off-model channel of tools/lowcx.py by
adapter_synth.from_templates.  Pure numpy."""
from __future__ import annotations

import os
import sys

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tools"))
import lowcx  # noqa: E402
from adapter_synth import encode, from_templates, noisy, rc  # noqa: E402,F401

KINDS = ("control", "control_rc", "partial", "concat", "random", "lowcx")


def decode(x):
    return "".join("ACGT"[int(c)] for c in x)


# two fixed, unrelated 2000-base test controls (fixed seeds, so that tests name them in a FASTA)
TEST_CONTROL = decode(np.random.default_rng(20020).integers(0, 4, 2000))
TEST_CONTROL_B = decode(np.random.default_rng(20021).integers(0, 4, 2000))


def template(rng, kind, L, control):
    """a template of kind `kind` around `control` (codes); L is the length of the random part of partial, and of random and lowcx"""
    rnd = lambda m: rng.integers(0, 4, int(m), dtype=np.uint8)
    C = np.asarray(control, np.uint8)
    M = len(C)
    if kind == "control":
        return C.copy()
    if kind == "control_rc":
        return rc(C)
    if kind == "partial":
        m = int(rng.integers((30 * M + 99) // 100, 45 * M // 100 + 1))
        s = int(rng.integers(0, M - m + 1))
        part = C[s:s + m] if rng.random() < 0.5 else rc(C[s:s + m])
        a = int(rng.integers(0, L + 1))
        return np.concatenate([rnd(a), part, rnd(L - a)])
    if kind == "concat":
        return np.concatenate([C, rnd(rng.integers(0, 201)), C])
    if kind == "random":
        return rnd(L)
    if kind == "lowcx":
        return lowcx.lowcx_template(rng, L)
    raise ValueError(kind)


def make(n, passes, length, seed, control=TEST_CONTROL, kinds=KINDS, channel=1.0):
    """(api.Batch, kind index into `kinds` [n]).  passes / length: int or (lo, hi); the kinds take turns.  Odd passes are reverse complements"""
    rng = np.random.default_rng(seed)
    C = encode(control) if isinstance(control, str) else np.asarray(control, np.uint8)
    plo, phi = (passes, passes) if isinstance(passes, int) else passes
    llo, lhi = (length, length) if isinstance(length, int) else length
    tpls, npass, kk = [], [], []
    for z in range(n):
        k = z % len(kinds)
        kk.append(k); npass.append(int(rng.integers(plo, phi + 1)))
        tpls.append(template(rng, kinds[k], int(rng.integers(llo, lhi + 1)), C))
    return from_templates(tpls, npass, rng, channel), np.array(kk, np.int32)

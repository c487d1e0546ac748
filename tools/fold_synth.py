#!/usr/bin/env python3
"""Synthetic ZMWs for adapter-palindrome detection (DESIGN.md §2 "Adapter palindromes"): templates X·A·rc(X) that a missed adapter makes (A a random
45-base loop), asymmetric ones X·A·rc(suffix of X), and three kinds of controls: random templates, templates with an internal inverted repeat that does not
reach the ends, and templates with tandem tracts.  Reads go through the off-model channel of tools/lowcx.py.  Pure numpy."""
from __future__ import annotations

import os
import sys

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tools"))
from ccs_amd import api  # noqa: E402
import lowcx  # noqa: E402
import tandem_synth  # noqa: E402

CLASSES = ("palindrome", "asymmetric", "random", "inverted", "tandem")
PLANTED = ("palindrome", "asymmetric")
LOOP = 45


def rc(x):
    return (3 - np.asarray(x, np.uint8)[::-1]).astype(np.uint8)


def template(rng, kind, L):
    """(template of about L bases, fold centre or -1).  palindrome: arms of (L - 45) / 2; asymmetric: the second arm is 30-80 % of the first;
    inverted: a 500-bp inverted repeat with a 45-500 bp gap inside the middle half; tandem: one tract of a quarter to a half of L"""
    rnd = lambda m: rng.integers(0, 4, m, dtype=np.uint8)
    if kind == "palindrome":
        m = max(1, (L - LOOP) // 2)
        X = rnd(m)
        return np.concatenate([X, rnd(LOOP), rc(X)]), m + LOOP // 2
    if kind == "asymmetric":
        m = max(2, int((L - LOOP) / 1.55))
        s = int(m * rng.uniform(0.3, 0.8))
        X = rnd(m)
        return np.concatenate([X, rnd(LOOP), rc(X[m - s:])]), m + LOOP // 2
    if kind == "random":
        return rnd(L), -1
    if kind == "inverted":
        t = rnd(L)
        margin = max(250, L // 8)                                   # both copies stay this far from the ends
        gap = int(rng.integers(LOOP, 501))
        ir = min(500, (L - 2 * margin - gap) // 2)
        if ir < 50:
            gap, ir = LOOP, max(0, min(500, (L - 2 * margin - LOOP) // 2))
        p = int(rng.integers(margin, max(margin + 1, L - margin - 2 * ir - gap + 1)))
        t[p + ir + gap:p + 2 * ir + gap] = rc(t[p:p + ir])
        return t, -1
    if kind == "tandem":
        return tandem_synth.tract_template(rng, L, int(rng.integers(L // 4, L // 2 + 1)), "aggggt" if rng.random() < 0.5 else "kmer"), -1
    raise ValueError(kind)


def make(n, passes, length, seed, classes=CLASSES, channel=1.0):
    """(api.Batch, class index into `classes` [n], fold centre in template coordinates [n], -1 for controls).  passes / length: int or (lo, hi); the
    classes take turns.  Odd passes are reverse complements, read 0 has the template's orientation."""
    rng = np.random.default_rng(seed)
    plo, phi = (passes, passes) if isinstance(passes, int) else passes
    llo, lhi = (length, length) if isinstance(length, int) else length
    zmw_id, snr, read_off, base_off, flags, tpls, tpl_off, kinds, centres = [], [], [0], [0], [], [], [0], [], []
    bases, pws = [], []
    for z in range(n):
        P = int(rng.integers(plo, phi + 1))
        k = z % len(classes)
        t, c = template(rng, classes[k], int(rng.integers(llo, lhi + 1)))
        kinds.append(k); centres.append(c)
        tpls.append(t); tpl_off.append(tpl_off[-1] + len(t))
        zmw_id.append(z)
        snr.append(np.maximum(4.0, np.array([9.0, 16.0, 8.0, 13.0]) * (1 + 0.1 * rng.standard_normal(4))))
        for q in range(P):
            b, p = lowcx.sequence_read(rng, t, channel)
            if q & 1:
                b, p = rc(b), p[::-1]
            bases.append(b); pws.append(p); flags.append(q & 1)
            base_off.append(base_off[-1] + len(b))
        read_off.append(read_off[-1] + P)
    nb = base_off[-1]
    batch = api.Batch(np.array(zmw_id, np.int32), np.ascontiguousarray(np.array(snr, np.float32)), np.array(read_off, np.int32),
                      np.array(base_off, np.int64), np.ascontiguousarray(np.concatenate(bases), np.uint8),
                      np.ascontiguousarray(np.concatenate(pws), np.uint8), rng.integers(1, 61, nb).astype(np.uint8),
                      np.array(flags, np.uint8), tpl_off=np.array(tpl_off, np.int64), tpl=np.concatenate(tpls).astype(np.uint8))
    return batch, np.array(kinds, np.int32), np.array(centres, np.int32)

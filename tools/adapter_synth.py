#!/usr/bin/env python3
"""Synthetic ZMWs for the adapter screen (DESIGN.md §2 "Adapter screen"): templates that carry SMRTbell adapter sequence the adapter finder missed, and
controls.  dimer: 4-40 adapter copies in either orientation with spacers of 0-60 random bases; near_end: a random insert with an adapter 0-150 bases from one
end and the reverse complement of that short arm on its other side (the short-arm X·A·rc(X)); interior: one adapter in the middle of a random insert, arms
unrelated; palindrome: X·A·rc(X) with the adapter at the fold (tools/fold_synth.py's palindrome with the real loop); random and lowcx (tools/lowcx.py) controls.
Reads go through the off-model channel of tools/lowcx.py.  Pure numpy."""
from __future__ import annotations

import os
import sys

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tools"))
from ccs_amd import api  # noqa: E402
import lowcx  # noqa: E402

KINDS = ("dimer", "near_end", "interior", "palindrome", "random", "lowcx")
SMRTBELL = "ATCTCTCTCTTTTCCTCCTCCTCCGTTGTTGTTGTTGAGAGAGAT"
# a 40-base test adapter that is not the built-in one (fixed, so that tests name it in a FASTA)
TEST_ADAPTER = "GCATGTCAGTACCGATAGCTTGCAAGTCCGTATGACGTCA"


def encode(s):
    return np.array(["ACGT".index(c) for c in s.upper()], np.uint8)


def rc(x):
    return (3 - np.asarray(x, np.uint8)[::-1]).astype(np.uint8)


def template(rng, kind, L, adapter):
    """a template of about L bases (dimer: as long as its copies make it) that carries `adapter` (codes) as its kind says"""
    rnd = lambda m: rng.integers(0, 4, int(m), dtype=np.uint8)
    A = np.asarray(adapter, np.uint8)
    one = lambda: A if rng.random() < 0.5 else rc(A)
    if kind == "dimer":
        parts = []
        for _ in range(int(rng.integers(4, 41))):
            parts += [one(), rnd(rng.integers(0, 61))]
        return np.concatenate(parts[:-1])
    if kind == "near_end":
        arm = rnd(rng.integers(0, 151))
        ins = rnd(max(500, L))
        t = np.concatenate([arm, one(), rc(arm), ins])
        return t if rng.random() < 0.5 else rc(t)
    if kind == "interior":
        h = max(400, L // 2)
        return np.concatenate([rnd(h), one(), rnd(h)])
    if kind == "palindrome":
        X = rnd(max(300, (L - len(A)) // 2))
        return np.concatenate([X, one(), rc(X)])
    if kind == "random":
        return rnd(L)
    if kind == "lowcx":
        return lowcx.lowcx_template(rng, L)
    raise ValueError(kind)


def noisy(rng, t, sub=0.02, indel=0.01):
    """t with substitutions and indels at the given rates (the CPU behaviour tests' stand-in for a draft)"""
    out = []
    for b in t:
        u = rng.random()
        if u < indel / 2:
            continue
        if u < indel:
            out.append(int(rng.integers(0, 4)))
        out.append(int((b + rng.integers(1, 4)) & 3) if rng.random() < sub else int(b))
    return np.array(out, np.uint8)


def make(n, passes, length, seed, adapter=SMRTBELL, kinds=KINDS, channel=1.0):
    """(api.Batch, kind index into `kinds` [n]).  passes / length: int or (lo, hi); the kinds take turns.  Odd passes are reverse complements"""
    rng = np.random.default_rng(seed)
    A = encode(adapter) if isinstance(adapter, str) else np.asarray(adapter, np.uint8)
    plo, phi = (passes, passes) if isinstance(passes, int) else passes
    llo, lhi = (length, length) if isinstance(length, int) else length
    tpls, npass, kk = [], [], []
    for z in range(n):
        k = z % len(kinds)
        kk.append(k); npass.append(int(rng.integers(plo, phi + 1)))
        tpls.append(template(rng, kinds[k], int(rng.integers(llo, lhi + 1)), A))
    return from_templates(tpls, npass, rng, channel), np.array(kk, np.int32)


def from_templates(tpls, npass, rng, channel=1.0):
    zmw_id, snr, read_off, base_off, flags, bases, pws = [], [], [0], [0], [], [], []
    for z, t in enumerate(tpls):
        zmw_id.append(z)
        snr.append(np.maximum(4.0, np.array([9.0, 16.0, 8.0, 13.0]) * (1 + 0.1 * rng.standard_normal(4))))
        for q in range(npass[z]):
            b, p = lowcx.sequence_read(rng, t, channel)
            if q & 1:
                b, p = rc(b), p[::-1]
            bases.append(b); pws.append(p); flags.append(q & 1); base_off.append(base_off[-1] + len(b))
        read_off.append(read_off[-1] + npass[z])
    nb = base_off[-1]
    return api.Batch(np.array(zmw_id, np.int32), np.ascontiguousarray(np.array(snr, np.float32)), np.array(read_off, np.int32),
                     np.array(base_off, np.int64), np.ascontiguousarray(np.concatenate(bases), np.uint8),
                     np.ascontiguousarray(np.concatenate(pws), np.uint8), rng.integers(1, 61, nb).astype(np.uint8),
                     np.array(flags, np.uint8), tpl_off=np.concatenate([[0], np.cumsum([len(t) for t in tpls])]).astype(np.int64),
                     tpl=np.concatenate(tpls).astype(np.uint8))

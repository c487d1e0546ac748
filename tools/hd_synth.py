#!/usr/bin/env python3
"""Synthetic heteroduplexes (and homoduplex controls) for the heteroduplex finder, pure numpy on tools/lowcx.sequence_read's channel.

A ZMW alternates forward and reverse passes.  Forward passes read template t; reverse passes are revcomp(sequence_read(t')), where t' is t with `k_sub`
planted substitutions and / or one planted insertion (indel > 0) or deletion (indel < 0) of |indel| bases.  A control has t' = t.  Templates are random
or low-complexity (lowcx.lowcx_template).  `make` returns the batch and the truth: the HD flag, both strand templates (forward orientation) and the
planted positions (columns of t; an indel's is where it starts).
"""
from __future__ import annotations

import os
import sys

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tools"))
from ccs_amd import api  # noqa: E402
from lowcx import lowcx_template, sequence_read  # noqa: E402


def revcomp(s):
    return (3 - s[::-1]).astype(np.uint8)


def plant(rng, t, k_sub=0, indel=0, margin=60, spacing=40):
    """t' and the planted columns: k_sub substitutions and at most one indel, at least `spacing` apart and `margin` from the ends"""
    L = len(t)
    want = k_sub + (1 if indel else 0)
    cols = []
    while len(cols) < want:
        c = int(rng.integers(margin, L - margin - abs(indel)))
        if all(abs(c - d) >= spacing + abs(indel) for d in cols):
            cols.append(c)
    cols.sort()
    ind_col = int(cols[rng.integers(0, len(cols))]) if indel else -1
    t2 = t.copy()
    subs = [c for c in cols if c != ind_col]
    for c in subs:
        t2[c] = (t[c] + rng.integers(1, 4)) & 3
    if indel > 0:
        t2 = np.concatenate([t2[:ind_col], rng.integers(0, 4, indel, dtype=np.uint8), t2[ind_col:]]).astype(np.uint8)
    elif indel < 0:
        t2 = np.concatenate([t2[:ind_col], t2[ind_col - indel:]]).astype(np.uint8)
    return t2, subs, ind_col


def make(n, passes_per_strand, length, seed, k_sub=0, indel=0, tpl="random", control=False, partial=False):
    """an api.Batch of n ZMWs with 2 x passes_per_strand passes and templates of `length` bases (each an int or (lo, hi)), and the truth dict:
    hd [n] bool, t_fwd / t_rev lists (forward orientation), subs (columns of t), indel_col (-1 = none), indel (signed length)"""
    rng = np.random.default_rng(seed)
    plo, phi = (passes_per_strand, passes_per_strand) if isinstance(passes_per_strand, int) else passes_per_strand
    zmw_id, snr, read_off, base_off, flags, bases, pws = [], [], [0], [0], [], [], []
    truth = dict(hd=np.zeros(n, bool), t_fwd=[], t_rev=[], subs=[], indel_col=[], indel=indel)
    llo, lhi = (length, length) if isinstance(length, int) else length
    for z in range(n):
        L = int(round(np.exp(rng.uniform(np.log(llo), np.log(lhi))))) if lhi > llo else llo
        t = lowcx_template(rng, L) if tpl == "lowcx" else rng.integers(0, 4, L, dtype=np.uint8)
        if control:
            t2, subs, ic = t.copy(), [], -1
        else:
            t2, subs, ic = plant(rng, t, k_sub, indel)
        truth["hd"][z] = not control and (len(subs) > 0 or ic >= 0)
        truth["t_fwd"].append(t); truth["t_rev"].append(t2); truth["subs"].append(subs); truth["indel_col"].append(ic)
        zmw_id.append(z)
        snr.append(np.maximum(4.0, np.array([9.0, 16.0, 8.0, 13.0]) * (1 + 0.1 * rng.standard_normal(4))))
        P = 2 * int(rng.integers(plo, phi + 1))
        reads = []
        for k in range(P):
            if k & 1:
                b, p = sequence_read(rng, t2)
                b, p = revcomp(b), p[::-1]
            else:
                b, p = sequence_read(rng, t)
            reads.append((b, p, k & 1))
        if partial:                                   # a partial pass at each end of the polymerase read: a suffix of the first, a prefix of the last
            b, p = sequence_read(rng, t)
            cut = int(rng.integers(len(b) // 4, 3 * len(b) // 4))
            reads.append((b[cut:], p[cut:], 2 | 4))          # (adapter at its end)
            b, p = sequence_read(rng, t2)
            b, p = revcomp(b), p[::-1]
            cut = int(rng.integers(len(b) // 4, 3 * len(b) // 4))
            reads.append((b[:cut], p[:cut], 1 | 2))          # (adapter at its start)
        for b, p, f in reads:
            bases.append(b); pws.append(p); flags.append(f)
            base_off.append(base_off[-1] + len(b))
        read_off.append(read_off[-1] + len(reads))
    nb = base_off[-1]
    tpl_all = np.concatenate(truth["t_fwd"]).astype(np.uint8)
    tpl_off = np.concatenate([[0], np.cumsum([len(t) for t in truth["t_fwd"]])]).astype(np.int64)
    batch = api.Batch(np.array(zmw_id, np.int32), np.ascontiguousarray(np.array(snr, np.float32)), np.array(read_off, np.int32),
                      np.array(base_off, np.int64), np.ascontiguousarray(np.concatenate(bases), np.uint8),
                      np.ascontiguousarray(np.concatenate(pws), np.uint8), rng.integers(1, 61, nb).astype(np.uint8),
                      np.array(flags, np.uint8), tpl_off=tpl_off, tpl=tpl_all)
    return batch, truth

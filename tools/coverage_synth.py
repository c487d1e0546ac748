"""Planted layouts for the coverage screen (DESIGN.md §2 "Coverage rule"): ZMWs whose passes are given one by one — the template each pass reads, its strand,
and for a partial pass the end of the molecule it is anchored at — through the channel of tools/lowcx.py (about 11 % errors)."""
import os
import sys

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tools"))
import lowcx  # noqa: E402
from ccs_amd import api  # noqa: E402


def rnd(rng, m):
    return rng.integers(0, 4, int(m), dtype=np.uint8)


def rc(x):
    return (3 - np.asarray(x, np.uint8)[::-1]).astype(np.uint8)


def with_block(t, block, at):
    return np.concatenate([t[:at], block, t[at:]]).astype(np.uint8)


class Pass:
    """one pass: the bases it reads in the molecule's forward orientation, its strand, and for a partial pass which end of the molecule it holds
    ("head": it ends early, "tail": it starts late; None: full length)"""

    def __init__(self, tpl, rev=False, part=None):
        self.tpl, self.rev, self.part = np.asarray(tpl, np.uint8), bool(rev), part

    def flags(self):
        f = int(self.rev)
        if self.part is not None:
            from_end = self.part == "tail"               # anchored at the molecule's end, in forward orientation
            f |= 2 | (4 if from_end != self.rev else 0)  # bit 2: the adapter is at the pass's own end
        return f


def strands(n, both):
    return [bool(q & 1) and both for q in range(n)]


def clean(t, n, both=False):
    return [Pass(t, r) for r in strands(n, both)]


def blocked(t, block, at, which, n, both=False):
    """n passes of t, those in `which` with `block` inserted before position `at`"""
    return [Pass(with_block(t, block, at) if q in which else t, r) for q, r in enumerate(strands(n, both))]


def with_partials(t, n_full, fractions, both=False):
    """n_full passes of t, then partial passes that hold the given fractions of it, heads and tails in turn"""
    out = clean(t, n_full, both)
    for k, f in enumerate(fractions):
        m = int(len(t) * f)
        out.append(Pass(t[:m] if k % 2 == 0 else t[len(t) - m:], both and bool(k & 1), "head" if k % 2 == 0 else "tail"))
    return out


def batch(zmws, rng, channel=1.0, first_id=0):
    """an api.Batch of the given ZMWs (a list of Pass each; partial passes last).  tpl: the first pass's template"""
    zmw_id, snr, read_off, base_off, flags, bases, pws, tpls = [], [], [0], [0], [], [], [], []
    for z, passes in enumerate(zmws):
        zmw_id.append(first_id + z)
        snr.append(np.maximum(4.0, np.array([9.0, 16.0, 8.0, 13.0]) * (1 + 0.1 * rng.standard_normal(4))))
        tpls.append(passes[0].tpl)
        for p in passes:
            b, w = lowcx.sequence_read(rng, p.tpl, channel)
            if p.rev:
                b, w = rc(b), w[::-1]
            bases.append(b); pws.append(w); flags.append(p.flags()); base_off.append(base_off[-1] + len(b))
        read_off.append(read_off[-1] + len(passes))
    nb = base_off[-1]
    return api.Batch(np.array(zmw_id, np.int32), np.ascontiguousarray(np.array(snr, np.float32)), np.array(read_off, np.int32),
                     np.array(base_off, np.int64), np.ascontiguousarray(np.concatenate(bases), np.uint8),
                     np.ascontiguousarray(np.concatenate(pws), np.uint8), rng.integers(1, 61, nb).astype(np.uint8),
                     np.array(flags, np.uint8), tpl_off=np.concatenate([[0], np.cumsum([len(t) for t in tpls])]).astype(np.int64),
                     tpl=np.concatenate(tpls).astype(np.uint8))


# the planted layouts of tests/test_coverage.py on a template t, eight passes each: name -> passes
def layouts(rng, L=600, both=False):
    t = rnd(rng, L)
    at = L // 2 + 7
    b300, b60, b35 = rnd(rng, 300), rnd(rng, 60), rnd(rng, 35)
    return t, at, {
        "clean": clean(t, 8, both),
        "block300_2of8": blocked(t, b300, at, {5, 6}, 8, both),
        "block300_last4": blocked(t, b300, at, {4, 5, 6, 7}, 8, both),
        "block300_alternating": blocked(t, b300, at, {1, 3, 5, 7}, 8, both),
        "block60_4of8": blocked(t, b60, at, {4, 5, 6, 7}, 8, both),
        "block35_4of8": blocked(t, b35, at, {4, 5, 6, 7}, 8, both),
        "block300_first5": blocked(t, b300, at, {0, 1, 2, 3, 4}, 8, both),
        "partials": with_partials(t, 6, (0.6, 0.5), both),
    }

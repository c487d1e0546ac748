"""The planted batches of tests/test_kinetics_gpu.py (engine against tests/kinetics_ref.py) and the `rq` tolerance measured on them with the oracle
(tests/test_kinetics_ref.py::test_rq_deviation_on_the_gpu_batches).  Everything here runs without a GPU: tools/coverage_synth.py makes the passes, the oracle's
window rule (a function of the draft alone) places the plants in the middle of a window."""
from __future__ import annotations

import numpy as np

import coverage_synth as S
import lowcx
import oracle_lib as O
from ccs_amd import api

# ---- rq (DESIGN.md §2 "QVs (A6), stitch"): measured by test_rq_deviation_on_the_gpu_batches over the oracle's results for every batch below
RQ_DEV_MEASURED = 1.36e-3         # largest |(1 - rq_oracle) - (1 - rq_ref)| / (1 - rq_ref) seen (1.358e-3), rounded up
MIN_RQ_LOW = 0.9985               # min_rq of the LOW_RQ test: ZMWs of the `low_rq` batch lie on both sides and none within the bound of it


def rq_bound(rq_ref: float) -> float:
    """the largest |rq - rq_ref| allowed: 4 x the measured relative deviation of 1 - rq, plus one float32 ulp of rq"""
    return 4.0 * RQ_DEV_MEASURED * (1.0 - rq_ref) + float(np.spacing(np.float32(rq_ref)))


def kin_opts(**kw):
    o = api.default_opts()
    o.hifi_kinetics = 1
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def whole_range(b, seed):
    """ipd and pw codes over the whole 0..255 range (pw: one base in ten, the others keep the channel's pulse widths: the HMM reads them)"""
    rng = np.random.default_rng(seed)
    n = len(b.bases)
    b.ipd = rng.integers(0, 256, n).astype(np.uint8)
    b.pw = np.where(rng.random(n) < 0.9, b.pw, rng.integers(0, 256, n)).astype(np.uint8)
    return b


def run_of(t, at, k):
    """k copies of a base that differs from both neighbours of position `at`: the alignments keep such a run as one insertion"""
    return np.full(k, [x for x in range(4) if x not in (int(t[at - 1]), int(t[at]))][0], np.uint8)


def mid_windows(t):
    """the middle of every inner window of template t (the windows its draft gets when the draft is t)"""
    wb = O.windows(t)
    return [int(wb[w] + wb[w + 1]) // 2 for w in range(1, len(wb) - 2)], wb


def runs_zmw(t, ks, n=12, both=True):
    """n passes of t; pass 2 + i carries a run of ks[i] bases in the middle of inner window 1 + i"""
    mids, _ = mid_windows(t)
    z = S.clean(t, n, both)
    for i, k in enumerate(ks):
        at = mids[1 + i]
        z[2 + i] = S.Pass(S.with_block(t, run_of(t, at, k), at), z[2 + i].rev)
    return z


HEAD, TAIL = 30, 32


def ends_template(rng, L=257):
    """a random template whose first 30 and last 32 bases are G and T alone, followed by a C / preceded by an A: a pass that lacks one of the two ends has one
    best alignment (the base next to the gap finds no chance match inside it), so the first / last window keeps no base of that pass"""
    t = S.rnd(rng, L)
    t[:HEAD] = 2 + rng.integers(0, 2, HEAD)
    t[L - TAIL:] = 2 + rng.integers(0, 2, TAIL)
    t[HEAD], t[L - TAIL - 1] = 1, 0
    return t


def emptied_zmw(t, n=12, both=True):
    """n passes of ends_template's t; passes 3 and 4 (one of each strand) lack the head, passes 5 and 6 the tail: a segment of 0 bases in the first / last window"""
    z = S.clean(t, n, both)
    for p in (3, 4):
        z[p] = S.Pass(t[HEAD:], z[p].rev)
    for p in (5, 6):
        z[p] = S.Pass(t[:len(t) - TAIL], z[p].rev)
    return z


def segment_limits(seed=101):
    """segments of 31, 32, 63, 64 and more bases, of 0 bases, a 70-base block: runs of k bases, k swept around J + k = 31.5 and 63.5 for windows of 24 to 29
    columns, through a quiet channel (ZMWs 0-3) and the usual one (ZMWs 4-7)"""
    parts = []
    for channel, sd in ((0.1, seed), (1.0, seed + 1)):
        rng = np.random.default_rng(sd)
        t = [S.rnd(rng, 300), S.rnd(rng, 300), ends_template(rng), S.rnd(rng, 300)]
        zs = [runs_zmw(t[0], range(3, 11)), runs_zmw(t[1], range(34, 43)), emptied_zmw(t[2]), runs_zmw(t[3], (5, 37, 6, 38, 4, 36, 7, 39))]
        zs[2][9] = S.Pass(S.with_block(t[2], S.rnd(rng, 70), 100), zs[2][9].rev)
        parts.append(S.batch(zs, rng, channel))
    return whole_range(api.concat(parts), seed)


def groups70(seed=111):
    """70 passes of 120 bases on both strands: three groups of 32 + 32 + 6 under top_passes 0"""
    rng = np.random.default_rng(seed)
    return whole_range(S.batch([S.clean(S.rnd(rng, 120), 70, True)], rng), seed)


def groups255(seed=112):
    """255 passes of 100 bases on one strand through a fiftieth of the channel's errors (about half of the columns see all 255 passes agree), every ipd and
    pw code 255"""
    rng = np.random.default_rng(seed)
    b = S.batch([S.clean(S.rnd(rng, 100), 255, False)], rng, 0.02)
    b.ipd = np.full(len(b.bases), 255, np.uint8)
    b.pw = np.full(len(b.bases), 255, np.uint8)
    return b


def strand_reference(seed=121):
    """ZMW 0: pass 0 on the reverse strand.  ZMWs 1, 2: pass 0 is random sequence, a third longer than the others (never the pass closest to the median
    length): the fallback draft takes another backbone — in ZMW 1 every other pass is on the reverse strand, in ZMW 2 the strands alternate.  ZMW 3: eight full
    passes and two partial ones.  ZMW 4: three unrelated passes (no consensus).  ZMW 5: a 60-base template.  ZMW 6: ten passes, two of them through three
    times the channel's errors: they align, and most windows' gates drop one (np, the mode over windows, is below fn + rn)"""
    rng = np.random.default_rng(seed)
    t = [S.rnd(rng, n) for n in (201, 180, 230, 420, 200, 60)]
    z0 = [S.Pass(t[0], not (q & 1)) for q in range(9)]
    z1 = [S.Pass(S.rnd(rng, 240), False)] + [S.Pass(t[1], True) for _ in range(9)]
    z2 = [S.Pass(S.rnd(rng, 306), True)] + S.clean(t[2], 10, True)
    z3 = S.with_partials(t[3], 8, (0.6, 0.5), True)
    bad = [S.Pass(S.rnd(rng, 200), False) for _ in range(3)]
    rng6 = np.random.default_rng(5)
    t6 = S.rnd(rng6, 240)
    z6 = S.clean(t6, 10, True)
    for p in (3, 6):
        z6[p] = S.Pass(lowcx.sequence_read(rng6, t6, 3.0)[0], z6[p].rev)
    return whole_range(api.concat([S.batch([z0, z1, z2, z3, bad, S.clean(t[5], 7, True)], rng), S.batch([z6], rng6)]), seed)


def many_windows(seed=131):
    """templates whose window rule gives 63 .. 66 windows and one of 80, five passes each through a quiet channel (the draft is the template, nearly always)"""
    rng = np.random.default_rng(seed)
    zs, want = [], []
    for nw in (63, 64, 65, 66, 64, 65, 80):
        L = 22 * nw
        while True:
            t = S.rnd(rng, L)
            got = len(O.windows(t)) - 1
            if got == nw:
                break
            L += 11 * (nw - got)
        zs.append(S.clean(t, 5, True)); want.append(nw)
    return whole_range(S.batch(zs, rng, 0.1), seed), want


def low_rq(seed=141):
    """ZMWs of 3 .. 14 passes: predicted accuracies on both sides of MIN_RQ_LOW"""
    rng = np.random.default_rng(seed)
    return whole_range(S.batch([S.clean(S.rnd(rng, 250), n, True) for n in (3, 3, 4, 4, 5, 6, 8, 10, 12, 14)], rng), seed)


BATCHES = {"segment_limits": segment_limits, "groups70": groups70, "groups255": groups255, "strand_reference": strand_reference,
           "many_windows": lambda: many_windows()[0], "low_rq": low_rq}
OPTS = {"groups70": dict(top_passes=0), "groups255": dict(top_passes=0)}     # what the GPU tests run each batch under, beside hifi_kinetics


def result_bytes(res) -> bytes:
    """every result of a run, the written part of each per-base array"""
    out = [res.status, res.seq_len, res.rq, res.np_, res.ec, res.iters, res.n_windows, res.fn, res.rn]
    for z in range(len(res.status)):
        out += [res.sequence(z), res.quals(z), res.raw(z), res.kinetics(z)]
    return b"".join(np.ascontiguousarray(a).tobytes() for a in out)

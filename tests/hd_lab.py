"""The planted batches of tests/test_hd_plain.py (oracle stages) and tests/test_hd_limits_gpu.py (engine stages): each drives the heteroduplex finder (DESIGN.md §2
"Heteroduplex rule") to one limit of its kernels.  Everything here runs without a GPU.  Passes are clean copies of edited templates (tools/coverage_synth.py through
a channel of 0), except in `noisy_small`; the test supplies the draft (the template), so the windows are the window rule's on the template and every plant sits where
its batch says."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import coverage_synth as S
import hd_ref
import oracle_lib as O
from ccs_amd import api
from kinetics_lab import ends_template, run_of

MAX_PASSES, RESCUE_MIN_EXCESS = 255, 24
UNTESTED, DOUBLE_STRAND, HETERODUPLEX = 0, 1, 2
DEFAULTS = dict(min_strand_passes=3, min_sites=1, min_indel=21, min_alt_frac=0.5, max_pvalue=1e-3)
EVERY_CANDIDATE = dict(max_pvalue=1.0, min_alt_frac=0.0, min_strand_passes=1)        # every column with an alt is a site and reports its p


@dataclass
class Lab:
    batch: api.Batch
    drafts: list                      # per ZMW (draft, backbone pass)
    opt_sets: list                    # the option sets the batch runs under: dicts over DEFAULTS
    top_passes: int = 60              # the engine option the batch needs (0: all passes, at most 255)


def ref_opts(kw) -> hd_ref.Opts:
    return hd_ref.Opts(**{**DEFAULTS, **kw})


def hd_opts(kw) -> api.HdOpts:
    o = api.HdOpts()
    for k, v in {**DEFAULTS, **kw}.items():
        setattr(o, k, v)
    return o


def engine_opts(lab: Lab):
    o = api.default_opts()
    o.top_passes = lab.top_passes
    return o


def drafts_of(lab: Lab) -> api.Drafts:
    d = api.Drafts.allocate(lab.batch)
    for z, (t, bb) in enumerate(lab.drafts):
        d.set_draft(z, t, backbone=bb)
    return d


def used_records(zmws):
    """the records with the passes a ZMW uses (the first 255): what both CPU references are given"""
    return [hd_ref.Zmw(Z.draft, Z.wb, Z.status, Z.backbone, Z.reads[:MAX_PASSES]) for Z in zmws]


def oracle_stage(lab: Lab):
    """the stages of the polish seam on the supplied drafts, from the oracle (step 3 of orc_consensus_zmw with a given draft): per ZMW an hd_ref.Zmw whose reads hold
    every pass given (the unused ones not valid)"""
    b, out = lab.batch, []
    top = MAX_PASSES if lab.top_passes <= 0 or lab.top_passes > MAX_PASSES else lab.top_passes
    for z, (d, bb) in enumerate(lab.drafts):
        r0, r1 = int(b.read_off[z]), int(b.read_off[z + 1])
        n = min(r1 - r0, top)
        fl = [int(f) for f in b.flags[r0:r1]]
        nfull = next((q for q in range(n) if fl[q] & 2), n)
        wb = O.windows(d)
        cols = hd_ref.need_cols(wb, len(d))
        need = np.array(cols, np.int32)
        reads, npass = [], 0
        for q in range(r1 - r0):
            bases = b.read(r0 + q)[0]
            v, rs = 0, np.full(len(d) + 1, -1, np.int32)
            if q < n and nfull >= 3:
                st = (fl[q] & 1) ^ (fl[bb] & 1)
                ob = O.orient(bases, st)
                if q >= nfull:
                    if len(need) >= 2:
                        rs, v, _, _ = O.align_partial(ob, d, need, ((fl[q] >> 2) & 1) ^ st)
                else:
                    rs, v, _, _ = O.align_ev_w(ob, d, need, 0)
                    if not v and len(ob) - len(d) > RESCUE_MIN_EXCESS and len(need) >= 3:
                        rs, v, _, _ = O.align_rescue(ob, d, need)
                    npass += int(v)
            reads.append((bases, fl[q], bool(v), np.array([rs[c] for c in cols], np.int64)))
        status = 1 if nfull < 3 else 3 if 2 * npass <= nfull else 0
        out.append(hd_ref.Zmw(np.asarray(d, np.uint8), wb, status, bb, reads))
    return out


# ---------------------------------------------------------------- building blocks
def alternating(n):
    return [bool(q & 1) for q in range(n)]


def template(rng, nw, last=24):
    """a random template that the window rule cuts into nw windows, the last core `last` columns wide -> (template, bounds)"""
    for _ in range(2000):
        t = S.rnd(rng, 25 * nw + 40)
        wb = O.windows(t)
        if len(wb) - 1 < nw:
            continue
        t = t[: int(wb[nw - 1]) + last] if nw > 1 else t[:last]
        wb = O.windows(t)
        if len(wb) - 1 == nw and int(wb[-1] - wb[-2]) == last:
            return t, [int(x) for x in wb]
    raise RuntimeError("no template")


def alt_of(t, col, step=1):
    return (int(t[col]) + step) & 3


def edited(t, edits):
    """the template with ("sub", column, base), ("ins", column, block: inserted before the column) and ("del", column, k columns from it) applied"""
    out = np.array(t, np.uint8)
    for kind, col, x in sorted(edits, key=lambda e: -e[1]):
        if kind == "sub":
            out[col] = x
        elif kind == "ins":
            out = np.concatenate([out[:col], np.asarray(x, np.uint8), out[col:]])
        else:
            out = np.concatenate([out[:col], out[col + x:]])
    return out.astype(np.uint8)


def zmw(t, strands, plan=None, rev_all=(), fwd_all=()):
    """one pass per entry of `strands` (True: reverse), each the template with the edits of its strand and of plan[pass]"""
    plan = plan or {}
    return [S.Pass(edited(t, list(plan.get(q, [])) + list(rev_all if rev else fwd_all)), rev) for q, rev in enumerate(strands)]


def insertion(rng, t, wb, at, k):
    """("ins", at, block): a run of one base up to 20 bases; beyond that (the alignment takes at most 20 rows in one column and spreads or loses longer
    runs) a random block that the oracle's alignment keeps whole: every window edge behind it lies k rows further, every other one where it was"""
    if k <= 20:
        return ("ins", at, run_of(t, at, k))
    cols = hd_ref.need_cols(np.asarray(wb), len(t))
    need = np.array(cols, np.int32)
    for _ in range(500):
        block = S.rnd(rng, k)
        rs, v, _, _ = O.align_ev_w(edited(t, [("ins", at, block)]), t, need, 0)
        if v and {int(rs[c]) - c for c in cols} <= {0, k} and int(rs[cols[-1]]) - cols[-1] == k:
            return ("ins", at, block)
    raise RuntimeError("no insertion that the alignment keeps whole")


def deletion(t, wb, w, k):
    """("del", start, k) inside window w, behind its first core column, where the oracle's alignment leaves the window's two edges where the plant puts them
    (a deletion next to a chance match slides): the start nearest to the window's middle"""
    cols = hd_ref.need_cols(np.asarray(wb), len(t))
    need = np.array(cols, np.int32)
    a, b = max(wb[w] - 2, 0), min(wb[w + 1] + 2, len(t))
    for start in sorted(range(wb[w] + 1, b - k + 1), key=lambda c: abs(2 * c + k - a - b)):
        rs, v, _, _ = O.align_ev_w(edited(t, [("del", start, k)]), t, need, 0)
        if v and int(rs[a]) == a and int(rs[b]) == b - k:
            return ("del", start, k)
    raise RuntimeError("no deletion that the alignment keeps in the window")


def mid(wb, w):
    return (wb[w] + wb[w + 1]) // 2


def make(zs, drafts, rng, opt_sets, channel=0.0, **kw) -> Lab:
    return Lab(S.batch(zs, rng, channel), [(np.asarray(t, np.uint8), bb) for t, bb in drafts], opt_sets, **kw)


def subs_rev(t, cols):
    return [("sub", c, alt_of(t, c)) for c in cols]


# ---------------------------------------------------------------- the batches
def segment_rows(seed=201):
    """8 + 8 passes.  ZMWs 0, 2 (template of 3 windows, bounds 0 22 44 72: the last window has J = 30 columns): seven passes of one strand (reverse in ZMW 0,
    forward in ZMW 2) carry a run of 1, 2, 3, 4, 18, 19, 20 bases in the middle of the last window: segments of 31, 32, 33, 34, 48, 49 and 50 rows (the two
    64-bit words of k_hd_pile switch at row 32 / 33; 50 rows are left out).  ZMWs 1, 3 (13 windows): windows 1 .. 10 carry, in one pass each, a run of 1, 9, 10,
    20, 21 bases or a deletion of 1, 9, 10, 20, 21: |n - J| of min_indel - 1 and min_indel at min_indel 21, 10 and 1, both signs.  ZMW 4: ends_template with a
    last core of at most 12 columns; passes 3, 4 lack the head and 5, 6 the tail: segments of 0 rows, which the last window (J < 21) counts as deletions.  Every
    planted window has a substitution on all reverse passes away from the plant: the site's rev_n / fwd_n tells whether the planted pass was counted
    (max_pvalue 0.01, so that 7 of 8 against 0 of 8, p = 1.4e-3, is still a site)."""
    rng = np.random.default_rng(seed)
    st = alternating(16)
    zs, drafts = [], []
    for rev in (True, False):
        carriers = [q for q in range(16) if st[q] == rev][1:]
        t, wb = template(rng, 3, last=28)
        at = mid(wb, 2)
        plan = {q: [("ins", at, run_of(t, at, k))] for q, k in zip(carriers, (1, 2, 3, 4, 18, 19, 20))}
        zs.append(zmw(t, st, plan, rev_all=subs_rev(t, [wb[2] + 3]))); drafts.append((t, 0))
        while True:
            t, wb = template(rng, 13, last=28)
            plan, sub_cols = {}, []
            try:
                for i, (kind, k) in enumerate([("ins", 1), ("ins", 9), ("ins", 10), ("ins", 20), ("ins", 21), ("del", 1), ("del", 9), ("del", 10), ("del", 20), ("del", 21)]):
                    w, q = 1 + i, carriers[i % 7]
                    e = insertion(rng, t, wb, mid(wb, w), k) if kind == "ins" else deletion(t, wb, w, k)
                    plan.setdefault(q, []).append(e)
                    sub_cols.append(wb[w] + 2 if kind == "ins" or e[1] > wb[w] + 2 else wb[w])
                break
            except RuntimeError:
                continue
        zs.append(zmw(t, st, plan, rev_all=subs_rev(t, sub_cols))); drafts.append((t, 0))
    while True:
        t = ends_template(rng, int(rng.integers(250, 300)))
        wb = [int(x) for x in O.windows(t)]
        if wb[-1] - wb[-2] <= 12:
            break
    z = zmw(t, st, rev_all=[("sub", len(t) - 3, 0), ("sub", 5, 0)])
    for p in (3, 4):
        z[p] = S.Pass(z[p].tpl[30:], z[p].rev)
    for p in (5, 6):
        z[p] = S.Pass(z[p].tpl[: len(t) - 32], z[p].rev)
    zs.append(z); drafts.append((t, 0))
    return make(zs, drafts, rng, [dict(max_pvalue=0.01, min_indel=m) for m in (21, 10, 1)])


def strand_totals(seed=202):
    """top_passes 0.  ZMW 0: 252 forward + 3 reverse passes of a 110-base template; ZMW 1: 254 + 1; ZMW 2: 300 passes, the first 255 as in ZMW 0 and 45 more
    reverse passes that carry the alt at a further column (255 are used: that column is no site).  Three columns of each ZMW carry the alt on every reverse
    pass: the forward counts of the draft base, one byte of a 32-bit word in k_hd_pile, reach 252 and 254."""
    rng = np.random.default_rng(seed)
    zs, drafts = [], []
    for nf, nr, extra in ((252, 3, 0), (254, 1, 0), (252, 3, 45)):
        t, wb = template(rng, 5, last=22)
        cols = [mid(wb, 0), mid(wb, 2), mid(wb, 4)]
        z = zmw(t, [False] * nf + [True] * nr, rev_all=subs_rev(t, cols))
        z += [S.Pass(edited(t, subs_rev(t, cols + [mid(wb, 1)])), True) for _ in range(extra)]
        zs.append(z); drafts.append((t, 0))
    sets = [dict(min_strand_passes=m, max_pvalue=p) for m in (3, 1) for p in (1e-3, 0.01)]
    return make(zs, drafts, rng, sets, top_passes=0)


def pass_groups(seed=203):
    """top_passes 0.  ZMW 0: 255 passes, alternating strands; a 25-base insertion only on the reverse passes with index >= 192 (the fourth group of 64 of
    k_hd_indel) and a 25-base deletion elsewhere only on the reverse passes 64 .. 127 (the second).  ZMW 1: 64 passes, the insertion on the reverse passes from
    41 on; ZMW 2: 65 passes, pass 64 (the second group's only pass) is a reverse pass and carries it too."""
    rng = np.random.default_rng(seed)
    zs, drafts = [], []
    t, wb = template(rng, 10, last=24)
    a, d = mid(wb, 2), mid(wb, 6)
    ins = insertion(rng, t, wb, a, 25)
    plan = {q: [ins] for q in range(192, 255) if q & 1}
    plan.update({q: [("del", d, 25)] for q in range(64, 128) if q & 1})
    zs.append(zmw(t, alternating(255), plan)); drafts.append((t, 0))
    for n in (64, 65):
        t, wb = template(rng, 6, last=24)
        st = alternating(64) + [True] * (n - 64)
        a = mid(wb, 3)
        ins = insertion(rng, t, wb, a, 25)
        zs.append(zmw(t, st, {q: [ins] for q in range(41, n) if st[q]})); drafts.append((t, 0))
    return make(zs, drafts, rng, [dict()], top_passes=0)


def _pairs(rng, nf, nr, want, first):
    """(j, k) = alt on j forward and k reverse passes: `first`, then random further pairs, `want` in all, none twice"""
    seen = list(dict.fromkeys(first))
    while len(seen) < want:
        p = (int(rng.integers(0, nf + 1)), int(rng.integers(0, nr + 1)))
        if p not in seen and p != (0, 0):
            seen.append(p)
    return seen[:want]


def fisher_tables(seed=204):
    """top_passes 0.  16 ZMWs of 20 + 20 passes, 8 of 13 + 27, 4 of 100 + 155 (forward passes first); templates of 5 windows; 16 planted columns per ZMW, at most 4
    per window, so every site is listed.  Column by column the alt is carried by the first j forward and the first k reverse passes: every (0, k) and (k, 0) of
    20 + 20 and 13 + 27, a ladder of them at 100 + 155 (p from 1 / C(255, 100) to 1), and random pairs.  At 20 + 20 every table with j != k has a mirror image of
    exactly equal probability, which only the (1 + 1e-7) of the tie rule keeps in the sum."""
    rng = np.random.default_rng(seed)
    zs, drafts = [], []
    ladder = (1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 99, 100, 120, 154, 155)
    groups = ((16, 20, 20, [(0, k) for k in range(1, 21)] + [(k, 0) for k in range(1, 21)] + [(20, 20), (10, 10), (19, 20), (20, 19), (1, 2), (2, 1)]),
              (8, 13, 27, [(0, k) for k in range(1, 28)] + [(k, 0) for k in range(1, 14)] + [(13, 27), (6, 13), (13, 26)]),
              (4, 100, 155, [(0, k) for k in ladder] + [(k, 0) for k in ladder if k <= 100] + [(100, 155), (50, 77), (100, 154), (99, 155)]))
    for nz, nf, nr, first in groups:
        pairs = _pairs(rng, nf, nr, 16 * nz, first)
        for zi in range(nz):
            t, wb = template(rng, 5, last=24)
            cols = [wb[w] + 2 + 5 * i for w in range(4) for i in range(4)]
            plan = {}
            for c, (j, k) in zip(cols, pairs[16 * zi: 16 * zi + 16]):
                for q in list(range(j)) + list(range(nf, nf + k)):
                    plan.setdefault(q, []).append(("sub", c, alt_of(t, c)))
            zs.append(zmw(t, [False] * nf + [True] * nr, plan)); drafts.append((t, 0))
    return make(zs, drafts, rng, [dict(EVERY_CANDIDATE), dict()], top_passes=0)


def option_edges(seed=205):
    """Small ZMWs, one rule clause each (the alt on every reverse pass unless said otherwise):
    0: 3 + 2 passes; 1: 2 + 3; 2: 3 + 3, the alt on two reverse passes; 3: 3 + 2 and a partial reverse pass over the planted column, the alt on it and on one full reverse pass (the column
    has n_r = 3, k_post's rn is 2); 4: 10 + 10 with columns of 5, 4 and 3 of the 10 reverse passes; 5: the same on the forward strand; 6: 12 + 12 with 3 of 12; 7: two alts,
    three reverse passes each (the lower code wins); 8: every pass of both strands reads the alt; 9: a one-base deletion on every reverse pass (counted, no site);
    10, 11, 12: exactly 1, 2, 3 sites; 13: the backbone is a reverse pass and the draft the reverse complement; 14: three unrelated passes (not SUCCESS);
    15: one window of 26 columns."""
    rng = np.random.default_rng(seed)
    zs, drafts = [], []

    def add(z, t, bb=0):
        zs.append(z); drafts.append((t, bb))

    for nf, nr in ((3, 2), (2, 3)):
        t, wb = template(rng, 2)
        add(zmw(t, [False] * nf + [True] * nr, rev_all=subs_rev(t, [mid(wb, 0)])), t)
    t, wb = template(rng, 3)
    c = mid(wb, 1)
    add(zmw(t, [False] * 3 + [True] * 3, {3: subs_rev(t, [c]), 4: subs_rev(t, [c])}), t)
    t, wb = template(rng, 3)
    c = mid(wb, 0)
    z = zmw(t, [False] * 3 + [True] * 2, {4: subs_rev(t, [c])})
    add(z + [S.Pass(edited(t, subs_rev(t, [c]))[: wb[2]], True, "head")], t)
    for rev in (True, False):
        t, wb = template(rng, 3)
        st = alternating(20)
        mine = [q for q in range(20) if st[q] == rev]
        plan = {}
        for w, k in enumerate((5, 4, 3)):
            for q in mine[:k]:
                plan.setdefault(q, []).append(("sub", mid(wb, w), alt_of(t, mid(wb, w))))
        add(zmw(t, st, plan), t)
    t, wb = template(rng, 2)
    add(zmw(t, alternating(24), {q: subs_rev(t, [mid(wb, 1)]) for q in (1, 3, 5)}), t)
    t, wb = template(rng, 2)
    c = mid(wb, 0)
    lo, hi = sorted(b for b in range(4) if b != int(t[c]))[:2]
    add(zmw(t, alternating(20), {**{q: [("sub", c, hi)] for q in (1, 3, 5)}, **{q: [("sub", c, lo)] for q in (7, 9, 11)}}), t)
    t, wb = template(rng, 2)
    e = subs_rev(t, [mid(wb, 1)])
    add(zmw(t, alternating(20), rev_all=e, fwd_all=e), t)
    t, wb = template(rng, 2)
    add(zmw(t, alternating(20), rev_all=[("del", mid(wb, 0), 1)]), t)
    for k in (1, 2, 3):
        t, wb = template(rng, 3)
        add(zmw(t, alternating(20), rev_all=subs_rev(t, [mid(wb, w) for w in range(k)])), t)
    t, wb = template(rng, 3)
    z = zmw(t, alternating(20), rev_all=subs_rev(t, [mid(wb, 1)]))
    add(z, S.rc(t), 1)
    add([S.Pass(S.rnd(rng, 70), bool(q & 1)) for q in range(3)], S.rnd(rng, 70))
    t, wb = template(rng, 1, last=26)
    add(zmw(t, alternating(20), rev_all=subs_rev(t, [13])), t)
    every = dict(max_pvalue=1.0, min_strand_passes=3)
    sets = [dict(), dict(every), dict(every, min_alt_frac=0.3), dict(every, min_alt_frac=0.25), dict(min_sites=2), dict(min_sites=3), dict(max_pvalue=0.0),
            dict(max_pvalue=0.1), dict(max_pvalue=1.0, min_strand_passes=2), dict(max_pvalue=1.0, min_strand_passes=1)]
    return make(zs, drafts, rng, sets)


def site_lists(seed=206):
    """7 + 7 passes (16 + 16 where said); substitutions on every reverse pass.
    0: windows with 9, 10 and 26 sites (the last core, every column), 45 in all; 1: 17 sites over three windows; 2: 132 windows, 22 sites in windows 60 .. 70 (the list
    of k_hd_verdict fills across its 64-window rounds); 3: 134 windows, sites only in windows 129 and 131; 4: a 25-base insertion on every reverse pass and a
    substitution on the first core column of the first window of its cluster (equal column: kind 0 before 1); 5 (8 + 8): a 25-base insertion on the reverse and a
    25-base deletion on the forward passes whose clusters start at the same window (kind 1 before 2); 6: 94 windows, a one-base insertion on every reverse pass in
    the middle of every fifth window: at min_indel 1, 18 indel sites of which 16 are listed."""
    rng = np.random.default_rng(seed)
    zs, drafts = [], []
    st = alternating(14)
    while True:                                        # the last core reads A / C on the draft and G / T on the reverse passes: no base to match out of place
        t, wb = template(rng, 8, last=26)
        t[wb[7]:] = rng.integers(0, 2, 26)
        if [int(x) for x in O.windows(t)] == wb:
            break
    cols = [wb[1] + 2 * i for i in range(9)] + [wb[3] + 2 * i for i in range(10)]
    every = [("sub", c, 2 + int(rng.integers(0, 2))) for c in range(wb[7], wb[8])]
    zs.append(zmw(t, st, rev_all=[("sub", c, alt_of(t, c, 2)) for c in cols] + every)); drafts.append((t, 0))
    t, wb = template(rng, 6)
    cols = [wb[w] + 1 + 3 * i for w, k in ((1, 6), (2, 6), (4, 5)) for i in range(k)]
    zs.append(zmw(t, st, rev_all=subs_rev(t, cols))); drafts.append((t, 0))
    t, wb = template(rng, 132)
    cols = [wb[w] + o for w in range(60, 71) for o in (4, 14)]
    zs.append(zmw(t, st, rev_all=subs_rev(t, cols))); drafts.append((t, 0))
    t, wb = template(rng, 134)
    zs.append(zmw(t, st, rev_all=subs_rev(t, [mid(wb, 129), mid(wb, 131), mid(wb, 131) + 4]))); drafts.append((t, 0))
    t, wb = template(rng, 9)
    zs.append(zmw(t, st, rev_all=[insertion(rng, t, wb, mid(wb, 5), 25), ("sub", wb[3], alt_of(t, wb[3]))])); drafts.append((t, 0))
    t, wb = template(rng, 9)
    zs.append(zmw(t, alternating(16), rev_all=[insertion(rng, t, wb, mid(wb, 5), 25)], fwd_all=[("del", wb[5] + 1, 25)])); drafts.append((t, 0))
    t, wb = template(rng, 94)
    zs.append(zmw(t, st, rev_all=[("ins", mid(wb, w), run_of(t, mid(wb, w), 1)) for w in range(4, 94, 5)])); drafts.append((t, 0))
    return make(zs, drafts, rng, [dict(), dict(min_indel=1)])


def indel_spans(seed=207):
    """8 + 8 passes, min_indel 21, events on every reverse pass.  0 .. 3: an insertion of 20, of 21, a deletion of 20, of 21 bases in the middle of window 3 of 8;
    4: a 21-base insertion at a core bound (inside the 4-column overlap of two overhangs: one cluster); 5: a 30-base deletion over two windows that no single
    window sees; 6: an insertion in the first window; 7, 8, 9: one in the last, the last but one, the last but two (the spans stop at the last window);
    10: a one-window ZMW with a 10-base insertion (the alignment's score gate takes no longer one on 26 columns): an event in the second option set, min_indel 10; 11: as 1, with three partial passes: a reverse one that starts inside the cluster's first window (it has the event in the
    later ones: counted), a forward one that ends inside the cluster (not counted) and a forward one that covers it (counted without the event)."""
    rng = np.random.default_rng(seed)
    zs, drafts = [], []
    st = alternating(16)

    def add(t, edits, extra=()):
        zs.append(zmw(t, st, rev_all=edits) + list(extra)); drafts.append((t, 0))

    for kind, k in (("ins", 20), ("ins", 21), ("del", 20), ("del", 21)):
        t, wb = template(rng, 8)
        add(t, [insertion(rng, t, wb, mid(wb, 3), k)] if kind == "ins" else [("del", mid(wb, 3) - 10, k)])
    t, wb = template(rng, 6)
    add(t, [insertion(rng, t, wb, wb[2], 21)])
    t, wb = template(rng, 6)
    add(t, [("del", mid(wb, 1) - 3, 30)])
    t, wb = template(rng, 6)
    add(t, [insertion(rng, t, wb, mid(wb, 0), 25)])
    for back in (1, 2, 3):
        t, wb = template(rng, 7)
        add(t, [insertion(rng, t, wb, mid(wb, 7 - back), 25)])
    t, wb = template(rng, 1, last=26)
    add(t, [insertion(rng, t, wb, 13, 10)])
    t, wb = template(rng, 8)
    m = mid(wb, 3)
    ins = insertion(rng, t, wb, m, 21)
    e = edited(t, [ins])
    add(t, [ins],
        [S.Pass(e[wb[1] + 8:], True, "tail"), S.Pass(t[: wb[2] + 8], False, "head"), S.Pass(t[: wb[5] + 8], False, "head")])
    return make(zs, drafts, rng, [dict(), dict(min_indel=10)])


def noisy_small(seed=208):
    """64 ZMWs of 12 passes of 60 .. 100 bases through the usual channel, the draft being the template: run at the defaults, and with every candidate a site, where
    n_sub_sites and the first 16 records expose the pileup counts of nearly every column"""
    rng = np.random.default_rng(seed)
    ts = [S.rnd(rng, int(rng.integers(60, 101))) for _ in range(64)]
    return make([S.clean(t, 12, True) for t in ts], [(t, 0) for t in ts], rng, [dict(), dict(EVERY_CANDIDATE)], channel=1.0)


BATCHES = {"segment_rows": segment_rows, "strand_totals": strand_totals, "pass_groups": pass_groups, "fisher_tables": fisher_tables,
           "option_edges": option_edges, "site_lists": site_lists, "indel_spans": indel_spans, "noisy_small": noisy_small}


# ---------------------------------------------------------------- what each batch must reach, read from the census of tests/hd_plain.py (cens[option set][zmw])
def _excess(cens, reason):
    return {n - J for c in cens for (_, _, n, J, why) in c["segments"] if why == reason}


def check_census(name, lab: Lab, cens, reps):
    """the limit the batch is named for, from the censuses and reports of hd_plain over `lab.opt_sets` on some stage outputs (the oracle's or the engine's);
    every pass valid, every ZMW SUCCESS except the one meant not to be, and no borderline case in a planted batch"""
    for c in cens[0]:
        ok = name == "option_edges" and c is cens[0][14]
        assert (c["status"] != 0) == ok and (ok or all(c["valid"])), (name, c["status"], c["valid"])
    if name != "noisy_small":
        assert not any(c["borderline_p"] or c["near_tie"] for cs in cens for c in cs), name
    c0, r0 = cens[0], reps[0]
    if name == "segment_rows":
        for z in (0, 2):
            rows = {n: why for (w, _, n, J, why) in c0[z]["segments"] if w == 2 and J == 30}
            assert rows == {30: "counted", 31: "counted", 32: "counted", 33: "counted", 34: "counted", 48: "counted", 49: "counted", 50: "rows"}, rows
            s = r0[z]["sites"][0]
            assert (s["rev_n"], s["fwd_n"]) == ((7, 8) if z == 0 else (8, 7)), s           # seven of the eight planted-strand passes were counted
        assert any(n == 0 and why == "counted" for (_, _, n, J, why) in c0[4]["segments"])
        for cs, kw in zip(cens, lab.opt_sets):
            mi = kw["min_indel"]
            assert {mi - 1, 1 - mi} <= _excess(cs, "counted") and {mi, -mi} <= _excess(cs, "indel"), mi
    elif name == "strand_totals":
        assert [c["max_count"] for c in c0] == [252, 254, 252]
        assert (c0[2]["passes_given"], c0[2]["passes_used"]) == (300, 255) and [r["n_sub"] for r in r0] == [3, 0, 3]
        assert [r["n_sub"] for r in reps[3]] == [3, 3, 3]                                   # min_strand_passes 1, max_pvalue 0.01: 1 of 1 against 0 of 254
    elif name == "pass_groups":
        assert [c["passes_used"] for c in c0] == [255, 64, 65]
        assert sorted((k, g) for (k, _, g) in c0[0]["clusters"]) == [(1, (3,)), (2, (1,))]
        assert [g for (_, _, g) in c0[1]["clusters"]] == [(0,)] and [g for (_, _, g) in c0[2]["clusters"]] == [(0, 1)]
        assert [r["n_indel"] for r in r0] == [2, 1, 1]
    elif name == "fisher_tables":
        ps = [s["p"] for r in r0 for s in r["sites"]]
        assert all(r["n_sub"] == len(r["sites"]) for r in r0) and len(ps) >= 16 * 28 - 1 and min(ps) < 1e-60 and max(ps) == 1.0
        assert max(c["max_count"] for c in c0) == 155
    elif name == "option_edges":
        every, f03, f025, ms2, ms3, p0, p01, msp2, msp1 = reps[1:]
        assert [r["verdict"] for r in r0[:4]] == [UNTESTED, UNTESTED, DOUBLE_STRAND, UNTESTED]
        assert every[3]["sites"][0]["rev_n"] == 3 and every[3]["verdict"] == HETERODUPLEX   # the partial pass counts in the column, not in rn
        assert [r["n_sub"] for r in (every[4], f03[4], f025[4], every[5], f03[5], f025[5], f03[6], f025[6])] == [1, 2, 3, 1, 2, 3, 0, 1]
        assert f025[7]["sites"][0]["alt"] == min(b for b in range(4) if b != int(lab.drafts[7][0][f025[7]["sites"][0]["column"]]))
        assert (every[8]["n_sub"], every[8]["sites"][0]["p"], r0[8]["n_sub"]) == (1, 1.0, 0) and all(r[9]["n_sub"] == 0 for r in reps)
        assert [[r[z]["verdict"] for z in (10, 11, 12)] for r in (r0, ms2, ms3)] == [[2, 2, 2], [1, 2, 2], [1, 1, 2]]
        assert all(r["n_sub"] == 0 for r in p0) and p01[4]["n_sub"] == 1 and r0[13]["n_sub"] == 1 and r0[15]["n_sub"] == 1
        assert all(r[14] == dict(verdict=UNTESTED, n_sub=0, n_indel=0, sites=[], min_p=1.0) for r in reps)
        assert (msp2[0]["n_sub"], msp2[1]["n_sub"], msp1[0]["n_sub"]) == (1, 1, 1) and every[0]["n_sub"] == 0
    elif name == "site_lists":
        assert sorted(c0[0]["sites_per_window"])[-3:] == [9, 10, 26] and c0[0]["windows_over"] == 3 and r0[0]["n_sub"] == 45 and len(r0[0]["sites"]) == 16
        assert r0[1]["n_sub"] == 17 and sum(1 for k in c0[1]["sites_per_window"] if k) == 3
        for z, lo, hi, k in ((2, 60, 70, 22), (3, 128, 133, 3)):
            spw = c0[z]["sites_per_window"]
            assert len(spw) >= 130 and sum(spw) == k and all(lo <= w <= hi for w, q in enumerate(spw) if q), (z, spw)
        assert [(s["kind"]) for s in r0[4]["sites"]] == [0, 1] and r0[4]["sites"][0]["column"] == r0[4]["sites"][1]["column"]
        assert [(s["kind"]) for s in r0[5]["sites"]] == [1, 2] and r0[5]["sites"][0]["column"] == r0[5]["sites"][1]["column"]
        assert (reps[1][6]["n_indel"], len(reps[1][6]["sites"]), r0[6]["n_indel"]) == (18, 16, 0)
        assert len({len(c["sites_per_window"]) % 16 for c in c0}) > 1 and len({c["passes_used"] for c in c0}) > 1
    elif name == "indel_spans":
        assert [r["n_indel"] for r in r0] == [0, 1, 0, 1, 1, 1, 1, 1, 1, 1, 0, 1] and reps[1][10]["n_indel"] == 1
        assert len(c0[4]["clusters"]) == 1 and len(c0[4]["clusters"][0][1]) > 1             # both windows of the overlap, one cluster
        one = [n - J for (_, _, n, J, _) in c0[5]["segments"]]
        assert min(one) > -21 and r0[5]["sites"][0]["kind"] == 2                            # no single window sees the 30-base deletion
        assert 0 in c0[6]["clusters"][0][1]
        for z, back in ((7, 1), (8, 2), (9, 3)):
            nw = len(c0[z]["sites_per_window"])
            assert max(c0[z]["clusters"][0][1]) == nw - back, (z, c0[z]["clusters"])
        s = r0[11]["sites"][0]
        assert (c0[11]["passes_used"], s["fwd_alt"], s["fwd_n"], s["rev_alt"], s["rev_n"]) == (19, 0, 9, 9, 9), s
    elif name == "noisy_small":
        assert sum(1 for z in range(64) if any(cs[z]["borderline_p"] or cs[z]["near_tie"] for cs in cens)) <= 1
        assert sum(r["n_sub"] for r in reps[1]) > 16 * 64                                   # every column with an alt is a site: more than the lists hold


def differences(got, want, rel=1e-9):
    """the fields in which two lists of reports differ (p and min_p to `rel`, relative): [] when they agree"""
    out = []
    for z, (g, w) in enumerate(zip(got, want)):
        head = lambda r: (r["verdict"], r["n_sub"], r["n_indel"], len(r["sites"]))
        if head(g) != head(w):
            out.append((z, "head", head(g), head(w)))
            continue
        for k, (s, e) in enumerate(zip(g["sites"], w["sites"])):
            if any(s[f] != e[f] for f in ("column", "kind", "alt", "fwd_alt", "fwd_n", "rev_alt", "rev_n")) or abs(s["p"] - e["p"]) > rel * e["p"]:
                out.append((z, k, s, e))
        if abs(g["min_p"] - w["min_p"]) > rel * w["min_p"]:
            out.append((z, "min_p", g["min_p"], w["min_p"]))
    return out

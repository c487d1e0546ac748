"""The heteroduplex rule of DESIGN.md §2 "Heteroduplex rule" (rule version 1) once more, written from the text alone: plain Python loops per ZMW, per window,
per pass; a full integer DP matrix with an explicit trace-back; counts in dicts, clusters as sets of windows, lists by sorted(); the Fisher test in exact
arithmetic (fractions.Fraction, no log-factorial table).  It takes the `hd_ref.Zmw` records that `hd_ref.collect_stage` produces and returns the report dicts of
`hd_ref.hd_zmws` plus a census per ZMW: which limits of the kernels the input reached (tests/test_hd_plain.py, tests/test_hd_limits_gpu.py).  Slow on purpose."""
from __future__ import annotations

from fractions import Fraction
from math import comb

import numpy as np

from hd_ref import Opts, Zmw  # noqa: F401  (the records and the options are shared; nothing of the restatement's logic is)

OVERHANG, MAX_ROWS, WIN_SITES, MAX_SITES, MAX_PASSES = 2, 49, 8, 16, 255
SUCCESS = 0
UNTESTED, DOUBLE_STRAND, HETERODUPLEX = 0, 1, 2
TIE = 1 + Fraction(1, 10 ** 7)                 # the rule's (1 + 1e-7)
NEAR = Fraction(1, 10 ** 6)                    # what the census calls borderline: within 1e-6, relative


def fisher_exact(a: int, nf: int, c: int, nr: int):
    """two-sided Fisher exact test of [[a, nf - a], [c, nr - c]] -> (p as a Fraction, capped at 1; True when some table's probability differs from the
    observed one by at most 1e-6 of it without being equal: rounding could move it across the tie rule).  P(x) = C(nf, x) C(nr, m - x) / C(N, m)."""
    m, N = a + c, nf + nr
    weight = {x: comb(nf, x) * comb(nr, m - x) for x in range(max(0, m - nr), min(nf, m) + 1)}
    obs = weight[a]
    total = sum(w for w in weight.values() if w <= obs * TIE)
    near = any(w != obs and abs(w - obs) <= NEAR * obs for w in weight.values())
    return min(Fraction(total, comb(N, m)), Fraction(1)), near


def edit_walk(seg, tpl):
    """global unit-cost alignment of seg (rows) to tpl (columns); the walk from (n, J) to (0, 0) by the first of diagonal, deletion, insertion that attains the
    cell's minimum -> {template column: read base | 4 (deletion)}"""
    n, J = len(seg), len(tpl)
    D = [[0] * (J + 1) for _ in range(n + 1)]
    for i in range(n + 1):
        D[i][0] = i
    for j in range(J + 1):
        D[0][j] = j
    for i in range(1, n + 1):
        for j in range(1, J + 1):
            D[i][j] = min(D[i - 1][j - 1] + (1 if seg[i - 1] != tpl[j - 1] else 0), D[i][j - 1] + 1, D[i - 1][j] + 1)
    out, i, j = {}, n, J
    while i > 0 or j > 0:
        if i == 0:
            move = "del"
        elif j == 0:
            move = "ins"
        elif D[i][j] == D[i - 1][j - 1] + (1 if seg[i - 1] != tpl[j - 1] else 0):
            move = "diag"
        elif D[i][j] == D[i][j - 1] + 1:
            move = "del"
        else:
            move = "ins"
        if move == "diag":
            out[j - 1] = int(seg[i - 1]); i -= 1; j -= 1
        elif move == "del":
            out[j - 1] = 4; j -= 1
        else:
            i -= 1
    return out


def _window(wb, nw, Ld, w):
    ws, we = max(int(wb[w]) - OVERHANG, 0), min(int(wb[w + 1]) + OVERHANG, Ld)
    return ws, we, (0 if w == 0 else 2 * w - 1), (2 * nw - 1 if w == nw - 1 else 2 * (w + 1))


def _near_threshold(p: Fraction, max_pvalue: float) -> bool:
    if max_pvalue <= 0.0 or max_pvalue >= 1.0:        # p <= 0 and p <= 1 cannot flip: p is a sum of positive terms, capped at 1
        return False
    mp = Fraction(max_pvalue)
    return abs(p - mp) <= NEAR * mp


def hd_zmw(Z: Zmw, o: Opts):
    """the rule for one ZMW -> (report, census)"""
    given = len(Z.reads)
    used = Z.reads[:MAX_PASSES]                        # "every used pass": at most CCSX_MAX_PASSES, the first ones
    census = dict(passes_given=given, passes_used=len(used), valid=[bool(v) for (_, _, v, _) in used], segments=[], max_count=0, sites_per_window=[],
                  windows_over=0, n_sub=0, n_indel=0, clusters=[], borderline_p=0, near_tie=0, status=int(Z.status))
    if Z.status != SUCCESS:
        return dict(verdict=UNTESTED, n_sub=0, n_indel=0, sites=[], min_p=1.0), census
    draft, wb = [int(x) for x in Z.draft], [int(x) for x in Z.wb]
    nw, Ld = len(wb) - 1, len(draft)
    f0 = int(used[Z.backbone][1]) & 1
    frac = float(np.float32(o.min_alt_frac))
    max_p = Fraction(o.max_pvalue)
    passes = []                                        # (index, bases in draft orientation, strand, entry rows, full-length) of the valid passes
    for q, (bases, fl, valid, ent) in enumerate(used):
        if valid:
            st = (int(fl) & 1) ^ f0
            seq = [3 - int(x) for x in bases[::-1]] if st else [int(x) for x in bases]
            passes.append((q, seq, st, [int(e) for e in ent], not (int(fl) & 2)))

    def test(fa, nf, ra, nr):
        p, near = fisher_exact(fa, nf, ra, nr)
        census["near_tie"] += 1 if near else 0
        census["borderline_p"] += 1 if _near_threshold(p, o.max_pvalue) else 0
        return p, p <= max_p

    # ---- substitution pileup and sites, window by window
    sub_sites, listed_sub = [], []
    for w in range(nw):
        ws, we, iws, iwe = _window(wb, nw, Ld, w)
        tpl, J = draft[ws:we], we - ws
        count = {}                                     # (column, strand) -> {outcome: passes}
        for (q, seq, st, ent, _) in passes:
            a, n = ent[iws], ent[iwe] - ent[iws]
            if a < 0 or n < 0 or a + n > len(seq):
                continue                               # no segment
            reason = "rows" if n > MAX_ROWS else "indel" if abs(n - J) >= o.min_indel else "counted"
            census["segments"].append((w, q, n, J, reason))
            if reason != "counted":
                continue
            for col, oc in edit_walk(seq[a:a + n], tpl).items():
                if wb[w] - ws <= col < wb[w + 1] - ws:
                    d = count.setdefault((col, st), {})
                    d[oc] = d.get(oc, 0) + 1
        here = []
        for col in range(wb[w] - ws, wb[w + 1] - ws):
            cf, cr = count.get((col, 0), {}), count.get((col, 1), {})
            census["max_count"] = max([census["max_count"]] + list(cf.values()) + list(cr.values()))
            nf, nr = sum(cf.values()), sum(cr.values())
            totals = sorted((-(cf.get(b, 0) + cr.get(b, 0)), b) for b in range(4) if b != tpl[col])
            if -totals[0][0] == 0:
                continue
            alt = totals[0][1]
            fa, ra = cf.get(alt, 0), cr.get(alt, 0)
            if nf < o.min_strand_passes or nr < o.min_strand_passes:
                continue
            if not (float(fa) >= frac * nf or float(ra) >= frac * nr):
                continue
            p, is_site = test(fa, nf, ra, nr)
            if is_site:
                here.append(dict(column=ws + col, kind=0, alt=alt, fwd_alt=fa, fwd_n=nf, rev_alt=ra, rev_n=nr, p=float(p)))
        census["sites_per_window"].append(len(here))
        census["windows_over"] += 1 if len(here) > WIN_SITES else 0
        sub_sites += here
        listed_sub += sorted(here, key=lambda s: s["column"])[:WIN_SITES]

    # ---- large indels: events of the 1-, 2- and 3-window spans, clusters of adjacent windows, one table per cluster
    indel_sites = []
    events = {1: {}, 2: {}}                            # kind -> {window: set of passes with the event there}
    covers = {}                                        # pass -> set of windows its one-window span covers
    for (q, seq, st, ent, _) in passes:
        covers[q] = set()
        for w in range(nw):
            ws = _window(wb, nw, Ld, w)[0]
            for s in (1, 2, 3):
                if w + s - 1 > nw - 1:
                    continue
                we = _window(wb, nw, Ld, w + s - 1)[1]
                ln = ent[_window(wb, nw, Ld, w + s - 1)[3]] - ent[_window(wb, nw, Ld, w)[2]]
                if not (0 <= ln <= len(seq)):
                    continue
                if s == 1:
                    covers[q].add(w)
                excess = ln - (we - ws)
                if excess >= o.min_indel:
                    events[1].setdefault(w, set()).add(q)
                if excess <= -o.min_indel:
                    events[2].setdefault(w, set()).add(q)
    strand_of = {q: st for (q, _, st, _, _) in passes}
    for kind in (1, 2):
        clusters, cur = [], set()
        for w in sorted(events[kind]):
            if cur and w - 1 not in cur:
                clusters.append(cur); cur = set()
            cur.add(w)
        if cur:
            clusters.append(cur)
        for cl in clusters:
            with_event = set().union(*(events[kind][w] for w in cl))
            counted = {q for q in strand_of if q in with_event or cl <= covers[q]}
            census["clusters"].append((kind, tuple(sorted(cl)), tuple(sorted({q // 64 for q in with_event}))))
            fn = sum(1 for q in counted if strand_of[q] == 0); rn = len(counted) - fn
            fa = sum(1 for q in with_event if strand_of[q] == 0); ra = len(with_event) - fa
            if fn < o.min_strand_passes or rn < o.min_strand_passes:
                continue
            p, is_site = test(fa, fn, ra, rn)
            if is_site:
                indel_sites.append(dict(column=wb[min(cl)], kind=kind, alt=-1, fwd_alt=fa, fwd_n=fn, rev_alt=ra, rev_n=rn, p=float(p)))

    # ---- verdict, counts, list
    key = lambda s: (s["column"], s["kind"])
    listed = sorted(listed_sub[:MAX_SITES] + sorted(indel_sites, key=key)[:MAX_SITES], key=key)[:MAX_SITES]
    full = [st for (_, _, st, _, is_full) in passes if is_full]
    if len(sub_sites) >= o.min_sites or indel_sites:
        verdict = HETERODUPLEX
    elif full.count(0) >= o.min_strand_passes and full.count(1) >= o.min_strand_passes:
        verdict = DOUBLE_STRAND
    else:
        verdict = UNTESTED
    census["n_sub"], census["n_indel"] = len(sub_sites), len(indel_sites)
    min_p = min([1.0] + [s["p"] for s in sub_sites + indel_sites])
    return dict(verdict=verdict, n_sub=len(sub_sites), n_indel=len(indel_sites), sites=listed, min_p=min_p), census


def hd_zmws(zmws, opts: Opts = Opts()):
    """-> (reports as hd_ref.hd_zmws gives them, censuses)"""
    both = [hd_zmw(Z, opts) for Z in zmws]
    return [r for r, _ in both], [c for _, c in both]


def borderline(census) -> bool:
    return census["borderline_p"] > 0 or census["near_tie"] > 0

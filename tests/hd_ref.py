"""CPU restatement of DESIGN.md §2 "Heteroduplex rule" (rule version 1), operation for operation, in numpy.

It takes what the engine's stages produced (draft, window bounds, per-pass validity and entry rows, the status after the alignment) and computes
what ccsx_hd_batch reports: verdict, site counts, the listed sites and min p.  The segment DPs are vectorised across segments.  The inputs come
from the engine (`collect_stage`, after a ccsx_hd_batch call) or from the oracle's stages (tools/hd_study.py); nothing here calls a kernel.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

OVERHANG, IMAX, WIN_SITES, MAX_SITES, LF_N = 2, 49, 8, 16, 511
SUCCESS = 0
UNTESTED, DOUBLE_STRAND, HETERODUPLEX = 0, 1, 2


@dataclass
class Opts:
    min_strand_passes: int = 3
    min_sites: int = 1
    min_indel: int = 21
    min_alt_frac: float = 0.5          # (used as the float32 the C struct holds)
    max_pvalue: float = 1e-3


@dataclass
class Zmw:
    """one ZMW's stage outputs: draft, core bounds wb[0..nw], status after the alignment, and per used pass: oriented-read source, flags, validity, entry rows"""
    draft: np.ndarray
    wb: np.ndarray
    status: int
    backbone: int
    reads: list = field(default_factory=list)     # (bases (native orientation), flags, valid, ent[2 nw])


def log_factorials() -> np.ndarray:
    """log k! for k = 0 .. 510: a sequential sum of log(k) in double (np.cumsum adds in order)"""
    lf = np.zeros(LF_N)
    lf[1:] = np.cumsum(np.log(np.arange(1, LF_N, dtype=np.float64)))
    return lf


_LF = log_factorials()


def fisher(a: int, nf: int, c: int, nr: int, lf=_LF) -> float:
    """two-sided Fisher exact p of [[a, nf - a], [c, nr - c]]: the tables with the same margins whose probability is <= p_obs (1 + 1e-7), summed in
    increasing order of the top-left cell, capped at 1"""
    m, N = a + c, nf + nr
    base = lf[nf] + lf[nr] + lf[m] + lf[N - m] - lf[N]
    thr = np.exp(base - lf[a] - lf[nf - a] - lf[m - a] - lf[nr - m + a]) * (1.0 + 1e-7)
    x = np.arange(max(0, m - nr), min(nf, m) + 1)
    px = np.exp(base - lf[x] - lf[nf - x] - lf[m - x] - lf[nr - m + x])
    p = float(np.cumsum(np.where(px <= thr, px, 0.0))[-1])
    return p if p < 1.0 else 1.0


def win(wb, nw, Ld, w):
    """window w: template draft[ws, we) and the indices of its two entry rows (k_polish's expressions)"""
    ws = max(int(wb[w]) - OVERHANG, 0)
    we = min(int(wb[w + 1]) + OVERHANG, Ld)
    return ws, we, (0 if w == 0 else 2 * w - 1), (2 * nw - 1 if w == nw - 1 else 2 * (w + 1))


def oriented(bases, st):
    return (3 - bases[::-1]).astype(np.uint8) if st else bases


def segment_outcomes(segs, tpls, cores, chunk=100_000):
    """unit-cost global edit DP of every segment against its template; trace-back from the end with the tie order diagonal, deletion, insertion.
    Returns (segment index, template column, outcome 0..3 = base, 4 = deletion) for every core column [cs, ce) the trace-back passes."""
    out_s, out_c, out_o = [], [], []
    for c0 in range(0, len(segs), chunk):
        S_, T_ = segs[c0:c0 + chunk], tpls[c0:c0 + chunk]
        N = len(S_)
        if N == 0:
            continue
        I = np.array([len(s) for s in S_]); J = np.array([len(t) for t in T_])
        Im, Jm = max(int(I.max()), 1), max(int(J.max()), 1)
        S = np.full((N, Im), 255, np.uint8); T = np.full((N, Jm), 254, np.uint8)
        for k in range(N):
            S[k, :I[k]] = S_[k]; T[k, :J[k]] = T_[k]
        mv = np.zeros((N, Im + 1, Jm + 1), np.int8)
        prev = np.tile(np.arange(Jm + 1, dtype=np.int32), (N, 1))
        for i in range(1, Im + 1):
            cur = np.empty_like(prev)
            cur[:, 0] = i
            rb = S[:, i - 1]
            for j in range(1, Jm + 1):
                dv = prev[:, j - 1] + (rb != T[:, j - 1])
                dl = cur[:, j - 1] + 1
                up = prev[:, j] + 1
                m = np.where((dv <= dl) & (dv <= up), 0, np.where(dl <= up, 1, 2)).astype(np.int8)
                cur[:, j] = np.where(m == 0, dv, np.where(m == 1, dl, up))
                mv[:, i, j] = m
            prev = cur
        cs = np.array([c[0] for c in cores[c0:c0 + chunk]]); ce = np.array([c[1] for c in cores[c0:c0 + chunk]])
        i, j, idx = I.copy(), J.copy(), np.arange(N)
        while True:
            act = (i > 0) | (j > 0)
            if not act.any():
                break
            m = np.where(i == 0, 1, np.where(j == 0, 2, mv[idx, i, j]))
            col = j - 1
            rec = act & (m != 2) & (col >= cs) & (col < ce)
            outc = np.where(m == 0, S[idx, np.maximum(i - 1, 0)], 4)
            out_s.append(idx[rec] + c0); out_c.append(col[rec]); out_o.append(outc[rec])
            j = np.where(act & (m != 2), j - 1, j)
            i = np.where(act & (m != 1), i - 1, i)
    cat = lambda a: np.concatenate(a) if a else np.zeros(0, np.int64)
    return cat(out_s).astype(np.int64), cat(out_c).astype(np.int64), cat(out_o).astype(np.int64)


def _site_key(s):
    return (s["column"], s["kind"])


def hd_zmws(zmws, opts: Opts = Opts()):
    """the rule for a list of Zmw: per ZMW a dict(verdict, n_sub, n_indel, sites (list of dicts, listed order), min_p)"""
    mi, msp = int(opts.min_indel), int(opts.min_strand_passes)
    frac = float(np.float32(opts.min_alt_frac))
    # ---- substitution pileup: every (pass, window) segment of every ZMW at once; windows numbered across the batch (gw)
    segs, tpls, cores, seg_gw, seg_st = [], [], [], [], []
    geo, wgeo = [], []                                 # per ZMW (nw, Ld, f0, first gw); per window (zmw, ws, cs, ce, template)
    for zi, Z in enumerate(zmws):
        nw = len(Z.wb) - 1 if Z.status == SUCCESS else 0
        Ld = len(Z.draft)
        f0 = int(Z.reads[Z.backbone][1]) & 1 if Z.reads else 0
        geo.append((nw, Ld, f0, len(wgeo)))
        for w in range(nw):
            ws, we, iws, iwe = win(Z.wb, nw, Ld, w)
            J = we - ws
            gw = len(wgeo)
            wgeo.append((zi, ws, int(Z.wb[w]) - ws, int(Z.wb[w + 1]) - ws, Z.draft[ws:we]))
            for (bases, fl, valid, ent) in Z.reads:
                if not valid:
                    continue
                L = len(bases)
                a, n = int(ent[iws]), int(ent[iwe]) - int(ent[iws])
                if a < 0 or n < 0 or a + n > L or n > IMAX or n - J >= mi or J - n >= mi:
                    continue
                st = (int(fl) & 1) ^ f0
                segs.append((oriented(bases, st)[a:a + n]) if not st else (3 - bases[L - a - n:L - a][::-1]).astype(np.uint8))
                tpls.append(Z.draft[ws:we]); cores.append((int(Z.wb[w]) - ws, int(Z.wb[w + 1]) - ws)); seg_gw.append(gw); seg_st.append(st)
    W = len(wgeo)
    si, col, oc = segment_outcomes(segs, tpls, cores)
    cnt = np.zeros((max(W, 1), 2, 32, 5), np.int32)
    if len(si):
        np.add.at(cnt, (np.array(seg_gw)[si], np.array(seg_st)[si], col, oc), 1)
    # ---- the column test, vectorised over every (window, column); Fisher only where the cheap conditions hold
    site_rec = {}                                      # gw -> list of sites in column order
    if W:
        tb = np.full((W, 32), 4, np.int64)
        core = np.zeros((W, 32), bool)
        for g, (zi, ws, cs, ce, t) in enumerate(wgeo):
            tb[g, :len(t)] = t; core[g, cs:ce] = True
        f, r = cnt[:, 0], cnt[:, 1]
        nf, nr = f.sum(-1), r.sum(-1)
        tot = (f[..., :4] + r[..., :4]).astype(np.int64)
        tot[np.arange(4)[None, None, :] == tb[..., None]] = -1          # never the draft base
        alt = tot.argmax(-1)                                            # (first maximum: the lowest code)
        best = np.take_along_axis(tot, alt[..., None], -1)[..., 0]
        fa = np.take_along_axis(f[..., :4], alt[..., None], -1)[..., 0]
        ra = np.take_along_axis(r[..., :4], alt[..., None], -1)[..., 0]
        cand = core & (best > 0) & (nf >= msp) & (nr >= msp) & ((fa.astype(float) >= frac * nf) | (ra.astype(float) >= frac * nr))
        for g, c in zip(*np.nonzero(cand)):
            p = fisher(int(fa[g, c]), int(nf[g, c]), int(ra[g, c]), int(nr[g, c]))
            if p <= opts.max_pvalue:
                site_rec.setdefault(int(g), []).append(dict(column=wgeo[g][1] + int(c), kind=0, alt=int(alt[g, c]), fwd_alt=int(fa[g, c]),
                                                            fwd_n=int(nf[g, c]), rev_alt=int(ra[g, c]), rev_n=int(nr[g, c]), p=p))
    res = []
    for zi, Z in enumerate(zmws):
        nw, Ld, f0, g0 = geo[zi]
        n_sub, subs, minp = 0, [], 1.0
        for w in range(nw):
            wsites = site_rec.get(g0 + w, [])
            n_sub += len(wsites)
            if wsites:
                minp = min(minp, min(s["p"] for s in wsites))
            subs += wsites[:WIN_SITES]
        # ---- large indels: events of 1-3-window spans, clusters of adjacent windows with an event of the same sign
        indels = []
        R = [(b, fl, ent) for (b, fl, v, ent) in Z.reads if v]
        if nw > 0 and R:
            E = np.array([e for (_, _, e) in R], np.int64)                  # [pass, 2 nw]
            Ls = np.array([len(b) for (b, _, _) in R], np.int64)[:, None]
            G = [win(Z.wb, nw, Ld, w) for w in range(nw)]
            ws_ = np.array([g[0] for g in G]); we_ = np.array([g[1] for g in G]); iws_ = np.array([g[2] for g in G]); iwe_ = np.array([g[3] for g in G])
            ev = np.zeros((len(R), nw, 2), bool); cov = np.zeros((len(R), nw), bool)
            for s in range(3):
                w = np.arange(nw - s)
                ln = E[:, iwe_[w + s]] - E[:, iws_[w]]
                ok = (ln >= 0) & (ln <= Ls)
                ex = ln - (we_[w + s] - ws_[w])[None, :]
                if s == 0:
                    cov[:, w] = ok
                ev[:, w, 0] |= ok & (ex >= mi)
                ev[:, w, 1] |= ok & (-ex >= mi)
            stq = np.array([(int(fl) & 1) ^ f0 for (_, fl, _) in R], np.int64)
            for sign in (0, 1):
                anyw = ev[:, :, sign].any(0)
                w = 0
                while w < nw:
                    if not anyw[w]:
                        w += 1
                        continue
                    w1 = w
                    while w1 + 1 < nw and anyw[w1 + 1]:
                        w1 += 1
                    e = ev[:, w:w1 + 1, sign].any(1); cv = cov[:, w:w1 + 1].all(1)
                    cn = e | cv
                    fa_, fn = int((cn & e & (stq == 0)).sum()), int((cn & (stq == 0)).sum())
                    ra_, rn = int((cn & e & (stq == 1)).sum()), int((cn & (stq == 1)).sum())
                    if fn >= msp and rn >= msp:
                        p = fisher(fa_, fn, ra_, rn)
                        if p <= opts.max_pvalue:
                            indels.append(dict(column=int(Z.wb[w]), kind=1 + sign, alt=-1, fwd_alt=fa_, fwd_n=fn, rev_alt=ra_, rev_n=rn, p=p))
                    w = w1 + 1
        n_ind = len(indels)
        if indels:
            minp = min(minp, min(s["p"] for s in indels))
        listed = sorted(subs[:MAX_SITES] + sorted(indels, key=_site_key)[:MAX_SITES], key=_site_key)[:MAX_SITES]
        full = [(int(fl) & 1) ^ f0 for (b, fl, v, ent) in Z.reads if v and not (int(fl) & 2)]
        fn_, rn_ = full.count(0), full.count(1)
        if Z.status != SUCCESS:
            verdict, n_sub, n_ind, listed, minp = UNTESTED, 0, 0, [], 1.0
        elif n_sub >= opts.min_sites or n_ind >= 1:
            verdict = HETERODUPLEX
        elif fn_ >= msp and rn_ >= msp:
            verdict = DOUBLE_STRAND
        else:
            verdict = UNTESTED
        res.append(dict(verdict=verdict, n_sub=n_sub, n_indel=n_ind, sites=listed, min_p=minp))
    return res


def need_cols(wb, Ld):
    """the window-edge column of every entry-row index (k_align's list: 0, b1-2, b1+2, ..., Ld)"""
    nw = len(wb) - 1
    return [0 if k == 0 else (Ld if k == 2 * nw - 1 else int(wb[(k + 1) >> 1]) + (-OVERHANG if k & 1 else OVERHANG)) for k in range(2 * nw)]


def collect_stage(handle, batch, status, backbone, zmws=None):
    """the engine's stage outputs after a ccsx_hd_batch call (ccsx_stage_draft / _windows / _align) as Zmw records"""
    out = []
    for z in (range(batch.n_zmw) if zmws is None else zmws):
        d = handle.stage_draft(z)
        wb = handle.stage_windows(z) if len(d) else np.zeros(1, np.int32)
        cols = need_cols(wb, len(d)) if len(wb) > 1 else []
        reads = []
        for r in range(int(batch.read_off[z]), int(batch.read_off[z + 1])):
            rs, v, _ = handle.stage_align(r, len(d))
            reads.append((batch.read(r)[0], int(batch.flags[r]), bool(v), np.array([rs[c] for c in cols], np.int64)))
        out.append(Zmw(d, wb, int(status[z]), int(backbone[z]), reads))
    return out

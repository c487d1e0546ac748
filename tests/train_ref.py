"""Float64 restatement of the model training of DESIGN.md §2 "Model training" (numpy only; no ctypes, nothing of train_core.h or the library).

E-step: the full forward and backward recurrences of arrow_ref.loglik over EXPLICIT oriented templates (the caller reverse-complements a template for a
reverse-strand pass), vectorised over pairs, unscaled probabilities; per pair the posterior event tables of the core columns.  M-step: the fitter's rule with
numpy.linalg.lstsq.  A generator SAMPLES passes from a parameter set and records the row at which every template column is entered, so that pairs can be cut on
the generating path.  Shares tables64, ctx, revcomp with arrow_ref.py.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import arrow_ref as ar

NCTX, NOBS = ar.NCTX, ar.NOBS
FRAC = 2.0 ** 32


def model_ns(model):
    """a parameter set as plain float64 arrays (what tables64 reads), from anything with the six attributes"""
    f = lambda a: np.array(a, dtype=np.float64)
    return SimpleNamespace(trans_poly=f(model.trans_poly), em_match=f(model.em_match), em_branch=f(model.em_branch), em_stick=f(model.em_stick),
                           snr_lo=float(model.snr_lo), snr_hi=float(model.snr_hi))


def make_pair(tpl, lf, cs, ce, obs, snr_index=0):
    """one pair: template in the pass's orientation, its left flank (4 = none), core [cs, ce), observation codes, and which table set (ZMW) it uses"""
    return dict(tpl=np.asarray(tpl, np.int64), lf=int(lf), cs=int(cs), ce=int(ce), obs=np.asarray(obs, np.int64), z=int(snr_index))


def oriented(tpl, lf, rf, cs, ce, rev):
    """(template, left flank, cs, ce) of a window in the orientation of a pass on strand `rev`"""
    if not rev:
        return np.asarray(tpl, np.uint8), int(lf), int(cs), int(ce)
    J = len(tpl)
    return ar.revcomp(tpl), (3 - int(rf)) if rf < 4 else 4, J - int(ce), J - int(cs)


def e_step(tabs_by_z, pairs, want_counts=True):
    """Full forward / backward of every pair.  tabs_by_z: list of (ME[16,12], INS[16,12], DL[16]) probabilities per table set.
    Returns dict(log2L[P] (alpha), log2B[P] (beta(0,0)), match[P,16,12], stay[P,16,12], dele[P,16], cells_m / cells_s [P,16,12], cells_d [P,16]):
    posterior events of the core columns per pair, and how many cells contribute to each entry."""
    P = len(pairs)
    J = np.array([len(p["tpl"]) for p in pairs], np.int64); n = np.array([len(p["obs"]) for p in pairs], np.int64)
    Jm, nm = int(J.max()), int(n.max())
    K = np.zeros((P, Jm + 1), np.int64); O = np.zeros((P, nm + 1), np.int64)
    for q, p in enumerate(pairs):
        t = p["tpl"]
        K[q, :len(t)] = ar.ctx(np.concatenate([[p["lf"]], t[:-1]]), t)
        O[q, :len(p["obs"])] = p["obs"]
    zi = np.array([p["z"] for p in pairs], np.int64)
    ME = np.stack([t[0] for t in tabs_by_z])[zi]; INS = np.stack([t[1] for t in tabs_by_z])[zi]; DL = np.stack([t[2] for t in tabs_by_z])[zi]
    ar_ = np.arange(P)
    me = lambda j, i: ME[ar_, K[:, j], O[:, i]]
    ins = lambda j, i: INS[ar_, K[:, j], O[:, i]]
    dl = lambda j: DL[ar_, K[:, j]]
    A = np.zeros((nm + 2, Jm + 2, P))
    for j in range(Jm + 1):
        for i in range(nm + 1):
            v = np.zeros(P)
            if i == 0 and j == 0: v = v + 1.0
            if j > 0:
                v = v + A[i, j - 1] * dl(j - 1)
                if i > 0: v = v + A[i - 1, j - 1] * me(j - 1, i - 1)
            if i > 0: v = v + A[i - 1, j] * ins(j, i - 1) * (j < J)
            A[i, j] = v * ((i <= n) & (j <= J))
    B = np.zeros((nm + 2, Jm + 2, P))
    for j in range(Jm, -1, -1):
        for i in range(nm, -1, -1):
            v = dl(j) * B[i, j + 1]
            if i < nm: v = v + (me(j, i) * B[i + 1, j + 1] + ins(j, i) * B[i + 1, j]) * (i < n)
            B[i, j] = np.where((i == n) & (j == J), 1.0, v * ((i <= n) & (j < J)))
    L = A[n, J, ar_]
    with np.errstate(divide="ignore"):
        out = dict(log2L=np.log2(L), log2B=np.log2(B[0, 0]))
    if not want_counts:
        return out
    M = np.zeros((P, NCTX, NOBS)); S = np.zeros((P, NCTX, NOBS)); D = np.zeros((P, NCTX))
    cm = np.zeros((P, NCTX, NOBS), np.int64); cd = np.zeros((P, NCTX), np.int64)
    cs = np.array([p["cs"] for p in pairs], np.int64); ce = np.array([p["ce"] for p in pairs], np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(L > 0, 1.0 / L, 0.0)
    for j in range(Jm):
        core = (j >= cs) & (j < ce)
        if not core.any(): continue
        kj = K[:, j]
        for i in range(nm + 1):
            rowd = core & (i <= n)
            np.add.at(D, (ar_, kj), np.where(rowd, A[i, j] * dl(j) * B[i, j + 1] * inv, 0.0))
            np.add.at(cd, (ar_, kj), rowd.astype(np.int64))
            if i < nm:
                row = core & (i < n)
                oi = O[:, i]
                np.add.at(M, (ar_, kj, oi), np.where(row, A[i, j] * me(j, i) * B[i + 1, j + 1] * inv, 0.0))
                np.add.at(S, (ar_, kj, oi), np.where(row, A[i, j] * ins(j, i) * B[i + 1, j] * inv, 0.0))
                np.add.at(cm, (ar_, kj, oi), row.astype(np.int64))
    out.update(match=M, stay=S, dele=D, cells_m=cm, cells_s=cm, cells_d=cd)
    return out


def bin_centres(lo, hi, nb):
    return lo + (np.arange(nb) + 0.5) * (hi - lo) / nb if hi > lo else np.full(nb, float(lo))     # (a range of one point: every row is in bin 0, at that point)


def m_step(start, match, stay, dele, snr, degree=1, snr_bins=64, min_events=200.0, pseudo=0.5):
    """The fitter's rule restated.  start: model_ns; match / stay [n,16,12], dele [n,16]: events per ZMW row (float64); snr [n,4].
    Returns (model_ns, info) with info = dict(kept=contexts whose match row kept the start's, populated={k: bins}, degree={k: d})."""
    S = model_ns(start)
    match, stay, dele, snr = (np.asarray(a, np.float64) for a in (match, stay, dele, snr))
    lo, hi, nb = S.snr_lo, S.snr_hi, int(snr_bins)
    cen = bin_centres(lo, hi, nb)
    M = model_ns(S)
    kept, populated, degs = 0, {}, {}
    first, last = nb, -1
    for k in range(NCTX):
        cur = k & 3
        tm = match[:, k].sum(0)
        if tm.sum() >= min_events and tm.sum() > 0: M.em_match[k] = (tm + pseudo) / (tm.sum() + 12 * pseudo)
        else: kept += 1
        st = stay[:, k].sum(0).reshape(4, 3)
        br = st[cur]; sk = st.sum(0) - st[cur]
        if br.sum() >= min_events and br.sum() > 0: M.em_branch[k] = (br + pseudo) / (br.sum() + 3 * pseudo)
        if sk.sum() >= min_events and sk.sum() > 0: M.em_stick[k] = (sk + pseudo) / (sk.sum() + 3 * pseudo)
        s = np.clip(np.where(np.isnan(snr[:, cur]), lo, snr[:, cur]), lo, hi)
        b = np.clip(np.floor((s - lo) / (hi - lo) * nb).astype(np.int64), 0, nb - 1) if hi > lo else np.zeros(len(s), np.int64)
        N = np.zeros((nb, 4))
        np.add.at(N[:, 0], b, match[:, k].sum(1))
        stz = stay[:, k].reshape(-1, 4, 3).sum(2)
        np.add.at(N[:, 1], b, stz[:, cur]); np.add.at(N[:, 2], b, stz.sum(1) - stz[:, cur]); np.add.at(N[:, 3], b, dele[:, k])
        pop = np.flatnonzero((N[:, 0] >= min_events) & (N[:, 0] > 0))
        populated[k] = pop
        if not len(pop): continue
        first, last = min(first, int(pop[0])), max(last, int(pop[-1]))
        d = min(int(degree), len(pop) - 1); degs[k] = d
        x0 = 0.5 * (cen[pop[0]] + cen[pop[-1]]); xs = 0.5 * (cen[pop[-1]] - cen[pop[0]])
        if not xs > 0: xs = 1.0
        u = (cen[pop] - x0) / xs
        V = np.vander(u, d + 1, increasing=True); sw = np.sqrt(N[pop, 0])
        for mv in range(3):
            y = N[pop, 1 + mv] / N[pop, 0]
            a = np.linalg.lstsq(V * sw[:, None], y * sw, rcond=None)[0]
            c = np.polynomial.Polynomial(a)(np.polynomial.Polynomial([-x0 / xs, 1.0 / xs])).coef
            M.trans_poly[k, mv] = 0.0
            M.trans_poly[k, mv, :len(c)] = c
    if last >= first and last >= 0:
        M.snr_lo, M.snr_hi = float(np.float32(cen[first])), float(np.float32(cen[last]))
    for key in ("trans_poly", "em_match", "em_branch", "em_stick"):
        setattr(M, key, getattr(M, key).astype(np.float32).astype(np.float64))     # the parameter file holds float32
    return M, dict(kept=kept, populated=populated, degree=degs)


def _choice_rows(rng, probs):
    """one draw per row of a [n, m] table of probabilities (rows sum to 1)"""
    c = np.cumsum(probs, 1)
    u = rng.random(len(probs)) * c[:, -1]
    return np.minimum((u[:, None] >= c).sum(1), probs.shape[1] - 1)


def sample_pass(model, snr, tpl, lf, rng):
    """One pass GENERATED by the model from an oriented template: per position a geometric number of stays with their emissions, then a match (emission) or a
    deletion.  Returns (obs codes, enter[len(tpl) + 1]): enter[j] = read bases emitted before column j is entered (enter[-1] = the pass's length)."""
    S = model_ns(model)
    pM, pB, pS, pD = ar.transitions64(S, snr)
    t = np.asarray(tpl, np.int64); L = len(t)
    k = ar.ctx(np.concatenate([[lf], t[:-1]]), t)
    pA, pI = pM[k] + pD[k], pB[k] + pS[k]
    nst = rng.geometric(pA) - 1
    adv = rng.random(L) < pM[k] / pA
    om = _choice_rows(rng, S.em_match[k] / S.em_match[k].sum(1, keepdims=True))
    pos = np.repeat(np.arange(L), nst); ks = k[pos]
    br = rng.random(len(pos)) < pB[ks] / pI[pos]
    pwb = _choice_rows(rng, S.em_branch[ks] / S.em_branch[ks].sum(1, keepdims=True)) if len(pos) else np.zeros(0, np.int64)
    pws = _choice_rows(rng, S.em_stick[ks] / S.em_stick[ks].sum(1, keepdims=True)) if len(pos) else np.zeros(0, np.int64)
    other = (t[pos] + 1 + rng.integers(0, 3, len(pos))) & 3
    ost = np.where(br, t[pos] * 3 + pwb, other * 3 + pws)
    per = nst + adv                                         # bases position j emits
    enter = np.concatenate([[0], np.cumsum(per)])
    obs = np.zeros(int(enter[-1]), np.int64)
    stay_at = enter[pos] + (np.arange(len(pos)) - np.repeat(np.cumsum(nst) - nst, nst))
    obs[stay_at] = ost
    obs[(enter[:-1] + nst)[adv]] = om[adv]
    return obs.astype(np.uint8), enter.astype(np.int64)


def cut_pairs(tpl, passes, z, core=22, overhang=2, imax=63):
    """Pairs of one ZMW cut on the generating path: cores of `core` columns (the last one takes the rest), +-overhang, the segment between the rows at which
    the window's first column and the column after its last are entered.  passes: [(rev, obs, enter)] with obs / enter in the pass's own orientation.
    Pairs of more than imax bases are left out (the rule's limit)."""
    t = np.asarray(tpl, np.uint8); L = len(t)
    bounds = list(range(0, L, core)) + [L]
    if len(bounds) > 2 and L - bounds[-2] < 5: del bounds[-2]          # (a short rest joins the core before it)
    out = []
    for w in range(len(bounds) - 1):
        ws, we = max(0, bounds[w] - overhang), min(L, bounds[w + 1] + overhang)
        if we - ws > 31: continue
        lf, rf = (int(t[ws - 1]) if ws > 0 else 4), (int(t[we]) if we < L else 4)
        for rev, obs, enter in passes:
            a, b = (L - we, L - ws) if rev else (ws, we)
            seg = obs[int(enter[a]):int(enter[b])]
            if len(seg) > imax: continue
            to, lfo, cs, ce = oriented(t[ws:we], lf, rf, bounds[w] - ws, bounds[w + 1] - ws, rev)
            out.append(make_pair(to, lfo, cs, ce, seg, z))
    return out

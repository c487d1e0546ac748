"""The filter lab: a small planted batch that takes k_polish's candidate filter and z-score gate (DESIGN.md §2 "Candidate filter", "z-score gate", "Polish loop",
"QVs") to the cases their rules name.  Every ZMW has a name, a class, a draft that is handed in through the polish seam (so the planted template IS the draft), and
passes that are error-free copies of a truth except where an entry plants something: the pile-up margins are therefore known by construction.  Every ZMW carries
`checks`: what the windows and dirty bits of the run (the engine's stage outputs on the device, the restatement's alignments on the CPU) and the float64 reference's
verdicts on them must show for the class to have occurred; a class that does not occur is a failure, never a skip.

Built deterministically: sequences come from seeded generators, every edit is placed by construction relative to the window bounds of the draft.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

from ccs_amd import api
import arrow_ref as A
import oracle_lib as O

SNR0 = (9.0, 16.0, 8.0, 13.0)
PARTIAL, ADAPTER_AT_END = 2, 4
RUNS = ((True, 50, -3.4), (True, 93, -3.4), (False, 50, -3.4), (False, 93, -1.0), (False, 50, 0.0), (True, 93, 0.0))      # (qv_only, max_qv, min_zscore)


@dataclass
class Zmw:
    name: str
    cls: str
    draft: np.ndarray
    passes: list                                     # (native-orientation bases, pw, flags)
    checks: list = field(default_factory=list)       # (what, fn(W) -> bool), W = the ZMW's windows with margins and reference verdicts of the DEFAULT run (full polish, max_qv 50, z -3.4)
    zchecks: dict = field(default_factory=dict)      # {min_zscore: [(what, fn(W) -> bool)]} on the full-polish run at that threshold
    planted_z: list = field(default_factory=list)    # (window, pass): z decisions that must be decided (planted drops and the planted keeps next to them)


def hash_str(s):
    h = 2166136261
    for c in s.encode(): h = ((h ^ c) * 16777619) & 0xffffffff
    return h


def _rng(tag): return np.random.default_rng(hash_str(tag))


def template(tag, n):
    """n bases without two equal neighbours: every homopolymer of the lab is planted"""
    g = _rng(tag); t = np.zeros(n, np.uint8); prev = 4
    for i in range(n):
        b = int(g.integers(0, 4))
        if b == prev: b = (b + 1 + int(g.integers(0, 3))) & 3
        t[i] = prev = b
    return t


def other(*bs):
    """a base different from all of bs"""
    return next(b for b in range(4) if b not in [int(x) for x in bs])


def run_at(t, at, n):
    """plant a homopolymer of n bases at t[at:at+n] whose base differs from both neighbours"""
    t = t.copy(); b = other(t[at - 1] if at > 0 else 4, t[at + n] if at + n < len(t) else 4)
    t[at:at + n] = b
    return t


def sub(t, p): s = t.copy(); s[p] = (int(s[p]) + 2) & 3; return fix(s, t, p)
def fix(s, t, p):
    """keep a substituted base from making a homopolymer with a neighbour"""
    for step in (2, 1, 3):
        b = (int(t[p]) + step) & 3
        if (p == 0 or b != t[p - 1]) and (p + 1 >= len(t) or b != t[p + 1]): s[p] = b; return s
    return s
def delete(t, p, n=1): return np.concatenate([t[:p], t[p + n:]]).astype(np.uint8)
def insert(t, p, bases): return np.concatenate([t[:p], np.asarray(bases, np.uint8), t[p:]]).astype(np.uint8)
def rc(t): return (3 - np.asarray(t)[::-1]).astype(np.uint8)


def make_passes(tag, truth, n, mods=None, junk=(), extra=(), pw_of=None, pw_const=None):
    """n full-length passes, strands alternating: copies of `truth` (draft orientation) except pass k = mods[k](truth); `junk` passes are random sequence (they fail the
    alignment); extra: (draft-orientation bases, flags) appended (partial passes)"""
    g = _rng(tag + "/pw"); out = []
    for k in range(n):
        b = mods[k](truth) if mods and k in mods else truth
        if k in junk: b = g.integers(0, 4, len(truth)).astype(np.uint8)
        fl = k & 1
        out.append((rc(b) if fl else np.asarray(b, np.uint8).copy(), fl))
    for b, fl in extra: out.append((rc(b) if fl & 1 else np.asarray(b, np.uint8).copy(), fl))
    out = [(b, g.integers(1, 4, len(b)).astype(np.uint8), fl) for b, fl in out]
    for k, (lo, pw) in (pw_of or {}).items(): out[k][1][lo:lo + len(pw)] = pw          # (native orientation)
    for k, v in (pw_const or {}).items(): out[k][1][:] = v
    return out


def stable(tag, n, plant, tries=60):
    """a template of n bases and what `plant(t, wb)` makes of it — (draft, anything else) — such that the DRAFT's windows are those the planting was placed by"""
    for k in range(tries):
        t = template(f"{tag}#{k}", n); wb = O.windows(t)
        res = plant(t, wb)
        if res is not None and np.array_equal(O.windows(res[0]), wb): return (wb,) + tuple(res)
    raise AssertionError(f"{tag}: no template whose windows survive the planting")


def col(W, w, p): return p - W[w]["ws"]                      # window column of draft position p
def g_at(W, w, p): return W[w]["g"][col(W, w, p)]
def ev_at(W, w, p): return W[w]["ev"][col(W, w, p)]


def _zsums(t, flank):
    MU, VAR = A.zmoments(api.default_model(), SNR0)
    t = np.asarray(t, np.int64); k = A.ctx(np.concatenate([[flank], t[:-1]]), t)
    return float(MU[k].sum()), float(VAR[k].sum())


def _between_strand_thresholds(d, wb, w, zmin=3.4, margin=0.15):
    """substitution sites (draft positions, inside the core of window w, out of the neighbours' sight) and pulse widths (native offset, values) for a REVERSE pass whose
    log2-likelihood L in window w has L - M_rev < -zmin sqrt(V_rev) but L - M_fwd > -zmin sqrt(V_fwd), each by `margin` bits: float64, seeded, first hit"""
    ws, we = int(wb[w]) - 2, int(wb[w + 1]) + 2; tpl = d[ws:we]; lf, rf = int(d[ws - 1]), int(d[we])
    tr = A.revcomp(tpl); Mr, Vr = _zsums(tr, 3 - rf); Mf, Vf = _zsums(tpl, lf)
    lo, hi = sorted((Mr - zmin * np.sqrt(Vr), Mf - zmin * np.sqrt(Vf)))
    assert hi - lo > 4 * margin and Mr - zmin * np.sqrt(Vr) == hi, "the window's strand sums are too close (or the other way round)"
    t64 = A.tables64(api.default_model(), SNR0); g = _rng("m7/zr")
    for nsub in range(3, 12):
        sites = [int(wb[w]) + 3 + 2 * k for k in range(nsub)]
        if sites[-1] > int(wb[w + 1]) - 4: break
        t = d.copy()
        for q in sites: t = sub(t, q)
        seg = A.revcomp(t[ws:we])
        for _ in range(120):
            pw = g.integers(1, 4, len(seg)).astype(np.uint8)
            L = A.loglik(t64, tr, 3 - rf, A.obs_codes(seg, pw))[0]
            if lo + margin < L < hi - margin: return sites, (len(d) - we, pw)
    raise AssertionError("no reverse pass between the two thresholds")


def _strand_sums_disagree(w, k):
    """pass k of window w (a reverse pass): dropped with the reverse strand's sums, kept with the forward strand's"""
    r = w["idx"].index(k); dz, V, _ = w["last"]["z"][r]
    Mr, Vr = _zsums(A.revcomp(w["tpl"]), 3 - w["rf"] if w["rf"] < 4 else 4); Mf, Vf = _zsums(w["tpl"], w["lf"])
    L = dz + Mr
    return w["strands"][k] == 1 and abs(V - Vr) < 1e-9 and dz < -3.4 * np.sqrt(Vr) and not (L - Mf < -3.4 * np.sqrt(Vf))


def build():
    Z = []

    # ---- margin threshold: 5 clean passes (nothing may be skipped), 6 clean (g exactly 6), 7 with one dirty (g 5 there, 7 beside)
    def p(t, wb):
        return run_at(t, int(wb[1]) + 8, 3), None
    wb, d, _ = stable("m5", 66, p)
    Z.append(Zmw("m5", "margin", d, make_passes("m5", d, 5), [
        ("g = 5 on every column and no evidence", lambda W: all(g == 5 for w in W for g in w["g"]) and not any(e for w in W for e in w["ev"])),
        ("the reference skips nothing and calls nothing quiet", lambda W: not any(any(w["last"]["skipped"]) or any(w["last"]["quiet"]) for w in W))]))

    # m6: a quiet run in a window's middle; runs of two across the left and the right edge of a middle window's template (column 0 / J - 1 inside a homopolymer by the
    # flank alone); an evidence position at J - 1 of the last window outside any homopolymer: the four insertions after the last column go with it
    def p(t, wb):
        d = run_at(t, int(wb[1]) + 9, 4)
        ws, we = int(wb[3]) - 2, int(wb[4]) + 2
        d[ws - 1] = d[ws]; d[we] = d[we - 1]
        if d[ws - 2] == d[ws - 1] or d[ws + 1] == d[ws] or d[we - 2] == d[we - 1] or d[we + 1] == d[we]: return None
        return d, (int(wb[1]) + 9,)
    wb, d, (hp0,) = stable("m6", 132, p)
    def last_col_skipped(W):
        w = W[-1]; J = len(w["tpl"]); L = w["last"]
        return w["rf"] == 4 and L["skipped"][J - 1] and not any(L["valid"][s * 32 + J] for s in range(4, 8)) and not any(L["valid"][s * 32 + J - 1] for s in range(8))
    Z.append(Zmw("m6", "margin", d, make_passes("m6", d, 6), [
        ("g = 6 on every column, evidence everywhere", lambda W: all(g == 6 for w in W for g in w["g"]) and all(e for w in W for e in w["ev"])),
        ("a quiet run of 4 in the middle of window 1", lambda W, hp0=hp0: all(W[1]["last"]["quiet"][col(W, 1, hp0 + k)] for k in range(4)) and W[1]["cs"] + 4 < col(W, 1, hp0) < W[1]["ce"] - 8),
        ("only the two run-length lanes of the run are enumerated, at its first base", lambda W, hp0=hp0: sorted(int(m) >> 5 for m in np.flatnonzero(W[1]["last"]["valid"]) if col(W, 1, hp0) <= (int(m) & 31) < col(W, 1, hp0) + 4)
            == [3, 4 + int(W[1]["tpl"][col(W, 1, hp0)])] and all((int(m) & 31) == col(W, 1, hp0) for m in np.flatnonzero(W[1]["last"]["valid"]) if col(W, 1, hp0) <= (int(m) & 31) < col(W, 1, hp0) + 4)),
        ("column 0 of window 3 is inside a homopolymer by its left flank alone", lambda W: W[3]["lf"] == W[3]["tpl"][0] != W[3]["tpl"][1] and W[3]["last"]["quiet"][0]),
        ("column J - 1 of window 3 is inside a homopolymer by its right flank alone", lambda W: W[3]["rf"] == W[3]["tpl"][-1] != W[3]["tpl"][-2] and W[3]["last"]["quiet"][len(W[3]["tpl"]) - 1]),
        ("first and last window have no flank", lambda W: W[0]["lf"] == 4 and W[-1]["rf"] == 4),
        ("the last column carries evidence outside a homopolymer: skipped, the insertions after it with it", last_col_skipped)]))

    # m7: 7 passes, one dirty at a column; the draft starts AND ends with a run of two (first / last window without a flank: column 0 / J - 1 are core columns inside a
    # homopolymer: quiet, and of the insertions after the last column none stays)
    def p(t, wb):
        d = t.copy(); d[1] = d[0]; d[-2] = d[-1]
        if d[2] == d[1] or d[-3] == d[-2]: return None
        return d, (int(wb[2]) + 10,)
    wb, d, (p7,) = stable("m7", 110, p)
    def last_col_quiet(W):
        w = W[-1]; J = len(w["tpl"]); L = w["last"]
        return L["quiet"][J - 1] and L["quiet"][J - 2] and not any(L["valid"][s * 32 + J] for s in range(4, 8)) and [int(m) >> 5 for m in np.flatnonzero(L["valid"]) if (int(m) & 31) == J - 2] != []
    # ... and reverse pass 5 carries substitutions in window 1 and pulse widths chosen so that its z sqrt(V) lies between the threshold of the REVERSE strand's sums (it is
    # dropped) and what the forward strand's sums would give (it would stay): the two differ by about one bit here, the reference itself places the pass (as the
    # existing Arrow lab lets the reference choose its 33-base insertion site)
    zr_sites, zr_pw = _between_strand_thresholds(d, wb, 1)
    Z.append(Zmw("m7", "margin, z drop", d, make_passes("m7", d, 7, {3: lambda t, p7=p7: sub(t, p7), 5: lambda t: [t := sub(t, q) for q in zr_sites][-1]}, pw_of={5: zr_pw}), [
        ("reverse pass 5 is dropped by z-score in window 1 by the reverse strand's sums; the forward strand's sums would keep it", lambda W: [bool(w["zdrop"][5]) for w in W] == [k == 1 for k in range(len(W))]
            and _strand_sums_disagree(W[1], 5)),
        ("g = 5 at the planted column, 7 beside it", lambda W, p7=p7: g_at(W, 2, p7) == 5 and g_at(W, 2, p7 - 1) == 7 and g_at(W, 2, p7 + 1) == 7),
        ("the g = 5 column has no evidence and is polished in full; its neighbours are skipped", lambda W, p7=p7: not ev_at(W, 2, p7) and not W[2]["last"]["skipped"][col(W, 2, p7)]
            and W[2]["last"]["skipped"][col(W, 2, p7) - 1] and W[2]["last"]["skipped"][col(W, 2, p7) + 1]),
        ("column 0 of the first window is a quiet core column", lambda W: W[0]["cs"] == 0 and W[0]["last"]["quiet"][0]),
        ("the last column is quiet: no insertion after it stays", last_col_quiet)], planted_z=[(1, 5), (1, 3), (1, 1)]))

    # split6: 6 clean passes and one with a 60-base block (a split pass: dirty everywhere) — g = 7 - 2 = 5 where it has a segment, nothing is skipped anywhere
    def blk(tag, n): return _rng(tag).integers(0, 4, n).astype(np.uint8)
    t = template("split6", 132); wb = O.windows(t); at = int(wb[3]) + 5
    Z.append(Zmw("split6", "dirty everywhere", t, make_passes("split6", t, 7, {4: lambda t, at=at: insert(t, at, blk("split6/b", 60))}), [
        ("the split pass is dirty everywhere", lambda W: all(all(w["dirty"][4]) for w in W)),
        ("g = 5 wherever the split pass has a segment, and no evidence anywhere", lambda W: all(set(w["g"]) == ({5} if w["seg"][4] else {6}) for w in W) and sum(1 for w in W if w["seg"][4]) >= len(W) - 1
            and not any(e for w in W if w["seg"][4] for e in w["ev"]))]))

    # g11_13: 13 passes, one dirty at a column (g = 11 there, 13 beside)
    t = template("g13", 88); wb = O.windows(t); p13 = int(wb[1]) + 7
    Z.append(Zmw("g11_13", "margin", t, make_passes("g13", t, 13, {5: lambda t: sub(t, p13)}), [
        ("g = 11 at the planted column, 13 elsewhere", lambda W: g_at(W, 1, p13) == 11 and sorted(set(g for w in W for g in w["g"])) == [11, 13])]))

    # g12_tracts: 16 passes; two dirty at one column (g = 12), one at another (g = 14); a closed homopolymer of 9 in whose window pass 6 carries foreign sequence of the
    # right length (dropped by z-score there: the 100 / np^2 scale of the tract's floor is that of 15 passes, not 16); a period-2 tract of 12 with evidence: skipped, yet
    # floored at 0.2 / 12
    def p(t, wb):
        d = run_at(t, int(wb[2]) + 6, 9)
        a = int(wb[4]) + 5; x, y = 1, 2
        d[a:a + 12] = [x, y] * 6; d[a - 1] = other(y, d[a - 2], x); d[a + 12] = other(x, d[a + 13], y)
        if d[a - 1] == d[a - 2] or d[a + 12] == d[a + 13]: return None
        if int(wb[3]) - int(wb[2]) < 21: return None
        return d, (int(wb[2]) + 6, a)
    wb, d, (hp9, tr2) = stable("g12", 154, p)
    p12, p14 = int(wb[0]) + 9, int(wb[0]) + 15
    # foreign sequence of the right length: every base before and after the run and every other base of the run, out of the neighbouring windows' sight
    fz = list(range(int(wb[2]) + 2, hp9)) + list(range(hp9 + 1, hp9 + 9, 2)) + list(range(hp9 + 10, int(wb[3]) - 2))
    def foreign(t, at):
        """the bases at `at` replaced by bases that match neither the position nor a neighbour of it (no path one column off explains them), no two equal in a row"""
        s = t.copy()
        for q in at:
            bad = [int(t[q - 1]), int(t[q]), int(t[q + 1])]
            ok = [b for b in range(4) if b not in bad]
            s[q] = next((b for b in ok if b != s[q - 1]), ok[0])
        return s
    def tract_floored(W):
        w = W[4]; L = w["last"]; cs = [col(W, 4, tr2 + k) for k in range(1, 11)]
        core = [c for c in cs if w["cs"] <= c < w["ce"]]
        return all(w["ev"][c] and L["skipped"][c] for c in cs) and len(core) >= 8 and all(w["p"][c - w["cs"]] == w["floor"][c - w["cs"]] > L["p_skip"][c]
            and abs(w["floor"][c - w["cs"]] - 0.2 / 12 * 100 / 256) < 1e-12 for c in core)
    Z.append(Zmw("g12_tracts", "margin, tracts, z drop", d, make_passes("g12", d, 16, {2: lambda t: sub(t, p12), 9: lambda t: sub(sub(t, p12), p14), 6: lambda t: foreign(t, fz),
                                                                                                 11: lambda t: sub(t, hp9 + 4), 13: lambda t: sub(t, hp9 + 4)}), [
        ("a substitution in 2 of 16 passes inside the quiet run: g = 12 there, still quiet, its substitution lanes stay excluded and its sum starts at p_skip",
         lambda W: g_at(W, 2, hp9 + 4) == 12 and W[2]["last"]["quiet"][col(W, 2, hp9 + 4)] and not any(W[2]["last"]["valid"][s * 32 + col(W, 2, hp9 + 4)] for s in range(8))
                   and W[2]["p"][col(W, 2, hp9 + 4) - W[2]["cs"]] >= W[2]["last"]["p_skip"][col(W, 2, hp9 + 4)] > 0),
        ("g = 12 and g = 14 at the planted columns of window 0", lambda W: g_at(W, 0, p12) == 12 and g_at(W, 0, p14) == 14),
        ("pass 6 is dropped by z-score in window 2 and nowhere else", lambda W: [bool(w["zdrop"][6]) for w in W] == [k == 2 for k in range(len(W))]),
        ("the closed run of 9 is floored at the scale of 15 usable passes, not 16", lambda W: W[2]["last"]["n_use"] == 15 and
            all(abs(W[2]["floor"][col(W, 2, hp9 + k) - W[2]["cs"]] - 0.2 / 9 * 100 / 225) < 1e-12 for k in range(9))),
        ("the period-2 tract of 12 carries evidence, is skipped, and reports the floor 0.2 / 12 (closed, 16 passes: x 100 / 256), not p_skip", tract_floored)],
        zchecks={0.0: [("with the gate off pass 6 stays and the floor takes 16 passes", lambda W: W[2]["last"]["n_use"] == 16 and not any(W[2]["zdrop"]))]},
        planted_z=[(2, 6), (2, 5), (2, 7), (1, 6), (3, 6)]))

    # spread: draft errors (substitutions against all 8 passes: a dirty majority, g = -8) — in a window's middle (a position 3 away has no evidence, one 4 away has);
    # at window column 0; at column J - 1; in the two-base overhang (two windows see it at different columns); just outside a window's template (it must not count there)
    # ... and a run of 5 in window 0 that the passes have with 4 bases: the aligner marks ONE end of the run, the polish deletes the run's first base; the positions within
    # 3 of the applied site that carried evidence are re-opened and report a computed QV in the next round, not p_skip
    d = run_at(template("spreadA", 220), 9, 5); wb = O.windows(d)
    e_mid = int(wb[1]) + 11; e_c0 = int(wb[3]) - 2; e_cl = int(wb[5]) + 1; e_ov = int(wb[7]); e_out = int(wb[9]) + 2
    t = d.copy()
    for q in (e_mid, e_c0, e_cl, e_ov, e_out): t = sub(t, q)
    t = delete(t, 9)
    def reopened(W):
        w = W[0]; L = w["last"]
        return w["rounds"] >= 2 and len(L["tpl"]) == len(w["tpl"]) - 1 and sum(1 for c in range(6, 13) if w["ev"][c + (c >= 9)] and not L["ev"][c]) >= 1 and min(w["g"]) < 0
    def spread_ok(W):
        ok = g_at(W, 1, e_mid) == -8 and not ev_at(W, 1, e_mid - 3) and not ev_at(W, 1, e_mid + 3) and ev_at(W, 1, e_mid - 4) and ev_at(W, 1, e_mid + 4)
        ok = ok and col(W, 3, e_c0) == 0 and not ev_at(W, 3, e_c0 + 3) and ev_at(W, 3, e_c0 + 4) and col(W, 2, e_c0) == len(W[2]["tpl"]) - 4 and not ev_at(W, 2, e_c0 - 3) and ev_at(W, 2, e_c0 - 4)
        ok = ok and col(W, 4, e_cl) == len(W[4]["tpl"]) - 1 and not ev_at(W, 4, e_cl - 3) and ev_at(W, 4, e_cl - 4) and col(W, 5, e_cl) == 3 and not ev_at(W, 5, e_cl + 3) and ev_at(W, 5, e_cl + 4)
        ok = ok and col(W, 6, e_ov) == len(W[6]["tpl"]) - 2 and col(W, 7, e_ov) == 2 and not ev_at(W, 6, e_ov - 3) and not ev_at(W, 7, e_ov + 3)
        return ok
    def outside_ok(W):
        J = len(W[8]["tpl"])
        return W[8]["we"] == e_out and all(W[8]["ev"][J - k] for k in (1, 2, 3)) and not ev_at(W, 9, e_out - 1) and all(W[8]["last"]["skipped"][J - k] for k in (3, 4))
    Z.append(Zmw("spread", "spread", d, make_passes("spread", t, 8), [
        ("a dirty majority spreads over 3 columns and not 4: mid-window, from column 0, from column J - 1, from the overhang", spread_ok),
        ("a dirty majority just outside a window's template does not count for that window", outside_ok),
        ("a deletion at a run start re-opens positions within 3 that carried evidence", reopened),
        ("every draft error is repaired", lambda W, t=t: np.array_equal(np.concatenate([w["core"] for w in W]), t))]))

    # masks: 8 passes, single dirty bits on each side of the b - 2 and b + 2 edge columns of a middle window (the second and third interval mask of a window), and in
    # the first and the last window (two intervals each); each dirty bit in its own pass, g = 6 there and 8 beside
    t = template("masks", 132); wb = O.windows(t)
    b = int(wb[3]); sites = [b - 3, b - 2, b + 1, b + 2, int(wb[1]) - 3, int(wb[1]) + 2, 1, int(wb[-2]) + 2, len(t) - 2]
    def masks_ok(W):
        for q in sites:
            for w in range(len(W)):
                if W[w]["ws"] <= q < W[w]["we"] and g_at(W, w, q) != 6: return False
        return all(g in (6, 8) for w in W for g in w["g"]) and sum(1 for w in W for g in w["g"] if g == 6) >= len(sites)
    def subs(at): return lambda t: [t := sub(t, q) for q in at][-1]
    Z.append(Zmw("masks", "mask composition", t, make_passes("masks", t, 8, {k: subs(sites[k::8]) for k in range(8)}), [
        ("g = 6 at every planted site (both sides of b - 2 and b + 2; first and last window), 8 elsewhere", masks_ok)]))

    # one window: Ld = 26 <= 28, 8 passes, one dirty bit
    t = template("one", 26)
    Z.append(Zmw("one_window", "mask composition", t, make_passes("one", t, 8, {2: lambda t: sub(t, 17)}), [
        ("one window of 26 columns without flanks, g = 6 at column 17", lambda W: len(W) == 1 and len(W[0]["tpl"]) == 26 and W[0]["lf"] == 4 and W[0]["rf"] == 4 and W[0]["g"][17] == 6 and W[0]["g"][16] == 8)]))

    # travel: a window that needs an insertion and, 8 columns to its right, a deletion in round 0 (applied in descending order: the deletion first); an insertion exactly
    # at a core start and one exactly at a core end; a last window of 30 columns that needs an insertion (J reaches 31, evidence moves into bit 31)
    for L in range(190, 190 + 23 * 12):
        d = template(f"travel{L}", 190 + L % 23); wb = O.windows(d)
        a = int(wb[1]) + 5; cst = int(wb[4]); ain = len(d) - 12
        if len(d) - int(wb[-2]) + 2 == 30 and d[a + 7] != d[a + 9]: break
    else: raise AssertionError("travel: no draft with a 30-column last window")
    tt = insert(d, ain, [other(d[ain - 1], d[ain])])            # the draft lacks a base of its last window
    tt = insert(tt, cst, [other(d[cst - 1], d[cst])])           # ... and a base between the core of window 3 and the core of window 4
    tt = delete(tt, a + 8)                                      # it has an extra base 8 columns right of ...
    tt = insert(tt, a, [other(d[a - 1], d[a])])                 # ... a base it lacks
    def travel_ok(W):
        w = W[1]
        return w["rounds"] >= 2 and len(w["core"]) == w["ce"] - w["cs"] and not np.array_equal(w["core"], w["tpl"][w["cs"]:w["ce"]])
    Z.append(Zmw("travel", "travel", d, make_passes("travel", tt, 8), [
        ("window 1 applies an insertion and a deletion", travel_ok),
        ("an insertion exactly at a core start: it belongs to window 4, not to window 3", lambda W: len(W[4]["core"]) == W[4]["ce"] - W[4]["cs"] + 1 and len(W[3]["core"]) == W[3]["ce"] - W[3]["cs"]
            and len(W[3]["last"]["tpl"]) == len(W[3]["tpl"]) + 1),
        ("the last window has 30 columns and reaches 31 by an applied insertion", lambda W: len(W[-1]["tpl"]) == 30 and len(W[-1]["last"]["tpl"]) == 31),
        ("every draft error is repaired", lambda W: np.array_equal(np.concatenate([w["core"] for w in W]), tt))]))

    # groups: 33, 40 and 70 passes; the dirty passes of one position are planted ONLY in the second / third group of 32; a junk pass in each group (the usable count
    # differs per group); a pass with a 40-base block (split, and its segment trimmed) in a later group; foreign sequence in one window of a forward pass, of a reverse
    # pass, and of a pass with index >= 32
    for n, dirty_in, junk, blockpass, zf, zr in ((33, (32,), (3,), None, 4, None), (40, (33, 36, 39), (5, 34), 37, None, 35), (70, (64, 66, 69), (7, 40, 65), 67, 38, 41)):
        if n == 40:      # a run of 3 in window 0 and one in window 4 (see `minority` below)
            def p40(t0, wb0):
                dd = run_at(run_at(t0, int(wb0[0]) + 8, 3), int(wb0[4]) + 5, 3); q = int(wb0[4]) + 5
                return (dd, None) if len({int(dd[q]), int(dd[q + 3]), int(dd[q + 4]), int(dd[q + 5])}) == 4 else None      # (run, the base after it, the doubled base and its successor all differ)
            wb, d, _ = stable("groups40", 110, p40)
        else:
            d = template(f"groups{n}", 88 if n == 70 else 110); wb = O.windows(d)
        pd = int(wb[1]) + 6; wz = 2; atb = int(wb[3]) + 4
        r0, s4 = int(wb[0]) + 8, int(wb[-2]) + 5
        # (40 passes: a draft error in the z window — a mutation is applied there and the drop must outlast it; and every pass has the run of window 4 with 2 bases)
        t = delete(sub(d, int(wb[wz]) + 12), s4) if n == 40 else d
        fzz = list(range(int(wb[wz]) + 2, int(wb[wz + 1]) - 2))          # foreign sequence over the window's core, out of the neighbouring windows' sight
        mild = [int(wb[wz]) + 4 + 3 * k for k in range(5)]; zm = 8          # five substitutions in pass 8: kept at -3.4, dropped at -1.0
        mods_mild = lambda t, mild=mild: foreign(t, mild)
        mods = {k: (lambda t, pd=pd: sub(t, pd)) for k in dirty_in}
        if blockpass is not None: mods[blockpass] = lambda t, atb=atb, n=n: insert(t, atb, blk(f"groups{n}/b", 40))
        for k in (zf, zr):
            if k is not None: mods[k] = lambda t, fzz=fzz: foreign(t, fzz)
        mods[zm] = mods_mild
        pmaj = int(wb[3]) + 9
        if n == 70:      # every pass of the second and third group carries a substitution the first group does not: a dirty majority (36 of 67) that the first group alone would call clean
            for k in range(32, n): mods[k] = (lambda t, f=mods.get(k), pmaj=pmaj: sub(f(t) if f else t, pmaj)) if k != blockpass else (lambda t, f=mods[k], pmaj=pmaj: f(sub(t, pmaj)))
        zp = [k for k in (zf, zr) if k is not None]
        nuse = n - len(junk)
        # 40 passes: a MINORITY of 15 usable passes (with the split pass 16 of 38 dirty: g = 6, evidence stays) that the likelihood follows all the same, because a
        # pulse width of 3 on an extra base makes a supporting read gain about 4 bits where an opposing read loses about 2.3 (substitutions are symmetric: only a
        # length change can be planted like this).  They have (a) the run of window 0 with 4 bases: a QUIET run that really needs a length change — the insertion lane
        # at its first base must find it; (b) the base 4 columns after the start of window 4's run twice (one base lies between it and the run, so that no single mismatch explains run and doubling together): a skipped position (evidence, no homopolymer, 4 columns from
        # the dirty majority at the run's start) whose insertion lane exists only after the deletion at the run's start has re-opened the positions within 3 of it
        minority = [0, 1, 2, 3, 4, 6, 7, 9, 10, 11, 12, 13, 14, 15, 16] if n == 40 else []
        longer = lambda t, r0=r0, s4=s4: insert(insert(t, s4 + 3, [t[s4 + 3]]), r0, [t[r0]])
        for k in minority: mods[k] = longer
        checks = [
            (f"g = n_use - 2 * {len(dirty_in)} at the planted column: every dirty pass sits in a later group",
             lambda W, pd=pd, nuse=nuse, k=len(dirty_in), b=int(blockpass is not None), lo=min(dirty_in): g_at(W, 1, pd) == nuse - 2 * (k + b) and g_at(W, 1, pd + 1) == nuse - 2 * b and lo >= 32),
            ("a junk pass in each group has no segment", lambda W, junk=junk: all(not w["seg"][k] for w in W for k in junk)),
            ("the planted passes are dropped by z-score in their window only", lambda W, zp=zp, wz=wz: all([bool(w["zdrop"][k]) for w in W] == [i == wz for i in range(len(W))] for k in zp)),
            ("the pass with five substitutions is kept at -3.4", lambda W, zm=zm: not any(w["zdrop"][zm] for w in W) and all(w["seg"][zm] for w in W)),
            ("a forward / reverse / second-word pass is among the dropped", lambda W, zf=zf, zr=zr, n=n: (zf is None or (zf % 2 == 0)) and (zr is None or zr % 2 == 1) and max(k for k in (zf, zr) if k is not None) >= (32 if n > 33 else 0))]
        if n == 40:
            checks.append(("a quiet run start (g = 6: 15 passes and the split pass dirty, of 38) needs a length change and its insertion lane finds it in round 0",
                           lambda W, r0=r0: g_at(W, 0, r0) == 6 and ev_at(W, 0, r0) and g_at(W, 0, r0 + 1) == 36 and min(W[0]["g"]) == 6 and W[0]["rounds"] == 2 and len(W[0]["core"]) == W[0]["ce"] - W[0]["cs"] + 1))
            checks.append(("round 1 of the last window applies an insertion at a position that carried evidence outside a homopolymer: enumerated only because the deletion 4 columns to its left re-opened it",
                           lambda W, s4=s4, d=d: g_at(W, -1, s4) == -38 and g_at(W, -1, s4 + 4) == 6 and ev_at(W, -1, s4 + 4) and not ev_at(W, -1, s4 + 3) and d[s4 + 4] not in (d[s4 + 3], d[s4 + 5])
                           and W[-1]["rounds"] == 3 and len(W[-1]["core"]) == W[-1]["ce"] - W[-1]["cs"]))
            checks.append(("the consensus is the minority's sequence where the likelihood follows it", lambda W, t=t, longer=longer: np.array_equal(np.concatenate([w["core"] for w in W]), longer(t))))
            checks.append(("a mutation is applied in the z window and the dropped pass stays dropped in the round after it", lambda W, wz=wz, zr=zr, nuse=nuse: W[wz]["rounds"] == 2 and W[wz]["last"]["n_use"] == nuse - 1
                           and not np.array_equal(W[wz]["core"], W[wz]["tpl"][W[wz]["cs"]:W[wz]["ce"]])))
        if n == 70:
            checks.append(("36 of 67 usable passes, all in the second and third group, are dirty at one column: g = -5, and the polish follows them",
                           lambda W, pmaj=pmaj, d=d: g_at(W, 3, pmaj) == -5 and W[3]["rounds"] == 2 and W[3]["core"][pmaj - int(W[3]["ws"]) - W[3]["cs"]] != d[pmaj]))
        if blockpass is not None:
            checks.append(("a trimmed segment in a later group", lambda W, k=blockpass: k >= 32 and any(w["trimmed"][k] for w in W) and all(all(w["dirty"][k]) for w in W)))
        Z.append(Zmw(f"groups{n}", "groups, z drop", d, make_passes(f"groups{n}", t, n, mods, junk=junk, pw_const={k: 3 for k in minority}), checks,
                     zchecks={0.0: [("with the gate off nothing is dropped", lambda W: not any(any(w["zdrop"]) for w in W))],
                              -1.0: [("at -1.0 the pass with five substitutions is dropped too, in its window only", lambda W, zm=zm, wz=wz, zp=zp: all([bool(w["zdrop"][k]) for w in W] == [i == wz for i in range(len(W))] for k in zp + [zm]))]},
                     planted_z=[(wz, k) for k in zp + [zm]] + [(wz, k + 2) for k in zp + [zm] if k + 2 < n and k + 2 not in junk and k + 2 not in mods]))

    # split8 / partial: 8 clean passes, one with a 60-base block (g = 9 - 2 = 7 where it has a segment) and a partial pass that reaches half the draft (dirty everywhere:
    # n_use and g differ between the windows it reaches and the others)
    t = template("split8", 200); wb = O.windows(t); at = int(wb[6]) + 5; half = int(wb[4]) + 3
    Z.append(Zmw("split8_partial", "dirty everywhere", t, make_passes("split8", t, 9, {6: lambda t: insert(t, at, blk("split8/b", 60))}, extra=[(t[:half].copy(), PARTIAL)]), [
        ("split and partial pass are dirty everywhere", lambda W: all(all(w["dirty"][6]) and (not w["seg"][9] or all(w["dirty"][9])) for w in W)),
        ("g = 7 where only the split pass reaches, 6 where the partial pass does too; both kinds occur", lambda W: all(set(w["g"]) == {9 + int(w["seg"][9]) - 2 * (1 + int(w["seg"][9]))} for w in W if w["seg"][6])
            and {bool(w["seg"][9]) for w in W} == {True, False}),
        ("usable reads: 10 in the windows the partial pass reaches, of them 9 full-length", lambda W: all((w["last"]["n_use"], w["last"]["n_full"]) == ((10, 9) if w["seg"][9] else (9, 9)) for w in W if w["seg"][6] and not w["trimmed"][6]))]))
    return Z


@lru_cache(maxsize=None)
def lab():
    Z = build()
    # drafts of 60-200 bases but for: one_window (26: the class is Ld <= 28); spread (220: five spread sites two windows apart from each other and from the re-opened run,
    # one of them beside a window without any: ten windows); travel (190-212: the first length at which the seeded draft ends in a 30-column window).  80-odd windows in all.
    assert len(Z) <= 14 and all(60 <= len(z.draft) <= 200 or z.name in ("one_window", "spread", "travel") for z in Z) and all(len(z.passes) <= 70 for z in Z)
    assert len(Z[[z.name for z in Z].index("spread")].draft) == 220 and len(Z[[z.name for z in Z].index("travel")].draft) <= 212 and sum(len(O.windows(z.draft)) - 1 for z in Z) <= 90
    return Z


def batch_of(zmws):
    reads = [r for z in zmws for r in z.passes]; n = len(zmws)
    return api.Batch(np.arange(n, dtype=np.int32), np.tile(np.array(SNR0, np.float32), (n, 1)), np.concatenate([[0], np.cumsum([len(z.passes) for z in zmws])]).astype(np.int32),
                     np.concatenate([[0], np.cumsum([len(r[0]) for r in reads])]).astype(np.int64), np.ascontiguousarray(np.concatenate([r[0] for r in reads])),
                     np.ascontiguousarray(np.concatenate([r[1] for r in reads])), np.full(sum(len(r[0]) for r in reads), 5, np.uint8), np.array([r[2] for r in reads], np.uint8))


def opts(max_qv=50, min_zscore=-3.4):
    """the product's defaults (heuristics on, z-score gate on) but for the knobs the runs vary, min_rq, which would only hide a ZMW, and top_passes 0 = all passes (the
    default of 60 would keep the 70-pass ZMW out of the third group of 32)"""
    o = api.default_opts(); o.min_rq = 0.0; o.top_passes = 0; o.max_qv = max_qv; o.min_zscore = min_zscore
    return o


def cut(draft, wb, passes, al, maxins=30):
    """The windows of one ZMW and, per pass, the segment scored there (the segment and trim rules of DESIGN.md §2 restated as in arrow_ref.collect_stage) with the pass's dirty
    flags on the window's columns.  al[r] = (rstart, valid, dirty[Ld]) in draft orientation.  Per window: ws, we, tpl, lf, rf, cs, ce, reads (obs codes or None), seg (the
    pass has a usable segment: what n_use counts), strands, full, trimmed, dirty (rows [R][J])."""
    Ld = len(draft); out = []
    for w in range(len(wb) - 1):
        ws, we = max(0, int(wb[w]) - 2), min(Ld, int(wb[w + 1]) + 2); J = we - ws
        rec = dict(ws=ws, we=we, tpl=draft[ws:we].copy(), lf=int(draft[ws - 1]) if ws > 0 else 4, rf=int(draft[we]) if we < Ld else 4, cs=int(wb[w]) - ws, ce=int(wb[w + 1]) - ws,
                   reads=[], seg=[], strands=[], full=[], trimmed=[], dirty=[])
        for (bases, pw, fl), (rs, v, dirty) in zip(passes, al):
            rev = int((fl & 1) != (passes[0][2] & 1))
            rec["strands"].append(rev); rec["full"].append(not fl & PARTIAL); rec["dirty"].append([int(x) for x in dirty[ws:we]])
            n = int(rs[we] - rs[ws]) if v else -1
            obs, trimmed = None, False
            if v and 0 <= n <= len(bases):
                na = len(bases) - int(rs[we]) if rev else int(rs[ws])
                sb, sp = bases[na:na + n], pw[na:na + n]
                if maxins > 0 and n > J + maxins:
                    keep = A.trim_segment(sb, A.revcomp(rec["tpl"]) if rev else rec["tpl"]); obs, trimmed = A.obs_codes(sb[keep], sp[keep]), True
                elif n <= A.IMAX: obs = A.obs_codes(sb, sp)
            rec["reads"].append(obs); rec["seg"].append(obs is not None); rec["trimmed"].append(trimmed)
        out.append(rec)
    return out


def cut_oracle(z):
    """the windows of lab ZMW z cut with the restatement's own alignments (O.windows, O.route): the CPU side"""
    d = z.draft; al = []
    for bases, pw, fl in z.passes:
        b = rc(bases) if fl & 1 else bases
        name, rs, v, sc, dirty = O.route(b, d, partial=((fl >> 2) & 1) ^ (fl & 1) if fl & PARTIAL else None)
        al.append((np.asarray(rs, np.int64), bool(v), dirty))
    return cut(d, O.windows(d), z.passes, al)


def cut_engine(handle, batch, zi, z):
    """the same from the engine's stage outputs of the run it just made (ccsx_stage_windows, ccsx_stage_align_ev) on ZMW index zi of `batch`"""
    d = handle.stage_draft(zi); wb = handle.stage_windows(zi)
    assert np.array_equal(d, z.draft), f"zmw {z.name}: the engine did not polish the draft it was handed"
    r0 = int(batch.read_off[zi]); al = []
    for k in range(len(z.passes)):
        rs, v, sc, dirty = handle.stage_align_ev(r0 + k, len(d))
        al.append((np.asarray(rs, np.int64), bool(v), dirty))
    return cut(d, wb, z.passes, al)


_CACHES = {}


def caches_for(z, W):
    """one gains cache per window of lab ZMW z, kept for the process and shared by every run on the SAME segments (the key holds them)"""
    out = []
    for wi, w in enumerate(W):
        key = (z.name, wi, w["tpl"].tobytes(), tuple(w["strands"]), tuple(None if o is None else o.tobytes() for o in w["reads"]))
        out.append(_CACHES.setdefault(key, {}))
    return out


def reference(model, W, qv_only, max_qv, min_zscore, caches, filtered=True):
    """arrow_ref.filter_margins and polish_ref on every window of one ZMW (W from cut_*; filtered = False: evidence all false, the heuristics switched off), in place: g, ev, p_skip, core, rounds, amb, last, zdrop (per pass of the ZMW),
    z_und (passes whose z decision is undecided), p / qv / floor per core base of the last round.  caches: one dict per window, shared by the runs."""
    t64 = A.tables64(model, SNR0)
    for w, cache in zip(W, caches):
        J = len(w["tpl"])
        w["g"], w["ev"], w["p_skip"] = A.filter_margins(w["dirty"], w["seg"], J, max_qv)
        if not filtered: w["ev"] = [False] * J
        idx = [r for r, o in enumerate(w["reads"]) if o is not None]
        core, rounds, amb, last = A.polish_ref_ev(t64, w["tpl"], w["lf"], w["rf"], w["cs"], w["ce"], [w["reads"][r] for r in idx], [w["strands"][r] for r in idx],
                                               ev=w["ev"], p_skip=w["p_skip"], min_zscore=min_zscore, zmodel=(model, SNR0), full=[w["full"][r] for r in idx], qv_only=qv_only, cache=cache)
        w.update(core=core, rounds=rounds, amb=amb, last=last, idx=idx)
        w["zdrop"] = [False] * len(w["reads"]); w["z_und"] = [idx[r] for r in last["z_undecided"]]
        for k, r in enumerate(idx): w["zdrop"][r] = bool(last["zdrop"][k])
        _, w["p"], w["qv"], w["floor"] = A.perr(last["delta"], last["valid"], last["tpl"], w["lf"], w["rf"], last["cs"], last["ce"], last["n_use"], max_qv,
                                              skipped=last["skipped"], quiet=last["quiet"], p_skip=last["p_skip"])
    return W


QV_SLACK = 3.0103 * 2e-5 + 1e-5          # as tests/test_arrow_gpu.py check_raw_qvs: det_log2's 2e-5 in QV units, float32 rounding of a value <= 93


def check_window_qvs(raw, w, max_qv, S, tag):
    """raw: the engine's (or restatement's) raw QVs of this window's core.  A base the reference calls SKIPPED must report clamp(-10 log10 max(p_skip, floors), 0, 93) within
    QV_SLACK; every other base must lie inside the propagated bound of its float64 error probability, a quiet base's sum starting at p_skip.  This is the witness that what
    was skipped is what the SPEC says and nothing else.  S counts bases, left_out, skipped, quiet."""
    L = w["last"]; g = L["gains"]; use = L["use"]; n = L["n_use"]; bound = n * A.PER_READ; J = len(L["tpl"])
    lens = np.array([len(w["reads"][r]) for r in w["idx"]], np.int64).reshape(-1, 1)
    scaled = g["mut"] + 2 * lens if len(w["idx"]) else g["mut"]
    assert len(raw) == L["ce"] - L["cs"], f"{tag}: core of {len(raw)} bases, reference {L['ce'] - L['cs']}"
    for k, c in enumerate(range(L["cs"], L["ce"])):
        q = float(raw[k]); S["bases"] += 1; fl = float(w["floor"][k])
        if L["skipped"][c]:
            S["skipped"] += 1
            want = min(93.0, max(0.0, -10 * np.log10(max(L["p_skip"][c], fl))))
            assert abs(q - want) <= QV_SLACK, f"{tag} column {c}: the reference SKIPS this base (p_skip {L['p_skip'][c]:.3g}, floor {fl:.3g} -> QV {want:.4f}) but the QV is {q:.4f}: the filter skipped something else than the SPEC says"
            continue
        lanes_c = A.base_lanes(L["valid"], c, J)
        clean = all(n == 0 or (bool(np.all(scaled[use, m] > A.LOG2_TINY)) and bool(np.all(np.abs(g["d"][use, m]) < A.DQ_CLAMP - A.PER_READ))) for m in lanes_c)
        if not clean: S["left_out"] += 1; continue
        s_lo = sum(2.0 ** min(float(L["delta"][m]) - bound, 20.0) for m in lanes_c); s_hi = sum(2.0 ** min(float(L["delta"][m]) + bound, 20.0) for m in lanes_c)
        if L["quiet"][c]: S["quiet"] += 1; s_lo += L["p_skip"][c] * (1 - A.FLOOR_F32); s_hi += L["p_skip"][c] * (1 + A.FLOOR_F32)
        p_lo, p_hi = s_lo / (1 + s_lo) * (1 - A.P_F32), s_hi / (1 + s_hi) * (1 + A.P_F32)
        p_lo, p_hi = max(p_lo, fl * (1 - A.FLOOR_F32)), max(p_hi, fl * (1 + A.FLOOR_F32))
        q_hi = min(93.0, max(0.0, -10 * np.log10(p_lo))) + QV_SLACK; q_lo = min(93.0, max(0.0, -10 * np.log10(p_hi))) - QV_SLACK
        assert q_lo <= q <= q_hi, (f"{tag} column {c}: QV {q:.4f} outside [{q_lo:.4f}, {q_hi:.4f}] of the reference ({'quiet: the sum starts at p_skip' if L['quiet'][c] else 'not skipped'}; "
                                   f"{len(lanes_c)} lanes, {n} usable reads): the filter enumerated other lanes than the SPEC says")


def _mode(xs):
    return min(set(xs), key=lambda v: (-xs.count(v), v))


def compare_run(res, zi_of, W_of, qv_only, max_qv, tag, core_len=None, zmws=None):
    """results of one run (engine or restatement) against the reference windows W_of[name] (after F.reference): per window core and raw QVs, per ZMW np / ec / iters / status.
    core_len(name, wi): the run's own core length of a window where it is known (the engine's wmeta); else it follows from the ZMW's length and the other windows.
    Returns the counts (windows, ambiguous, bases, left_out, skipped, quiet, pairs, undecided)."""
    S = dict(windows=0, ambiguous=0, bases=0, left_out=0, skipped=0, quiet=0, pairs=0, undecided=0)
    for z in (lab() if zmws is None else zmws):
        zi = zi_of[z.name]; W = W_of[z.name]; seq, raw = res.sequence(zi), res.raw(zi)
        assert int(res.status[zi]) == 0, f"{tag} zmw {z.name}: status {int(res.status[zi])}"
        out = [w["amb"] or bool(w["z_und"]) for w in W]
        lens = [None if o else len(w["core"]) for w, o in zip(W, out)]
        if core_len is not None: lens = [core_len(z.name, wi) for wi in range(len(W))]
        elif out.count(True) == 1: lens[out.index(True)] = len(seq) - sum(n for n in lens if n is not None)
        pos = 0
        for wi, (w, o) in enumerate(zip(W, out)):
            S["windows"] += 1; S["pairs"] += len(w["idx"]); S["undecided"] += len(w["z_und"]); n = lens[wi]
            where = f"{tag} zmw {z.name} ({z.cls}) window {wi}"
            if o:
                S["ambiguous"] += 1; S["bases"] += w["ce"] - w["cs"]; S["left_out"] += w["ce"] - w["cs"]
                if n is None: break                                           # (two left-out windows in one ZMW and no core lengths: the rest cannot be placed)
                pos += n; continue
            assert n == len(w["core"]) and np.array_equal(seq[pos:pos + n], w["core"]), f"{where}: core differs from the reference's ({w['rounds']} rounds)"
            check_window_qvs(raw[pos:pos + n], w, max_qv, S, where)
            pos += n
        else:
            assert pos == len(seq), f"{tag} zmw {z.name}: {pos} bases placed, {len(seq)} reported"
        if not any(out):
            assert int(res.np_[zi]) == _mode([w["last"]["n_full"] for w in W]), f"{tag} zmw {z.name}: np {int(res.np_[zi])}, reference {[w['last']['n_full'] for w in W]}"
            assert abs(float(res.ec[zi]) - np.mean([w["last"]["n_use"] for w in W])) < 1e-3, f"{tag} zmw {z.name}: ec {float(res.ec[zi])}, reference {[w['last']['n_use'] for w in W]}"
            assert int(res.iters[zi]) == sum(w["rounds"] for w in W), f"{tag} zmw {z.name}: {int(res.iters[zi])} rounds, reference {[w['rounds'] for w in W]}"
    return S


def assert_caps(S, W_of, tag):
    """the three left-out shares within their caps, no planted decision among the excused"""
    print(f"\n[filter lab] {tag}: windows {S['windows']}, left out as ambiguous {S['ambiguous']} ({100 * S['ambiguous'] / S['windows']:.1f} %, cap 5 %); core bases {S['bases']}, left out of the QV "
          f"check {S['left_out']} ({100 * S['left_out'] / S['bases']:.2f} %, cap 2 %); (pass, window) pairs {S['pairs']}, undecided z {S['undecided']} ({100 * S['undecided'] / S['pairs']:.2f} %, cap 2 %); "
          f"skipped bases {S['skipped']}, quiet {S['quiet']}")
    assert S["ambiguous"] <= 0.05 * S["windows"] and S["left_out"] <= 0.02 * S["bases"] and S["undecided"] <= 0.02 * S["pairs"]
    assert S["skipped"] > 0.5 * S["bases"] and S["quiet"] >= 10
    for z in lab():
        if z.name not in W_of: continue
        for wi, k in z.planted_z: assert k not in W_of[z.name][wi]["z_und"], f"zmw {z.name} window {wi} pass {k}: a planted z decision is undecided"
        if z.name in W_of and z.checks: assert not any(w["amb"] or w["z_und"] for w in W_of[z.name]), f"zmw {z.name} ({z.cls}): a window of a planted class is among the excused"


def run_checks(z, W, checks):
    for what, fn in checks:
        assert fn(W), f"zmw {z.name} ({z.cls}): the planted class did not occur — {what}"

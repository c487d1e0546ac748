"""CPU references for DESIGN.md §2 "Polisher hand-off" (rule version 1).

Two of them.  `handoff_batch` restates the rule in numpy on what the engine's stages produced (tests/pileup_ref.py: `collect_stage`, the segments of
`window_segments`, the vectorised kinetics alignment `diag_rows`) and gives every array ccsx_consensus_handoff fills.  `brute_window_cells` is an independent
brute force for hand-made windows: a plain Python DP whose explicit trace-back path, turned into SEQ orientation as a list of events, gives the cells — no
`rows` array and none of the r - r_prev arithmetic.  Nothing here calls a kernel."""
from __future__ import annotations

import numpy as np

from pileup_ref import IMAX, MATCH, MISMATCH, INS, DEL, Zmw, collect_stage, diag_rows, window_segments

NO_BASE, NO_SEGMENT = 4, 5


def row_passes(zmw: Zmw, max_rows: int) -> list:
    """the passes of the rows: the valid ones among the passes used, in batch order, at most max_rows"""
    return [p for p, (_, _, valid, _) in enumerate(zmw.reads) if valid][:max_rows]


def zmw_cells(zmws, passes, kin):
    """per ZMW the cells [len(passes[z]), L, 4] over its concatenated window cores.  passes[z]: the row passes (indices into zmws[z].reads); kin[z][p] = (pw,
    ip or None) of pass p in its native orientation"""
    segs, tpls, who = [], [], []
    for zi, z in enumerate(zmws):
        nw = len(z.tpls)
        for w in range(nw):
            t = np.asarray(z.tpls[w], np.int64)
            iws, iwe = (0 if w == 0 else 2 * w - 1), (2 * nw - 1 if w == nw - 1 else 2 * (w + 1))
            for k, p in enumerate(passes[zi]):
                one = window_segments(Zmw(z.tpls, z.cores, z.ref_strand, [z.reads[p]]), w)      # the kinetics' test of this pass alone
                if not one:
                    continue
                seg, st = one[0]
                bases, _, _, ent = z.reads[p]
                off = len(bases) - int(ent[iwe]) if st else int(ent[iws])
                segs.append(seg); tpls.append(3 - t[::-1] if st else t); who.append((zi, w, k, p, st, off))
    rows = diag_rows(segs, tpls) if segs else []
    starts = [np.concatenate([[0], np.cumsum([ce - cs for cs, ce in z.cores])]).astype(np.int64) for z in zmws]
    out = []
    for zi, z in enumerate(zmws):
        c = np.zeros((len(passes[zi]), int(starts[zi][-1]), 4), np.uint8)
        c[:, :, 0] = NO_SEGMENT
        out.append(c)
    for (zi, w, k, p, st, off), seg, rw in zip(who, segs, rows):
        cs, ce = zmws[zi].cores[w]
        o, J, n = int(starts[zi][w]), len(rw), len(seg)
        pw, ip = kin[zi][p]
        c = out[zi]
        c[k, o:o + ce - cs, 0] = NO_BASE
        prev = None
        for col in (range(J - 1, -1, -1) if st else range(J)):      # the template's columns from left to right in SEQ
            r = int(rw[col])
            if r < 0:
                continue
            jf = J - 1 - col if st else col
            if st:
                ins = prev - r - 1 if prev is not None else n - 1 - r
            else:
                ins = r - prev - 1 if prev is not None else r
            prev = r
            if cs <= jf < ce:
                b = int(seg[r])
                c[k, o + jf - cs] = (3 - b if st else b, pw[off + r], ip[off + r] if ip is not None else 0, ins)
    return out


def handoff_batch(zmws, quals, kin, tile_len: int, max_rows: int, skip_above: int, max_tiles: int) -> dict:
    """every array of ccsx_handoff_out for the slots that are written (min(selected, max_tiles) of them).  zmws: the Zmw records of the batch; quals[z]: the
    qual bytes of ZMW z's consensus (empty: none); kin[z][p]: (pw, ip or None) of its pass p"""
    T, R = int(tile_len), int(max_rows)
    total, sel = 0, []
    for z, q in enumerate(quals):
        q = np.asarray(q, np.int64)
        for t in range((len(q) + T - 1) // T):
            total += 1
            ln = min(T, len(q) - t * T)
            qs = int(q[t * T:t * T + ln].sum())
            if qs < skip_above * ln:
                sel.append((z, t * T, ln, qs))
    m = min(len(sel), int(max_tiles))
    need = sorted({z for z, _, _, _ in sel[:m]})
    passes = [row_passes(zmws[z], R) for z in need]
    cz = dict(zip(need, zmw_cells([zmws[z] for z in need], passes, [kin[z] for z in need])))
    pz = dict(zip(need, passes))
    out = dict(counts=np.array([total, len(sel)], np.int32), tile_zmw=np.zeros(m, np.int32), tile_start=np.zeros(m, np.int32), tile_len=np.zeros(m, np.int32),
               tile_qsum=np.zeros(m, np.int32), tile_rows=np.zeros(m, np.int32), row_pass=np.full((m, R), 255, np.uint8), row_strand=np.zeros((m, R), np.uint8),
               cells=np.zeros((m, R, T, 4), np.uint8))
    out["cells"][:, :, :, 0] = NO_SEGMENT
    for g, (z, start, ln, qs) in enumerate(sel[:m]):
        assert cz[z].shape[1] == len(quals[z]), "the window cores do not add up to the consensus"
        rows = pz[z]
        out["tile_zmw"][g], out["tile_start"][g], out["tile_len"][g], out["tile_qsum"][g], out["tile_rows"][g] = z, start, ln, qs, len(rows)
        out["row_pass"][g, :len(rows)] = rows
        out["row_strand"][g, :len(rows)] = [(int(zmws[z].reads[p][1]) ^ zmws[z].ref_strand) & 1 for p in rows]
        out["cells"][g, :len(rows), :ln] = cz[z][:, start:start + ln]
    return out


def batch_kin(batch, ipd: bool = True) -> list:
    """kin of every ZMW of an api.Batch: per pass its (pw, ipd) arrays (ipd None when the engine is given none)"""
    out = []
    for z in range(batch.n_zmw):
        ps = []
        for r in range(int(batch.read_off[z]), int(batch.read_off[z + 1])):
            a, b = int(batch.base_off[r]), int(batch.base_off[r + 1])
            ps.append((batch.pw[a:b], batch.ipd[a:b] if ipd else None))
        out.append(ps)
    return out


def from_engine(handle, batch, res, opts, max_tiles: int, ipd: bool = True):
    """the restatement on the stages of the synchronous run the handle has just made (ccsx_consensus_handoff): (expected arrays, the Zmw records)"""
    zmws = collect_stage(handle, batch)
    quals = [res.quals(z) for z in range(batch.n_zmw)]
    return handoff_batch(zmws, quals, batch_kin(batch, ipd), opts.tile_len, opts.max_rows, opts.skip_above, max_tiles), zmws


# ---------------------------------------------------------------- the brute force
def brute_path(seg, tpl) -> list:
    """the kinetics alignment of seg (rows) to tpl (columns) by a plain DP; its whole path from (0, 0) to (n, J) as events in path order: ('M', read row, column)
    for a DIAG cell, ('I', read row) for a read base without a column (UP, and the rows left when the walk reaches column 0), ('D', column) for a column
    without a read base (LEFT, and the columns left when the walk reaches row 0)"""
    n, J = len(seg), len(tpl)
    H = [[0] * (J + 1) for _ in range(n + 1)]
    mv = [[None] * (J + 1) for _ in range(n + 1)]
    for i in range(1, n + 1):
        H[i][0] = i * INS
    for j in range(1, J + 1):
        H[0][j] = j * DEL
    for i in range(1, n + 1):
        for j in range(1, J + 1):
            diag = H[i - 1][j - 1] + (MATCH if int(seg[i - 1]) == int(tpl[j - 1]) else MISMATCH)
            left, up = H[i][j - 1] + DEL, H[i - 1][j] + INS
            h = max(diag, left)
            mv[i][j] = "U" if up > h else ("D" if diag >= left else "L")
            H[i][j] = max(h, up)
    ev, i, j = [], n, J
    while i > 0 and j > 0:
        m = mv[i][j]
        if m == "D":
            ev.append(("M", i - 1, j - 1)); i -= 1; j -= 1
        elif m == "U":
            ev.append(("I", i - 1)); i -= 1
        else:
            ev.append(("D", j - 1)); j -= 1
    while i > 0:
        ev.append(("I", i - 1)); i -= 1
    while j > 0:
        ev.append(("D", j - 1)); j -= 1
    return ev[::-1]


def brute_window_cells(tpl, cs: int, ce: int, seg, st: int, pw, ip=None) -> np.ndarray:
    """the cells [ce - cs, 4] one pass gives on the core [cs, ce) of the window template tpl (SEQ orientation).  seg / pw / ip: the pass's segment in the window
    in the pass's own orientation; st: 1 when the pass is on the strand opposite to SEQ"""
    tpl = [int(x) for x in tpl]
    J, n = len(tpl), len(seg)
    out = np.zeros((ce - cs, 4), np.uint8)
    if n > IMAX:
        out[:, 0] = NO_SEGMENT
        return out
    out[:, 0] = NO_BASE
    ev = brute_path(seg, [3 - x for x in reversed(tpl)] if st else tpl)
    if st:                                                           # the same path read from the other end: SEQ orientation
        ev = [(e[0], e[1], J - 1 - e[2]) if e[0] == "M" else (("D", J - 1 - e[1]) if e[0] == "D" else e) for e in reversed(ev)]
    gap = 0                                                          # the pass's bases since its last base on a column (or since the segment's SEQ-left end)
    for e in ev:
        if e[0] == "I":
            gap += 1
        elif e[0] == "M":
            r, col = e[1], e[2]
            if cs <= col < ce:
                b = int(seg[r]) & 3
                out[col - cs] = (3 - b if st else b, pw[r], ip[r] if ip is not None else 0, gap)
            gap = 0
    return out


def single_window(tpl, cs, ce, segs):
    """a one-window Zmw of hand-made segments for zmw_cells: segs = [(segment in the pass's own orientation, st, pw, ip)].  Returns (Zmw, passes, kin)"""
    reads, kin = [], []
    for seg, st, pw, ip in segs:
        seg = np.asarray(seg, np.uint8)
        reads.append((seg, st, True, np.array([0, len(seg)], np.int64)))
        kin.append((np.asarray(pw, np.uint8), None if ip is None else np.asarray(ip, np.uint8)))
    return Zmw([np.asarray(tpl, np.uint8)], [(cs, ce)], 0, reads), list(range(len(segs))), kin

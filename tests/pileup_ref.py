"""CPU restatement of DESIGN.md §2 "Pileup summary" (rule version 1), operation for operation, in numpy.

It takes what the engine's stages produced (the passes used and their entry rows, the strand reference, the converged window templates with their cores)
and computes the three per-base planes ccsx_consensus_pileup reports: coverage (sa before run-length encoding), matches (sm) and mismatches (sx).  The
segment alignments are the kinetics alignment (DESIGN.md §2 "HiFi kinetics"), vectorised across segments.  The inputs come from the engine
(`collect_stage`, after a ccsx_consensus_pileup call) or are made by hand (tests/test_pileup.py); nothing here calls a kernel.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

IMAX, OVERHANG = 63, 2
MATCH, MISMATCH, INS, DEL = 3, -5, -4, -4


@dataclass
class Zmw:
    """one ZMW's inputs: per window the converged template (J bases) and its core [cs, ce); the strand reference (flags bit 0 of the backbone pass);
    per used pass its native bases, flags, validity and the entry rows of its 2 nw window-edge columns"""
    tpls: list
    cores: list
    ref_strand: int
    reads: list = field(default_factory=list)     # (bases (native orientation), flags, valid, ent[2 nw])


class Read(tuple):
    """a pass of a Zmw: the 4-tuple (bases, flags, valid, ent) every reader of Zmw.reads unpacks, which also carries the pass's `ipd` and `pw` code bytes
    (native orientation, one per base) for tests/kinetics_ref.py"""

    def __new__(cls, bases, flags, valid, ent, ipd=None, pw=None):
        self = super().__new__(cls, (bases, flags, valid, ent))
        self.ipd, self.pw = ipd, pw
        return self


def diag_rows(segs, tpls, chunk=50_000):
    """global alignment of every segment to its template with the kinetics rule: H[i][0] = -4i, H[0][j] = -4j, diag = H[i-1][j-1] + (3 | -5),
    left = H[i][j-1] - 4, up = H[i-1][j] - 4, h = max(diag, left), cell = max(h, up); move UP iff up > h, else DIAG iff diag >= left, else LEFT.  The
    trace-back walks from (n, J) while both are > 0.  Returns per segment an int array [J]: the read row a DIAG cell puts on each column, or -1."""
    out = []
    for c0 in range(0, len(segs), chunk):
        S_, T_ = segs[c0:c0 + chunk], tpls[c0:c0 + chunk]
        N = len(S_)
        I = np.array([len(s) for s in S_], np.int64); J = np.array([len(t) for t in T_], np.int64)
        Im, Jm = max(int(I.max()), 1), max(int(J.max()), 1)
        S = np.full((N, Im), 255, np.int16); T = np.full((N, Jm), 254, np.int16)
        for k in range(N):
            S[k, :I[k]] = S_[k]; T[k, :J[k]] = T_[k]
        mv = np.zeros((N, Im + 1, Jm + 1), np.int8)           # 0 DIAG, 1 LEFT, 2 UP
        prev = np.tile(np.arange(Jm + 1, dtype=np.int32) * DEL, (N, 1))
        for i in range(1, Im + 1):
            cur = np.empty_like(prev)
            cur[:, 0] = i * INS
            rb = S[:, i - 1]
            for j in range(1, Jm + 1):
                diag = prev[:, j - 1] + np.where(rb == T[:, j - 1], MATCH, MISMATCH)
                left = cur[:, j - 1] + DEL
                up = prev[:, j] + INS
                h = np.maximum(diag, left)
                m = np.where(up > h, 2, np.where(diag >= left, 0, 1)).astype(np.int8)
                cur[:, j] = np.maximum(h, up)
                mv[:, i, j] = m
            prev = cur
        rows = np.full((N, Jm), -1, np.int64)
        i, j, idx = I.copy(), J.copy(), np.arange(N)
        while True:
            act = (i > 0) & (j > 0)
            if not act.any():
                break
            m = np.where(act, mv[idx, i, j], -1)
            d = act & (m == 0)
            rows[idx[d], j[d] - 1] = i[d] - 1
            i = np.where(act & (m != 1), i - 1, i)
            j = np.where(act & (m != 2), j - 1, j)
        out += [rows[k, :J[k]] for k in range(N)]
    return out


def window_segments(zmw: Zmw, w: int):
    """the segments of window w: (oriented read segment, strand) of every pass that counts there (valid, 0 <= n <= IMAX; k_kinetics' test)"""
    nw = len(zmw.tpls)
    iws, iwe = (0 if w == 0 else 2 * w - 1), (2 * nw - 1 if w == nw - 1 else 2 * (w + 1))
    out = []
    for bases, flags, valid, ent in zmw.reads:
        if not valid:
            continue
        a, b = int(ent[iws]), int(ent[iwe])
        n = b - a
        if n < 0 or n > IMAX:
            continue
        st = (int(flags) ^ zmw.ref_strand) & 1
        L = len(bases)
        off = L - b if st else a                                # the segment in the read's own orientation, aligned to the template in that orientation
        assert 0 <= off and off + n <= L, "a segment outside its pass (the engine would read a neighbouring pass's bases)"
        out.append((np.asarray(bases[off:off + n], np.int64) & 3, st))
    return out


def pileup_zmws(zmws):
    """(coverage, matches, mismatches) per ZMW: uint8 planes over the concatenated window cores (orientation of the consensus)"""
    segs, tpls, where = [], [], []
    for zi, z in enumerate(zmws):
        for w, t in enumerate(z.tpls):
            t = np.asarray(t, np.int64)
            trc = 3 - t[::-1]
            for seg, st in window_segments(z, w):
                segs.append(seg); tpls.append(trc if st else t); where.append((zi, w, st))
    rows = diag_rows(segs, tpls) if segs else []
    cnt = [[np.zeros((3, len(t)), np.int64) for t in z.tpls] for z in zmws]
    for (zi, w, st), seg, t, rw in zip(where, segs, tpls, rows):
        c = cnt[zi][w]
        c[0] += 1                                                # coverage: every counted pass, on every column
        J = len(t)
        for col in np.flatnonzero(rw >= 0):
            jf = J - 1 - col if st else col
            c[1 if seg[rw[col]] == t[col] else 2, jf] += 1
    out = []
    for z, cz in zip(zmws, cnt):
        parts = [cz[w][:, cs:ce] for w, (cs, ce) in enumerate(z.cores)]
        p = np.concatenate(parts, axis=1) if parts else np.zeros((3, 0), np.int64)
        assert p.max(initial=0) <= 255
        out.append(tuple(p[k].astype(np.uint8) for k in range(3)))
    return out


def need_cols(wb, Ld):
    """the window-edge column of every entry-row index (k_align's list: 0, b1-2, b1+2, ..., Ld)"""
    nw = len(wb) - 1
    return [0 if k == 0 else (Ld if k == 2 * nw - 1 else int(wb[(k + 1) >> 1]) + (-OVERHANG if k & 1 else OVERHANG)) for k in range(2 * nw)]


def collect_stage(handle, batch, zmws=None):
    """the engine's stage outputs after a ccsx_consensus_pileup call (ccsx_stage_polished / _draft / _windows / _align) as Zmw records"""
    out = []
    for z in (range(batch.n_zmw) if zmws is None else zmws):
        tpl, meta, nused, bb = handle.stage_polished(z)
        nw = len(meta)
        reads = []
        if nw:
            d = handle.stage_draft(z)
            wb = handle.stage_windows(z)
            assert len(wb) == nw + 1
            cols = need_cols(wb, len(d))
            r0 = int(batch.read_off[z])
            for r in range(r0, r0 + nused):
                rs, v, _ = handle.stage_align(r, len(d))
                a, b = int(batch.base_off[r]), int(batch.base_off[r + 1])
                reads.append(Read(batch.bases[a:b], int(batch.flags[r]), bool(v), np.array([rs[c] for c in cols], np.int64), batch.ipd[a:b], batch.pw[a:b]))
        ref = int(batch.flags[int(batch.read_off[z]) + bb]) & 1 if nw else 0
        out.append(Zmw([tpl[w, :meta[w, 0]] for w in range(nw)], [(int(meta[w, 1]), int(meta[w, 2])) for w in range(nw)], ref, reads))
    return out

"""CPU restatement of the end of the path: DESIGN.md §2 "HiFi kinetics" (the fi fp ri rp planes of k_kinetics_t<1, *>) and "QVs (A6), stitch" (what k_stitch and
k_post put into the record), in numpy and Python integers.

The inputs are what the engine's stages produced (`collect`, after a synchronous ccsx_consensus_pileup call on a handle with opts.hifi_kinetics) or are made
by hand (tests/test_kinetics_ref.py).  The segment alignment is the one of tests/pileup_ref.py (`window_segments`, `diag_rows`): it is not copied here.  The codec
is a table written from the four ranges of the text, the mean is the text's integer formula, the stitch is the text's list.  Nothing here calls a kernel, and
nothing here was transcribed from the kernels' or the oracle's arithmetic."""
from __future__ import annotations

import bisect
from collections import Counter, namedtuple

import numpy as np

from pileup_ref import IMAX, Zmw, collect_stage, diag_rows, window_segments

SUCCESS, NON_CONVERGENT, LOW_RQ, EMPTY_WINDOW = 0, 4, 7, 8          # enum ccsx_status (include/ccsx.h)
GROUP = 32                                                          # passes per group of the kernels (PW_MAXREADS)

# ---------------------------------------------------------------- CodecV1
# "codes < 64 are the frame count itself", then 64 codes in steps of 2 from 64, 64 in steps of 4 from 192, 64 in steps of 8 from 448
DEC = [c for c in range(64)] + [64 + 2 * k for k in range(64)] + [192 + 4 * k for k in range(64)] + [448 + 8 * k for k in range(64)]
assert len(DEC) == 256 and DEC[-1] == 952


def dec(c: int) -> int:
    return DEC[int(c)]


def enc(f: int) -> int:
    """the code of the representable value nearest to f frames; of two equally near the upper one; everything above 952 is 952"""
    f = int(f)
    if f <= 0:
        return 0
    if f >= DEC[-1]:
        return 255
    hi = bisect.bisect_left(DEC, f)                                 # DEC[hi - 1] < f <= DEC[hi]
    return hi if DEC[hi] - f <= f - DEC[hi - 1] else hi - 1


def mean_frames(total: int, n: int) -> int:
    """`(2 sum + n) div (2 n)`: the mean of n frame counts, halves up (Python ints, or int64 arrays)"""
    return (2 * total + n) // (2 * n)


def mean_code(total: int, n: int) -> int:
    return enc(mean_frames(int(total), int(n))) if int(n) else 0


# ---------------------------------------------------------------- kinetics
Seg = namedtuple("Seg", "zi w p st off seg tpl rows")               # a usable segment: ZMW, window, pass, strand, offset in the pass, bases, oriented template, DIAG rows


def aligned_segments(zmws) -> list:
    """every usable segment of every window (window_segments' test on each pass alone) with its alignment (diag_rows)"""
    out = []
    for zi, z in enumerate(zmws):
        nw = len(z.tpls)
        for w in range(nw):
            t = np.asarray(z.tpls[w], np.int64)
            iws, iwe = (0 if w == 0 else 2 * w - 1), (2 * nw - 1 if w == nw - 1 else 2 * (w + 1))
            for p, rd in enumerate(z.reads):
                one = window_segments(Zmw(z.tpls, z.cores, z.ref_strand, [rd]), w)
                if not one:
                    continue
                seg, st = one[0]
                off = len(rd[0]) - int(rd[3][iwe]) if st else int(rd[3][iws])      # the segment's first base in the pass's own orientation
                out.append([zi, w, p, st, off, seg, 3 - t[::-1] if st else t])
    rows = diag_rows([s[5] for s in out], [s[6] for s in out]) if out else []
    return [Seg(*s, r) for s, r in zip(out, rows)]


def kinetics_sums(zmws, segs=None, keep=None):
    """per ZMW, per window an int64 array [2 strands, 3 (ipd, pw, n), J] of the sums over forward columns: DIAG cells on core columns whose bases agree.
    keep(zi, p): the passes that count (None: all)"""
    segs = aligned_segments(zmws) if segs is None else segs
    sums = [[np.zeros((2, 3, len(t)), np.int64) for t in z.tpls] for z in zmws]
    for s in segs:
        if keep is not None and not keep(s.zi, s.p):
            continue
        z = zmws[s.zi]
        rd = z.reads[s.p]
        cs, ce = z.cores[s.w]
        J = len(s.tpl)
        acc = sums[s.zi][s.w][s.st]
        for col in np.flatnonzero(s.rows >= 0):
            r = int(s.rows[col])
            jf = J - 1 - col if s.st else col
            if not cs <= jf < ce or int(s.seg[r]) != int(s.tpl[col]):
                continue
            acc[0, jf] += dec(rd.ipd[s.off + r]); acc[1, jf] += dec(rd.pw[s.off + r]); acc[2, jf] += 1
    return sums


def codes_of(zmws, sums) -> list:
    """per ZMW uint8 [4, len]: fi fp ri rp over the concatenated cores"""
    out = []
    for z, sz in zip(zmws, sums):
        planes = [[], [], [], []]
        for (cs, ce), sw in zip(z.cores, sz):
            for c in range(cs, ce):
                for k, (st, q) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
                    planes[k].append(mean_code(sw[st, q, c], sw[st, 2, c]))
        out.append(np.array(planes, np.uint8).reshape(4, -1))
    return out


def kinetics_zmws(zmws, segs=None) -> list:
    return codes_of(zmws, kinetics_sums(zmws, segs))


def census(zmws, segs=None) -> Counter:
    """what the compared windows contain, from the Zmw records alone (never from an output under test)"""
    segs = aligned_segments(zmws) if segs is None else segs
    c = Counter()
    for z in zmws:
        nw = len(z.tpls)
        c["zmws"] += nw > 0; c["windows"] += nw
        c["zmw_of_64_windows"] += nw == 64; c["zmw_of_65_windows"] += nw == 65; c["zmw_above_65_windows"] += nw > 65
        c["passes_above_64"] += max(0, len(z.reads) - 64)
        for w in range(nw):
            cs, ce = z.cores[w]
            c["core_not_19"] += ce - cs != 19
            iws, iwe = (0 if w == 0 else 2 * w - 1), (2 * nw - 1 if w == nw - 1 else 2 * (w + 1))
            for g0 in range(0, len(z.reads), GROUP):                    # the kernel's task plan per group: two short segments share a wave
                short = long_ = 0
                for rd in z.reads[g0:g0 + GROUP]:
                    if not rd[2]:
                        c["invalid_pass"] += 1
                        continue
                    n = int(rd[3][iwe]) - int(rd[3][iws])
                    c["n<0" if n < 0 else "n>64" if n > 64 else f"n={n}" if n in (0, 1, 31, 32, 63, 64) else "n_other"] += 1
                    short += 0 <= n <= 31; long_ += 31 < n <= IMAX
                c["lone_half_wave"] += short & 1
                c["paired_and_unpaired"] += short >= 2 and long_ >= 1
    for s in segs:
        z = zmws[s.zi]
        rd = z.reads[s.p]
        cs, ce = z.cores[s.w]
        J = len(s.tpl)
        fwd = s.rows[::-1] if s.st else s.rows                          # the DIAG row of every forward column (rows count in the pass's own orientation)
        c["opposite_segments"] += s.st; c["partial_segments"] += bool(rd[1] & 2)
        agree = [fwd[j] >= 0 and int(s.seg[fwd[j]]) == int(s.tpl[J - 1 - j if s.st else j]) for j in range(J)]
        c["diag_on_overhang"] += int(sum(fwd[j] >= 0 for j in range(J) if not cs <= j < ce))
        c["core_mismatch"] += int(sum(fwd[j] >= 0 and not agree[j] for j in range(cs, ce)))
        c["partial_cells"] += int(sum(agree[cs:ce])) if rd[1] & 2 else 0
        if len(s.seg) and ce > cs:
            c["del_first_core_col"] += int(fwd[cs] < 0); c["del_last_core_col"] += int(fwd[ce - 1] < 0)
            for a, b in ((cs - 1, cs), (ce - 1, ce)):                  # read bases between the DIAG cells on the two sides of a core edge
                if 0 <= a and b < J and fwd[a] >= 0 and fwd[b] >= 0 and abs(int(fwd[b]) - int(fwd[a])) > 1:
                    c["seam_insertion"] += 1
    return c


def strand_counts(z: Zmw):
    """(fn, rn): the valid full-length passes (flags bit 1 clear) among the passes used, by strand against the backbone"""
    st = [(int(rd[1]) ^ z.ref_strand) & 1 for rd in z.reads if rd[2] and not rd[1] & 2]
    return st.count(0), st.count(1)


# ---------------------------------------------------------------- stitch
def stitch_zmw(tpls, cores, wmeta, raw_qv, opts, pre_status=SUCCESS) -> dict:
    """the record's scalars from the converged windows.  tpls / cores: as in Zmw; wmeta: int [nw, 5] = (core length, used_all, used_full, non-convergent,
    rounds) (ccsx_stage_wmeta); raw_qv: the run's un-rounded QVs of this ZMW (float32); opts: min_rq is read.  rq is `rq_ref`, float64"""
    if pre_status != SUCCESS:
        return dict(status=pre_status, seq=np.zeros(0, np.uint8), seq_len=0, qual=np.zeros(0, np.uint8), n_windows=0, iters=0, ec=np.float32(0), rq_ref=0.0, np=None)
    nw = len(tpls)
    wmeta = np.asarray(wmeta, np.int64).reshape(nw, 5)
    seq = np.concatenate([np.asarray(t, np.uint8)[cs:ce] for t, (cs, ce) in zip(tpls, cores)] + [np.zeros(0, np.uint8)])
    assert [ce - cs for cs, ce in cores] == wmeta[:, 0].tolist(), "the cores are not the lengths the polish reported"
    raw = np.asarray(raw_qv, np.float32)[:len(seq)]
    assert len(raw) == len(seq)
    qual = (raw + np.float32(0.5)).astype(np.uint8)
    rq = 1.0 - float(np.mean(10.0 ** (-raw.astype(np.float64) / 10.0))) if len(seq) else 0.0
    hist = Counter(wmeta[:, 2].tolist())
    mode = min(hist, key=lambda v: (-hist[v], v)) if nw else 0       # the most windows, then the smaller count
    ec = np.float32(float(int(wmeta[:, 1].sum())) / nw) if nw else np.float32(0)
    if len(seq) == 0:
        status = EMPTY_WINDOW
    elif wmeta[:, 3].any():
        status = NON_CONVERGENT
    elif rq < float(opts.min_rq):
        status = LOW_RQ
    else:
        status = SUCCESS
    return dict(status=status, seq=seq, seq_len=len(seq), qual=qual, n_windows=nw, iters=int(wmeta[:, 4].sum()), ec=ec, rq_ref=rq, np=int(mode))


def collect(handle, batch):
    """after a synchronous ccsx_consensus_pileup call: (Zmw records (collect_stage), per ZMW the stage_wmeta array, per ZMW the backbone pass)"""
    zmws = collect_stage(handle, batch)
    wmeta = [handle.stage_wmeta(z) for z in range(batch.n_zmw)]
    backbone = [handle.stage_polished(z)[3] for z in range(batch.n_zmw)]
    return zmws, wmeta, backbone

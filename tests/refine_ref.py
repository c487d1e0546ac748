"""The polisher hand-back's rule (DESIGN.md §2 "Polisher hand-back") restated in numpy — classes, codes, splice, merged quals, rq_merged from the engine's
exported table — and an independent brute force over Python lists for hand-made cases.  Neither reads what the kernels wrote."""
import numpy as np

from ccs_amd import api

SKIPPED, RESCORED, REFINED = 0, 1, 2
BAD_TILE, BAD_ORDER, BAD_SYMBOL, TOO_LONG, EMPTY, BAD_BACKBONE, BAD_LIST = -1, -2, -3, -4, -5, -6, -7


def perr_table() -> np.ndarray:
    return api.refine_perr_table()


def rq_of(quals, perr) -> np.float32:
    """1 - mean error probability of the quals: the uint64 sum of the table, then the rule's one division (in double, rounded to float once)"""
    q = np.asarray(quals).astype(np.int64)
    if len(q) == 0:
        return np.float32(0.0)
    s = int(np.where(q < 94, perr[np.minimum(q, 93)], np.uint64(0)).astype(np.uint64).sum(dtype=np.uint64))
    return np.float32(1.0 - float(s) / 4294967296.0 / float(len(q)))


def list_violations(tile_zmw, n_zmw: int) -> int:
    z = np.asarray(tile_zmw).astype(np.int64)
    bad = (z < 0) | (z >= n_zmw)
    bad[1:] |= z[1:] < z[:-1]
    return int(bad.sum())


def refine(seq_off, base_len, base_seq, base_qual, passes, backbone, tiles: dict, stride: int, perr=None) -> dict:
    """tiles: tile_zmw, tile_start, tile_len, new_len [m], new_seq, new_qual [m, stride] (numpy).  Returns counts [3], code / n_applied / new_len [n],
    rq_merged [n] float32, drafts / quals: per ZMW the refined draft D_z and the merged quals M_z"""
    perr = perr_table() if perr is None else perr
    n, U = len(base_len), int(stride)
    tz, ts, tl, nl = (np.asarray(tiles[k]).astype(np.int64) for k in ("tile_zmw", "tile_start", "tile_len", "new_len"))
    m = len(tz)
    viol = list_violations(tz, n)
    # the classes of every tile whose ZMW exists, from its raw values
    cls = np.zeros(m, np.int64)
    for g in range(m):
        if not 0 <= tz[g] < n:
            continue
        L = int(base_len[tz[g]])
        len_ok = 0 <= nl[g] <= U
        if ts[g] < 0 or tl[g] < 1 or ts[g] + tl[g] > L or not len_ok:
            cls[g] |= 1
        if g > 0 and tz[g - 1] == tz[g] and ts[g] < ts[g - 1] + tl[g - 1]:
            cls[g] |= 2
        if len_ok and ((tiles["new_seq"][g, :nl[g]] > 3).any() or (tiles["new_qual"][g, :nl[g]] > 93).any()):
            cls[g] |= 4
    out = dict(counts=np.zeros(3, np.int32), code=np.zeros(n, np.int32), n_applied=np.zeros(n, np.int32), new_len=np.zeros(n, np.int32),
               rq_merged=np.zeros(n, np.float32), drafts=[], quals=[])
    out["counts"][2] = viol
    for z in range(n):
        L, C_ = int(base_len[z]), int(seq_off[z + 1] - seq_off[z])
        o = int(seq_off[z])
        bs, bq = base_seq[o:o + max(L, 0)], base_qual[o:o + max(L, 0)]
        none = (np.zeros(0, np.uint8), np.zeros(0, np.uint8))
        if L <= 0 or backbone[z] < 0:
            code, d = SKIPPED, none
        elif backbone[z] >= passes[z]:
            code, d = BAD_BACKBONE, none
        elif viol:
            code, d = BAD_LIST, (bs, bq)
        else:
            run = np.flatnonzero(tz == z)
            d = (bs, bq)
            if len(run) == 0:
                code = RESCORED
            else:
                c = int(np.bitwise_or.reduce(cls[run]))
                Lp = L + int((nl[run] - tl[run]).sum())
                if c & 1:
                    code = BAD_TILE
                elif c & 2:
                    code = BAD_ORDER
                elif c & 4:
                    code = BAD_SYMBOL
                elif Lp > C_:
                    code = TOO_LONG
                elif Lp < 1:
                    code = EMPTY
                else:
                    code = REFINED
                    ps, pq, at = [], [], 0
                    for g in run:
                        ps += [bs[at:ts[g]], tiles["new_seq"][g, :nl[g]]]
                        pq += [bq[at:ts[g]], tiles["new_qual"][g, :nl[g]]]
                        at = int(ts[g] + tl[g])
                    d = (np.concatenate(ps + [bs[at:]]).astype(np.uint8), np.concatenate(pq + [bq[at:]]).astype(np.uint8))
                    assert len(d[0]) == Lp
                    out["n_applied"][z] = len(run)
        out["code"][z], out["new_len"][z] = code, len(d[0])
        out["drafts"].append(d[0]); out["quals"].append(d[1])
        out["rq_merged"][z] = rq_of(d[1], perr)
    out["counts"][0] = int((out["code"] == REFINED).sum())
    out["counts"][1] = int(out["n_applied"].sum())
    return out


def brute(bases: list, quals: list, caps: list, passes: list, backbone: list, tiles: list, stride: int, perr: list) -> dict:
    """The same rule position by position over Python lists.  bases / quals: per ZMW a list of ints; tiles: a list of (zmw, start, len, new_len, seq row, qual row),
    the rows lists of at most `stride` ints.  Returns code, n_applied, drafts, quals, sums (the integer sum of the table over the merged quals), violations"""
    n = len(bases)
    viol = 0
    for g, t in enumerate(tiles):
        if t[0] < 0 or t[0] >= n or (g > 0 and t[0] < tiles[g - 1][0]):
            viol += 1
    res = dict(code=[], n_applied=[], drafts=[], quals=[], sums=[], violations=viol)
    for z in range(n):
        L = len(bases[z])
        mine = [t for t in tiles if t[0] == z]
        code, d, q = None, list(bases[z]), list(quals[z])
        if L <= 0 or backbone[z] < 0:
            code, d, q = 0, [], []
        elif backbone[z] >= passes[z]:
            code, d, q = -6, [], []
        elif viol:
            code = -7
        elif not mine:
            code = 1
        else:
            found = set()
            end_before = None
            for (_, start, ln, nlen, srow, qrow) in mine:
                ok_len = 0 <= nlen <= stride
                if start < 0 or ln < 1 or start + ln > L or not ok_len:
                    found.add(1)
                if end_before is not None and start < end_before:
                    found.add(2)
                end_before = start + ln
                if ok_len and any(s > 3 for s in srow[:nlen]) or ok_len and any(x > 93 for x in qrow[:nlen]):
                    found.add(3)
            if found:
                code = -min(found)
            else:
                by_start = {t[1]: t for t in mine}
                d, q, p = [], [], 0
                while p < L:
                    if p in by_start:
                        _, _, ln, nlen, srow, qrow = by_start[p]
                        d.extend(srow[:nlen]); q.extend(qrow[:nlen])
                        p += ln
                    else:
                        d.append(bases[z][p]); q.append(quals[z][p])
                        p += 1
                if len(d) > caps[z]:
                    code = -4
                elif len(d) < 1:
                    code = -5
                else:
                    code = 2
                if code != 2:
                    d, q = list(bases[z]), list(quals[z])
        res["code"].append(code); res["n_applied"].append(len(mine) if code == 2 else 0)
        res["drafts"].append(d); res["quals"].append(q)
        res["sums"].append(sum(perr[x] if 0 <= x <= 93 else 0 for x in q))
    return res


def spliced_drafts(batch, ref: dict, backbone) -> "api.Drafts":
    """a Drafts holding (D_z, L', backbone[z]) of a restatement, for Handle.polish(batch, drafts, QV_ONLY)"""
    d = api.Drafts.allocate(batch)
    for z in range(batch.n_zmw):
        o = int(d.seq_off[z])
        k = len(ref["drafts"][z])
        d.seq[o:o + k] = ref["drafts"][z]
        d.len[z], d.backbone[z] = k, backbone[z]
    return d

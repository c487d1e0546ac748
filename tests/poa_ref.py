"""A plain reference of the POA draft ("POA draft (D1-D3)"), written from the SPEC paragraph alone: test infrastructure, like align_ref.py.

Two parts.

opt_unbanded(graph, read): an int64 score DP over the whole DAG with full columns of I + 1 rows.  It knows the four scores (+3 / -5 / -4 / -4) and the START column
`M[l] = -4 l` that stands in for the predecessors of a vertex without in-edges, and nothing else: no band, no tie-break, no move word, no in-edge order.  With
`F[v][i]` the best score of `read[:i]` on a path that ends in vertex v, and `B[v][i]` the best score of `read[i:]` on a path that leaves v (and may end anywhere),
`OPT = max_v F[v][I]`, and some optimal alignment passes through (v, i) iff `F[v][i] + B[v][i] = OPT`.

poa_spec(reads, flags, max_poa_cov, backbone, band): D1-D3 on an object graph — vertices are Python objects, in-edges a list, the topological order a Python list
with `insert` — with every tie-break the SPEC states, and one record per pass of what the DP saw and what the threading did.  band = None gives full columns.
"""
from __future__ import annotations

import numpy as np

MATCH, MISMATCH, INS, DEL = 3, -5, -4, -4
NEG = -(1 << 28)
MAXPRED = 7


# ---- part 1: the unbanded optimum -------------------------------------------------------------------------------------------------------------------------
class Dag:
    """a graph in topological order: base[k] of the vertex at position k, preds[k] the positions of its in-edges' sources (all < k)"""

    def __init__(self, base, preds):
        self.base = [int(b) for b in base]
        self.preds = [list(p) for p in preds]
        self.n = len(self.base)
        assert all(0 <= u < k for k, p in enumerate(self.preds) for u in p), "not a topological order"
        self.succs = [[] for _ in range(self.n)]
        for k, p in enumerate(self.preds):
            for u in p: self.succs[u].append(k)


def _ins_chain(c):
    """x[l] = max(c[l], x[l - 1] - 4) for a whole column: a running maximum of c[l] + 4 l"""
    ramp = 4 * np.arange(len(c), dtype=np.int64)
    return np.maximum.accumulate(c + ramp) - ramp


def _rchain(c):
    """x[i] = max(c[i], x[i + 1] - 4): the same from the other end"""
    return _ins_chain(c[::-1])[::-1]


class Opt:
    """forward and backward matrices of one read on one graph"""

    def __init__(self, dag: Dag, read):
        r = np.asarray(read, np.int64)
        I, n = len(r), dag.n
        self.I, self.dag = I, dag
        sc = [np.where(r == b, MATCH, MISMATCH).astype(np.int64) for b in range(4)]       # sc[b][i] = s(b, read[i])
        start = INS * np.arange(I + 1, dtype=np.int64)
        low = np.int64(-(1 << 40))
        F = np.empty((n, I + 1), np.int64)
        for k in range(n):
            s = sc[dag.base[k]]
            c = np.full(I + 1, low, np.int64)
            for col in ([F[u] for u in dag.preds[k]] or [start]):
                c[1:] = np.maximum(c[1:], col[:-1] + s)                                   # diagonal: read[i - 1] on this vertex
                c = np.maximum(c, col + DEL)                                              # deletion: the vertex without a base
            F[k] = _ins_chain(c)                                                          # insertions: bases after this vertex
        self.F = F
        self.opt = int(F[:, I].max()) if n else None
        B = np.empty((n, I + 1), np.int64)
        for k in range(n - 1, -1, -1):
            c = np.full(I + 1, low, np.int64)
            c[I] = 0                                                                      # the alignment may end on any vertex once the read is used up
            for w in dag.succs[k]:
                c[:-1] = np.maximum(c[:-1], B[w][1:] + sc[dag.base[w]])
                c = np.maximum(c, B[w] + DEL)
            B[k] = _rchain(c)
        self.B = B

    def on_optimal(self, k: int, i: int) -> bool:
        """does some optimal alignment pass through (vertex at position k, read row i) — the state "read[:i] used, standing on vertex k" """
        return int(self.F[k, i] + self.B[k, i]) == self.opt


def opt_unbanded(dag: Dag, read) -> Opt:
    return Opt(dag, read)


def brute_force(dag: Dag, read):
    """OPT and the set of (k, i) on optimal alignments by enumerating every path of the graph and every alignment of the read to it (tiny inputs only).
    An alignment starts at a vertex without in-edges after any number of leading insertions, and ends on any vertex with the read used up."""
    I = len(read)
    paths = []

    def grow(p):
        paths.append(list(p))
        for w in dag.succs[p[-1]]: grow(p + [w])
    for k in range(dag.n):
        if not dag.preds[k]: grow([k])
    best, cells = None, set()

    def walk(path, j, i, score, seen):
        """standing on path[j] with read[:i] used"""
        nonlocal best, cells
        seen = seen + [(path[j], i)]
        if j == len(path) - 1:
            rest = score + INS * (I - i)                                                  # trailing insertions on the last vertex
            full = seen + [(path[j], x) for x in range(i + 1, I + 1)]
            if best is None or rest > best: best, cells = rest, set(full)
            elif rest == best: cells |= set(full)
            return
        if i < I: walk(path, j, i + 1, score + INS, seen)
        w = path[j + 1]
        walk(path, j + 1, i, score + DEL, seen)
        if i < I: walk(path, j + 1, i + 1, score + (MATCH if dag.base[w] == read[i] else MISMATCH), seen)

    for p in paths:
        for lead in range(I + 1):                                                          # leading insertions, then the first vertex by a diagonal or a deletion
            walk(p, 0, lead, INS * lead + DEL, [])
            if lead < I: walk(p, 0, lead + 1, INS * lead + (MATCH if dag.base[p[0]] == read[lead] else MISMATCH), [])
    return best, cells


# ---- part 2: D1-D3 on an object graph -------------------------------------------------------------------------------------------------------------------
class Vertex:
    __slots__ = ("base", "reads", "preds", "lo", "W", "full", "mv", "cmax", "brow", "tie", "tied")

    def __init__(self, base):
        self.base, self.reads, self.preds = int(base), 1, []


class _Start:
    """the virtual START column: M[l] = -4 l, band start 0, its maximum in row 0"""

    def __init__(self, I, W):
        self.lo, self.cmax, self.brow = 0, 0, 0
        self.full = np.full(I + 2 + W, NEG, np.int64)
        self.full[1:I + 2] = INS * np.arange(I + 1, dtype=np.int64)


class PassRecord:
    """what one pass of a generator did.  The first five fields are the engine's POA log record (include/ccsx.h)."""

    def __init__(self, **kw): self.__dict__.update(kw)

    def log(self): return (self.I, self.score, self.kend, int(self.threaded), self.nverts)

    def __repr__(self): return "PassRecord(%s)" % ", ".join(f"{k}={v}" for k, v in self.__dict__.items() if k not in ("path", "path_pos", "dag", "edges"))


def orient(bases, rev):
    b = np.asarray(bases, np.uint8) & 3
    return (3 - b[::-1]).astype(np.uint8) if rev else b.copy()


def _add_edge(u: Vertex, v: Vertex) -> bool:
    """SPEC: the edge is appended unless present or the in-edge cap is hit; True iff the cap refused it"""
    if any(p is u for p in v.preds): return False
    if len(v.preds) >= MAXPRED: return True
    v.preds.append(u)
    return False


def _column(v: Vertex, cols, sc, I, band):
    """one DP column of vertex v from its predecessor columns `cols`, in their order.  A column is kept as `full`, indexed by read row + 1 and NEG outside its
    rows, so that row i - 1 of any predecessor is a slice whatever the two bands' starts are"""
    v.tie = False
    if band is None: lo, W = 0, I + 1
    else:
        W = band
        ustar = cols[0]
        for u in cols[1:]:
            if u.cmax > ustar.cmax: ustar = u                                              # the largest column maximum, first on ties
        v.tie = any(u.cmax == ustar.cmax and u.lo != ustar.lo for u in cols)               # (for the lab: the tie-break decided where the band goes)
        lo = min(max(ustar.brow + 1 - band // 2, ustar.lo), ustar.lo + 2)
        lo = max(min(lo, max(0, I - (band - 1))), 0)
    nlive = min(W, I + 1 - lo)                                                             # rows lo .. min(lo + W - 1, I)
    best = np.full(nlive, NEG, np.int64)
    mv = np.zeros(nlive, np.int16)                                                         # 2 * slot + (1 = deletion), -1 = insertion
    tied = np.zeros(nlive, bool)
    s = sc[v.base][lo:lo + nlive]                                                          # s[l] = s(v, read[lo + l - 1]) (sc is shifted by one, row 0 has no base)
    for slot, u in enumerate(cols):
        for kind in (0, 1):                                                                # the diagonal M[u][i - 1] + s, then the deletion M[u][i] - 4
            src = u.full[lo + kind:lo + kind + nlive]
            c = np.where(src > NEG // 2, src + (s if kind == 0 else DEL), NEG)
            take = c > best                                                                # a later candidate wins only if strictly greater
            tied |= (c == best) & (c > NEG // 2)                                           # (for the lab: the order of the candidates decided this cell)
            best = np.where(take, c, best)
            mv[take] = 2 * slot + kind
            tied[take] = False
    x = _ins_chain(best)
    mv[x > best] = -1                                                                      # the insertion wins only if strictly greater
    x[x < NEG // 2] = NEG
    tied[x > best] = False
    v.lo, v.W, v.mv, v.tied = int(lo), W, mv, tied
    v.full = np.full(I + 2 + W, NEG, np.int64)
    v.full[lo + 1:lo + 1 + nlive] = x
    v.brow = int(lo + int(np.argmax(x)))                                                    # the first row that attains the column maximum
    v.cmax = int(x.max())


def poa_spec(reads, flags, max_poa_cov, backbone=0, band=32, snapshots=False):
    """D1-D3 for one generator: backbone pass `backbone`, then the passes after it in order, wrapping around, min(full passes, max_poa_cov) in all.
    reads: the ZMW's passes in native orientation (codes 0..3); flags: bit 0 = reverse strand, bit 1 = partial (a suffix: never threaded).
    Returns (draft as a uint8 array, or None for DRAFT_FAILURE; [PassRecord of pass rr = 1, 2, ...]).  snapshots: every record also carries `dag`, the
    graph before the pass (a Dag in topological order)."""
    flags = [int(f) for f in flags]
    nfull = len(reads)
    while nfull > 0 and (flags[nfull - 1] & 2): nfull -= 1
    npoa = min(nfull, max_poa_cov)
    recs = []
    if npoa <= 0: return None, recs
    maxL = max(len(r) for r in reads[:nfull])
    vcap, dcap = (5 * maxL) // 2 + 256, maxL + maxL // 4 + 64
    rev0 = flags[backbone] & 1
    order, nadded = [], 0
    for rr in range(npoa):
        ri = (backbone + rr) % nfull
        r = orient(reads[ri], (flags[ri] & 1) != rev0)
        I = len(r)
        if rr == 0:
            prev = None
            for b in r:                                                                     # the backbone becomes a chain, whatever its length
                v = Vertex(b)
                if prev is not None: v.preds.append(prev)
                order.append(v); prev = v
            nadded = 1
            if not order: return None, recs                                                 # an empty backbone: nothing can be threaded into it
            continue
        pos = {id(v): k for k, v in enumerate(order)}
        rec = PassRecord(rr=rr, read=ri, I=I, score=NEG, kend=-1, threaded=False, nverts=len(order), max_indeg=0, cap_refused=False, max_dist=0,
                         edges=set(), path=None, overflow=False, new_pos=[], path_pos=None, ustar_ties=0, lead_ins=0, path_ties=0, max_lo=0)
        if snapshots: rec.dag = Dag([v.base for v in order], [[pos[id(u)] for u in v.preds] for v in order])
        recs.append(rec)
        sc = [np.concatenate([[NEG], np.where(r == b, MATCH, MISMATCH)]).astype(np.int64) for b in range(4)]   # sc[b][i] = s(b, read[i - 1])
        start = _Start(I, I + 1 if band is None else band)
        for k, v in enumerate(order):
            for slot, u in enumerate(v.preds):
                d = k - pos[id(u)]
                rec.max_dist = max(rec.max_dist, d)
                if d >= 7: rec.edges.add((d, slot, len(v.preds)))                           # (distance, in-edge slot, in-edges of the vertex) of the long edges read
            _column(v, v.preds or [start], sc, I, band)
            rec.ustar_ties += int(v.tie)
            rec.max_lo = max(rec.max_lo, v.lo)
        end = None
        for k, v in enumerate(order):                                                       # the end cell: the best M[v][I], first in topological order
            x = int(v.full[I + 1]) if v.lo <= I < v.lo + v.W else NEG
            if x > NEG // 2 and (end is None or x > rec.score): end, rec.score, rec.kend = v, x, k
        rec.max_indeg = max(len(v.preds) for v in order)
        if end is None or rec.score < I: continue                                           # the gate
        # trace-back: per read base the vertex it matched, or None (a new vertex)
        path = [None] * I
        v, i = end, I
        while v is not None:
            m = int(v.mv[i - v.lo])
            rec.path_ties += int(v.tied[i - v.lo])                                          # cells of the path where a diagonal and a deletion (or two in-edges) tied
            if m < 0: path[i - 1] = None; i -= 1; continue
            u = v.preds[m >> 1] if v.preds else None
            if not (m & 1):
                path[i - 1] = v if v.base == int(r[i - 1]) else None
                i -= 1
            v = u
        rec.lead_ins = i                                                                    # the i bases left are leading insertions at START: new vertices
        rec.path_pos = [pos[id(w)] if w is not None else -1 for w in path]                  # per read base: the position of its vertex before the pass, -1 = new
        prevv, at = None, -1                                                                # at: position of prevv in `order`
        n_new = sum(1 for w in path if w is None)
        if len(order) + n_new > vcap:
            rec.overflow = True
            return None, recs                                                               # vertex capacity: DRAFT_FAILURE
        for i in range(I):
            w = path[i]
            if w is None:
                w = Vertex(r[i])
                at += 1
                order.insert(at, w)                                                         # spliced in right after the previous path vertex (list head if none)
            else:
                w.reads += 1
                at += 1
                while order[at] is not w: at += 1
            if prevv is not None and _add_edge(prevv, w): rec.cap_refused = True
            prevv = w
            path[i] = w
        nadded += 1
        rec.threaded, rec.nverts, rec.path = True, len(order), path
        mine = {id(w) for w in path}
        rec.new_pos = [k for k, w in enumerate(order) if id(w) in mine and id(w) not in pos]   # where this pass's new vertices landed
        rec.max_indeg = max(len(v.preds) for v in order)
    # consensus: the heaviest path
    best, back = {}, {}
    top, vtop = None, None
    for v in order:
        b, p = 0, None
        for u in v.preds:
            if best[id(u)] > b: b, p = best[id(u)], u                                       # the first strictly greater predecessor
        best[id(v)] = b + 2 * v.reads - nadded
        back[id(v)] = p
        if top is None or best[id(v)] > top: top, vtop = best[id(v)], v                     # the first maximum in topological order
    out = []
    while vtop is not None: out.append(vtop.base); vtop = back[id(vtop)]
    if len(out) > dcap: return None, recs
    return np.array(out[::-1], np.uint8), recs


# ---- the draft cascade's choice of backbones ("Draft cascade") ----------------------------------------------------------------------------
def closest_to_median(lengths, excluded=()):
    """the pass whose length is closest to the median of `lengths` (element n/2 of the sorted lengths), the first one on ties, `excluded` passes aside"""
    med = sorted(lengths)[len(lengths) // 2]
    best = None
    for k, n in enumerate(lengths):
        if k in excluded: continue
        if best is None or abs(n - med) < abs(lengths[best] - med): best = k
    return best


def fallback_backbone(reads, flags):
    n = len(reads)
    while n > 0 and (int(flags[n - 1]) & 2): n -= 1
    return closest_to_median([len(r) for r in reads[:n]])

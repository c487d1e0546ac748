"""Pass orientation (DESIGN.md §2 "Pass orientation", rule version 1): the rule restated in numpy for a whole api.Batch — anchor, votes, call, resolved flags — and
a brute-force reading of it that compares k-mers as strings and reverse-complements with string operations (no codes, no hashing).  tests/test_orient_ref.py
checks the restatement against the brute force on the CPU; tests/test_orient_gpu.py holds k_orient to the restatement, field for field, on an MI355X."""
import numpy as np

K = 13
UNKNOWN = 0x8                                                        # flags bit 3 (CCSX_PASS_STRAND_UNKNOWN)
GIVEN, ANCHOR, SAME, OPPOSITE, UNDETERMINED, NO_ANCHOR = range(6)
FIELDS = ("strand", "call", "votes_same", "votes_opp")
DEFAULTS = dict(min_votes=16, ratio=3)


def _opts(o):
    r = dict(DEFAULTS)
    r.update(o or {})
    return r


def revcomp(x):
    return (3 - (np.asarray(x, np.uint8) & 3)[::-1]).astype(np.uint8)


def codes(d):
    """(F, R) of every 13-mer position 0 .. N - K: 2 bits per base, first base most significant; R is the code of the reverse complement.  Only the low two
    bits of a base byte count"""
    d = np.asarray(d, np.int64) & 3
    if len(d) < K:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    w = np.lib.stride_tricks.sliding_window_view(d, K)
    pw = 4 ** np.arange(K - 1, -1, -1, dtype=np.int64)
    return w @ pw, (3 - w[:, ::-1]) @ pw


def anchor(lengths, flags):
    """the anchor pass of a ZMW (index within the ZMW), -1 without a full-length pass: among the full-length passes (bit 1 clear) the one whose length is closest
    to the median = element n // 2 of the sorted lengths, ties to the first"""
    full = [i for i in range(len(lengths)) if not (int(flags[i]) & 2)]
    if not full:
        return -1
    med = sorted(int(lengths[i]) for i in full)[len(full) // 2]
    return min(full, key=lambda i: (abs(int(lengths[i]) - med), i))


def call(vs, vo, opts):
    if vs >= opts["min_votes"] and vs >= opts["ratio"] * vo:
        return SAME
    if vo >= opts["min_votes"] and vo >= opts["ratio"] * vs:
        return OPPOSITE
    return UNDETERMINED


def _empty(batch):
    R = int(batch.read_off[-1])
    f = np.asarray(batch.flags, np.uint8)
    return dict(strand=(f & 1).astype(np.uint8), call=np.zeros(R, np.uint8), votes_same=np.zeros(R, np.int32), votes_opp=np.zeros(R, np.int32),
                flags=f.copy(), anchor=np.full(batch.n_zmw, -1, np.int32))


def _decide(out, r, f, a_rev, vs, vo, opts):
    c = call(vs, vo, opts)
    s = a_rev if c == SAME else (a_rev ^ 1) if c == OPPOSITE else f & 1
    out["strand"][r], out["call"][r], out["votes_same"][r], out["votes_opp"][r] = s, c, vs, vo
    out["flags"][r] = (f & 0xf6) | s


def orient(batch, opts=None):
    """the report of a batch as a dict of arrays: FIELDS per pass, `flags` = what the engine goes on to use, `anchor` per ZMW"""
    op = _opts(opts)
    out = _empty(batch)
    for z in range(batch.n_zmw):
        r0, r1 = int(batch.read_off[z]), int(batch.read_off[z + 1])
        fl = out["flags"][r0:r1].copy()
        lens = np.diff(batch.base_off[r0:r1 + 1])
        a = out["anchor"][z] = anchor(lens, fl)
        unk = [q for q in range(r1 - r0) if fl[q] & UNKNOWN]
        if not unk:
            continue
        if a < 0:
            for q in unk:
                out["call"][r0 + q] = NO_ANCHOR
                out["flags"][r0 + q] = int(fl[q]) & 0xf7
            continue
        SA = np.unique(codes(batch.read(r0 + a)[0])[0])
        a_rev = int(fl[a]) & 1
        for q in unk:
            f = int(fl[q])
            if q == a:
                out["call"][r0 + q] = ANCHOR
                out["flags"][r0 + q] = f & 0xf7
                continue
            F, R = codes(batch.read(r0 + q)[0])
            _decide(out, r0 + q, f, a_rev, int(np.isin(F, SA).sum()), int(np.isin(R, SA).sum()), op)
    return out


def orient_bruteforce(batch, opts=None):
    """the rule read literally: sequences as strings, the reverse complement by string operations, the anchor's k-mers a Python set of strings"""
    op = _opts(opts)
    out = _empty(batch)
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    text = lambda r: "".join("ACGT"[int(x) & 3] for x in batch.read(r)[0])
    rc = lambda s: "".join(comp[c] for c in reversed(s))
    for z in range(batch.n_zmw):
        r0, r1 = int(batch.read_off[z]), int(batch.read_off[z + 1])
        fl = [int(x) for x in out["flags"][r0:r1]]
        seqs = [text(r) for r in range(r0, r1)]
        full = [(len(seqs[q]), q) for q in range(r1 - r0) if not fl[q] & 2]
        a = -1
        if full:
            med = sorted(full)[len(full) // 2][0]
            best = None
            for n, q in full:                                        # in pass order: a later pass wins only when it is strictly closer
                if best is None or abs(n - med) < best:
                    best, a = abs(n - med), q
        out["anchor"][z] = a
        for q in range(r1 - r0):
            if not fl[q] & UNKNOWN:
                continue
            if a < 0 or q == a:
                out["call"][r0 + q] = NO_ANCHOR if a < 0 else ANCHOR
                out["flags"][r0 + q] = int(fl[q]) & 0xf7
                continue
            SA = {seqs[a][j:j + K] for j in range(len(seqs[a]) - K + 1)}
            s = seqs[q]
            vs = sum(1 for i in range(len(s) - K + 1) if s[i:i + K] in SA)
            vo = sum(1 for i in range(len(s) - K + 1) if rc(s[i:i + K]) in SA)
            _decide(out, r0 + q, fl[q], fl[a] & 1, vs, vo, op)
    return out

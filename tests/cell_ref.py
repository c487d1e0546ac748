"""The cell-tag rule restated (DESIGN.md §2 "Cell-tag rule", rule version 1), and the limit set the library and the kernel are checked on.

cell_reads() takes the ends from barcode_ref.call_reads, the poly(A) scan from cdna_ref (polya_scan over polya_x) and the hits inside the read from
segment_ref.table_hits, as cdna_ref.cdna_reads does; none of them is stated again here.  What is this rule's own is plain Python on tuples of bases: the tag end,
the fields, the candidates (candidates(): tuples spliced, nothing packed, no table), what they reach in a dict of the whitelist, the decision, the UMI, the widened
clip.  correct_brute() is the correction by the definition, over the whole whitelist: a barcode w is reached if w == raw, hamming(w, raw) == 1, raw[0 : b - 1] is
w with one base deleted, or raw . next is w with one base inserted.  The table (slots, first slot, probing) is restated in table_of() on dup_ref.hash32.  Nothing
is shared with cell_core.h.

limit_cases() lists (name, primers, roles, opts, design, whitelist, reads): the smallest shapes at which the kernel can still go wrong (see each block);
expected() is cell_reads() on a case, computed once per process and shared by the CPU and the GPU tests."""
from __future__ import annotations

import functools

import numpy as np

import barcode_ref
import cdna_ref
import dup_ref
import segment_ref
from cdna_ref import A, C_, DEFAULTS, FULL_LENGTH, NO_TAIL, SHORT, CONCATEMER, body, both, cat, rand, random_set, rc   # noqa: F401

CELL_PLANES = ("tag", "bc_raw", "bc", "bc_hi", "kind", "shift", "umi", "tag_clip")
FIELDS = cdna_ref.FIELDS + CELL_PLANES
NONE, RAW, EXACT, CORRECTED, AMBIGUOUS, ABSENT = range(6)
DESIGN = dict(umi_len=12, bc_len=16, side=1, bc_first=1, indels=1)
SHIFT = {0: 0, 1: 0, 2: -1, 3: 1}


def pack(bases) -> int:
    """a field in a uint32, the first base most significant"""
    x = 0
    for b in bases:
        x = x * 4 + int(b)
    return x


def unpack(x: int, n: int) -> tuple:
    return tuple((x >> (2 * (n - 1 - j))) & 3 for j in range(n))


def candidates(raw: tuple, nxt, indels: int) -> list:
    """(kind, barcode) of every candidate of the field raw; nxt: the base behind the field, None where the insert has none"""
    b = len(raw)
    out = [(1, raw[:i] + (x,) + raw[i + 1:]) for i in range(b) for x in range(4) if x != raw[i]]
    if indels:
        short = raw[: b - 1]
        out += [(2, short[:i] + (x,) + short[i:]) for i in range(b) for x in range(4)]
        if nxt is not None:
            ext = raw + (nxt,)
            out += [(3, ext[:i] + ext[i + 1:]) for i in range(b)]
    return out


def decide(reach: dict) -> tuple:
    """(tag, bc, bc_hi, kind, shift) from {index: smallest kind}"""
    if not reach:
        return ABSENT, -1, -1, 0, 0
    lo, hi = min(reach), max(reach)
    if lo != hi:
        return AMBIGUOUS, lo, hi, 0, 0
    return CORRECTED, lo, lo, reach[lo], SHIFT[reach[lo]]


def correct(raw: tuple, nxt, indels: int, index: dict) -> tuple:
    if raw in index:
        return EXACT, index[raw], index[raw], 0, 0
    reach = {}
    for kind, cand in candidates(raw, nxt, indels):
        w = index.get(cand)
        if w is not None:
            reach[w] = min(reach.get(w, 9), kind)
    return decide(reach)


def correct_brute(raw: tuple, nxt, indels: int, wl: np.ndarray) -> tuple:
    """the same by the definition, every barcode of the whitelist [n, b] looked at"""
    b = len(raw)
    r = np.array(raw, np.int64)
    exact = np.flatnonzero((wl == r).all(axis=1))
    if len(exact):
        return EXACT, int(exact[0]), int(exact[0]), 0, 0
    kind = np.full(len(wl), 9)
    kind[(wl != r).sum(axis=1) == 1] = 1
    if indels:
        for i in range(b):                                           # raw[0 : b - 1] is w with base i deleted
            hit = (np.delete(wl, i, axis=1) == r[: b - 1]).all(axis=1)
            kind[hit & (kind > 2)] = 2
        if nxt is not None:
            ext = np.append(r, nxt)
            for i in range(b + 1):                                   # raw . next is w with one base inserted at i
                hit = (wl == np.delete(ext, i)).all(axis=1)
                kind[hit & (kind > 3)] = 3
    return decide({int(w): int(kind[w]) for w in np.flatnonzero(kind < 9)})


def n_slots(n: int) -> int:
    s = 64
    while s < 2 * n:
        s *= 2
    return s


def first_slot(keys, slots: int):
    return dup_ref.hash32(keys) & np.uint32(slots - 1)


def table_of(wl) -> np.ndarray:
    """the whitelist's table: slots (key << 32) | (index + 1), linear probing from first_slot"""
    slots = n_slots(len(wl))
    t = np.zeros(slots, np.uint64)
    keys = [pack(w) for w in wl]
    for k, (x, s) in enumerate(zip(keys, first_slot(keys, slots).tolist())):
        while t[s]:
            s = (s + 1) % slots
        t[s] = (x << 32) | (k + 1)
    return t


def cell_reads(primers, roles, reads, design=None, whitelist=None, brute=False, **opts) -> dict:
    """brute: the correction by correct_brute, not by the candidates"""
    o, d = {**DEFAULTS, **opts}, {**DESIGN, **(design or {})}
    n, b, u = len(reads), d["bc_len"], d["umi_len"]
    T = b + u
    reads = [np.asarray(c, np.uint8) & 3 for c in reads]
    ends = barcode_ref.call_reads(primers, reads, window=o["window"], max_dist_pct=o["max_dist_pct"], min_margin=o["min_margin"])
    out = {k: np.zeros(n, np.int32) for k in cdna_ref.READ_PLANES}
    out.update({k: ends[k].copy() for k in cdna_ref.END_PLANES})
    out.update({k: np.zeros(n, np.uint32 if k in ("bc_raw", "umi") else np.int32) for k in CELL_PLANES})
    out["tested"][:] = ends["tested"]
    out["strand"][:] = -1
    out["first_internal"][:] = -1
    out["bc"][:] = -1
    out["bc_hi"][:] = -1
    wl = np.array([np.asarray(w, np.int64) for w in whitelist], np.int64).reshape(len(whitelist), b) if whitelist is not None else None
    index = {tuple(int(v) for v in w): k for k, w in enumerate(wl)} if wl is not None else None
    for z, c in enumerate(reads):
        L = len(c)
        if L == 0:
            continue
        call, idx, clip = int(ends["call"][z]), ends["idx"][z], ends["clip"][z]
        if call != 3:
            out["cls"][z] = cdna_ref.NO_PRIMER if call == 0 else cdna_ref.ONE_END
            continue
        if roles[idx[0]] == roles[idx[1]]:
            out["cls"][z] = cdna_ref.SAME_ROLE
            continue
        strand = out["strand"][z] = int(roles[idx[0]])
        clips = [int(clip[0]), int(clip[1])]
        ins_len = L - clips[0] - clips[1]
        if ins_len < 1 or ins_len < T:
            out["cls"][z] = SHORT
            continue
        e_t = 0 if strand == d["side"] else 1
        s = c if e_t == 0 else rc(c)                                 # the tag end's strand, read away from the primer
        p0 = clips[e_t]
        p = p0 + (0 if d["bc_first"] else u)
        raw = tuple(int(v) for v in s[p: p + b])
        tag, bc, bc_hi, kind, shift = RAW, -1, -1, 0, 0
        if b > 0 and wl is not None:
            nxt = int(s[p + b]) if ins_len >= T + 1 else None
            tag, bc, bc_hi, kind, shift = correct_brute(raw, nxt, d["indels"], wl) if brute else correct(raw, nxt, d["indels"], index)
        at = p0 + b + shift if d["bc_first"] else p0
        out["tag"][z], out["bc_raw"][z], out["bc"][z], out["bc_hi"][z], out["kind"][z], out["shift"][z] = tag, pack(raw), bc, bc_hi, kind, shift
        out["umi"][z], out["tag_clip"][z] = pack(s[at: at + u]), T + shift
        clips[e_t] += T + shift
        ins2 = ins_len - T - shift
        if ins2 < 1:
            out["cls"][z] = SHORT
            continue
        clip0, clip1 = clips
        tail = cdna_ref.polya_scan(cdna_ref.polya_x(c, strand, clip0, clip1, min(o["polya_max"], ins2)), o["polya_mismatch"], o["polya_xdrop"])
        starts = []
        for q in range(2 * len(primers)):
            pat = segment_ref.search_pattern(primers, q)
            starts += [s0 for s0, e0, _ in segment_ref.table_hits(pat, c, len(pat) * o["max_dist_pct"] // 100) if clip0 <= s0 and e0 <= L - clip1]
        out["polya_len"][z], out["n_internal"][z], out["first_internal"][z] = tail, len(starts), min(starts) if starts else -1
        cls = SHORT if ins2 - tail < o["min_len"] else CONCATEMER if starts else NO_TAIL if o["min_polya"] > 0 and tail < o["min_polya"] else FULL_LENGTH
        out["cls"][z] = cls
        if cls >= CONCATEMER:
            out["start"][z], out["end"][z] = (clip0 + tail, L - clip1) if strand else (clip0, L - clip1 - tail)
    return out


# ---- the limit set
def cmol(d, p5, p3, insert, bc, umi, tail=30) -> np.ndarray:
    """the sense read of a molecule whose fields, as they are read behind the design's primer, are bc and umi (of any length: a lost or a gained base)"""
    f = cat(bc, umi) if d["bc_first"] else cat(umi, bc)
    t = np.full(tail, A, np.uint8) if isinstance(tail, int) else tail
    return cat(p5, insert, t, rc(f), rc(p3)) if d["side"] else cat(p5, f, insert, t, rc(p3))


def steady(rng, n) -> np.ndarray:
    """n random bases of which no two neighbours are equal: a lost or a gained base is no substitution of the field"""
    out = [int(rng.integers(0, 4))]
    while len(out) < n:
        out.append(int((out[-1] + rng.integers(1, 4)) % 4))
    return np.array(out[:n], np.uint8)


def whitelist(rng, n, b, steady_first=0) -> list:
    """n different random barcodes of b bases; the first steady_first of them steady()"""
    seen, out = set(), []
    while len(out) < n:
        w = steady(rng, b) if len(out) < steady_first else rand(rng, b)
        if tuple(w.tolist()) not in seen:
            seen.add(tuple(w.tolist()))
            out.append(w)
    return out


def sub(w, i) -> np.ndarray:
    v = np.array(w, np.uint8)
    v[i] = (v[i] + 1) % 4
    return v


def lost(w, i) -> np.ndarray:
    return np.delete(np.asarray(w, np.uint8), i)


def gained(w, i, x=None) -> np.ndarray:
    w = np.asarray(w, np.uint8)
    return np.insert(w, i, (w[i] + 2) % 4 if x is None else x)


def colliding(rng, n, slots, home) -> list:
    """n different 16-base barcodes whose first slot in a table of `slots` is `home`"""
    out = {}
    while len(out) < n:
        keys = rng.integers(0, 1 << 32, 4096, dtype=np.uint64)
        for x in keys[first_slot(keys, slots) == home].tolist():
            out.setdefault(int(x), np.array(unpack(int(x), 16), np.uint8))
    return list(out.values())[:n]


@functools.lru_cache(maxsize=None)
def limit_cases() -> tuple:
    rng = np.random.default_rng(20261022)
    cases = []
    S = random_set(rng, 2, [25])
    p5, p3 = S
    R2 = (0, 1)

    def add(name, reads, design=None, wl=None, primers=S, roles=R2, **opts):
        cases.append((name, tuple(primers), tuple(roles), {**DEFAULTS, **opts}, {**DESIGN, **(design or {})}, None if wl is None else tuple(wl), tuple(reads)))

    def variants(d, w, u, insert=120, tail=30, mid=None):
        """a molecule with barcode w and UMI u as they are, and with a substitution, a lost and a gained base at `mid` of the barcode"""
        mid = len(w) // 2 if mid is None else mid
        fields = [w] if len(w) == 0 else [w, sub(w, mid), lost(w, mid), gained(w, mid)]
        return [cmol(d, p5, p3, body(rng, insert), f, u, tail) for f in fields]

    # ---- whitelists of 1, 2, 1000 and 4096 barcodes (4096: slots = 2 n exactly): the first and the last barcode as they are, a substitution at the first, a
    # middle and the last base, a barcode that is not there; both strands.  Without a whitelist: RAW
    D = dict(DESIGN)
    for n in (1, 2, 1000, 4096):
        wl = whitelist(rng, n, 16)
        w = wl[n // 2]
        reads = [cmol(D, p5, p3, body(rng, 100), f, rand(rng, 12)) for f in (wl[0], wl[-1], sub(w, 0), sub(w, 7), sub(w, 15), rand(rng, 16))]
        add(f"wl{n}", both(reads), wl=wl)
    add("raw", both(reads))
    # ---- A x 16 and T x 16 (keys 0 and 0xFFFFFFFF) as members, as they are and with a substitution
    wl = [np.zeros(16, np.uint8), np.full(16, 3, np.uint8)] + whitelist(rng, 30, 16)
    add("wl_AT", both([cmol(D, p5, p3, body(rng, 100), f, rand(rng, 12)) for f in (wl[0], wl[1], sub(wl[0], 3), sub(wl[1], 15))]), wl=wl)
    # ---- keys that collide in one run of 8 and of 70 slots (a probe passes the wave's width), and a run of 8 that wraps round the table's end: the first and the
    # last key of the run as they are and with a substitution, and one more key of the same first slot that is no member (its probe walks the whole run)
    for name, n, home in (("run8", 8, 5), ("run70", 70, 100), ("wrap8", 8, 61)):
        keys = colliding(rng, n + 1, n_slots(n), home)
        wl, stranger = keys[:n], keys[n]
        add("table_" + name, both([cmol(D, p5, p3, body(rng, 100), f, rand(rng, 12)) for f in (wl[0], wl[-1], sub(wl[0], 2), sub(wl[-1], 9), stranger)]), wl=wl)
    # ---- each kind at the first, a middle and the last place, in a barcode without equal neighbours; the same without indels (kinds 2 and 3 become ABSENT)
    wl = whitelist(rng, 64, 16, steady_first=64)
    w = wl[20]
    reads = [cmol(D, p5, p3, body(rng, 100), f(w, i), steady(rng, 12)) for f in (sub, lost, gained) for i in (0, 8, 15)]
    add("kinds", both(reads), wl=wl)
    add("kinds_noindels", both(reads), design=dict(indels=0), wl=wl)
    # ---- homopolymers.  A barcode that lost its last base is also one substitution away (kinds 1 and 2: kind 1, shift 0).  The alternating barcode AC x 8 behind
    # a gained C reads C . (AC x 7) . A, next C: reached by an insertion at the first place and by a deletion there (kinds 2 and 3: kind 2, shift -1)
    alt = np.array([0, 1] * 8, np.uint8)
    wl = [alt] + whitelist(rng, 20, 16)
    reads = [cmol(D, p5, p3, body(rng, 100), lost(wl[3], 15), np.array([(wl[3][15] + 1) % 4] + [2] * 11, np.uint8)), cmol(D, p5, p3, body(rng, 100), gained(alt, 0, 1), steady(rng, 12)),
             cmol(D, p5, p3, body(rng, 100), np.zeros(16, np.uint8), rand(rng, 12))]
    add("homopolymer", both(reads), wl=wl)
    # ---- two barcodes two substitutions apart and the field between them: AMBIGUOUS, bc < bc_hi
    wl = whitelist(rng, 40, 16)
    wl[31] = sub(sub(wl[4], 5), 11)
    add("ambiguous", both([cmol(D, p5, p3, body(rng, 100), sub(wl[4], 5), rand(rng, 12)), cmol(D, p5, p3, body(rng, 100), sub(wl[4], 11), rand(rng, 12))]), wl=wl)
    # ---- designs: bc_len 0, 8, 16 and umi_len 0, 1, 12, 16, both sides, both orders, both strands
    for b, u in ((0, 1), (0, 12), (0, 16), (8, 0), (8, 1), (8, 12), (8, 16), (16, 0), (16, 1), (16, 12), (16, 16)):
        wl = whitelist(rng, 4 if b == 8 else 50, b, steady_first=4) if b else None
        for side in (0, 1):
            for first in (0, 1):
                d = dict(umi_len=u, bc_len=b, side=side, bc_first=first, indels=1)
                add(f"design_b{b}_u{u}_s{side}_f{first}", both(variants(d, wl[1] if b else np.zeros(0, np.uint8), steady(rng, u))), design=d, wl=wl)
    # ---- lengths (min_len 1, no tail required): an insert of T - 1, T and T + 1 bases.  T + 1 is where kind 3 appears: the gained base's molecule is CORRECTED
    # there with shift +1 and ins_len' = 0 (SHORT), and at T bases it is not
    wl = whitelist(rng, 16, 16, steady_first=16)
    w, u = wl[5], steady(rng, 12)
    for side in (0, 1):
        d = dict(DESIGN, side=side)
        f = cat(w, u)
        reads = [cmol(d, p5, p3, f[:0], w, u[:11], 0), cmol(d, p5, p3, f[:0], w, u, 0), cmol(d, p5, p3, rand(rng, 1), w, u, 0),
                 cmol(d, p5, p3, f[:0], gained(w, 4), u[:11], 0), cmol(d, p5, p3, f[:0], gained(w, 4), u, 0), cmol(d, p5, p3, f[:0], lost(w, 4), u, 0),
                 cmol(d, p5, p3, rand(rng, 1), lost(w, 4), u, 0), cmol(d, p5, p3, rand(rng, 2), gained(w, 4), u, 0)]
        add(f"lengths_s{side}", both(reads), design=d, wl=wl, min_len=1, min_polya=0)
    # ---- the shift and the poly(A): a tail of exactly min_polya and of min_polya - 1 bases behind the fields, the UMI's last base A and not A, under shifts of
    # 0, -1, +1 and under the homopolymer's wrong shift (the scan's first base moves on or off an A)
    wl = [alt] + whitelist(rng, 15, 16, steady_first=15)
    for last in (A, C_):
        u = steady(rng, 12)
        u[-1] = last if D["side"] == 0 else 3 - last                 # (the 3' side's fields stand reverse-complemented in the sense read)
        reads = [cmol(D, p5, p3, body(rng, 80), f, u, t) for t in (20, 19) for f in (wl[2], sub(wl[2], 8), lost(wl[2], 8), gained(wl[2], 8), gained(alt, 0, 1))]
        add(f"polya_shift_{'A' if last == A else 'C'}", both(reads), wl=wl)
    # ---- a primer hit in the field region (primer 2, of 12 bases, is the UMI's first 12): inside the primers' insert, outside the widened one: not internal; the
    # same hit in the insert is (window 30: the copy behind the primer must not stand in the end's window)
    Q = steady(rng, 12)
    d = dict(umi_len=16, bc_len=16, side=1, bc_first=0, indels=1)
    reads = [cmol(d, p5, p3, body(rng, 100), rand(rng, 16), cat(rand(rng, 4), rc(Q))), cmol(d, p5, p3, cat(body(rng, 60), Q, body(rng, 40)), rand(rng, 16), rand(rng, 16))]
    add("internal_in_fields", both(reads), design=d, primers=[p5, p3, Q], roles=(0, 1, 0), window=30)
    # ---- every class at which the rule ends before the tag, both strands; reads of 0, m - 1 and 3001 bases; bytes with high bits set
    wl = whitelist(rng, 16, 16)
    one = cmol(D, p5, p3, body(rng, 150), wl[3], rand(rng, 12))
    reads = [rand(rng, 400), cat(p5, body(rng, 200)), cat(body(rng, 200), rc(p3)), cat(p5, body(rng, 150), rc(p5)), cat(p3, body(rng, 150), rc(p3)), cat(p5, rc(p3)),
             cat(one, one)]
    add("classes", both(reads), wl=wl)
    long = cmol(D, p5, p3, body(rng, 3001 - 50 - 28 - 30), sub(wl[7], 1), rand(rng, 12))
    high = (one | (rng.integers(0, 64, len(one)).astype(np.uint8) << 2)).astype(np.uint8)
    add("sizes", [np.zeros(0, np.uint8), p5[:24], long, rc(long), high, rc(one) | np.uint8(0x80)], wl=wl)
    # ---- n = 0, 1 and 257 reads
    add("n0", [], wl=wl)
    add("n1", [one], wl=wl)
    add("n257", [cmol(D, p5, p3, body(rng, 60), sub(wl[k % 16], k % 16) if k % 3 else wl[k % 16], rand(rng, 12), 22) if k % 50 else np.zeros(0, np.uint8) for k in range(257)],
        wl=wl)
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def _expected(i: int) -> dict:
    _, primers, roles, opts, design, wl, reads = limit_cases()[i]
    return cell_reads(primers, roles, reads, design, wl, **opts)


def expected(i: int) -> dict:
    return _expected(i)


def reversed_order(want: dict) -> dict:
    return {k: v[::-1] for k, v in want.items()}


def diff(got, want, fields=FIELDS) -> list:
    """the fields and reads at which a report (an object with FIELDS as attributes, or a dict) differs from `want`"""
    bad = []
    for k in fields:
        g = np.asarray(got[k] if isinstance(got, dict) else getattr(got, k))
        w = np.asarray(want[k])
        if g.shape != w.shape:
            bad.append((k, "shape", g.shape, w.shape))
            continue
        ne = (g.astype(np.int64) != w.astype(np.int64)).reshape(len(w), -1).any(axis=1) if len(w) else np.zeros(0, bool)
        for z in np.flatnonzero(ne)[:4]:
            bad.append((k, int(z), g[z].tolist(), w[z].tolist()))
    return bad

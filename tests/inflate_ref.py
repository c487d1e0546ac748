"""Raw DEFLATE streams for the inflate tests: zlib's own output in every block type, hand-assembled streams for what zlib does not emit on request,
the fixed list of corrupt streams, the limit set (hand-assembled streams at the format's and the decoder's edges, with the block reader that measures them) and
the corrupted streams of the accept-set differential.  The reference of every valid stream is the bytes it was made from (and zlib.decompress agrees: checked
here)."""
from __future__ import annotations

import functools
import random
import zlib

OK, TRUNCATED_INPUT, BAD_BLOCK_TYPE, BAD_STORED_LENGTH, BAD_CODE_LENGTHS, BAD_SYMBOL, BAD_DISTANCE, OUTPUT_OVERRUN, OUTPUT_SHORT = range(9)

OUT_LENGTHS = [0, 1, 2, 257, 258, 259, 32768, 32769, 65280, 65536]


def deflate_raw(data: bytes, level: int = 6, strategy: int = zlib.Z_DEFAULT_STRATEGY, mem_level: int = 8, flush_every: int = 0) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem_level, strategy)
    if not flush_every:
        return c.compress(data) + c.flush()
    out = b""
    for at in range(0, len(data), flush_every):
        out += c.compress(data[at:at + flush_every]) + c.flush(zlib.Z_FULL_FLUSH)
    return out + c.flush()


def block_types(stream: bytes) -> int:
    """BTYPE of the first block"""
    return (stream[0] >> 1) & 3


# ---- content
def acgt(n: int, seed: int) -> bytes:
    r = random.Random(seed)
    return bytes(r.choice(b"ACGT") for _ in range(n))


def codec_noise(n: int, seed: int) -> bytes:
    """pulse-width / IPD codes as CodecV1 stores them: small values with a long tail, barely compressible"""
    r = random.Random(seed)
    return bytes(min(255, int(r.expovariate(1 / 12.0))) for _ in range(n))


def noise(n: int, seed: int) -> bytes:
    return random.Random(seed).randbytes(n)


def text(n: int, seed: int) -> bytes:
    r = random.Random(seed)
    words = [bytes(r.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(r.randint(2, 9))) for _ in range(60)]
    out = bytearray()
    while len(out) < n:
        out += r.choice(words) + b" "
    return bytes(out[:n])


CONTENT = {"acgt": acgt, "codec": codec_noise, "noise": noise, "text": text, "equal": lambda n, seed: bytes([seed & 255]) * n}


# ---- a bit writer and a block encoder for the hand-assembled streams
class Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value: int, nbits: int):          # least significant bit first (header fields, extra bits)
        self.acc |= (value & ((1 << nbits) - 1)) << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code: int, nbits: int):          # a Huffman code: most significant bit first
        for k in range(nbits - 1, -1, -1):
            self.put((code >> k) & 1, 1)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def bytes(self) -> bytes:
        self.align()
        return bytes(self.out)


def canonical(lens) -> dict:
    """symbol -> (code, length) of the canonical code with these lengths (RFC 1951 §3.2.2)"""
    code, out = 0, {}
    for ln in range(1, 16):
        for s, l in enumerate(lens):
            if l == ln:
                out[s] = (code, ln)
                code += 1
        code <<= 1
    return out


LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
PRECODE_LENS = [4] * 13 + [5] * 6          # a complete code over the 19 code-length symbols
PRECODE_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def put_tokens(w: Bits, lit_lens, dist_lens, tokens):
    """tokens: ints (literals) and (length, distance) pairs; the end-of-block code follows"""
    lit, dist = canonical(lit_lens), canonical(dist_lens)
    for t in tokens:
        if isinstance(t, int):
            w.code(*lit[t])
            continue
        if len(t) == 4:                              # (length symbol - 257, its extra value, distance symbol, its extra value): the caller picks the symbols
            ls, lx, ds, dx = t
            w.code(*lit[257 + ls])
            w.put(lx, LEN_EXTRA[ls])
            w.code(*dist[ds])
            w.put(dx, DIST_EXTRA[ds])
            continue
        ln, d = t
        ls = 28 if ln == 258 else max(i for i in range(28) if LEN_BASE[i] <= ln)
        w.code(*lit[257 + ls])
        w.put(ln - LEN_BASE[ls], LEN_EXTRA[ls])
        ds = max(i for i in range(30) if DIST_BASE[i] <= d)
        w.code(*dist[ds])
        w.put(d - DIST_BASE[ds], DIST_EXTRA[ds])
    w.code(*lit[256])


def put_fixed(w: Bits, tokens, final: bool = True):
    w.put(1 if final else 0, 1)
    w.put(1, 2)
    put_tokens(w, FIXED_LIT, FIXED_DIST, tokens)


def put_stored(w: Bits, data: bytes, final: bool = True, nlen: int | None = None):
    w.put(1 if final else 0, 1)
    w.put(0, 2)
    w.align()
    w.put(len(data), 16)
    w.put((len(data) ^ 0xffff) if nlen is None else nlen, 16)
    w.out += data


def put_dynamic_header(w: Bits, hlit: int, hdist: int, cl_ops, final: bool = True, precode=None):
    """cl_ops: the code-length sequence as (symbol 0..18, extra value) pairs, chosen by the caller: that is the point.  precode: the 19 lengths of the
    code-length code (default: all 19 entries of PRECODE_LENS are written); one that is given is written with its trailing zero lengths, in the order of
    RFC 1951 §3.2.7, trimmed (HCLEN = the last non-zero entry, at least 4)"""
    lens, hclen = PRECODE_LENS, 19
    if precode is not None:
        lens = list(precode)
        hclen = max([4] + [k + 1 for k, s in enumerate(PRECODE_ORDER) if lens[s]])
    pre = canonical(lens)
    w.put(1 if final else 0, 1)
    w.put(2, 2)
    w.put(hlit - 257, 5)
    w.put(hdist - 1, 5)
    w.put(hclen - 4, 4)
    for s in PRECODE_ORDER[:hclen]:
        w.put(lens[s], 3)
    for s, extra in cl_ops:
        w.code(*pre[s])
        if s >= 16:
            w.put(extra, {16: 2, 17: 3, 18: 7}[s])


def zeros_ops(n: int):
    ops = []
    while n:
        k = min(n, 138)
        if k >= 11:
            ops.append((18, k - 11))
        elif k >= 3:
            ops.append((17, k - 3))
        else:
            ops += [(0, 0)] * k
        n -= k
    return ops


def plain_ops(lens):
    """every length spelled out, runs of zeros with 17 / 18"""
    ops, i = [], 0
    while i < len(lens):
        if lens[i] == 0:
            j = i
            while j < len(lens) and lens[j] == 0:
                j += 1
            ops += zeros_ops(j - i)
            i = j
        else:
            ops.append((lens[i], 0))
            i += 1
    return ops


def stream_15bit() -> tuple:
    """a literal / length code with lengths 1 .. 15: sub-tables of every depth, the longest code on the end-of-block symbol; one distance code (zlib's
    incomplete one-code tree)"""
    lit = [0] * 258
    syms = list(range(0x41, 0x41 + 14))
    for k, s in enumerate(syms):
        lit[s] = k + 1
    lit[256] = 15
    lit[257] = 15
    dist = [1]
    r = random.Random(15)
    tokens = [r.choice(syms) for _ in range(400)] + syms + [(3, 1)] + syms[::-1]
    w = Bits()
    put_dynamic_header(w, 258, 1, plain_ops(lit + dist))
    put_tokens(w, lit, dist, tokens)
    return w.bytes(), expand(tokens)


def stream_repeat16_across() -> tuple:
    """code-length symbol 16 (repeat the previous length) runs from the last literal / length codes into the distance codes"""
    lit = [0] * 259
    lit[0x41] = lit[256] = lit[257] = lit[258] = 2
    dist = [2, 2, 2, 2]
    ops = zeros_ops(65) + [(2, 0)] + zeros_ops(190) + [(2, 0), (16, 3)]     # 256: 2, then six repeats: 257, 258 and the four distance codes
    tokens = [0x41] * 5 + [(3, 4), (4, 2), 0x41, (3, 1)]
    w = Bits()
    put_dynamic_header(w, 259, 4, ops)
    put_tokens(w, lit, dist, tokens)
    return w.bytes(), expand(tokens)


def stream_repeat18_across() -> tuple:
    """code-length symbol 18 (a run of zeros) runs from the literal / length codes into the distance codes"""
    lit = [0] * 270
    lit[0x41], lit[256], lit[257] = 1, 2, 2
    dist = [0] * 10 + [1, 1]
    ops = zeros_ops(65) + [(1, 0)] + zeros_ops(190) + [(2, 0), (2, 0), (18, 22 - 11), (1, 0), (1, 0)]   # 12 zeros of the literal code + 10 of the distance code
    tokens = [0x41] * 50 + [(3, 33), (3, 49), 0x41]
    w = Bits()
    put_dynamic_header(w, 270, 12, ops)
    put_tokens(w, lit, dist, tokens)
    return w.bytes(), expand(tokens)


def stream_stored_after_dynamic() -> tuple:
    """a dynamic block that ends inside a byte, then a stored block: the decoder re-aligns to the byte boundary"""
    lit = [0] * 258
    lit[0x41], lit[0x43], lit[256], lit[257] = 1, 2, 3, 3
    dist = [1, 1]
    tokens = [0x41, 0x43, 0x41, (3, 2), 0x43]
    tail = b"stored bytes after a dynamic block"
    w = Bits()
    put_dynamic_header(w, 258, 2, plain_ops(lit + dist), final=False)
    put_tokens(w, lit, dist, tokens)
    put_stored(w, tail, final=False)
    put_fixed(w, [0x5a, (10, 1)])
    return w.bytes(), expand(tokens) + tail + b"Z" * 11


def stream_long_matches() -> tuple:
    """a match of length 258 at distance 32768, then at distances 1, 2 and 3 (overlapping copies)"""
    head = noise(32768, 258)
    tokens = list(head) + [(258, 32768), (258, 1), 0x61, 0x62, (258, 2), 0x63, (258, 3)]
    w = Bits()
    put_fixed(w, tokens)
    return w.bytes(), expand(tokens)


def expand(tokens) -> bytes:
    out = bytearray()
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            ln, d = (LEN_BASE[t[0]] + t[1], DIST_BASE[t[2]] + t[3]) if len(t) == 4 else t
            for _ in range(ln):
                out.append(out[-d])
    return bytes(out)


@functools.lru_cache(maxsize=None)
def valid_cases() -> tuple:
    """(name, stream, expected bytes) — computed once, shared by the host and the GPU tests"""
    cases = []

    def add(name, stream, data):
        assert zlib.decompress(stream, -15) == data, name          # the reference's own check
        cases.append((name, stream, data))

    for n in OUT_LENGTHS:
        add(f"len{n}-text", deflate_raw(text(n, n)), text(n, n))
        add(f"len{n}-noise-stored", deflate_raw(noise(n, n), level=0), noise(n, n))
    big = acgt(40000, 1)
    variants = {"stored": dict(level=0), "fixed": dict(strategy=zlib.Z_FIXED), "default": dict(), "huffman-only": dict(strategy=zlib.Z_HUFFMAN_ONLY),
                "rle": dict(strategy=zlib.Z_RLE), "memlevel1": dict(mem_level=1), "full-flush": dict(flush_every=5000)}
    for name, kw in variants.items():
        s = deflate_raw(big, **kw)
        assert block_types(s) == {"stored": 0, "fixed": 1}.get(name, 2), name
        add(f"acgt-{name}", s, big)
    for kind in ("codec", "noise", "text"):
        d = CONTENT[kind](65536, 7)
        add(f"{kind}-65536", deflate_raw(d), d)
        add(f"{kind}-65536-flush", deflate_raw(d, flush_every=5000), d)
    z = bytes(65536)
    assert len(deflate_raw(z)) == 78 and deflate_raw(b"") == b"\x03\x00"
    add("zeros-65536", deflate_raw(z), z)
    add("empty", deflate_raw(b""), b"")
    add("equal-1000", deflate_raw(b"\x07" * 1000), b"\x07" * 1000)
    for name, f in (("15-bit-code", stream_15bit), ("repeat16-across", stream_repeat16_across), ("repeat18-across", stream_repeat18_across),
                    ("stored-after-dynamic", stream_stored_after_dynamic), ("long-matches", stream_long_matches)):
        add(name, *f())
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def fuzz_cases(n: int = 300, seed: int = 20260) -> tuple:
    r = random.Random(seed)
    strategies = [zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FILTERED]
    out = []
    for i in range(n):
        length = r.choice([r.randint(0, 600), r.randint(0, 9000), r.randint(0, 65536)])
        data = CONTENT[r.choice(sorted(CONTENT))](length, r.randint(0, 1 << 30))
        stream = deflate_raw(data, level=r.randint(0, 9), strategy=r.choice(strategies), mem_level=r.randint(1, 9), flush_every=r.choice([0, 0, 700, 5000]))
        out.append((f"fuzz{i}", stream, data))
    return tuple(out)


def short_stream() -> tuple:
    data = b"GATTACA GATTACA CATTAGA GATTACA, the quick brown fox; GATTACA"
    return deflate_raw(data), data


@functools.lru_cache(maxsize=None)
def corrupt_cases() -> tuple:
    """(name, stream, out_len, status or None when more than one cause is possible) — the fixed list"""
    s, d = short_stream()
    cases = [(f"truncated-at-{k}", s[:k], len(d), TRUNCATED_INPUT) for k in range(len(s))]
    cases.append(("block-type-3", b"\x07\x00\x00", 4, BAD_BLOCK_TYPE))
    w = Bits()
    put_stored(w, b"abcd", nlen=0x1234)
    cases.append(("stored-len-nlen", w.bytes(), 4, BAD_STORED_LENGTH))
    w = Bits()
    lit = [0] * 257
    lit[0x41] = lit[0x42] = lit[256] = 1                                   # three codes of one bit
    put_dynamic_header(w, 257, 1, plain_ops(lit + [1]))
    w.put(0, 32)
    cases.append(("over-subscribed", w.bytes(), 4, BAD_CODE_LENGTHS))
    w = Bits()
    lit = [0] * 257
    lit[0x41], lit[256] = 1, 2                                             # a quarter of the code space is missing
    put_dynamic_header(w, 257, 1, plain_ops(lit + [1]))
    w.put(0, 32)
    cases.append(("under-subscribed", w.bytes(), 4, BAD_CODE_LENGTHS))
    w = Bits()
    w.put(1, 1)
    w.put(1, 2)
    lit, dist = canonical(FIXED_LIT), canonical(FIXED_DIST)
    for c in (lit[0x61], lit[257], dist[1], lit[256]):                     # 'a', then length 3 at distance 2
        w.code(*c)
    cases.append(("distance-before-start", w.bytes(), 4, BAD_DISTANCE))
    cases.append(("out-len-one-too-small", s, len(d) - 1, OUTPUT_OVERRUN))
    cases.append(("out-len-one-too-large", s, len(d) + 1, OUTPUT_SHORT))
    cases += more_corrupt_cases()
    return tuple(cases)


def flip_cases(n: int = 400, seed: int = 77) -> list:
    """single-byte flips of three short streams (stored, fixed, dynamic): (stream, out_len)"""
    r = random.Random(seed)
    d = text(700, 3) + acgt(500, 4)
    bases = [deflate_raw(d, level=0), deflate_raw(d, strategy=zlib.Z_FIXED), deflate_raw(d), stream_15bit()[0], stream_repeat18_across()[0]]
    lens = [len(d)] * 3 + [len(stream_15bit()[1]), len(stream_repeat18_across()[1])]
    out = []
    for _ in range(n):
        k = r.randrange(len(bases))
        b = bytearray(bases[k])
        # the header bytes are where a flip does the most: half the draws land in the first 40 bytes
        at = r.randrange(min(40, len(b))) if r.random() < 0.5 else r.randrange(len(b))
        b[at] ^= 1 << r.randrange(8)
        out.append((bytes(b), lens[k]))
    return out


# ---- a reader: the blocks of a valid stream, header by header and token by token (what the limit sets are measured with)
LIT_PRIMARY, DIST_PRIMARY = 10, 8        # CCSX_INFL_LIT_BITS, CCSX_INFL_DIST_BITS


class BitReader:
    def __init__(self, data: bytes):
        self.d, self.at = data, 0                    # at: the next bit

    def bit(self) -> int:
        byte = self.at >> 3
        if byte > len(self.d) + 8:                   # (a stream without a final block must not keep a walk going on zeros)
            raise ValueError("the stream ends before its final block")
        self.at += 1
        return (self.d[byte] >> ((self.at - 1) & 7)) & 1 if byte < len(self.d) else 0     # (behind the end: zeros, as the decoder's bit buffer reads)

    def get(self, n: int) -> int:
        return sum(self.bit() << k for k in range(n))

    def sym(self, dec: dict) -> tuple:
        code = 0
        for ln in range(1, 16):
            code = (code << 1) | self.bit()
            if (ln, code) in dec:
                return dec[(ln, code)], ln, code
        raise ValueError("a codeword that stands for nothing")


def decoder(lens) -> dict:
    return {(ln, code): s for s, (code, ln) in canonical(lens).items()}


def sub_tables(lens, primary: int) -> dict:
    """primary-bit prefix -> index bits of the sub-table behind it (the longest code with that prefix, less the primary bits)"""
    out = {}
    for code, ln in canonical(lens).values():
        if ln > primary:
            out[code >> (ln - primary)] = max(out.get(code >> (ln - primary), 0), ln - primary)
    return out


def _walk_symbol(r: BitReader, dec: dict, subs: dict, primary: int, seen: set) -> int:
    at = r.at
    s, ln, code = r.sym(dec)
    if ln > primary:                                 # the sub-table entry this look-up reads: the bits behind the prefix, as many as the sub-table has
        prefix = code >> (ln - primary)
        r.at = at + primary
        seen.add((prefix, r.get(subs[prefix])))
        r.at = at + ln
    return s


def walk_blocks(stream: bytes) -> list:
    """one dict per block of a valid stream: final, btype, tokens (literals and (length, distance) pairs), for a dynamic block hlit / hdist / hclen / pre / lit /
    dist (the three codes' lengths) and lit_seen / dist_seen, the (prefix, index) pairs of the sub-table entries the symbol loop looks up; end_bit on the last"""
    r, blocks = BitReader(stream), []
    while True:
        blk = dict(final=r.get(1), btype=r.get(2), tokens=[], lit_seen=set(), dist_seen=set())
        blocks.append(blk)
        if blk["btype"] == 3:
            raise ValueError("block type 3")
        if blk["btype"] == 0:
            r.at = (r.at + 7) & ~7
            n = r.get(16)
            if n ^ r.get(16) != 0xffff:
                raise ValueError("LEN / NLEN")
            blk["tokens"] = list(stream[r.at >> 3:(r.at >> 3) + n])
            r.at += 8 * n
        else:
            lit, dist = FIXED_LIT, FIXED_DIST
            if blk["btype"] == 2:
                hlit, hdist, hclen = r.get(5) + 257, r.get(5) + 1, r.get(4) + 4
                pre = [0] * 19
                for s in PRECODE_ORDER[:hclen]:
                    pre[s] = r.get(3)
                dec, lens = decoder(pre), []
                while len(lens) < hlit + hdist:
                    s = r.sym(dec)[0]
                    lens += [s] if s < 16 else [lens[-1]] * (3 + r.get(2)) if s == 16 else [0] * (3 + r.get(3)) if s == 17 else [0] * (11 + r.get(7))
                lit, dist = lens[:hlit], lens[hlit:hlit + hdist]
                blk.update(hlit=hlit, hdist=hdist, hclen=hclen, pre=pre)
            blk.update(lit=lit, dist=dist)
            ld, dd, ls, ds = decoder(lit), decoder(dist), sub_tables(lit, LIT_PRIMARY), sub_tables(dist, DIST_PRIMARY)
            while True:
                s = _walk_symbol(r, ld, ls, LIT_PRIMARY, blk["lit_seen"])
                if s == 256:
                    break
                if s < 256:
                    blk["tokens"].append(s)
                    continue
                ln = LEN_BASE[s - 257] + r.get(LEN_EXTRA[s - 257])
                d = _walk_symbol(r, dd, ds, DIST_PRIMARY, blk["dist_seen"])
                blk["tokens"].append((ln, DIST_BASE[d] + r.get(DIST_EXTRA[d])))
        if blk["final"]:
            blk["end_bit"] = r.at
            return blocks


def zlib_inflate(stream: bytes, limit: int = 65536):
    """what zlib makes of a raw stream: its bytes when it reaches the end of the final block with at most `limit` of them (bytes behind it are ignored), else None"""
    z = zlib.decompressobj(-15)
    try:
        out = z.decompress(stream, limit + 1)
    except zlib.error:
        return None
    return out if z.eof and len(out) <= limit else None


# ---- the limit set: hand-assembled valid streams at the format's and the decoder's edges
def grow_code(r: random.Random, n: int, maxlen: int, exact: bool = False) -> list:
    """the lengths of a complete code of n >= 2 codewords, none longer than maxlen, grown from (1, 1) by splitting random leaves; exact: the longest is maxlen
    (a spine first: n > maxlen)"""
    lens = [1, 1]

    def split(i):
        ln = lens.pop(i)
        lens.extend([ln + 1, ln + 1])

    while exact and max(lens) < maxlen:
        split(lens.index(max(lens)))
    while len(lens) < n:
        split(r.choice([i for i, ln in enumerate(lens) if ln < maxlen]))
    assert len(lens) == n and sum(1 << (15 - ln) for ln in lens) == 1 << 15 and (not exact or max(lens) == maxlen)
    return lens


def rle_ops(lens, r: random.Random) -> list:
    """the code-length sequence of these lengths with 16 / 17 / 18 wherever the draw says so, runs of random length"""
    ops, i = [], 0
    while i < len(lens):
        v, j = lens[i], i
        while j < len(lens) and lens[j] == v:
            j += 1
        run = j - i
        if v == 0 and run >= 3 and r.random() < 0.8:
            k = r.randint(3, min(run, 138))
            ops.append((18, k - 11) if k >= 11 else (17, k - 3))
        elif i > 0 and lens[i - 1] == v and run >= 3 and r.random() < 0.7:
            k = r.randint(3, min(run, 6))
            ops.append((16, k - 3))
        else:
            k = 1
            ops.append((v, 0))
        i += k
    return ops


def precode_for(ops, lens_by_rank=None, r: random.Random | None = None) -> list:
    """a complete code-length code over the symbols these ops use: lens_by_rank[k] for the k-th used symbol in ascending order, or a random code of up to 7 bits"""
    used = sorted({s for s, _ in ops})
    if len(used) < 2:
        used = sorted(set(used) | {0, 1})
    if lens_by_rank is None:
        lens_by_rank = grow_code(r, len(used), 7)
        r.shuffle(lens_by_rank)
    assert len(lens_by_rank) == len(used) and sum(1 << (7 - ln) for ln in lens_by_rank) == 128, (used, lens_by_rank)
    pre = [0] * 19
    for s, ln in zip(used, lens_by_rank):
        pre[s] = ln
    return pre


def dynamic_block(w: Bits, lit, dist, tokens, final: bool = True, hlit: int | None = None, hdist: int | None = None, ops=None, precode=None):
    lit = list(lit) + [0] * ((hlit or 257) - len(lit))
    dist = list(dist) + [0] * ((hdist or 1) - len(dist))
    put_dynamic_header(w, len(lit), len(dist), plain_ops(lit + dist) if ops is None else ops, final=final, precode=precode)
    put_tokens(w, lit, dist, tokens)


def stream_random_codes(seed: int, want_lit: int | None, want_dist: int | None, max_out: int = 4096) -> tuple:
    """random complete codes: 2 .. 286 literal / length symbols (256 and one literal among them) and 2 .. 30 distance symbols of up to 15 bits (want_*: the longest
    is exactly that), HLIT / HDIST anywhere above the highest used symbol, the lengths run-length coded at random under a random code-length code, then 0 .. 400
    random tokens with random extra bits"""
    r = random.Random(seed)
    nlit = r.choice([r.randint(max(2, (want_lit or 0) + 1), max(40, (want_lit or 0) + 1)), r.randint(max(2, (want_lit or 0) + 1), 286)])
    ndist = r.randint(max(2, (want_dist or 0) + 1), 30)
    used_lit = [256, r.randrange(256)]
    used_lit += r.sample([s for s in range(286) if s not in used_lit], nlit - 2)
    used_dist = r.sample(range(30), ndist)
    lit, dist = [0] * r.randint(max(257, max(used_lit) + 1), 286), [0] * r.randint(max(used_dist) + 1, 30)
    for s, ln in zip(used_lit, grow_code(r, nlit, want_lit or 15, exact=want_lit is not None)):      # (used_* are in random order already)
        lit[s] = ln
    for s, ln in zip(used_dist, grow_code(r, ndist, want_dist or 15, exact=want_dist is not None)):
        dist[s] = ln
    ops = rle_ops(lit + dist, r)
    lits, lsyms = [s for s in used_lit if s < 256], [s - 257 for s in used_lit if s > 256]
    tokens, op = [], 0
    for _ in range(r.randint(0, 400)):
        if lsyms and op and r.random() < 0.4:
            ls = r.choice(lsyms)
            lx = r.randrange(1 << LEN_EXTRA[ls])
            near = [d for d in used_dist if DIST_BASE[d] <= op]
            if near and op + LEN_BASE[ls] + lx <= max_out:
                ds = r.choice(near)
                tokens.append((ls, lx, ds, r.randint(0, min((1 << DIST_EXTRA[ds]) - 1, op - DIST_BASE[ds]))))
                op += LEN_BASE[ls] + lx
                continue
        if op >= max_out:
            break
        tokens.append(r.choice(lits))
        op += 1
    w = Bits()
    dynamic_block(w, lit, dist, tokens, hlit=len(lit), hdist=len(dist), ops=ops, precode=precode_for(ops, r=r))
    return w.bytes(), expand(tokens)


def _short_lens(nprefix: int, primary: int) -> list:
    """the lengths (<= primary) of the codes that fill what nprefix prefixes of `primary` bits leave free: one per binary digit of 2^primary - nprefix"""
    free = (1 << primary) - nprefix
    return [primary - k for k in range(primary - 1, -1, -1) if (free >> k) & 1]


def _deep(groups, primary: int) -> list:
    """(length, trailing bits: the index bits of its sub-table that the code itself does not fill) of the codes behind the primary table: each group fills one
    prefix exactly and the groups are in canonical order, so the canonical code keeps them together"""
    flat = [ln for g in groups for ln in g]
    assert flat == sorted(flat) and all(sum(1 << (15 - ln) for ln in g) == 1 << (15 - primary) for g in groups)
    return [(ln, max(g) - ln) for g in groups for ln in g]


def stream_lit_subtables(groups) -> tuple:
    """a literal / length code whose codes of more than 10 bits lie behind len(groups) prefixes, each group's lengths behind one; every entry of every (replicated)
    sub-table is looked up: a deep symbol is followed by every pattern of the index bits it leaves free, spelled with the short codes (0, 10, 110, ...: one
    short code per length) or, behind a length symbol, with the one-bit distance codes first"""
    short, deep = _short_lens(len(groups), LIT_PRIMARY), _deep(groups, LIT_PRIMARY)
    assert short[:5] == [1, 2, 3, 4, 5]
    lit = [0] * 259
    by_len = {}
    for k, ln in enumerate(short):
        lit[0x61 + k] = ln
        by_len[ln] = 0x61 + k
    # the deep symbols: literals '0' upward, the two length symbols 257 (3) and 258 (4) as the last codes of the first deep length, 256 the very last code
    syms, nxt = [], 0x30
    n_first = sum(1 for ln, _ in deep if ln == deep[0][0])
    for k, (ln, t) in enumerate(deep):
        if max(0, n_first - 2) <= k < n_first:
            syms.append(257 + k - max(0, n_first - 2))
        elif k == len(deep) - 1:
            assert t == 0
            syms.append(256)
        else:
            syms.append(nxt)
            nxt += 1
        lit[syms[-1]] = ln

    def spell(bits):
        out, run = [], 0
        for b in bits:
            if b:
                run += 1
            else:
                out.append(by_len[run + 1])
                run = 0
        return out + ([by_len[run + 1]] if run else [])

    tokens = [0x61, 0x62, 0x61]
    for s, (ln, t) in zip(syms, deep):
        if s == 256:
            continue
        for pattern in range(1 << t):
            bits = [(pattern >> k) & 1 for k in range(t)]
            tokens += [s] + spell(bits) if s < 256 else [(s - 257, 0, bits[0] if bits else 0, 0)] + spell(bits[1:])
    w = Bits()
    dynamic_block(w, lit, [1, 1], tokens, hlit=259, hdist=2)
    return w.bytes(), expand(tokens)


def stream_dist_subtables(groups) -> tuple:
    """the same behind the distance code's 8-bit primary table: the index bits a deep code leaves free are the first extra bits of its symbol, so the deep symbols
    are those with extra bits enough, every value of them is used, and the output before them is long enough for their distances"""
    short, deep = _short_lens(len(groups), DIST_PRIMARY), _deep(groups, DIST_PRIMARY)
    dist, deep_syms, s = [0] * 30, [], 4
    for ln, t in deep:                               # ascending symbols: the canonical order within a length is the order of this list
        while DIST_EXTRA[s] < t:
            s += 1
        deep_syms.append(s)
        dist[s] = ln
        s += 1
    short_syms = [k for k in range(30) if not dist[k]][:len(short)]
    assert short_syms[:2] == [0, 1]
    for k, ln in zip(short_syms, short):
        dist[k] = ln
    lit = [0] * 286
    lit[0x61], lit[0x62], lit[285], lit[256], lit[257] = 2, 2, 2, 3, 3
    far = max(DIST_BASE[k] + (1 << DIST_EXTRA[k]) for k in deep_syms + short_syms)
    tokens = [0x61, 0x62] + [(28, 0, 1, 0)] * (far // 258 + 1)                     # abab... : length 258 at distance 2
    for k, (ln, t) in zip(deep_syms, deep):
        tokens += [(0, 0, k, x) for x in range(1 << t)] + [0x61]
    tokens += [(0, 0, k, (1 << DIST_EXTRA[k]) - 1) for k in short_syms]
    w = Bits()
    dynamic_block(w, lit, dist, tokens, hlit=286, hdist=30)
    return w.bytes(), expand(tokens)


LIT_ONE_PREFIX = [[11, 12, 13, 14, 15, 15]]
LIT_ONE_PREFIX_B = [[12, 12, 12, 13, 14, 15, 15]]
LIT_MANY_PREFIXES = [[11, 11], [11, 11], [11, 12, 12], [12, 12, 13, 13, 13, 13], [13] * 4 + [14] * 8, [14] * 8 + [15] * 16]        # sub-tables of 1, 1, 2, 3, 4, 5 bits
DIST_ONE_PREFIX = [[9, 10, 11, 12, 13, 14, 15, 15]]
DIST_MANY_PREFIXES = [[9, 9], [9, 10, 10], [10, 10, 11, 11, 11, 11], [11] * 4 + [12] * 8]                                        # sub-tables of 1, 2, 3, 4 bits


def _fixed(tokens) -> tuple:
    w = Bits()
    put_fixed(w, tokens)
    return w.bytes(), expand(tokens)


def stream_precode(kind: str) -> tuple:
    """the code-length code at HCLEN 5, 12 and 19 and at 7 bits (HCLEN 4 writes 16, 17, 18 and 0 only: every length is then 0, there is no end-of-block code and
    no valid block - that one is in corrupt_cases())"""
    if kind == "hclen5":                             # 0 and 8 only: 256 literal / length codes of 8 bits, no distance code
        lit = [8] * 255 + [0, 8]
        ops, ranks = [(ln, 0) for ln in lit + [0]], [1, 1]
        dist, tokens = [0], list(b"HCLEN five") + [254, 0, 1]
    elif kind == "hclen12":                          # 4, 5 and the zero runs: fifteen codes of 4 bits, two of 5; sixteen distance codes of 4 bits
        lit = [0] * 258
        for s in range(0x61, 0x70):
            lit[s] = 4
        lit[256] = lit[257] = 5
        dist, ops, ranks = [4] * 16, None, [2, 2, 2, 2]
        tokens = list(b"abcdefghijklmno") + [(3, 15), (3, 1), 0x6f, (3, 16)]
    elif kind == "hclen19":                          # 1 .. 15 all used
        lit = [0] * 258
        for k in range(14):
            lit[0x41 + k] = k + 1
        lit[256] = lit[257] = 15
        dist, ops, ranks = [1, 1], None, None
        tokens = list(range(0x41, 0x4f)) + [(3, 1), (3, 2)]
    else:                                            # eight code-length symbols (1 .. 6, 17, 18) under lengths 3 4 5 6 7 7 | 2 1
        lit = [0] * 258
        lit[0x41], lit[0x45], lit[0x49], lit[0x4d], lit[0x51], lit[256], lit[257] = 1, 2, 3, 4, 5, 6, 6
        dist, ops, ranks = [1, 1], None, [3, 4, 5, 6, 7, 7, 2, 1]
        tokens = [0x41, 0x45, 0x49, 0x4d, 0x51, (3, 1), (3, 2), 0x41]
    w = Bits()
    full = lit + dist
    ops = plain_ops(full) if ops is None else ops
    put_dynamic_header(w, len(lit), len(dist), ops, precode=precode_for(ops, ranks, random.Random(19)))
    put_tokens(w, lit, dist, tokens)
    return w.bytes(), expand(tokens)


def stream_header_extreme(kind: str) -> tuple:
    w = Bits()
    if kind == "hlit286":                            # 285 (258, no extra bits) and 284 with extra 30 (257) and 31 (258 again, as zlib reads it)
        lit = [0] * 286
        lit[0x61], lit[256], lit[284], lit[285] = 1, 2, 3, 3
        tokens = [0x61, (28, 0, 0, 0), (27, 30, 1, 0), 0x61, (27, 31, 0, 0), (27, 0, 1, 0)]
        dynamic_block(w, lit, [1, 1], tokens, hlit=286, hdist=2)
    elif kind == "hlit257-hdist1-empty":             # the smallest header: no length symbol, HDIST 1 with length 0
        lit = [0] * 257
        lit[0x61], lit[256] = 1, 1
        tokens = [0x61] * 9
        dynamic_block(w, lit, [0], tokens)
    elif kind == "hlit257-one-distance":
        lit = [0] * 257
        lit[0x61], lit[256] = 1, 1
        tokens = [0x61] * 3
        dynamic_block(w, lit, [1], tokens)
    else:                                            # HDIST 30: symbols 28 and 29 at both ends of their 13 extra bits
        lit = [0] * 286
        lit[0x61], lit[0x62], lit[0x63], lit[256], lit[257], lit[285] = 3, 3, 3, 3, 2, 2
        dist = [0] * 30
        dist[2], dist[28], dist[29] = 1, 2, 2
        tokens = [0x61, 0x62, 0x63] + [(258, 3)] * 127 + [(3, 16385), (3, 24576), 0x62, (3, 24577), (3, 32768), 0x61]
        dynamic_block(w, lit, dist, tokens, hlit=286, hdist=30)
    return w.bytes(), expand(tokens)


def stream_lone_eob(then_stored: bool) -> tuple:
    """a dynamic block whose literal / length code is the end-of-block symbol alone, at 1 bit (zlib's `max == 1` rule): empty"""
    w = Bits()
    put_dynamic_header(w, 257, 1, zeros_ops(256) + [(1, 0), (0, 0)], final=not then_stored)
    w.code(0, 1)
    if then_stored:
        put_stored(w, b"behind a lone end-of-block code")
    return w.bytes(), b"behind a lone end-of-block code" if then_stored else b""


def _nine_bit(m: int) -> list:
    return [0x90 + k for k in range(m)]              # the fixed code gives the bytes from 144 nine bits: a fixed block of three 8-bit literals and m of these has (6 - m) % 8 pad bits


@functools.lru_cache(maxsize=None)
def limit_cases() -> tuple:
    """(name, stream, expected bytes): the hand-assembled streams at the limits, computed once"""
    cases = []

    def add(name, stream, data):
        assert zlib_inflate(stream) == data == zlib.decompress(stream, -15), name          # the reference's own check
        cases.append((name, stream, data))

    lit_max, dist_max = [None, 11, 12, 13, 14, 15], [None, 9, 10, 11, 12, 13, 14, 15]
    for i in range(200):
        add(f"codes{i}", *stream_random_codes(4000 + i, lit_max[i % 6], dist_max[i % 8]))
    for kind in ("hclen5", "hclen12", "hclen19", "precode-7-bits"):
        add(kind, *stream_precode(kind))
    for kind in ("hlit286", "hlit257-hdist1-empty", "hlit257-one-distance", "hdist30"):
        add(kind, *stream_header_extreme(kind))
    add("lit-one-prefix", *stream_lit_subtables(LIT_ONE_PREFIX))
    add("lit-one-prefix-b", *stream_lit_subtables(LIT_ONE_PREFIX_B))
    add("lit-many-prefixes", *stream_lit_subtables(LIT_MANY_PREFIXES))
    add("dist-one-prefix", *stream_dist_subtables(DIST_ONE_PREFIX))
    add("dist-many-prefixes", *stream_dist_subtables(DIST_MANY_PREFIXES))
    # overlapping copies over 64 lanes
    head = list(noise(300, 64))
    for d in (63, 64, 65, 127, 128, 129):
        add(f"overlap-258-at-{d}", *_fixed(head + [(258, d), 0x21, (258, d)]))
    add("three-at-one-after-a-literal", *_fixed([0x78, (3, 1), 0x79, (3, 1), (3, 4)]))
    w = Bits()
    put_stored(w, noise(100, 65), final=False)
    put_fixed(w, [(50, 60), (258, 100), 0x21, (40, 150)])
    add("match-from-a-stored-block", w.bytes(), expand(list(noise(100, 65)) + [(50, 60), (258, 100), 0x21, (40, 150)]))
    add("match-from-the-match-before", *_fixed(list(b"abcde") + [(20, 5), (20, 20), (258, 10), (258, 258), (100, 99)]))
    # bit-reader edges
    for m in range(8):
        w = Bits()
        put_fixed(w, list(b"pad") + _nine_bit(m))
        pad = (8 - w.n) % 8
        assert pad == (6 - m) % 8
        add(f"final-block-{pad}-pad-bits", w.bytes(), b"pad" + bytes(_nine_bit(m)))
    add("two-bytes", *_fixed([]))
    add("three-bytes", *_fixed([0x41]))
    add("three-bytes-nine-bit-literal", *_fixed([0xf0]))
    assert [len(c[1]) for c in cases[-3:]] == [2, 3, 3]
    w = Bits()
    put_fixed(w, list(b"before"), final=False)
    put_stored(w, b"", final=False)
    dynamic_block(w, *([0] * 0x61 + [1] + [0] * 158 + [2, 2], [1, 1], [0x61, (3, 1), (3, 2)]))
    add("empty-stored-between-huffman-blocks", w.bytes(), b"before" + b"a" * 7)
    for m in range(8):                               # a Huffman block that ends at every bit of a byte, two stored blocks of one byte, a last one of m bytes
        w = Bits()
        put_fixed(w, _nine_bit(m), final=False)
        put_stored(w, b"x", final=False)
        put_stored(w, b"y", final=False)
        put_stored(w, bytes(range(m)))
        add(f"stored-back-to-back-{m}", w.bytes(), bytes(_nine_bit(m)) + b"xy" + bytes(range(m)))
    add("lone-end-of-block", *stream_lone_eob(False))
    add("lone-end-of-block-then-stored", *stream_lone_eob(True))
    s, d = short_stream()
    add("bytes-behind-the-final-block", s + b"\xff" * 9, d)
    return tuple(cases)


def code_shape(stream: bytes) -> dict:
    """of the stream's dynamic blocks: the longest literal / length, distance and code-length code, and the HCLENs"""
    b = [k for k in walk_blocks(stream) if k["btype"] == 2]
    return dict(lit=max([max(k["lit"]) for k in b], default=0), dist=max([max(k["dist"]) for k in b], default=0), pre=max([max(k["pre"]) for k in b], default=0),
                hclen={k["hclen"] for k in b})


def _bad(put, tail_bits: int = 32) -> bytes:
    w = Bits()
    put(w)
    w.put(0, tail_bits)
    return w.bytes()


def more_corrupt_cases() -> list:
    """one stream per documented cause that corrupt_cases() did not hold: (name, stream, out_len, status).  zlib rejects every one (checked here)"""
    A = [0] * 65 + [1] + [0] * 190 + [2, 2]          # 'A' 1 bit, 256 and 257 two bits
    a_lit, a_eob, a_len = (0, 1), (2, 2), (3, 2)
    fl, fd = canonical(FIXED_LIT), canonical([5] * 32)
    c = []

    def lone_unused(w):
        put_dynamic_header(w, 257, 1, zeros_ops(256) + [(1, 0), (0, 0)])
        w.code(1, 1)
    c.append(("lone-eob-unused-codeword", _bad(lone_unused), 4, BAD_SYMBOL))

    def one_distance_unused(w):
        put_dynamic_header(w, 258, 1, plain_ops(A + [1]))
        for code in (a_lit, a_lit, a_lit, a_len, (1, 1)):
            w.code(*code)
    c.append(("one-code-distance-unused-codeword", _bad(one_distance_unused), 8, BAD_SYMBOL))

    def empty_distance_used(w):
        put_dynamic_header(w, 258, 1, plain_ops(A + [0]))
        for code in (a_lit, a_lit, a_lit, a_len):
            w.code(*code)
    c.append(("empty-distance-code-used", _bad(empty_distance_used), 8, BAD_SYMBOL))

    def fixed_286(w):
        w.put(3, 3)
        w.code(*fl[0x61])
        w.code(*fl[286])
    c.append(("fixed-litlen-286", _bad(fixed_286), 8, BAD_SYMBOL))

    def fixed_d30(w):
        w.put(3, 3)
        for code in (fl[0x61], fl[257], fd[30]):
            w.code(*code)
    c.append(("fixed-distance-30", _bad(fixed_d30), 8, BAD_SYMBOL))
    for name, hlit, hdist in (("hlit-287", 287, 1), ("hlit-288", 288, 1), ("hdist-31", 258, 31), ("hdist-32", 258, 32)):
        c.append((name, _bad(lambda w: put_dynamic_header(w, hlit, hdist, plain_ops(A + [1]))), 4, BAD_CODE_LENGTHS))
    c.append(("repeat-16-first", _bad(lambda w: put_dynamic_header(w, 258, 1, [(16, 0)] + plain_ops(A[3:] + [1]))), 4, BAD_CODE_LENGTHS))
    c.append(("zeros-18-past-the-end", _bad(lambda w: put_dynamic_header(w, 258, 1, plain_ops(A) + [(18, 0)])), 4, BAD_CODE_LENGTHS))
    c.append(("repeat-16-past-the-end", _bad(lambda w: put_dynamic_header(w, 258, 2, plain_ops(A) + [(2, 0), (16, 0)])), 4, BAD_CODE_LENGTHS))
    two = [0] * 65 + [1, 1] + [0] * 190
    c.append(("no-end-of-block-code", _bad(lambda w: put_dynamic_header(w, 257, 1, plain_ops(two + [1]))), 4, BAD_CODE_LENGTHS))
    for name, pre in (("precode-one-codeword", {0: 1}), ("precode-three-one-bit", {0: 1, 1: 1, 2: 1}), ("precode-all-zero", {}), ("hclen-4", {18: 1, 0: 1})):
        lens = [pre.get(s, 0) for s in range(19)]
        ops = [(18, 127), (18, 109)] if name == "hclen-4" else []                    # (HCLEN 4 is a complete code of 18 and 0: 258 lengths of 0)
        c.append((name, _bad(lambda w: put_dynamic_header(w, 257, 1, ops, precode=lens)), 4, BAD_CODE_LENGTHS))
    for name, dist in (("distance-three-one-bit", [1, 1, 1]), ("distance-lengths-1-2", [1, 2]), ("distance-one-codeword-of-2", [2])):
        c.append((name, _bad(lambda w: put_dynamic_header(w, 258, len(dist), plain_ops(A + dist))), 4, BAD_CODE_LENGTHS))
    w = Bits()
    w.put(1, 3)
    w.align()
    w.put(10, 16)
    w.put(10 ^ 0xffff, 16)
    c.append(("stored-len-10-three-bytes-left", w.bytes() + b"abc", 10, TRUNCATED_INPUT))
    c.append(("one-byte", b"\x03", 0, TRUNCATED_INPUT))                                    # (no valid stream has one byte: the shortest, an empty fixed block, has ten bits)
    for name, s, _, _ in c:
        assert zlib_inflate(s) is None, name
    return c


def diff_bases() -> list:
    """(stream, out_len) of the short streams that the accept-set differential corrupts"""
    return [(s, len(d)) for _, s, d in limit_cases() + valid_cases() if len(s) < 3000]


@functools.lru_cache(maxsize=None)
def diff_cases(n: int = 24000, seed: int = 1951) -> tuple:
    """(stream, the base stream's out_len): 1 .. 3 bit flips each, every flip in the first 40 bytes on one draw of two; a tenth are truncated as well"""
    r = random.Random(seed)
    bases = diff_bases()
    out = []
    for _ in range(n):
        s, n_out = r.choice(bases)
        b = bytearray(s)
        for _ in range(r.randint(1, 3)):
            at = r.randrange(min(40, len(b))) if r.random() < 0.5 else r.randrange(len(b))
            b[at] ^= 1 << r.randrange(8)
        if r.random() < 0.1:
            del b[r.randrange(len(b)):]
        out.append((bytes(b), n_out))
    return tuple(out)

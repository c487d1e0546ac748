"""Raw DEFLATE streams for the inflate tests: zlib's own output in every block type, hand-assembled streams for what zlib does not emit on request,
and the fixed list of corrupt streams.  The reference of every valid stream is the bytes it was made from (and zlib.decompress agrees: checked here)."""
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


def put_dynamic_header(w: Bits, hlit: int, hdist: int, cl_ops, final: bool = True):
    """cl_ops: the code-length sequence as (symbol 0..18, extra value) pairs, chosen by the caller: that is the point"""
    pre = canonical(PRECODE_LENS)
    w.put(1 if final else 0, 1)
    w.put(2, 2)
    w.put(hlit - 257, 5)
    w.put(hdist - 1, 5)
    w.put(19 - 4, 4)
    for s in PRECODE_ORDER:
        w.put(PRECODE_LENS[s], 3)
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
            ln, d = t
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

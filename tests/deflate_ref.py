"""Plain spans for the deflate tests: the payloads of tests/inflate_ref.py, the shapes at which an encoder goes wrong, and the two corpora of the compression
check.  The reference of every span is the span itself: zlib must inflate the stream back to it.  Everything is seeded and computed once."""
from __future__ import annotations

import functools
import gzip
import os
import random
import struct
import subprocess
import tempfile

import numpy as np

import inflate_ref as IR

MAX_IN = 65536
CRC_SLICE = 256          # CCSX_DEFL_CRC_SLICE
OK, OUTPUT_FULL = 0, 1


def fibonacci_literals() -> bytes:
    """23 distinct bytes with counts 1, 1, 2, 3, 5, ... shuffled (the last count is cut so that the sum, 65535, stays below 65536).  Over the whole span an unlimited
    Huffman tree of these counts is deeper than 15; the encoder codes sub-blocks of 8192 positions and finds matches among the frequent bytes, so what its
    limiter sees is shallower: the limit itself is pinned on counts (tests/test_deflate_ref.py, ccsx_deflate_code_lengths)"""
    counts, a, b = [], 1, 1
    for _ in range(23):
        counts.append(a)
        a, b = b, a + b
    total = sum(counts)
    if total >= MAX_IN:
        counts[-1] -= total - MAX_IN + 1
    r = random.Random(23)
    lst = [0x30 + k for k, c in enumerate(counts) for _ in range(c)]
    r.shuffle(lst)
    return bytes(lst)


def fibonacci_block() -> bytes:
    """the same skew inside ONE sub-block of 8192 positions: 18 distinct bytes, counts 1, 1, 2, ... 2584 (sum 6764), shuffled"""
    counts, a, b = [], 1, 1
    for _ in range(18):
        counts.append(a)
        a, b = b, a + b
    r = random.Random(18)
    lst = [0x41 + k for k, c in enumerate(counts) for _ in range(c)]
    r.shuffle(lst)
    return bytes(lst)


def deep_precode() -> bytes:
    """a literal / length length profile with few codes of the short lengths and many of the long ones (one literal of about half the bytes, one of a quarter ...
    hundreds of rare ones), so that the counts of the code-length symbols in the header are skewed themselves and the 19-symbol code over them comes out at its
    limit of 7 bits"""
    r = random.Random(7)
    lst = []
    want, a, b, sym = [], 1, 1, 0
    for ln in range(1, 12):
        want.append((ln, a))
        a, b = b, a + b
    for ln, how_many in want:
        for _ in range(how_many):
            if sym > 255:
                break
            lst += [sym] * max(1, (1 << 13) >> ln)
            sym += 1
    r.shuffle(lst)
    return bytes(lst[:8000])


def phrase_at(distance: int) -> bytes:
    """a 300-byte phrase, noise, and the phrase again at exactly `distance`"""
    phrase = IR.text(300, 300)
    return phrase + IR.noise(distance - 300, distance) + phrase + b"tail"


def qv_like(n: int, seed: int) -> bytes:
    """HiFi base qualities: long stretches of the cap (93) with dips"""
    r = random.Random(seed)
    out = bytearray()
    while len(out) < n:
        out += bytes([93]) * r.randint(1, 60)
        out += bytes(r.choice([93, 93, 80, 70, 61, 52, 40, 33, 25, 12]) for _ in range(r.randint(0, 6)))
    return bytes(out[:n])


def synthetic_bam_slice(ccs: str) -> bytes:
    """the first 0xff00 bytes of the BAM that `ccs --write-synthetic` makes, inflated"""
    with tempfile.TemporaryDirectory() as d:
        bam = os.path.join(d, "s.subreads.bam")
        p = subprocess.run([ccs, "--write-synthetic", "24,4-9,400-900,31", bam], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
        return gzip.open(bam, "rb").read()[:0xff00]


@functools.lru_cache(maxsize=None)
def encoder_cases() -> tuple:
    """(name, bytes): the shapes of the issue, each a few KiB unless its point is the size"""
    c = []
    for n in (0, 1, 2, 3, 4, 65535, 65536):
        c.append((f"len{n}-text", IR.text(n, n + 1)))
    c.append(("one-byte-x1", b"\x41"))
    c.append(("one-byte-x65536", b"\x41" * 65536))
    c.append(("two-alternating", b"ab" * 1500))
    c.append(("fibonacci-span", fibonacci_literals()))
    c.append(("fibonacci-block", fibonacci_block()))
    c.append(("deep-precode", deep_precode()))
    c.append(("noise-65536", IR.noise(65536, 5)))
    c.append(("noise-40000", IR.noise(40000, 6)))
    c.append(("phrase-at-32768", phrase_at(32768)))
    c.append(("phrase-at-32769", phrase_at(32769)))
    c.append(("match-ends-on-last-byte", IR.noise(700, 1) + IR.text(120, 2) + IR.noise(300, 3) + IR.text(120, 2)))
    c.append(("match-of-259", IR.text(259, 9) + IR.noise(400, 4) + IR.text(259, 9) + b"x"))
    c.append(("acgt-6000", IR.acgt(6000, 11)))
    c.append(("qv-6000", qv_like(6000, 12)))
    c.append(("codec-6000", IR.codec_noise(6000, 13)))
    c.append(("hifi-records-0xff00", hifi_corpus(False, 0xff00)))
    c.append(("hifi-kinetics-0xff00", hifi_corpus(True, 0xff00)))
    return tuple(c)


SUB = 8192               # CCSX_DEFL_SUB
CHUNK = 256              # CCSX_DEFL_CHUNK
MAX_MATCH = 258          # CCSX_DEFL_MAX_MATCH
BOUNDARY_LENGTHS = [255, 256, 257, 8191, 8192, 8193, 8449, 8450, 8451, 16383, 16384, 16385, 57343, 57344, 57345, 65279, 65280, 65281]
STRADDLE_PHRASE_AT = SUB - 100
NEAR_COPIES_AT = (100, 520, 600)     # the phrase of 'nearer-copy-in-the-same-chunk': chunk 0, and twice in chunk 2


def noise64(n: int, seed: int) -> bytes:
    """random bytes of 64 values: six bits a byte, so a span of them stays coded, and a chance 4-byte match is rare"""
    return bytes(0x30 + (b & 63) for b in random.Random(seed).randbytes(n))


@functools.lru_cache(maxsize=None)
def boundary_cases() -> tuple:
    """(name, bytes): every content at every length around a chunk, a sub-block, a sub-block + a longest match, several sub-blocks and the BGZF span, and the
    shapes that put a match across a sub-block's end"""
    longest = max(BOUNDARY_LENGTHS)
    content = {"zeros": bytes(longest), "ab": b"ab" * (longest // 2 + 1), "acgt": IR.acgt(longest, 21), "text": IR.text(longest, 22), "qv": qv_like(longest, 23)}
    c = [(f"{kind}-{n}", data[:n]) for kind, data in content.items() for n in BOUNDARY_LENGTHS]
    phrase = IR.text(MAX_MATCH, 258)
    straddle = noise64(1000, 1) + phrase + noise64(STRADDLE_PHRASE_AT - 1000 - len(phrase), 2) + phrase + noise64(1000, 3)
    assert straddle[STRADDLE_PHRASE_AT:STRADDLE_PHRASE_AT + len(phrase)] == phrase
    c.append(("match-straddles-the-sub-block", straddle))
    c.append(("span-ends-inside-the-straddling-match", straddle[:SUB + 100]))
    p40 = IR.text(40, 40)
    a, b, far = NEAR_COPIES_AT
    near = noise64(a, 4) + p40 + noise64(b - a - 40, 5) + p40 + noise64(far - b - 40, 6) + p40 + noise64(200, 7)
    assert [near[k:k + 40] for k in NEAR_COPIES_AT] == [p40] * 3 and a // CHUNK < b // CHUNK == far // CHUNK
    c.append(("nearer-copy-in-the-same-chunk", near))
    c.append(("text-then-noise", IR.text(SUB, 1) + IR.noise(MAX_IN - SUB, 2)))
    c.append(("noise-then-text", IR.noise(MAX_IN - SUB, 2) + IR.text(SUB, 1)))
    return tuple(c)


@functools.lru_cache(maxsize=None)
def skew_spans() -> tuple:
    """(skew of the span's first byte modulo 16, bytes): every length around the 16-byte pieces of the copy at every skew"""
    return tuple((skew, IR.text(n, 16 * n + skew)) for n in (0, 1, 15, 16, 17, 31, 32, 33) for skew in range(16))


@functools.lru_cache(maxsize=None)
def all_cases() -> tuple:
    """encoder_cases() + the plain bytes of every valid and fuzz case of the inflate tests (names made unique)"""
    seen, out = set(), []
    for name, data in list(encoder_cases()) + [(c[0], c[2]) for c in IR.valid_cases()] + [(c[0], c[2]) for c in IR.fuzz_cases()]:
        if (len(data), hash(data)) in seen:
            continue
        seen.add((len(data), hash(data)))
        out.append((name, data))
    return tuple(out)


# ---- the corpora of the compression check: HiFi records in the layout the driver writes (ccs_main.cpp: RG ec np rq sn zm, and fi fp fn ri rp rn with kinetics)
def _hifi_record(r: random.Random, zm: int, kinetics: bool) -> bytes:
    n = r.randint(9000, 21000)
    seq = np.frombuffer(r.randbytes(n), np.uint8) & 3
    nib = np.array([1, 2, 4, 8], np.uint8)[seq]
    if n & 1:
        nib = np.append(nib, 0).astype(np.uint8)
    packed = ((nib[0::2] << 4) | nib[1::2]).astype(np.uint8).tobytes()
    qual = qv_like(n, r.randint(0, 1 << 30))
    name = f"synth/{zm}/ccs".encode() + b"\0"
    body = struct.pack("<iiBBHHHiiii", -1, -1, len(name), 255, 4680, 0, 4, n, -1, -1, 0) + name + packed + qual
    body += b"RGZccsamd01\0" + b"ecf" + struct.pack("<f", r.uniform(5, 30)) + b"npi" + struct.pack("<i", r.randint(4, 30))
    body += b"rqf" + struct.pack("<f", 1 - 10 ** -r.uniform(2, 4)) + b"snBf" + struct.pack("<i4f", 4, *[r.uniform(4, 15) for _ in range(4)])
    body += b"zmi" + struct.pack("<i", zm)
    if kinetics:
        for tag in (b"fi", b"fp", b"ri", b"rp"):
            body += tag + b"BC" + struct.pack("<i", n) + IR.codec_noise(n, r.randint(0, 1 << 30))
            if tag in (b"fp", b"rp"):
                body += (b"fn" if tag == b"fp" else b"rn") + b"i" + struct.pack("<i", r.randint(2, 15))
    return struct.pack("<i", len(body)) + body


@functools.lru_cache(maxsize=None)
def hifi_corpus(kinetics: bool, nbytes: int = 2 << 20) -> bytes:
    r = random.Random(2026 + int(kinetics))
    out, zm = bytearray(), 100
    while len(out) < nbytes:
        out += _hifi_record(r, zm, kinetics)
        zm += r.randint(1, 40)
    return bytes(out[:nbytes])


def spans_of(data: bytes, size: int = 0xff00) -> list:
    return [data[a:a + size] for a in range(0, len(data), size)]

"""The BGZF deflate rule at its sub-block and chunk edges, on the host (one lane of deflate_core.h): the spans of deflate_ref.boundary_cases() against zlib
(it inflates every stream back to the span, and the CRC is zlib.crc32) and against the project's own decoder, and the block structure that the shaped spans are
there for.  No GPU; tests/test_deflate_limits_gpu.py is an equality with what is checked here.

Slips compiled into a scratch copy of deflate_core.h, one at a time, all indices in range, run on the host (one lane) — the test here that notices each, and
whether a test from before did:
  - `final_block = pos >= n` -> `end >= n`: test_zlib_inflates_every_stream_back on 13 spans (zeros / ab / qv at 8193, 16385 and 57345, acgt-8193 ...: the
    stream has no final block) and test_a_last_sub_block_without_a_token_leaves_bfinal_to_the_one_before; before: 2 of the spans of
    tests/test_deflate_ref.py, by luck (len32769-text, fuzz56).
  - the atomic_max insertion moved before the chunk's look-ups: every round trip stays green (the streams are valid, only other: 65 of the spans here, 169
    of those before), so nothing from before notices; test_the_copy_of_an_earlier_chunk_is_taken (no copy is found at all) and
    test_a_last_sub_block_without_a_token_leaves_bfinal_to_the_one_before (two blocks) read the tokens and do.
  - `per` rounded down: the same stream on one lane; tests/test_deflate_limits_gpu.py."""
import zlib

import pytest

import deflate_ref as R
from ccs_amd import api

CASES = R.boundary_cases()


@pytest.fixture(scope="module")
def encoded(built):
    """every span through the host path, once: {name: (data, stream, crc)}"""
    out = {}
    for at in range(0, len(CASES), 32):
        part = CASES[at:at + 32]
        streams, status, call = api.deflate_host([d for _, d in part])
        assert not status.any()
        for i, (name, d) in enumerate(part):
            assert call.out_len[i] == len(streams[i])
            out[name] = (d, streams[i], int(call.crc[i]))
    return out


def test_the_set_holds_every_content_at_every_length():
    names = {n for n, _ in CASES}
    assert len(names) == len(CASES)
    for kind in ("zeros", "ab", "acgt", "text", "qv"):
        for n in R.BOUNDARY_LENGTHS:
            assert f"{kind}-{n}" in names
    assert {8192 - 1, 8192, 8192 + 1, 8192 + 257, 8192 + 259, 0xff00} <= set(R.BOUNDARY_LENGTHS)
    assert all(len(d) <= R.MAX_IN for _, d in CASES)


def test_zlib_inflates_every_stream_back(encoded):
    for name, (d, s, _) in encoded.items():
        z = zlib.decompressobj(-15)
        assert z.decompress(s) + z.flush() == d, name
        assert z.eof and z.unused_data == b"", name


def test_crc_is_zlibs(encoded):
    for name, (d, _, crc) in encoded.items():
        assert crc == zlib.crc32(d), name


def test_our_decoder_inflates_every_stream_back(encoded):
    names = list(encoded)
    for at in range(0, len(names), 32):
        part = names[at:at + 32]
        _, status, call = api.inflate_host([encoded[n][1] for n in part], [len(encoded[n][0]) for n in part])
        assert not status.any(), [(n, int(s)) for n, s in zip(part, status) if s]
        for i, n in enumerate(part):
            assert call.output(i) == encoded[n][0], n


def _positions(blocks):
    """(position, token) of every token of a walked stream"""
    out, at = [], 0
    for b in blocks:
        for t in b["tokens"]:
            out.append((at, t))
            at += 1 if isinstance(t, int) else t[0]
    return out


def test_a_match_straddles_the_sub_block(encoded):
    d, s, _ = encoded["match-straddles-the-sub-block"]
    blocks = R.IR.walk_blocks(s)
    assert [b["btype"] for b in blocks] == [2, 2] and [b["final"] for b in blocks] == [0, 1]
    first = sum(1 if isinstance(t, int) else t[0] for t in blocks[0]["tokens"])
    assert first > R.SUB                                     # the first block's last token runs over the boundary: it belongs to the block it starts in
    straddling = [(at, t) for at, t in _positions(blocks) if not isinstance(t, int) and at < R.SUB < at + t[0]]
    assert len(straddling) == 1 and straddling[0][1][1] == R.STRADDLE_PHRASE_AT - 1000


def test_a_last_sub_block_without_a_token_leaves_bfinal_to_the_one_before(encoded):
    """the span ends inside the match that straddles the boundary: the loop leaves with base < n and pos >= n, and exactly one block header was written"""
    d, s, _ = encoded["span-ends-inside-the-straddling-match"]
    assert len(d) == R.SUB + 100
    blocks = R.IR.walk_blocks(s)
    assert len(blocks) == 1 and blocks[0]["btype"] == 2 and blocks[0]["final"] == 1
    at, last = _positions(blocks)[-1]
    assert at < R.SUB and at + last[0] == len(d)
    assert 8 * len(s) - blocks[0]["end_bit"] < 8


def test_the_copy_of_an_earlier_chunk_is_taken(encoded):
    """the phrase lies at 100 (chunk 0), 520 and 600 (both chunk 2): at 600 the rule's candidate is the largest position of an EARLIER chunk, 100, not 520"""
    d, s, _ = encoded["nearer-copy-in-the-same-chunk"]
    a, b, far = R.NEAR_COPIES_AT
    long_matches = {at: t for at, t in _positions(R.IR.walk_blocks(s)) if not isinstance(t, int) and t[0] >= 36}
    assert long_matches[b] == (40, b - a) and long_matches[far][1] == far - a and long_matches[far][0] >= 40
    assert all(t[1] != far - b for t in long_matches.values())


def test_text_beside_noise_stays_coded(encoded):
    for name in ("text-then-noise", "noise-then-text"):
        d, s, _ = encoded[name]
        blocks = R.IR.walk_blocks(s)
        assert [b["btype"] for b in blocks] == [2] * 8 and len(s) < len(d), name
    # where every sub-block is noise the same seven coded sub-blocks are written and thrown away: the stored form (tests/test_deflate_ref.py: noise-65536)

"""The DEFLATE decoder of k_inflate at the format's limits, on the host (one lane of inflate_core.h): the hand-assembled streams of inflate_ref.limit_cases()
against the bytes they were assembled from (zlib agrees: asserted in the generator), the conditions that make the set worth having, and the decoder's accept
set against zlib's.  No GPU; tests/test_inflate_limits_gpu.py hands the same streams to the wave.

What the set cannot hold, and where it went instead:
  - HCLEN 4 writes the lengths of 16, 17, 18 and 0 only, so every literal / length length is 0 and there is no end-of-block code: no valid block has it.  It is
    a corrupt case ("hclen-4", BAD_CODE_LENGTHS); the valid streams hold HCLEN 5, 12 and 19.
  - no valid stream has one byte (an empty fixed block, the shortest, has ten bits): "one-byte" is a corrupt case (TRUNCATED_INPUT); 2 and 3 bytes are here.
  - long codes of (11, 12, 12, 13, 14, 15, 15) bits do not fit behind ONE 10-bit prefix (their Kraft sum there is 5 / 4): the set holds (11, 12, 13, 14, 15, 15)
    and (12, 12, 12, 13, 14, 15, 15), which fill one prefix exactly.
  - a stored block finds at most 4 whole look-ahead bytes in the bit buffer, never 5 .. 7: the buffer is refilled to 64 bits behind the byte boundary and LEN /
    NLEN take 32 of them.  The counts 0 .. 4 are reached by "stored-back-to-back-*".  At that point the bit count is a multiple of 8, so handing back
    (cnt + 7) >> 3 bytes instead of cnt >> 3 is the same decoder: that slip is equivalent, not missed.

Slips compiled into a scratch copy of inflate_core.h, one at a time, all indices in range, run on the host (one lane): the streams of this file that each
one breaks (of the 245 limit streams / of the 24000 of the differential), and what the lists from before (valid_cases, fuzz_cases, the old corrupt list) did:
  - ccsx_infl_build `k += nl << rest` -> `nl << sub_bits`: 163 / 1528; before: 10 valid (zlib's long streams) and 12 fuzz streams.
  - ccsx_infl_build sub-table `maxl` from the first code behind the prefix: 183 / 1736; before: the same 10 and 12.
  - ccsx_infl_build `below` -> `below | self` in the rank: 245 / 3449; before: 29 valid, 235 fuzz.
  - match copy `i % dist` -> `i % (dist + 1)` for dist < len: 189 / 1987; before: 10 valid, 30 fuzz.
  - match copy `dist >= len` -> `dist > len`: 0 / 0, and equivalent: at dist == len, i % dist == i for every i < len.
  - stored copy hand-back `b.cnt >> 3` -> `(b.cnt + 7) >> 3`: 0 / 0, and equivalent (above).
  - the `max == 1` rule taken back (a lone end-of-block code refused): lone-end-of-block, lone-end-of-block-then-stored, the corrupt case
    lone-eob-unused-codeword (BAD_CODE_LENGTHS for BAD_SYMBOL) / 28; before: nothing.
  - the rule stretched to the code-length code: the corrupt case precode-one-codeword alone (tests/test_inflate_ref.py iterates the list) / 0 - no flip of
    the differential makes a one-codeword code-length code, the fixed list is what holds that line; before: nothing.
What only 64 lanes show is in tests/test_inflate_limits_gpu.py."""
import collections

import pytest

import inflate_ref as R
from ccs_amd import api

LIMITS = R.limit_cases()


@pytest.fixture(scope="module")
def shapes():
    return {c[0]: R.code_shape(c[1]) for c in LIMITS}


@pytest.mark.parametrize("case", LIMITS, ids=[c[0] for c in LIMITS])
def test_limit_stream_equals_its_bytes(built, case):
    name, stream, data = case
    out, status, call = api.inflate_host([stream], [len(data)], guard=32, fill=0xA5)
    assert status.tolist() == [R.OK], api.INFLATE_STATUS_NAMES[int(status[0])]
    assert out == data
    assert bytes(call.dst[:32]) == b"\xa5" * 32 and bytes(call.dst[32 + len(data):]) == b"\xa5" * 32


def test_all_limit_streams_in_one_call(built):
    out, status, _ = api.inflate_host([c[1] for c in LIMITS], [len(c[2]) for c in LIMITS], guard=3, gap=1)
    assert not status.any()
    assert out == b"".join(c[2] for c in LIMITS)


def test_the_set_reaches_the_deep_end_of_both_codes(shapes):
    """conditions on the set, measured with the header parser of inflate_ref (walk_blocks)"""
    random_codes = [shapes[c[0]] for c in LIMITS if c[0].startswith("codes")]
    assert len(random_codes) >= 200
    lit, dist = collections.Counter(s["lit"] for s in random_codes), collections.Counter(s["dist"] for s in random_codes)
    print("longest literal / length code -> streams:", sorted(lit.items()), " longest distance code -> streams:", sorted(dist.items()))
    for ln in range(11, 16):
        assert lit[ln] >= 10, (ln, lit[ln])
    for ln in range(9, 16):
        assert dist[ln] >= 10, (ln, dist[ln])
    assert shapes["hclen5"]["hclen"] == {5} and shapes["hclen12"]["hclen"] == {12} and shapes["hclen19"]["hclen"] == {19}
    assert shapes["precode-7-bits"]["pre"] == 7 and sum(1 for s in random_codes if s["pre"] == 7) >= 10
    assert {h for s in random_codes for h in s["hclen"]} >= {16, 17, 18, 19}


@pytest.mark.parametrize("name, code, primary, bits", [("lit-one-prefix", "lit", 10, [5]), ("lit-one-prefix-b", "lit", 10, [5]),
                                                       ("lit-many-prefixes", "lit", 10, [1, 1, 2, 3, 4, 5]), ("dist-one-prefix", "dist", 8, [7]),
                                                       ("dist-many-prefixes", "dist", 8, [1, 2, 3, 4])])
def test_every_sub_table_entry_is_looked_up(name, code, primary, bits):
    """the sub-table shapes: the sub-tables have the index bits the case is named for, and the tokens look up every entry of every one of them (an entry a
    build slip leaves wrong or empty is then read)"""
    stream = {c[0]: c[1] for c in LIMITS}[name]
    blk, = R.walk_blocks(stream)
    subs = R.sub_tables(blk[code], primary)
    assert sorted(subs.values()) == bits
    assert blk[code + "_seen"] == {(p, k) for p, b in subs.items() for k in range(1 << b)}


def test_bit_reader_edges_are_what_their_names_say():
    by_name = {c[0]: c[1] for c in LIMITS}
    for pad in range(8):
        s = by_name[f"final-block-{pad}-pad-bits"]
        assert 8 * len(s) - R.walk_blocks(s)[-1]["end_bit"] == pad
    assert [len(by_name[n]) for n in ("two-bytes", "three-bytes")] == [2, 3]
    assert [b["btype"] for b in R.walk_blocks(by_name["empty-stored-between-huffman-blocks"])] == [1, 0, 2]
    assert R.walk_blocks(by_name["empty-stored-between-huffman-blocks"])[1]["tokens"] == []
    for name in ("lone-end-of-block", "lone-end-of-block-then-stored"):
        blk = R.walk_blocks(by_name[name])[0]
        assert blk["btype"] == 2 and [k for k, ln in enumerate(blk["lit"]) if ln] == [256] and blk["lit"][256] == 1 and blk["tokens"] == []


def test_accept_set_is_zlibs(built):
    """The decoder accepts exactly what zlib.decompressobj(-15) accepts (end of the final block reached, at most 65536 bytes), with zlib's bytes, over 24000
    corrupted streams (inflate_ref.diff_cases: seed 1951).  No exception list.  The committed seed: zlib accepts 3645 and rejects 20355 of them."""
    cases = R.diff_cases()
    assert len(cases) >= 20000 and len(R.diff_bases()) >= 250
    ref = [R.zlib_inflate(s) for s, _ in cases]
    accepted = [i for i, o in enumerate(ref) if o is not None]
    rejected = [i for i, o in enumerate(ref) if o is None]
    print(f"zlib accepts {len(accepted)} and rejects {len(rejected)} of {len(cases)}")
    assert 10 * len(accepted) >= len(cases) and 10 * len(rejected) >= len(cases)
    for at in range(0, len(accepted), 1000):
        part = accepted[at:at + 1000]
        _, status, call = api.inflate_host([cases[i][0] for i in part], [len(ref[i]) for i in part])
        bad = [(i, api.INFLATE_STATUS_NAMES[int(s)]) for i, s in zip(part, status) if s != R.OK]
        assert not bad, f"zlib accepts, the decoder does not: {bad[:5]} ({len(bad)})"
        for k, i in enumerate(part):
            assert call.output(k) == ref[i], i
    for at in range(0, len(rejected), 1000):
        part = rejected[at:at + 1000]
        _, status, _ = api.inflate_host([cases[i][0] for i in part], [cases[i][1] for i in part])
        bad = [i for i, s in zip(part, status) if s == R.OK]
        assert not bad, f"zlib rejects, the decoder accepts: {bad[:5]} ({len(bad)})"

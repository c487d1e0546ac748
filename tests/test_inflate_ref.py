"""The DEFLATE decoder of k_inflate, run on the host (ccsx_inflate_blocks_host: the same inflate_core.h, one lane), against zlib byte for byte, and against the
fixed list of corrupt streams status for status.  No GPU."""
import zlib

import numpy as np
import pytest

import inflate_ref as R
from ccs_amd import api


def _host(streams, out_lens, **layout):
    return api.inflate_host(streams, out_lens, **layout)


def test_rule_version_and_status_names(built):
    assert api.lib().ccsx_inflate_rule_version() == 1
    assert api.INFLATE_STATUS_NAMES[R.OUTPUT_SHORT] == "OUTPUT_SHORT" and len(api.INFLATE_STATUS_NAMES) == 9


@pytest.mark.parametrize("case", R.valid_cases(), ids=[c[0] for c in R.valid_cases()])
def test_valid_stream_equals_zlib(built, case):
    name, stream, data = case
    out, status, call = _host([stream], [len(data)], guard=32, fill=0xA5)
    assert status.tolist() == [R.OK], api.INFLATE_STATUS_NAMES[int(status[0])]
    assert out == data == zlib.decompress(stream, -15)
    assert bytes(call.dst[:32]) == b"\xa5" * 32 and bytes(call.dst[32 + len(data):]) == b"\xa5" * 32      # nothing outside the block's range


def test_all_valid_streams_in_one_call(built):
    cases = R.valid_cases()
    assert {R.block_types(c[1]) for c in cases} == {0, 1, 2}            # stored, fixed and dynamic first blocks all go through the library here
    out, status, _ = _host([c[1] for c in cases], [len(c[2]) for c in cases], guard=7, gap=3)
    assert not status.any()
    assert out == b"".join(c[2] for c in cases)


def test_seeded_fuzz_equals_zlib(built):
    cases = R.fuzz_cases()
    assert len(cases) >= 300
    out, status, _ = _host([c[1] for c in cases], [len(c[2]) for c in cases], guard=5)
    bad = [c[0] for c, s in zip(cases, status) if s != R.OK]
    assert not bad, bad
    assert out == b"".join(c[2] for c in cases)


def test_corrupt_streams_get_their_status_and_neighbours_stay_intact(built):
    good, gdata = R.short_stream()
    for name, stream, out_len, want in R.corrupt_cases():
        out, status, call = _host([good, stream, good], [len(gdata), out_len, len(gdata)], guard=16, fill=0x5A)
        assert status[0] == R.OK and status[2] == R.OK, name
        assert call.output(0) == gdata and call.output(2) == gdata, name
        assert status[1] != R.OK, name
        if want is not None:
            assert status[1] == want, (name, api.INFLATE_STATUS_NAMES[int(status[1])])
        g = call.guard
        for i in range(3):                                     # the guard bytes around every block's range
            b = call.blocks[i]
            assert bytes(call.dst[b.out_off - g:b.out_off]) == b"\x5a" * g and bytes(call.dst[b.out_off + b.out_len:b.out_off + b.out_len + g]) == b"\x5a" * g, name


def test_single_byte_flips_end_in_a_status(built):
    flips = R.flip_cases()
    out, status, call = _host([f[0] for f in flips], [f[1] for f in flips], guard=8, fill=0x33)
    assert ((status >= 0) & (status <= R.OUTPUT_SHORT)).all()
    assert (status != R.OK).sum() > len(flips) // 2            # most flips are caught by the format alone; the rest is what the CRC is for
    for i in range(call.n):
        b = call.blocks[i]
        assert bytes(call.dst[b.out_off - 8:b.out_off]) == b"\x33" * 8, i
    assert bytes(call.dst[-8:]) == b"\x33" * 8


def test_argument_errors_fail_the_call(built):
    L = api.lib()
    good, gdata = R.short_stream()

    def rc_of(mutate):
        call = api.InflateCall([good, good], [len(gdata)] * 2, guard=4)
        mutate(call)
        rc = L.ccsx_inflate_blocks_host(*call.args())
        return rc, L.ccsx_last_error().decode(), call

    def set_(i, **kw):
        def m(call):
            for k, v in kw.items():
                setattr(call.blocks[i], k, v)
        return m

    for mutate, word in [(set_(1, in_off=10 ** 6), "outside src"), (set_(1, in_len=-1), "outside src"), (set_(0, out_off=10 ** 6), "outside dst"),
                         (set_(1, out_off=4 + len(gdata) - 1), "overlap"), (set_(1, out_off=4), "overlap"), (set_(0, out_len=65537), "out_len"),
                         (set_(0, out_len=-1), "out_len")]:
        rc, msg, call = rc_of(mutate)
        assert rc < 0 and word in msg, (rc, msg)
        assert (call.dst == 0).all() and (call.status == -1).all()           # nothing ran
    rc, msg, _ = rc_of(lambda call: None)
    assert rc == 0
    # an empty block that sorts between two overlapping ones hides nothing: A = [0, 10), Z = [5, 5), B = [5, 15)
    call = api.InflateCall([good, b"\x03\x00", good], [10, 0, 10])
    for i, (off, ln) in enumerate([(0, 10), (5, 0), (5, 10)]):
        call.blocks[i].out_off, call.blocks[i].out_len = off, ln
    assert L.ccsx_inflate_blocks_host(*call.args()) < 0 and "overlap" in L.ccsx_last_error().decode()
    assert (call.status == -1).all()
    for i, (off, ln) in enumerate([(0, 10), (10, 0), (10, 10)]):             # the same three side by side are fine (the streams then fail on their own: OUTPUT_OVERRUN)
        call.blocks[i].out_off, call.blocks[i].out_len = off, ln
    assert L.ccsx_inflate_blocks_host(*call.args()) == 0 and call.status.tolist() == [R.OUTPUT_OVERRUN, R.OK, R.OUTPUT_OVERRUN]


def test_bgzf_split_finds_the_payloads():
    import struct
    blocks, datas = b"", [R.text(3000, 1), b"", R.acgt(70, 2)]
    for d in datas:
        p = R.deflate_raw(d)
        blocks += bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 66, 67, 2, 0]) + struct.pack("<H", 18 + len(p) + 8 - 1) + p + struct.pack("<II", zlib.crc32(d), len(d))
    got = api.bgzf_split(blocks)
    assert [(zlib.decompress(p, -15), n, c) for p, n, c in got] == [(d, len(d), zlib.crc32(d)) for d in datas]
    with pytest.raises(ValueError):
        api.bgzf_split(blocks[:-3])

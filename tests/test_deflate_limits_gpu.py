"""k_deflate at the rule's sub-block and chunk edges: stream, out_len, crc and status byte for byte the host's run of the same encoder
(tests/test_deflate_limits.py pins that one to zlib and to the project's own decoder), the streams back through k_inflate, and the span's way from HBM into LDS
at every skew of the 16-byte pieces.  No test makes anything fail on purpose.

What the 256 lanes do that the host's one lane does not: a lane's slice of a sub-block is per = ceil((end - base) / 256) positions (1, with 255 idle lanes, for
the 1-byte last sub-block of the *-8193 / *-16385 / *-57345 spans; 2 with a short last lane for 257 bytes), the chunk's look-ups and its insertions are one
position per lane, and the counts, bit sums and bits meet in LDS atomics.  Slips tried in a scratch copy (values only, every index in range):
  - ccsx_defl_span `per` rounded down: nothing changes on one lane; on the device the tokens behind 256 * per positions of a sub-block are never written.
    Run once on an MI355X: test_boundary_spans_equal_the_host fails at both gaps (zeros-255, zeros-8191, zeros-16383, zeros-57343, zeros-65279, ab-255
    ...: the lengths that are no multiple of 256).  tests/test_deflate_gpu.py was not run against it; its lengths (1, 2, 3, 6000 ...) are no multiples
    of 256 either.
  - `final_block = pos >= n` -> `end >= n` and the atomic_max insertion before the look-ups change the host's stream as well: tests/test_deflate_limits.py."""
import numpy as np
import pytest

import deflate_ref as R
from ccs_amd import api

pytestmark = pytest.mark.gpu

GUARD = 32
CASES = R.boundary_cases()


@pytest.fixture(scope="module")
def deflater(built):
    f = api.Deflater(0, max_in_bytes=8 << 20, max_out_bytes=8 << 20, max_spans=128)
    yield f
    f.close()


@pytest.fixture(scope="module")
def host(built):
    """the host path's answer for every span, once: {name: (data, stream, crc)}"""
    out = {}
    for at in range(0, len(CASES), 32):
        part = CASES[at:at + 32]
        streams, status, call = api.deflate_host([d for _, d in part])
        assert not status.any()
        for i, (name, d) in enumerate(part):
            out[name] = (d, streams[i], int(call.crc[i]))
    return out


def _guards_untouched(call, fill):
    at = 0
    for i in range(call.n):
        b = call.spans[i]
        assert (call.dst[at:b.out_off] == fill).all(), f"bytes before span {i} were written"
        at = b.out_off + b.out_cap
    assert (call.dst[at:call.dst_len] == fill).all(), "bytes behind the last span were written"


def _equals_the_host(call, want):
    """want: (data, stream, crc) per span"""
    assert not call.status[:call.n].any()
    for i, (_, stream, crc) in enumerate(want):
        assert call.out_len[i] == len(stream), i
        assert call.stream(i) == stream, i
        assert int(call.crc[i]) == crc, i
    _guards_untouched(call, 0xC3)


@pytest.mark.parametrize("gap", [0, 3])
def test_boundary_spans_equal_the_host(deflater, host, gap):
    names = [n for n, _ in CASES]
    call = deflater.run(api.DeflateCall([host[n][0] for n in names], guard=GUARD, gap=gap, fill=0xC3))
    bad = [n for i, n in enumerate(names) if call.stream(i) != host[n][1] or int(call.crc[i]) != host[n][2] or call.status[i]]
    assert not bad, bad
    _equals_the_host(call, [host[n] for n in names])


def test_device_round_trip(deflater, host):
    names = [n for n, _ in CASES]
    call = deflater.run(api.DeflateCall([host[n][0] for n in names]))
    inflater = api.Inflater(0, max_in_bytes=8 << 20, max_out_bytes=8 << 20, max_blocks=len(names))
    try:
        out, status = inflater.inflate(call.streams(), [len(host[n][0]) for n in names])
    finally:
        inflater.close()
    assert not status.any() and out == b"".join(host[n][0] for n in names)


def _call_at_skews(spans, skews):
    """a call whose span i starts at in_off & 15 == skews[i] (the device buffer is 16-byte aligned, so that is the skew the kernel computes)"""
    call = api.DeflateCall(spans, guard=GUARD, gap=16, fill=0xC3)
    src = np.zeros_like(call.src)
    for i, (d, skew) in enumerate(zip(spans, skews)):
        call.spans[i].in_off += (skew - call.spans[i].in_off) & 15          # less than the gap: the spans stay apart and inside src
        assert call.spans[i].in_off & 15 == skew and call.spans[i].in_off + len(d) <= call.src_len
        src[call.spans[i].in_off:call.spans[i].in_off + len(d)] = np.frombuffer(d, np.uint8)
    call.src[:] = src
    return call


def test_every_skew_of_the_input(deflater):
    """128 spans: every length around the 16-byte pieces at every in_off & 15, then 65536 bytes at skews 1 and 15; against the host's run of the same call"""
    grid = R.skew_spans()
    assert len(grid) == 128 and {(s, len(d)) for s, d in grid} == {(s, n) for s in range(16) for n in (0, 1, 15, 16, 17, 31, 32, 33)}
    big = R.IR.text(65536, 78)
    for spans, skews in (([d for _, d in grid], [s for s, _ in grid]), ([big, big], [1, 15])):
        streams, status, _ = api.deflate_host(spans)
        assert not status.any()
        call = deflater.run(_call_at_skews(spans, skews))
        _equals_the_host(call, [(d, s, R.IR.zlib.crc32(d)) for d, s in zip(spans, streams)])

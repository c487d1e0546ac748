"""k_deflate through api.Deflater: stream, out_len, crc and status byte for byte the host's run of the same encoder (tests/test_deflate_ref.py pins that one to
zlib and to the project's own decoder).  No test makes anything fail on purpose: a refused argument never reaches the device."""
import os

import pytest

import deflate_ref as R
from ccs_amd import api

pytestmark = pytest.mark.gpu

CCS = os.path.join(os.path.dirname(api.LIB_PATH), "bin", "ccs")

GUARD = 32
MAX_SPANS = 400


@pytest.fixture(scope="module")
def deflater(built):
    f = api.Deflater(0, max_in_bytes=24 << 20, max_out_bytes=24 << 20, max_spans=MAX_SPANS)
    yield f
    f.close()


@pytest.fixture(scope="module")
def host(built):
    """the host path's answer for every input, once: {name: (data, stream, crc)}"""
    cases = list(R.all_cases()) + [("synthetic-bam-slice", R.synthetic_bam_slice(CCS))]
    out = {}
    for at in range(0, len(cases), 64):
        part = cases[at:at + 64]
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


def _run_and_compare(deflater, host, names, **layout):
    call = deflater.run(api.DeflateCall([host[n][0] for n in names], guard=GUARD, fill=0xC3, **layout))
    assert not call.status[:call.n].any()
    for i, n in enumerate(names):
        assert call.out_len[i] == len(host[n][1]), n
        assert call.stream(i) == host[n][1], n
        assert int(call.crc[i]) == host[n][2], n
    _guards_untouched(call, 0xC3)
    return call


def test_one_span_per_call(deflater, host):
    for name, _ in R.encoder_cases():
        _run_and_compare(deflater, host, [name])


def test_every_input_sixty_four_spans_per_call(deflater, host):
    names = list(host)
    for at in range(0, len(names), 64):
        _run_and_compare(deflater, host, names[at:at + 64], gap=1 if (at // 64) % 2 else 0)     # every second call at odd input offsets


def test_max_spans_in_one_call(deflater, host):
    small = [n for n in host if len(host[n][0]) < 12000]
    names = (small * (MAX_SPANS // len(small) + 1))[:MAX_SPANS]
    assert len(names) == deflater.max_spans
    _run_and_compare(deflater, host, names)


def test_mixed_kinds_and_lengths(deflater, host):
    names = ["len0-text", "len65536-text", "one-byte-x1", "noise-65536", "len1-text", "fibonacci-span", "one-byte-x65536", "deep-precode", "len2-text",
             "phrase-at-32768", "noise-40000", "phrase-at-32769", "len3-text", "hifi-kinetics-0xff00", "len4-text", "match-of-259", "len65535-text",
             "two-alternating", "match-ends-on-last-byte", "hifi-records-0xff00", "fibonacci-block", "synthetic-bam-slice"]
    _run_and_compare(deflater, host, names, gap=5)


def test_two_tickets_in_flight(deflater, host):
    names = list(host)
    a = api.DeflateCall([host[n][0] for n in names[:40]], guard=GUARD, fill=1)
    b = api.DeflateCall([host[n][0] for n in names[40:90]], guard=GUARD, fill=2)
    ta, tb = deflater.submit(a), deflater.submit(b)
    with pytest.raises(RuntimeError, match="two tickets"):
        deflater.submit(api.DeflateCall([host[names[0]][0]]))
    deflater.wait(tb)
    deflater.wait(ta)
    assert a.streams() == [host[n][1] for n in names[:40]] and not a.status[:a.n].any()
    assert b.streams() == [host[n][1] for n in names[40:90]] and not b.status[:b.n].any()
    _guards_untouched(a, 1)
    _guards_untouched(b, 2)
    with pytest.raises(RuntimeError, match="ticket"):
        deflater.wait(ta)


def test_exact_capacity_and_output_full_beside_ok_spans(deflater, host):
    names = ["len1-text", "two-alternating", "noise-40000", "acgt-6000", "qv-6000", "len0-text", "fibonacci-block", "hifi-kinetics-0xff00", "noise-65536"]
    lens = [len(host[n][1]) for n in names]
    caps = [n - 1 if i % 2 == 0 else n for i, n in enumerate(lens)]                 # out_cap == out_len - 1 beside out_cap == out_len
    call = deflater.run(api.DeflateCall([host[n][0] for n in names], caps, guard=GUARD, gap=1, fill=0x5A))
    _, host_status, host_call = api.deflate_host([host[n][0] for n in names], caps)
    assert call.status[:call.n].tolist() == host_status.tolist() == [R.OUTPUT_FULL if i % 2 == 0 else R.OK for i in range(len(names))]
    assert call.out_len[:call.n].tolist() == host_call.out_len[:call.n].tolist()
    assert call.crc[:call.n].tolist() == host_call.crc[:call.n].tolist()
    for i, n in enumerate(names):
        if i % 2:
            assert call.stream(i) == host[n][1], n
    _guards_untouched(call, 0x5A)


def test_device_round_trip(deflater, host):
    names = [n for n, _ in R.encoder_cases()]
    call = deflater.run(api.DeflateCall([host[n][0] for n in names]))
    inflater = api.Inflater(0, max_in_bytes=4 << 20, max_out_bytes=4 << 20, max_blocks=len(names))
    try:
        out, status = inflater.inflate(call.streams(), [len(host[n][0]) for n in names])
    finally:
        inflater.close()
    assert not status.any() and out == b"".join(host[n][0] for n in names)


def test_argument_errors_enqueue_nothing(deflater, host):
    d = host["acgt-6000"][0]

    def fails(mutate, word, f=deflater):
        call = api.DeflateCall([d, d], guard=4)
        mutate(call)
        with pytest.raises(RuntimeError, match=word):
            f.run(call)
        assert (call.dst == 0).all() and (call.status == -1).all() and (call.out_len == -1).all()

    def set_(i, **kw):
        def m(call):
            for k, v in kw.items():
                setattr(call.spans[i], k, v)
        return m

    fails(set_(1, in_off=1 << 40), "outside src")
    fails(set_(0, out_off=1 << 40), "outside dst")
    fails(set_(1, out_off=4), "overlap")
    fails(set_(0, in_len=65537), "in_len")
    small = api.Deflater(0, max_in_bytes=8000, max_out_bytes=1 << 16, max_spans=1)
    try:
        fails(lambda call: None, "capacities", f=small)
        streams, crc, status = small.deflate([d])                                  # and the deflater is still usable
        assert streams == [host["acgt-6000"][1]] and status.tolist() == [R.OK] and int(crc[0]) == host["acgt-6000"][2]
    finally:
        small.close()
    with pytest.raises(RuntimeError, match="capacities"):
        api.Deflater(0, max_in_bytes=0)

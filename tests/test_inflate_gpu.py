"""k_inflate through api.Inflater: byte for byte zlib, status for status the host's run of the same decoder (tests/test_inflate_ref.py pins that one to zlib)."""
import numpy as np
import pytest

import inflate_ref as R
from ccs_amd import api

pytestmark = pytest.mark.gpu

GUARD = 32


def _all_valid():
    return list(R.valid_cases()) + list(R.fuzz_cases())


@pytest.fixture(scope="module")
def inflater(built):
    f = api.Inflater(0, max_in_bytes=24 << 20, max_out_bytes=24 << 20, max_blocks=400)
    yield f
    f.close()


def _run_and_compare(inflater, cases, **layout):
    streams, lens = [c[1] for c in cases], [len(c[2]) for c in cases]
    call = inflater.run(api.InflateCall(streams, lens, guard=GUARD, fill=0xC3, **layout))
    _, host_status, _ = api.inflate_host(streams, lens)
    assert call.status[:call.n].tolist() == host_status.tolist()
    for i, c in enumerate(cases):
        assert call.output(i) == c[2], c[0]
    _guards_untouched(call, 0xC3)
    return call


def _guards_untouched(call, fill):
    at = 0
    for i in range(call.n):
        b = call.blocks[i]
        assert (call.dst[at:b.out_off] == fill).all(), f"bytes before block {i} were written"
        at = b.out_off + b.out_len
    assert (call.dst[at:call.dst_len] == fill).all(), "bytes behind the last block were written"


def test_one_block_per_call(inflater):
    for c in R.valid_cases():
        _run_and_compare(inflater, [c])


def test_sixty_four_blocks(inflater):
    cases = _all_valid()
    _run_and_compare(inflater, cases[:64])
    _run_and_compare(inflater, cases[-64:], gap=1)             # odd payload offsets


def test_max_blocks_in_one_call(inflater):
    cases = _all_valid()
    cases = (cases * (inflater.max_blocks // len(cases) + 1))[:inflater.max_blocks]
    assert len(cases) == inflater.max_blocks
    _run_and_compare(inflater, cases)


def test_mixed_kinds_and_lengths(inflater):
    by_name = {c[0]: c for c in R.valid_cases()}
    names = ["empty", "len65536-text", "len0-noise-stored", "acgt-fixed", "len1-text", "15-bit-code", "acgt-stored", "long-matches", "len0-text",
             "repeat18-across", "zeros-65536", "stored-after-dynamic", "len32769-noise-stored", "repeat16-across", "codec-65536-flush"]
    _run_and_compare(inflater, [by_name[n] for n in names], gap=5)


def test_two_tickets_in_flight(inflater):
    cases = _all_valid()
    a = api.InflateCall([c[1] for c in cases[:40]], [len(c[2]) for c in cases[:40]], guard=GUARD, fill=1)
    b = api.InflateCall([c[1] for c in cases[40:90]], [len(c[2]) for c in cases[40:90]], guard=GUARD, fill=2)
    ta, tb = inflater.submit(a), inflater.submit(b)
    with pytest.raises(RuntimeError, match="two tickets"):
        inflater.submit(api.InflateCall([cases[0][1]], [len(cases[0][2])]))
    inflater.wait(tb)
    inflater.wait(ta)
    assert a.outputs() == b"".join(c[2] for c in cases[:40]) and not a.status[:a.n].any()
    assert b.outputs() == b"".join(c[2] for c in cases[40:90]) and not b.status[:b.n].any()
    _guards_untouched(a, 1)
    _guards_untouched(b, 2)
    with pytest.raises(RuntimeError, match="ticket"):
        inflater.wait(ta)


def test_inflater_beside_a_consensus_handle(inflater):
    batch = api.synth(n_zmw=4, passes=5, length=400, seed=3)
    h = api.Handle(0)
    try:
        alone = h.consensus(batch)
        cases = _all_valid()[:64]
        want = b"".join(c[2] for c in cases)
        res = api.Results.allocate(batch)
        t = h.submit(batch, res)
        call = api.InflateCall([c[1] for c in cases], [len(c[2]) for c in cases], guard=GUARD, fill=9)
        ti = inflater.submit(call)
        h.wait(t)
        inflater.wait(ti)
        h.release(t)
        assert call.outputs() == want and not call.status[:call.n].any()
        assert np.array_equal(res.status, alone.status) and np.array_equal(res.seq_len, alone.seq_len)
        for z in range(batch.n_zmw):
            assert np.array_equal(res.sequence(z), alone.sequence(z)) and np.array_equal(res.raw(z), alone.raw(z))
    finally:
        h.close()


def test_corrupt_list_statuses_match_the_host(inflater):
    """the fixed list only (every entry has run through the decoder under AddressSanitizer on the CPU: tools/inflate_sanitize.py), once, in one call: each
    corrupt stream between two good ones"""
    good, gdata = R.short_stream()
    corrupt = R.corrupt_cases()
    streams, lens = [good], [len(gdata)]
    for _, s, n, _ in corrupt:
        streams += [s, good]
        lens += [n, len(gdata)]
    call = inflater.run(api.InflateCall(streams, lens, guard=GUARD, fill=0x77))
    _, host_status, _ = api.inflate_host(streams, lens)
    assert call.status[:call.n].tolist() == host_status.tolist()
    for k, (name, _, _, want) in enumerate(corrupt):
        assert call.status[2 * k + 1] != R.OK, name
        if want is not None:
            assert call.status[2 * k + 1] == want, name
    for i in range(0, call.n, 2):
        assert call.status[i] == R.OK and call.output(i) == gdata
    # guard bytes around every block's output range; a failed block's own range may hold anything
    for i in range(call.n):
        b = call.blocks[i]
        assert (call.dst[b.out_off - GUARD:b.out_off] == 0x77).all() and (call.dst[b.out_off + b.out_len:b.out_off + b.out_len + GUARD] == 0x77).all(), i


def test_argument_errors_enqueue_nothing(inflater):
    L = api.lib()
    good, gdata = R.short_stream()

    def fails(mutate, word, f=inflater):
        call = api.InflateCall([good, good], [len(gdata)] * 2, guard=4)
        mutate(call)
        with pytest.raises(RuntimeError, match=word):
            f.run(call)
        assert (call.dst == 0).all() and (call.status == -1).all()

    def set_(i, **kw):
        def m(call):
            for k, v in kw.items():
                setattr(call.blocks[i], k, v)
        return m

    fails(set_(1, in_off=1 << 40), "outside src")
    fails(set_(0, out_off=1 << 40), "outside dst")
    fails(set_(1, out_off=4), "overlap")
    fails(set_(0, out_len=65537), "out_len")
    small = api.Inflater(0, max_in_bytes=64, max_out_bytes=1 << 16, max_blocks=1)
    try:
        fails(lambda call: None, "capacities", f=small)
        with pytest.raises(RuntimeError, match="capacities"):
            small.inflate([good * 2], [len(gdata)])
        out, status = small.inflate([good], [len(gdata)])          # and the inflater is still usable
        assert out == gdata and status.tolist() == [R.OK]
    finally:
        small.close()
    with pytest.raises(RuntimeError, match="capacities"):
        api.Inflater(0, max_in_bytes=0)
    assert L.ccsx_inflate_rule_version() == 1

"""The call slots of the two BGZF codecs' device path (api.Inflater, api.Deflater: one codec host under two descriptions): a slot reused by calls of other
sizes, two tickets of unequal sizes in flight, a call of no items, a codec of one item, and both beside a consensus handle.  Every expectation is the host entry
point's (api.inflate_host / api.deflate_host) on the same payloads; the payloads are the small cases of tests/inflate_ref.py and tests/deflate_ref.py."""
import functools

import numpy as np
import pytest

import deflate_ref as DR
import inflate_ref as R
from ccs_amd import api

pytestmark = pytest.mark.gpu

GUARD, FILL = 16, 0xC3
INITIAL = {"status": -1, "out_len": -1, "crc": 0}          # what a call object's result arrays hold before a call


class Kind:
    """one codec for the tests: its object, its call, the host's run of a call's payloads, and an item's bytes in dst"""

    def __init__(self, name):
        self.name = name
        self.results = ("status",) if name == "inflate" else ("out_len", "crc", "status")

    @functools.lru_cache(maxsize=None)
    def pool(self):
        """the payloads: (what goes into a call, its range length or None) of every case of at most 600 plain bytes, 12 at least"""
        if self.name == "inflate":
            p = tuple((c[1], len(c[2])) for c in R.valid_cases() if len(c[2]) <= 600)
        else:
            p = tuple((data, None) for _, data in DR.all_cases() if len(data) <= 600)[:24]
        return p[::2] + p[1::2]                                # (the cases come sorted by length: every run of eight gets short and long ones)

    def create(self, max_items, nbytes=1 << 16):
        if self.name == "inflate":
            return api.Inflater(0, max_in_bytes=nbytes, max_out_bytes=nbytes, max_blocks=max_items)
        return api.Deflater(0, max_in_bytes=nbytes, max_out_bytes=nbytes, max_spans=max_items)

    def call(self, items):
        if self.name == "inflate":
            return api.InflateCall([p for p, _ in items], [n for _, n in items], guard=GUARD, fill=FILL)
        return api.DeflateCall([p for p, _ in items], guard=GUARD, fill=FILL)

    def host(self, items):
        """the host's call object of these payloads, in the layout of call()"""
        if self.name == "inflate":
            return api.inflate_host([p for p, _ in items], [n for _, n in items], guard=GUARD, fill=FILL)[2]
        return api.deflate_host([p for p, _ in items], guard=GUARD, fill=FILL)[2]


KINDS = {"inflate": Kind("inflate"), "deflate": Kind("deflate")}


@pytest.fixture(scope="module", params=["inflate", "deflate"])
def kind(request, built):
    k = KINDS[request.param]
    assert len(k.pool()) >= 12
    return k


@pytest.fixture(scope="module")
def codec(kind):
    f = kind.create(8)
    yield f
    f.close()


def shrink(call, n):
    """the call with its first n items only: the buffers and the result arrays keep the size of the whole list, so what lies behind item n must stay as it is"""
    call.n = n
    return call


def check(kind, call, want, n):
    """items < n of call are the host's (want: the host's call of the whole list); everything else of dst and of the result arrays is untouched"""
    dst = np.full(len(call.dst), FILL, dtype=np.uint8)
    for i in range(n):
        b = call.items[i]
        m = b.out_len if kind.name == "inflate" else int(want.out_len[i])
        dst[b.out_off:b.out_off + m] = want.dst[b.out_off:b.out_off + m]
    assert np.array_equal(call.dst, dst), "dst differs from the host's inside the first n ranges, or was written outside them"
    for r in kind.results:
        got = getattr(call, r)
        assert n == 0 or got[:n].tolist() == getattr(want, r)[:n].tolist(), r
        assert (got[n:] == INITIAL[r]).all(), f"{r}: an element behind the call's items was written"
    assert n == 0 or not want.status[:n].any()                 # (the payloads are valid: the host's statuses are OK)


def test_shrinking_calls_on_a_reused_slot(kind, codec):
    for k, n in enumerate((8, 3, 0, 1)):
        items = kind.pool()[k:k + 8]                           # other payloads every time: nothing of the call before passes for this one's
        want = kind.host(items)
        check(kind, codec.run(shrink(kind.call(items), n)), want, n)


def test_two_in_flight_of_unequal_sizes(kind, codec):
    big, small = kind.pool()[:8], kind.pool()[9:10]
    a, b = kind.call(big), kind.call(small)
    ta, tb = codec.submit(a), codec.submit(b)
    with pytest.raises(RuntimeError, match="two tickets"):
        codec.submit(kind.call(small))
    assert codec.wait(tb) is b and codec.wait(ta) is a
    check(kind, a, kind.host(big), 8)
    check(kind, b, kind.host(small), 1)
    c, d = kind.call(small), kind.call(big)                    # both slots are free again
    tc, td = codec.submit(c), codec.submit(d)
    codec.wait(tc)
    codec.wait(td)
    check(kind, c, kind.host(small), 1)
    check(kind, d, kind.host(big), 8)


def test_a_call_of_no_items(kind, codec):
    for call in (kind.call([]), shrink(kind.call(kind.pool()[:3]), 0)):
        t = codec.submit(call)
        assert t > 0
        assert codec.wait(t) is call
        assert (call.dst == FILL).all()
        for r in kind.results:
            assert (getattr(call, r) == INITIAL[r]).all(), r
        with pytest.raises(RuntimeError, match="unknown or already waited-for ticket"):
            codec.wait(t)


def test_a_codec_of_one_item(kind):
    one = kind.create(1)
    try:
        for k in (2, 5, 11):
            items = kind.pool()[k:k + 1]
            check(kind, one.run(kind.call(items)), kind.host(items), 1)
        two = kind.call(kind.pool()[:2])
        with pytest.raises(RuntimeError, match="capacities"):
            one.run(two)
        check(kind, two, None, 0)                              # refused: nothing was written
        items = kind.pool()[7:8]
        check(kind, one.run(kind.call(items)), kind.host(items), 1)
    finally:
        one.close()


def test_both_codecs_beside_a_consensus_handle(built):
    batch = api.synth(n_zmw=4, passes=5, length=400, seed=3)
    h = api.Handle(0)
    try:
        alone = h.consensus(batch)
        codecs = {name: k.create(8) for name, k in KINDS.items()}
        try:
            res = api.Results.allocate(batch)
            t = h.submit(batch, res)
            calls = {name: k.call(k.pool()[:8]) for name, k in KINDS.items()}
            tickets = {name: codecs[name].submit(calls[name]) for name in KINDS}
            h.wait(t)
            for name in KINDS:
                codecs[name].wait(tickets[name])
            h.release(t)
            for name, k in KINDS.items():
                check(k, calls[name], k.host(k.pool()[:8]), 8)
            assert np.array_equal(res.status, alone.status) and np.array_equal(res.seq_len, alone.seq_len)
            for z in range(batch.n_zmw):
                assert np.array_equal(res.sequence(z), alone.sequence(z)) and np.array_equal(res.raw(z), alone.raw(z))
        finally:
            for f in codecs.values():
                f.close()
    finally:
        h.close()

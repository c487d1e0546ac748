"""The argument checks of the two BGZF codecs' host entry points (ccsx_inflate_blocks_host, ccsx_deflate_spans_host), from one table: the return code and the
whole ccsx_last_error() text of every refusal, as literals, and that a refused call wrote nothing.  The two share one range / overlap check; its texts differ
in the function's name, the item's noun and the limited field only.  No GPU."""
import ctypes as C
import zlib

import numpy as np
import pytest

import inflate_ref as R
from ccs_amd import api

FILL = 0xA5
I64_MAX, I64_MIN = 2 ** 63 - 1, -2 ** 63


class Codec:
    def __init__(self, kind):
        self.kind = kind
        self.item = api.DeflateBlock if kind == "inflate" else api.DeflateSpan
        self.fn = "ccsx_inflate_blocks_host" if kind == "inflate" else "ccsx_deflate_spans_host"

    def limited(self, v):
        """the second of two items, with the length that has the 0 .. 65536 limit set to v, and the buffers that hold it: (items, src_len, dst_len)"""
        if self.kind == "inflate":
            return [(0, 2, 10, 0), (2, 2, v, 10)], 4, 10 + v
        return [(0, 2, 10, 0), (2, v, 10, 10)], 2 + v, 20

    def real(self, datas, caps=None):
        """a list that is accepted, of real payloads (inflate: the raw DEFLATE stream of each of datas and its length; deflate: each of datas and its bound, or
        caps[i]): the input ranges lie back to back and end at src_len, the output ranges touch and end at dst_len.  The arguments of call()"""
        pay = [R.deflate_raw(d) for d in datas] if self.kind == "inflate" else list(datas)
        olen = [len(d) for d in datas] if self.kind == "inflate" else [api.deflate_bound(len(d)) for d in datas]
        olen = [n if caps is None or caps[i] is None else caps[i] for i, n in enumerate(olen)]
        items, ioff, ooff = [], 0, 0
        for p, n in zip(pay, olen):
            items.append((ioff, len(p), n, ooff))
            ioff, ooff = ioff + len(p), ooff + n
        return dict(items=items, src_len=ioff, dst_len=ooff, src=b"".join(pay))

    def verify(self, items, src, dst, res):
        """an accepted call against zlib: every item's status, its bytes in dst (its lengths and CRC), and nothing written outside what belongs to an item"""
        own = np.zeros(len(dst), dtype=bool)
        for i, (in_off, in_len, olen, out_off) in enumerate(items):
            inp, st = src[in_off:in_off + in_len], int(res["status"][i])
            if self.kind == "inflate":
                d = zlib.decompressobj(-15)
                try:
                    out = d.decompress(inp)
                    ok = d.eof and len(out) == olen
                except zlib.error:
                    ok = False
                if ok:
                    assert st == R.OK and dst[out_off:out_off + olen].tobytes() == out, i
                else:
                    assert st != R.OK and (in_len > 0 or st == R.TRUNCATED_INPUT), (i, st)
                own[out_off:out_off + olen] = True           # (the bytes of a block that is not OK are unspecified)
            elif olen >= api.deflate_bound(in_len):          # the bound is never too small
                m = int(res["out_len"][i])
                assert st == 0 and 0 < m <= olen and zlib.decompress(dst[out_off:out_off + m].tobytes(), -15) == inp, i
                assert int(res["crc"][i]) == zlib.crc32(inp), i
                own[out_off:out_off + m] = True
            else:
                assert olen == 0 and st == 1 and int(res["out_len"][i]) == 0, (i, st)          # nothing fits into no bytes: OUTPUT_FULL
        assert (dst[:len(own)][~own] == FILL).all()

    def call(self, items, src_len, dst_len, n=None, null=(), src=None):
        """one raw call: items are (in_off, in_len, out_len | out_cap, out_off).  Returns (rc, the error text, dst, {result arrays})"""
        L = api.lib()
        n = len(items) if n is None else n
        arr = (self.item * max(len(items), 1))(*[self.item(*t) for t in items])
        s = np.zeros(max(src_len, 1), dtype=np.uint8)
        if src is not None:
            s[:len(src)] = np.frombuffer(src, dtype=np.uint8)
        dst = np.full(max(dst_len, 1), FILL, dtype=np.uint8)
        m = max(len(items), 1)
        res = {"status": np.full(m, -1, dtype=np.int32)}
        if self.kind == "deflate":
            res = {"out_len": np.full(m, -1, dtype=np.int32), "crc": np.zeros(m, dtype=np.uint32), **res}
        ty = {"status": C.c_int32, "out_len": C.c_int32, "crc": C.c_uint32}
        args = [None if "src" in null else api._ptr(s, C.c_uint8), src_len, None if "items" in null else arr, n, None if "dst" in null else api._ptr(dst, C.c_uint8),
                dst_len] + [None if k in null else api._ptr(a, ty[k]) for k, a in res.items()]
        rc = getattr(L, self.fn)(*args)
        return rc, L.ccsx_last_error().decode(), dst, res


TWO = [(0, 2, 10, 0), (2, 2, 10, 10)]          # two items whose input ranges end at src_len = 4 and whose output ranges touch and end at dst_len = 20


def two(i, **kw):
    """TWO with fields of item i replaced"""
    items = [list(t) for t in TWO]
    for k, v in kw.items():
        items[i][("in_off", "in_len", "olen", "out_off").index(k)] = v
    return [tuple(t) for t in items]


# name -> (the call's arguments as f(codec), {codec: (rc, text)}); rc 0: accepted, and the results are checked against zlib (Codec.verify)
CASES = {
    "negative src_len": (lambda c: dict(items=TWO, src_len=-1, dst_len=20), {
        "inflate": (-1, "ccsx_inflate_blocks_host: negative size"), "deflate": (-1, "ccsx_deflate_spans_host: negative size")}),
    "negative dst_len": (lambda c: dict(items=TWO, src_len=4, dst_len=-1), {
        "inflate": (-1, "ccsx_inflate_blocks_host: negative size"), "deflate": (-1, "ccsx_deflate_spans_host: negative size")}),
    "negative count": (lambda c: dict(items=TWO, src_len=4, dst_len=20, n=-1), {
        "inflate": (-1, "ccsx_inflate_blocks_host: negative size"), "deflate": (-1, "ccsx_deflate_spans_host: negative size")}),
    "null items": (lambda c: dict(items=TWO, src_len=4, dst_len=20, null=("items",)), {
        "inflate": (-1, "ccsx_inflate_blocks_host: null argument"), "deflate": (-1, "ccsx_deflate_spans_host: null argument")}),
    "null status": (lambda c: dict(items=TWO, src_len=4, dst_len=20, null=("status",)), {
        "inflate": (-1, "ccsx_inflate_blocks_host: null argument"), "deflate": (-1, "ccsx_deflate_spans_host: null argument")}),
    "null out_len": (lambda c: dict(items=TWO, src_len=4, dst_len=20, null=("out_len",)), {"deflate": (-1, "ccsx_deflate_spans_host: null argument")}),
    "null crc": (lambda c: dict(items=TWO, src_len=4, dst_len=20, null=("crc",)), {"deflate": (-1, "ccsx_deflate_spans_host: null argument")}),
    "null src": (lambda c: dict(items=TWO, src_len=4, dst_len=20, null=("src",)), {
        "inflate": (-1, "ccsx_inflate_blocks_host: null argument"), "deflate": (-1, "ccsx_deflate_spans_host: null argument")}),
    "null dst": (lambda c: dict(items=TWO, src_len=4, dst_len=20, null=("dst",)), {
        "inflate": (-1, "ccsx_inflate_blocks_host: null argument"), "deflate": (-1, "ccsx_deflate_spans_host: null argument")}),
    # (an empty stream is TRUNCATED_INPUT, an empty span an empty stored block; "\x03\x00" is the stream of no bytes, and no stream fits into no bytes)
    "null src of no bytes": (lambda c: dict(items=[(0, 0, 10, 0)], src_len=0, dst_len=10, null=("src",)), {"inflate": (0, ""), "deflate": (0, "")}),
    "null dst of no bytes": (lambda c: dict(items=[(0, 2, 0, 0)], src_len=2, dst_len=0, null=("dst",), src=b"\x03\x00"), {"inflate": (0, ""), "deflate": (0, "")}),
    "everything null, no items": (lambda c: dict(items=[], src_len=0, dst_len=0, null=("src", "items", "dst", "status", "out_len", "crc")), {
        "inflate": (0, ""), "deflate": (0, "")}),
    "limited length 65536": (lambda c: c.real([R.acgt(10, 1), R.text(65536, 2)]), {"inflate": (0, ""), "deflate": (0, "")}),
    "limited length 65537": (lambda c: dict(zip(("items", "src_len", "dst_len"), c.limited(65537))), {
        "inflate": (-1, "ccsx_inflate_blocks_host: block 1: out_len outside 0 .. 65536"), "deflate": (-1, "ccsx_deflate_spans_host: span 1: in_len outside 0 .. 65536")}),
    "ranges end at src_len and dst_len, outputs touch": (lambda c: c.real([R.text(10, 3), R.acgt(10, 4)]), {"inflate": (0, ""), "deflate": (0, "")}),
    "input range one past src_len": (lambda c: dict(items=two(1, in_off=3), src_len=4, dst_len=20), {
        "inflate": (-1, "ccsx_inflate_blocks_host: block 1: input range outside src"), "deflate": (-1, "ccsx_deflate_spans_host: span 1: input range outside src")}),
    "in_len -1": (lambda c: dict(items=two(0, in_len=-1), src_len=4, dst_len=20), {
        "inflate": (-1, "ccsx_inflate_blocks_host: block 0: input range outside src"), "deflate": (-1, "ccsx_deflate_spans_host: span 0: in_len outside 0 .. 65536")}),
    "in_off 2**63 - 1": (lambda c: dict(items=two(1, in_off=I64_MAX), src_len=4, dst_len=20), {
        "inflate": (-1, "ccsx_inflate_blocks_host: block 1: input range outside src"), "deflate": (-1, "ccsx_deflate_spans_host: span 1: input range outside src")}),
    "in_off -2**63": (lambda c: dict(items=two(1, in_off=I64_MIN), src_len=4, dst_len=20), {
        "inflate": (-1, "ccsx_inflate_blocks_host: block 1: input range outside src"), "deflate": (-1, "ccsx_deflate_spans_host: span 1: input range outside src")}),
    "in_off 1 << 40": (lambda c: dict(items=two(1, in_off=1 << 40), src_len=4, dst_len=20), {
        "inflate": (-1, "ccsx_inflate_blocks_host: block 1: input range outside src"), "deflate": (-1, "ccsx_deflate_spans_host: span 1: input range outside src")}),
    "out_off 2**63 - 1": (lambda c: dict(items=two(1, out_off=I64_MAX), src_len=4, dst_len=20), {
        "inflate": (-1, "ccsx_inflate_blocks_host: block 1: output range outside dst"), "deflate": (-1, "ccsx_deflate_spans_host: span 1: output range outside dst")}),
    "out_off -2**63": (lambda c: dict(items=two(1, out_off=I64_MIN), src_len=4, dst_len=20), {
        "inflate": (-1, "ccsx_inflate_blocks_host: block 1: output range outside dst"), "deflate": (-1, "ccsx_deflate_spans_host: span 1: output range outside dst")}),
    "out_off 1 << 40": (lambda c: dict(items=two(1, out_off=1 << 40), src_len=4, dst_len=20), {
        "inflate": (-1, "ccsx_inflate_blocks_host: block 1: output range outside dst"), "deflate": (-1, "ccsx_deflate_spans_host: span 1: output range outside dst")}),
    "output range one past dst_len": (lambda c: dict(items=two(1, out_off=11), src_len=4, dst_len=20), {
        "inflate": (-1, "ccsx_inflate_blocks_host: block 1: output range outside dst"), "deflate": (-1, "ccsx_deflate_spans_host: span 1: output range outside dst")}),
    "output ranges overlap by one byte": (lambda c: dict(items=two(1, out_off=9), src_len=4, dst_len=20), {
        "inflate": (-1, "ccsx_inflate_blocks_host: blocks 0 and 1: output ranges overlap"), "deflate": (-1, "ccsx_deflate_spans_host: spans 0 and 1: output ranges overlap")}),
    "output ranges overlap by one byte, descending": (lambda c: dict(items=[(0, 2, 10, 9), (2, 2, 10, 0)], src_len=4, dst_len=20), {
        "inflate": (-1, "ccsx_inflate_blocks_host: blocks 1 and 0: output ranges overlap"), "deflate": (-1, "ccsx_deflate_spans_host: spans 1 and 0: output ranges overlap")}),
    # A = [0, 10), Z = [5, 5), B = [5, 15): the empty range sorts between the two that overlap and hides nothing
    "empty range between two overlapping ones": (lambda c: dict(items=[(0, 2, 10, 0), (2, 0, 0, 5), (2, 2, 10, 5)], src_len=4, dst_len=15), {
        "inflate": (-1, "ccsx_inflate_blocks_host: blocks 0 and 2: output ranges overlap"), "deflate": (-1, "ccsx_deflate_spans_host: spans 0 and 2: output ranges overlap")}),
    "empty range between two that touch": (lambda c: c.real([R.text(10, 3), b"", R.acgt(10, 4)], caps=[None, 0, None]), {"inflate": (0, ""), "deflate": (0, "")}),
}
TABLE = [(kind, name) for name, (_, want) in CASES.items() for kind in ("inflate", "deflate") if kind in want]


@pytest.mark.parametrize("kind,name", TABLE, ids=[f"{k}: {n}" for k, n in TABLE])
def test_refusals_and_their_texts(built, kind, name):
    c = Codec(kind)
    make, want = CASES[name]
    kw = make(c)
    rc, msg, dst, res = c.call(**kw)
    want_rc, want_msg = want[kind]
    assert rc == want_rc, (rc, msg)
    if want_rc == 0:
        src = kw.get("src", b"") + bytes(max(kw["src_len"], 0))      # (what call() makes of it: zeros behind the bytes given)
        c.verify(kw["items"], src, dst, res)
        return
    assert msg == want_msg
    assert (dst == FILL).all() and (res["status"] == -1).all()       # a refused call wrote nothing
    if kind == "deflate":
        assert (res["out_len"] == -1).all() and (res["crc"] == 0).all()


@pytest.mark.parametrize("kind", ["inflate", "deflate"])
def test_descending_output_offsets_are_accepted_and_right(built, kind):
    c = Codec(kind)
    datas = [R.text(300, 1), R.acgt(200, 2), b"", R.text(77, 3)]
    payloads = [R.deflate_raw(d) for d in datas] if kind == "inflate" else datas
    olens = [len(d) for d in datas] if kind == "inflate" else [api.deflate_bound(len(d)) for d in datas]
    g, ioff, ooff, items = 3, 0, 3 + sum(n + 3 for n in olens), []
    for p, n in zip(payloads, olens):                        # inputs in order, outputs from the end of dst backwards, g guard bytes around each
        ooff -= n + g
        items.append((ioff, len(p), n, ooff))
        ioff += len(p)
    dst_len = g + sum(n + g for n in olens)
    rc, msg, dst, res = c.call(items, ioff, dst_len, src=b"".join(payloads))
    assert rc == 0, msg
    assert not res["status"].any()
    used = np.zeros(dst_len, dtype=bool)
    for i, (d, (_, _, n, off)) in enumerate(zip(datas, items)):
        if kind == "inflate":
            assert dst[off:off + n].tobytes() == d, i
            used[off:off + n] = True
        else:
            m = int(res["out_len"][i])
            assert 0 < m <= n and zlib.decompress(dst[off:off + m].tobytes(), -15) == d and int(res["crc"][i]) == zlib.crc32(d), i
            used[off:off + m] = True
    assert (dst[:dst_len][~used] == FILL).all()              # the guard bytes, and of a deflate range what the stream does not fill

"""The buffers the barcode calls and the segmentation share, on an MI355X (DESIGN.md §2 "Barcode calls", "Segment rule"): a handle has one staging buffer for
the caller's reads of ccsx_barcode_reads and ccsx_segment_reads, a slot one device buffer and one pinned set for whichever of the two requests its ticket
carries.  So the two analyses alternate here, on one handle: the synchronous calls with growing and shrinking read counts, each into a poisoned report and
compared field for field with the host rule; then five tickets in a row, so that a slot that carried one analysis is reused by the other, each compared with
the synchronous run of the same request; then a plain run."""
import numpy as np
import pytest

from ccs_amd import api
import segment_lab as LAB

pytestmark = pytest.mark.gpu
RES_FIELDS = ("status", "seq_len", "rq", "np_", "ec", "iters", "n_windows", "fn", "rn")
READ_COUNTS = (1, 2, 3, 64, 1)          # odd counts: both paddings of the staging buffer are non-zero for barcodes; 64 then 1: a grown buffer is reused
READ_LENGTHS = (0, 8, 65, 1025)         # 0: untested; mixed within a call
FIRST_LENGTH = (1, 0, 2, 0, 3)          # where in READ_LENGTHS call i starts, so that the two calls of one read differ


@pytest.fixture(scope="module")
def handle(built):
    h = api.Handle(0)
    yield h
    h.close()


def _poisoned(cls, n, pinned=False):
    rep = cls.allocate(n, pinned=pinned)
    for k in cls.FIELDS:
        getattr(rep, k).view(np.uint8)[...] = 0xA5
    return rep


def _same_report(got, want):
    assert type(got) is type(want)
    for k in type(got).FIELDS:
        assert getattr(got, k).tobytes() == getattr(want, k).tobytes(), k


def _same_results(a, b, n):
    for f in RES_FIELDS:
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f
    for z in range(n):
        assert np.array_equal(a.sequence(z), b.sequence(z)) and np.array_equal(a.quals(z), b.quals(z)), z
        assert np.array_equal(a.raw(z).view(np.uint32), b.raw(z).view(np.uint32)), z


def test_the_synchronous_calls_alternate_on_one_staging_buffer(handle):
    rng = np.random.default_rng(5)

    def pat(n, m):
        return [rng.integers(0, 4, m).astype(np.uint8) for _ in range(n)]

    bsets, ssets = [pat(1, 8), pat(3, 8)], [pat(2, 8), pat(3, 64)]
    for i, n in enumerate(READ_COUNTS):
        lens = [READ_LENGTHS[(FIRST_LENGTH[i] + k) % 4] for k in range(n)]
        for cls, sets, on_gpu, on_host in ((api.BarcodeReport, bsets, handle.barcode_reads, api.barcode_reads_host),
                                           (api.SegmentReport, ssets, handle.segment_reads, api.segment_reads_host)):
            S = sets[i % 2]
            reads = [rng.integers(0, 4, m).astype(np.uint8) for m in lens]
            for k, r in enumerate(reads):                            # (a pattern of the set in every read that has room for it, so that there are calls and cuts)
                p = S[k % len(S)]
                if len(r) >= 2 * len(p):
                    r[3: 3 + len(p)] = p
                    r[len(r) - len(p):] = p if cls is api.SegmentReport else 3 - p[::-1]
            pset = (api.BarcodeSet if cls is api.BarcodeReport else api.SegmentSet).from_codes(S)
            got = on_gpu(pset, reads, None, _poisoned(cls, n))
            want = on_host(pset, reads, None, _poisoned(cls, n))
            _same_report(got, want)
            assert got.tested.tolist() == [int(m > 0) for m in lens]


def test_tickets_alternate_on_the_slots(handle):
    b, _, S = LAB.batch()
    n = b.n_zmw
    plain = handle.consensus(b)
    bsets = [api.BarcodeSet.from_codes([a[:16] for a in S]), api.BarcodeSet.from_codes([a[:16] for a in S[:2]])]
    ssets = [api.SegmentSet.from_codes(S), api.SegmentSet.from_codes(S[:3])]
    # ticket i: barcodes when i is even, segments when it is odd; three slots, so tickets 3 and 4 take the slots of tickets 0 and 1 for the other analysis
    asks = [("barcodes", "barcode_set", api.BarcodeReport, bsets[0]), ("segments", "segment_set", api.SegmentReport, ssets[0]),
            ("barcodes", "barcode_set", api.BarcodeReport, bsets[1]), ("segments", "segment_set", api.SegmentReport, ssets[1]),
            ("barcodes", "barcode_set", api.BarcodeReport, bsets[0])]
    sync = [(handle.consensus_barcodes if key == "barcodes" else handle.consensus_segments)(b, pset) for key, _, _, pset in asks[:4]]
    sync.append(sync[0])
    assert any(int(rep.tested.sum()) > 0 for _, rep in sync)
    pb = b.pinned()
    out = []

    def finish(i):
        t, res, rep = out[i]
        handle.wait(t)
        _same_results(res, sync[i][0], n)
        _same_results(res, plain, n)                                 # (detection only)
        _same_report(rep, sync[i][1])
        handle.release(t)

    for i, (key, set_key, cls, pset) in enumerate(asks):
        if i >= 3:
            finish(i - 3)                                            # (before its slot is taken again)
        res, rep = api.Results.allocate(b, pinned=True), _poisoned(cls, n, pinned=True)
        out.append((handle.submit(pb, res, **{key: rep, set_key: pset}), res, rep))
    for i in (2, 3, 4):
        finish(i)
    _same_results(handle.consensus(b), plain, n)                     # a plain run after the requests: nothing of them is left in a slot

"""k_inflate at the format's limits: the hand-assembled streams of inflate_ref.limit_cases() through the wave (the bytes they were assembled from, and status for
status the host's run, which tests/test_inflate_limits.py pins to zlib), and the window's way out to HBM at every skew of the 16-byte pieces.  The corrupt
streams that inflate_ref.more_corrupt_cases() added reach the device through tests/test_inflate_gpu.py::test_corrupt_list_statuses_match_the_host, which
iterates the fixed list; nothing else that is corrupt goes to a GPU.

What the 64 lanes do that the host's one lane does not: the ballots that count and rank the code lengths, the sub-table fill (lane << rest), the copies
spread over the lanes, the 16-byte pieces.  Slips tried in a scratch copy (values only, every index in range), and what notices them:
  - ccsx_infl_build sub-table fill `lane << rest` -> `lane << sub_bits` (only lane 0 then fills a sub-table: the replicated entries stay unassigned; one lane
    does not show it): run once on an MI355X, test_limit_streams_sixty_four_per_call fails (BAD_SYMBOL on 5 of the first 6 streams where the host says
    OK), and so does tests/test_inflate_gpu.py::test_one_block_per_call from before.
  - ccsx_infl_build `k += nl << rest` -> `nl << sub_bits`: the same table on 64 lanes (either stride leaves a sub-table of at most 128 entries after one
    step), so it is equivalent on the device; one lane shows it, and the two other build slips: tests/test_inflate_limits.py.
  - k_inflate `head` from `skew` without `& 15`: only skew 0 changes, to a head of 16 bytes copied one by one and a body that starts 16 bytes later, still
    aligned: the same bytes.  Equivalent."""
import pytest

import inflate_ref as R
from ccs_amd import api

pytestmark = pytest.mark.gpu

GUARD = 32
LIMITS = R.limit_cases()
SKEW_LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33)


@pytest.fixture(scope="module")
def inflater(built):
    f = api.Inflater(0, max_in_bytes=4 << 20, max_out_bytes=8 << 20, max_blocks=256)
    yield f
    f.close()


def _guards_untouched(call, fill):
    order = sorted(range(call.n), key=lambda i: call.blocks[i].out_off)
    at = 0
    for i in order:
        b = call.blocks[i]
        assert (call.dst[at:b.out_off] == fill).all(), f"bytes before block {i} were written"
        at = b.out_off + b.out_len
    assert (call.dst[at:call.dst_len] == fill).all(), "bytes behind the last block were written"


def _run_and_compare(inflater, cases, skews=None, **layout):
    streams, lens = [c[1] for c in cases], [len(c[2]) for c in cases]
    call = api.InflateCall(streams, lens, guard=GUARD + 16 if skews else GUARD, fill=0xC3, **layout)
    if skews:                                                     # every output moved up by less than 16 bytes: at least GUARD bytes stay between two of them
        for i, skew in enumerate(skews):
            call.blocks[i].out_off += (skew - call.blocks[i].out_off) & 15
            assert call.blocks[i].out_off & 15 == skew
    inflater.run(call)
    _, host_status, _ = api.inflate_host(streams, lens)
    assert call.status[:call.n].tolist() == host_status.tolist() == [R.OK] * call.n
    for i, c in enumerate(cases):
        assert call.output(i) == c[2], c[0]
    _guards_untouched(call, 0xC3)
    return call


def test_limit_streams_sixty_four_per_call(inflater):
    for at in range(0, len(LIMITS), 64):
        _run_and_compare(inflater, LIMITS[at:at + 64], gap=(at // 64) % 2)          # every second call at odd payload offsets


def test_shaped_limit_streams_one_per_call(inflater):
    for c in LIMITS:
        if not c[0].startswith("codes"):
            _run_and_compare(inflater, [c])


def test_all_limit_streams_in_one_call_at_odd_offsets(inflater):
    _run_and_compare(inflater, LIMITS, gap=3)


def test_every_skew_of_the_output(inflater):
    """128 tiny streams: every output length around the 16-byte pieces at every out_off & 15 (the device buffer is 16-byte aligned, so that is the skew the
    kernel computes), then 65536 bytes at skews 1 and 15"""
    cases, skews = [], []
    for n in SKEW_LENGTHS:
        for skew in range(16):
            d = R.text(n, 100 * n + skew)
            cases.append((f"len{n}-skew{skew}", R.deflate_raw(d, strategy=(R.zlib.Z_FIXED if skew & 1 else R.zlib.Z_DEFAULT_STRATEGY), level=0 if skew % 4 == 2 else 6), d))
            skews.append(skew)
    assert len(cases) == 128
    _run_and_compare(inflater, cases, skews)
    big = R.acgt(65536, 77)
    _run_and_compare(inflater, [("skew1", R.deflate_raw(big), big), ("skew15", R.deflate_raw(big, level=0), big)], [1, 15])

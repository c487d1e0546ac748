"""k_cell on an MI355X (DESIGN.md §2 "Cell-tag rule", §4): Handle.cell_reads against tests/cell_ref.py on the whole limit set, field for field, on a poisoned
report, in one call per case and again with the reads in reverse order; calls that bring different whitelists in turn (the handle's resident copy follows the
whitelist's serial); a consensus ticket in flight around a call, completing with its own results."""
import numpy as np
import pytest

from ccs_amd import api
import cell_ref as R

pytestmark = pytest.mark.gpu
CASES = R.limit_cases()
NAMES = [c[0] for c in CASES]
RES_FIELDS = ("status", "seq_len", "rq", "np_", "ec", "iters", "n_windows", "fn", "rn")


@pytest.fixture(scope="module")
def handle(built):
    h = api.Handle(0)
    yield h
    h.close()


def _opts(d):
    o = api.CdnaOpts()
    for k in R.DEFAULTS:
        setattr(o, k, d[k])
    return o


def _design(d):
    x = api.CellDesign()
    for k in R.DESIGN:
        setattr(x, k, d[k])
    return x


def _poisoned(n):
    rep = api.CellReport.allocate(n)
    for k in R.FIELDS:
        getattr(rep, k).view(np.uint8)[...] = 0xA5
    return rep


def _run(handle, i, wl, reverse=False):
    name, S, roles, o, d, _, reads = CASES[i]
    reads = list(reads)[::-1] if reverse else list(reads)
    return handle.cell_reads(api.CdnaPrimers.from_codes(S, roles), reads, _design(d), wl, _opts(o), _poisoned(len(reads)))


@pytest.mark.parametrize("i", range(len(CASES)), ids=NAMES)
def test_reads_equal_the_restatement_on_the_limit_set(handle, i):
    name, want, wl = NAMES[i], R.expected(i), CASES[i][5]
    w = api.CellWhitelist(wl) if wl is not None else None
    rep = _run(handle, i, w)
    assert R.diff(rep, want) == [], (name, R.diff(rep, want))
    rev = _run(handle, i, w, reverse=True)
    assert R.diff(rev, R.reversed_order(want)) == [], (name, "reversed", R.diff(rev, R.reversed_order(want)))


def test_calls_with_different_whitelists_in_turn(handle):
    """the resident table is the last call's: two whitelists alternate, one is freed and a new one made in its place, and a call without one comes between"""
    a, b, raw = NAMES.index("wl1000"), NAMES.index("kinds"), NAMES.index("raw")
    wa, wb = api.CellWhitelist(CASES[a][5]), api.CellWhitelist(CASES[b][5])
    for i, w in ((a, wa), (b, wb), (a, wa), (a, wa), (raw, None), (b, wb)):
        assert R.diff(_run(handle, i, w), R.expected(i)) == [], NAMES[i]
    # the reads of one case under the other's whitelist: what the restatement says of that pairing, not what the resident table of the call before would give
    name, S, roles, o, d, _, reads = CASES[a]
    want = R.cell_reads(S, roles, reads, d, CASES[b][5], **o)
    assert R.diff(handle.cell_reads(api.CdnaPrimers.from_codes(S, roles), list(reads), _design(d), wb, _opts(o)), want) == [] and (want["tag"] == R.ABSENT).all()
    wb.close()
    wc = api.CellWhitelist(CASES[a][5])                             # (a new object, perhaps at the freed one's address: its serial is new)
    assert R.diff(_run(handle, a, wc), R.expected(a)) == []


def test_a_ticket_in_flight_completes_untouched(handle):
    """the call stages nothing: a consensus ticket submitted before it completes with the results of a plain run"""
    b = api.synth(n_zmw=6, passes=5, length=400, seed=9)
    plain = handle.consensus(b)
    res = api.Results.allocate(b, pinned=True)
    t = handle.submit(b.pinned(), res)
    i = NAMES.index("kinds")
    w = api.CellWhitelist(CASES[i][5])
    assert R.diff(_run(handle, i, w), R.expected(i)) == []
    handle.wait(t)
    handle.release(t)
    for f in RES_FIELDS:
        assert getattr(res, f).tobytes() == getattr(plain, f).tobytes(), f
    for z in range(b.n_zmw):
        assert np.array_equal(res.sequence(z), plain.sequence(z)) and np.array_equal(res.quals(z), plain.quals(z)), z
    assert R.diff(_run(handle, i, w), R.expected(i)) == []

"""k_represent on an MI355X (DESIGN.md §2 "Representative rule", §4): Handle.consensus_represent on the ZMWs of tests/represent_lab.py, for every combination of
subread_fallback and kinetics, against ccsx_represent_host applied to the results of the request-free run just before it and to the drafts Handle.stage_draft
read back after that run — report and every byte of every plane.  The planes come down whole, so the comparison covers what lies behind a sequence's end and
every slot of a POLISHED or NONE ZMW: the device's planes keep between the two runs whatever they held, and the request-free run writes them as it always
does, so a byte k_represent writes where the rule writes none is a difference.  The caller's planes are poisoned before every call (a plane that did not come
down shows).  The same comparison on what of the CPU limit set the engine reaches by construction (_limit_batch).  Then three tickets in flight with their own flags, a handle with min_passes 1 beside one with 2, the request beside another screen, the calls
that are refused, and a request-free run after all of it.

Which status each lab ZMW ends with is checked on the CPU oracle in tests/test_represent_ref.py; here the statuses the GPU returns are asserted."""
import numpy as np
import pytest

from ccs_amd import api
import represent_lab as LAB
import represent_ref as R

pytestmark = pytest.mark.gpu
COMBOS = ((0, 0), (1, 0), (0, 1), (1, 1))


def _opts(min_passes=2):
    o = api.default_opts()
    o.min_passes, o.hifi_kinetics, o.top_passes = min_passes, 1, 0     # top_passes 0: every pass up to CCSX_MAX_PASSES = 255, so that the cut is the engine's
    return o


@pytest.fixture(scope="module")
def handle(built):
    h = api.Handle(0, opts=_opts())
    yield h
    h.close()


@pytest.fixture(scope="module")
def lab(built):
    return LAB.batch()


def _plain_and_drafts(h, b):
    res = R.poisoned_results(b, kinetics=True)
    cb, cr = b.c_struct(), res.c_struct()
    h._check(h._L.ccsx_consensus_batch(h._h, cb, cr), "ccsx_consensus_batch")
    return res, [h.stage_draft(z) for z in range(b.n_zmw)]


def _expected(h, b, plain, drafts, fb, kin):
    want = R.clone(plain)
    rep = api.represent_host(b, h.opts, plain.status, drafts, want, fb, kin)
    return want, rep


def _valid_equal(a, b, n, cls, kin=0):
    """a and b agree in every per-ZMW word and in the first seq_len elements of every plane (the kinetics planes where the polish wrote them, or the rule
    with kin set)"""
    for f in R.ZMW_FIELDS:
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f
    for z in range(n):
        o, L = int(a.seq_off[z]), int(a.seq_len[z])
        for f in ("seq", "qual", "raw_qv"):
            assert getattr(a, f)[o:o + L].tobytes() == getattr(b, f)[o:o + L].tobytes(), (z, f)
        if cls[z] == R.POLISHED:
            assert a.kin[:, o:o + L].tobytes() == b.kin[:, o:o + L].tobytes(), z
        elif cls[z] == R.SUBREAD and kin:
            assert a.kin[:2, o:o + L].tobytes() == b.kin[:2, o:o + L].tobytes(), z


@pytest.fixture(scope="module")
def sync_runs(handle, lab):
    """per (fallback, kinetics): the request-free results, the staged drafts, what the host rule makes of them, and what the kernel returned"""
    b, kinds = lab
    out = {}
    for fb, kin in COMBOS:
        plain, drafts = _plain_and_drafts(handle, b)
        want, wrep = _expected(handle, b, plain, drafts, fb, kin)
        got, rep = handle.consensus_represent(b, bool(fb), bool(kin), res=R.poisoned_results(b, kinetics=True))
        out[(fb, kin)] = (plain, drafts, want, wrep, got, rep)
    return out


def test_statuses_the_lab_is_built_for(handle, lab, sync_runs):
    b, kinds = lab
    plain, drafts = sync_runs[(0, 0)][:2]
    for z, kind in enumerate(kinds):
        want = {"polished": (R.SUCCESS, R.LOW_RQ), "few": (R.TOO_FEW_PASSES,), "unrelated": (R.TOO_MANY_UNUSABLE,)}[kind]
        assert int(plain.status[z]) in want, (z, kind, int(plain.status[z]))
        assert (len(drafts[z]) > 0) == (kind != "few"), (z, kind)
        assert plain.seq_len[z] == 0 or kind == "polished"


@pytest.mark.parametrize("fb,kin", COMBOS)
def test_kernel_equals_the_host_rule_byte_for_byte(handle, lab, sync_runs, fb, kin):
    b, kinds = lab
    plain, drafts, want, wrep, got, rep = sync_runs[(fb, kin)]
    assert rep.cls.tolist() == wrep.cls.tolist() and rep.pass_.tolist() == wrep.pass_.tolist()
    assert R.diff(got, want) == []
    rcls, rpass = R.apply(b, handle.opts.top_passes, plain.status, drafts, R.clone(plain), fb, kin)   # (and the restatement says the same)
    assert rep.cls.tolist() == rcls.tolist() and rep.pass_.tolist() == rpass.tolist()
    for z, kind in enumerate(kinds):
        c = int(rep.cls[z])
        if c in (R.POLISHED, R.NONE):
            assert R.diff_zmw(got, plain, z) == [], z                # plane for plane the request-free run
        assert c == {"polished": R.POLISHED, "unrelated": R.SUBREAD if fb else R.DRAFT}.get(kind, R.NONE if b.read_off[z + 1] == b.read_off[z] else R.SUBREAD), (z, kind)
        assert got.status[z] == plain.status[z] and got.np_[z] == plain.np_[z]
        if c >= R.DRAFT:
            assert got.seq_len[z] > 0 and got.rq[z] == -1.0 and (got.quals(z) == 10).all() and (got.raw(z) == 10.0).all()
        if c == R.DRAFT:
            assert np.array_equal(got.sequence(z), drafts[z])
        if c == R.SUBREAD:
            r = int(b.read_off[z]) + int(rep.pass_[z])
            lo, hi = int(b.base_off[r]), int(b.base_off[r + 1])
            assert np.array_equal(got.sequence(z), b.bases[lo:hi] & 3)                      # native orientation, whatever the strand
            o = int(got.seq_off[z])
            if kin:
                assert np.array_equal(got.kin[0, o:o + hi - lo], b.ipd[lo:hi]) and np.array_equal(got.kin[1, o:o + hi - lo], b.pw[lo:hi])
    assert {R.POLISHED, R.NONE, R.SUBREAD} <= set(rep.cls.tolist()) and (fb or R.DRAFT in rep.cls.tolist())
    assert any(b.flags[int(b.read_off[z]) + int(rep.pass_[z])] & 1 for z in range(b.n_zmw) if rep.cls[z] == R.SUBREAD)   # a reverse-strand representative


def _limit_batch():
    """what of the CPU limit set the engine reaches by construction, as one batch: a single full-length pass of every length of R.LENGTHS with 0 - 2 partial
    ones behind it (TOO_FEW_PASSES: a subread of that length, sources and destinations at every alignment), partial passes only with ties at the median, 255
    passes, 260 passes (the cut), two unrelated passes of 255 | 256 | 257 and 3001 bases (a draft of about that length)"""
    rng = np.random.default_rng(77)
    rnd = lambda L: rng.integers(0, 4, int(L)).astype(np.uint8)
    zmws = []
    for k, L in enumerate(R.LENGTHS):
        zmws.append([(rnd(L), k & 1)] + [(rnd(3 + k), R.PARTIAL | (k & 1))] * (k % 3))
    zmws += [[(rnd(7), R.PARTIAL | (q & 1)) for q in range(k)] for k in (1, 2, 3, 4)]
    zmws.append([(rnd(5 + (q * 7) % 23), R.PARTIAL | (q & 1)) for q in range(255)])
    zmws.append([(rnd(40), 1)] + [(rnd(5 + (q * 5) % 31), R.PARTIAL) for q in range(259)])
    zmws.append([(rnd(5 + (q * 11) % 37), R.PARTIAL | (q & 1)) for q in range(260)])
    zmws += [[(rnd(L), 0), (rnd(L - 1), 1)] for L in (255, 256, 257, 3001)]
    return R.make_batch(zmws, seed=78)


@pytest.mark.parametrize("fb,kin", ((0, 1), (1, 0)))
def test_limit_set_through_the_kernel(handle, fb, kin):
    b = _limit_batch()
    plain, drafts = _plain_and_drafts(handle, b)
    want, wrep = _expected(handle, b, plain, drafts, fb, kin)
    got, rep = handle.consensus_represent(b, bool(fb), bool(kin), res=R.poisoned_results(b, kinetics=True))
    assert rep.cls.tolist() == wrep.cls.tolist() and rep.pass_.tolist() == wrep.pass_.tolist()
    assert R.diff(got, want) == []
    nl = len(R.LENGTHS)
    assert (plain.status[:nl + 7] == R.TOO_FEW_PASSES).all() and (rep.cls[:nl + 7] == R.SUBREAD).all()
    assert got.seq_len[:nl].tolist() == list(R.LENGTHS) and rep.pass_[:nl].tolist() == [0] * nl
    assert rep.pass_[nl:nl + 4].tolist() == [0, 1, 1, 2]              # equal lengths: rank |C| // 2 by index
    assert rep.pass_[nl + 5] == 0 and 0 <= rep.pass_[nl + 6] < 255     # one full-length pass among 260: the set; 260 partial ones: the first 255 count
    lens = [5 + (q * 11) % 37 for q in range(255)]
    assert rep.pass_[nl + 6] == sorted((l, q) for q, l in enumerate(lens))[127][1]
    assert (rep.cls[nl + 7:] == (R.SUBREAD if fb else R.DRAFT)).all() and (plain.status[nl + 7:] == R.TOO_MANY_UNUSABLE).all()


def test_three_tickets_with_their_own_flags(handle, lab, sync_runs):
    b, kinds = lab
    pb = b.pinned()
    flags = [(0, 1), (1, 0), (0, 0)]
    out = []
    for fb, kin in flags:
        res, rep = api.Results.allocate(b, kinetics=True, pinned=True), api.RepresentReport.allocate(b.n_zmw, pinned=True)
        for f in R.ZMW_FIELDS + R.PLANE_FIELDS:
            getattr(res, f).view(np.uint8)[...] = R.POISON
        out.append((handle.submit(pb, res, represent=rep, represent_fallback=bool(fb), represent_kinetics=bool(kin)), res, rep))
    for (t, res, rep), key in zip(out, flags):
        handle.wait(t)
        want, wrep = sync_runs[key][2:4]
        assert rep.cls.tolist() == wrep.cls.tolist() and rep.pass_.tolist() == wrep.pass_.tolist()
        _valid_equal(res, want, b.n_zmw, wrep.cls, key[1])
        handle.release(t)
    assert out[0][2].cls.tolist() != out[1][2].cls.tolist()                                 # (the tickets did differ)


def test_min_passes_1_polishes_the_single_pass(lab, sync_runs):
    """the docs' "brute force" contrast: with min_passes 1 the ZMW of one full-length pass is polished, with 2 it gets that pass as it is"""
    b, kinds = lab
    singles = [z for z in range(b.n_zmw) if kinds[z] == "few" and b.read_off[z + 1] - b.read_off[z] == 1 and not b.flags[b.read_off[z]] & 2]
    assert len(singles) == 1
    z = singles[0]
    rep2, got2 = sync_runs[(0, 0)][5], sync_runs[(0, 0)][4]
    assert rep2.cls[z] == R.SUBREAD and rep2.pass_[z] == 0 and got2.status[z] == R.TOO_FEW_PASSES
    h1 = api.Handle(0, opts=_opts(min_passes=1))
    try:
        got1, rep1 = h1.consensus_represent(b)
    finally:
        h1.close()
    assert rep1.cls[z] == R.POLISHED and got1.status[z] in (R.SUCCESS, R.LOW_RQ) and got1.rq[z] >= 0
    assert got1.seq_len[z] > 0


def test_beside_a_screen_refusals_and_a_plain_run_after(handle, lab, sync_runs):
    b, kinds = lab
    n = b.n_zmw
    plain, drafts, want, wrep = sync_runs[(0, 0)][:4]
    arep = api.AdapterReport.allocate(n)
    got, rep = handle.consensus_represent(b, adapters=arep)
    assert rep.cls.tolist() == wrep.cls.tolist()
    _valid_equal(got, want, n, wrep.cls)
    with pytest.raises(RuntimeError, match="coverage gate"):
        handle.consensus_represent(b, coverage=api.CoverageReport.allocate(n), coverage_gate=4)
    with pytest.raises(ValueError):
        handle.submit(b, got, represent=rep, hd=api.HdReport.allocate(n))
    with pytest.raises(ValueError):
        handle.submit(b, got, represent=rep, barcodes=api.BarcodeReport.allocate(n), barcode_set=api.BarcodeSet.from_codes([np.zeros(8, np.uint8)]))
    h0 = api.Handle(0)                                               # a handle without opts.hifi_kinetics: the kinetics flag is refused, nothing else
    try:
        with pytest.raises(RuntimeError, match="hifi_kinetics"):
            h0.consensus_represent(b, kinetics=True)
    finally:
        h0.close()
    after, _ = _plain_and_drafts(handle, b)                          # without the request: the request-free results again
    _valid_equal(after, plain, n, np.zeros(n, np.int32))
    assert (after.seq_len[[k != "polished" for k in kinds]] == 0).all()

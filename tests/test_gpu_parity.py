"""GPU parity: HIP path (through the C ABI) vs the CPU restatement on the same seeded inputs.

Bar (BASELINE.json north_star): HiFi sequences bit-identical, per-base QVs within 1e-4.  The oracle is
"parity unpinned" (docs-only reference) — these tests pin the HIP kernels to the specification.
"""
import os

import numpy as np
import pytest

from ccs_amd import api
import oracle_lib as O

pytestmark = pytest.mark.gpu

QV_TOL = 1e-4   # north_star: per-base QVs within 1e-4 of the CPU path


@pytest.fixture(scope="module")
def handle(built):
    h = api.Handle(0)
    yield h
    h.close()


def _oracle(h, batch):
    ref = api.Results.allocate(batch)
    O.consensus_batch(h.model, h.opts, batch, ref, nthreads=8)
    return ref


def _compare(res, ref, batch):
    assert np.array_equal(res.status, ref.status)
    assert np.array_equal(res.seq_len, ref.seq_len)
    assert np.array_equal(res.np_, ref.np_)
    assert np.array_equal(res.n_windows, ref.n_windows)
    assert np.array_equal(res.iters, ref.iters)
    for z in range(batch.n_zmw):
        assert np.array_equal(res.sequence(z), ref.sequence(z)), f"zmw {z}: sequence differs"
        assert np.array_equal(res.quals(z), ref.quals(z)), f"zmw {z}: phred differs"
        assert np.allclose(res.raw(z), ref.raw(z), atol=QV_TOL, rtol=0), f"zmw {z}: raw QV differs"
    assert np.allclose(res.rq, ref.rq, atol=1e-6, rtol=0)
    assert np.allclose(res.ec, ref.ec, atol=1e-6, rtol=0)


@pytest.mark.parametrize("n,passes,length,seed", [
    (8, 3, 1000, 1),          # BASELINE config 1 shape
    (6, 10, 2000, 2),
    (4, (3, 12), (300, 1500), 3),   # ragged mix
    (3, 30, 600, 4),          # deep coverage: several LDS chunks per window
])
def test_full_path_bit_exact(handle, n, passes, length, seed):
    batch = api.synth(n, passes, length, seed=seed)
    res = handle.consensus(batch)
    ref = _oracle(handle, batch)
    _compare(res, ref, batch)


@pytest.mark.parametrize("max_qv", [93, 30, 0])
def test_max_qv_option_bit_exact(built, max_qv):
    """ABI v6: opts.max_qv floors every per-base error probability at 10^(-max_qv/10) — 50 by default (SPEC v7 "honest QVs"), 93 = the
    reference's documented range (docs/faq/qv-binning.md:31).  Kernel and restatement agree bit for bit at every setting; the cap is what it says."""
    o = api.default_opts(); o.max_qv = max_qv; o.min_rq = 0.0
    batch = api.synth(6, 10, 900, seed=77)
    h = api.Handle(0, opts=o)
    try:
        res = h.consensus(batch)
        ref = _oracle(h, batch)
        _compare(res, ref, batch)
        cap = 50 if max_qv == 0 else max_qv
        top = max(int(res.quals(z).max()) for z in range(batch.n_zmw) if res.seq_len[z])
        assert top <= cap and (top == cap or cap == 93), (top, cap)
        if max_qv == 93:
            assert top > 50                                  # the HMM itself claims more than Q50 on clean synthetic data: the default caps it, 93 shows it
    finally:
        h.close()


def test_qv_calibration_at_scale(built):
    """the predicted accuracy is checked on a sample a CPU test cannot afford — 768 on-model ZMWs of 10 x 5 kb through the HIP library (bit-identical
    to the restatement), errors against the true templates binned by phred QV.  Bounds from profiles/r06_qv_calibration.txt (1024 ZMWs: overall 0.87; bins Q0-10 0.91,
    Q10-20 0.74, Q20-30 0.69 with 1014 / 357 / 73 errors; the bins above hold 23-63 errors each and scatter 0.5-1.7: they are bounded loosely and their counts printed)."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import lowcx
    import qv_calibration as QC
    o = api.default_opts(); o.min_rq = 0.0
    b = lowcx.make(768, 10, 5000, 61)
    h = api.Handle(0, opts=o)
    try:
        r = h.consensus(b)
    finally:
        h.close()
    q, e, pe, ee = [], [], 0.0, 0
    for z in range(b.n_zmw):
        if r.status[z] not in (0, 7): continue
        d, err = QC.error_positions(r.sequence(z), b.tpl[b.tpl_off[z]:b.tpl_off[z + 1]])
        if d < 0: continue
        q.append(r.quals(z).astype(np.int32)); e.append(err.astype(np.int32))
        pe += (1.0 - float(r.rq[z])) * int(r.seq_len[z]); ee += d
    q, e = np.concatenate(q), np.concatenate(e)
    assert 0.7 <= ee / pe <= 1.1, f"overall empirical / predicted = {ee / pe:.2f} ({ee} errors, {pe:.1f} predicted)"
    assert q.max() <= 50
    for lo, hi, rlo, rhi in [(0, 10, 0.7, 1.15), (10, 20, 0.55, 1.1), (20, 30, 0.4, 1.2), (30, 40, 0.5, 2.6), (40, 51, 0.4, 2.2)]:
        sel = (q >= lo) & (q < hi)
        pred, found = float(np.sum(10.0 ** (-q[sel] / 10.0))), int(e[sel].sum())
        print(f"Q{lo}-{hi}: {int(sel.sum())} bases, predicted {pred:.1f} errors, found {found}")
        assert rlo <= found / pred <= rhi, f"Q{lo}-{hi}: empirical / predicted = {found / pred:.2f} ({found} found, {pred:.1f} predicted)"


def test_poa_vertices_with_many_in_edges(built):
    """Round 6: the POA graph lives by topological position — column records (in-edges 0..2) + overflow records (in-edges 3..6), ping-pong, both remapped when a pass
    is threaded.  Passes that all differ from each other at the same few columns (every base, inserted bases, a deletion) give the vertices behind those columns four to
    seven in-edges, the cap included: draft and consensus must equal the restatement's, at a draft coverage high enough to thread all of them."""
    rng = np.random.default_rng(5)
    L, P = 600, 14
    tpl = rng.integers(0, 4, L, dtype=np.uint8)
    hot = list(range(40, L - 40, 37))
    reads = []
    for k in range(P):
        out = []
        for j in range(L):
            if j in hot:
                v = (k + hot.index(j)) % 9
                if v < 4: out.append(v)                                  # one of the four bases
                elif v < 8: out.extend([v - 4, int(tpl[j])])            # an inserted base in front
                # v == 8: deleted
            else:
                out.append(int(tpl[j]))
        reads.append(np.array(out, np.uint8))
    n = 3
    bases = np.concatenate(reads * n)
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads] * n)]).astype(np.int64)
    batch = api.Batch(np.arange(n, dtype=np.int32), np.tile(np.array([9.0, 16.0, 8.0, 13.0], np.float32), (n, 1)), (np.arange(n + 1) * P).astype(np.int32), off, bases,
                      np.full(len(bases), 2, np.uint8), np.full(len(bases), 5, np.uint8), np.zeros(n * P, np.uint8))
    o = api.default_opts(); o.max_poa_cov = P; o.min_rq = 0.0
    h = api.Handle(0, opts=o)
    try:
        h.upload(batch); h.run(); h.sync()
        for z in range(n):
            assert np.array_equal(h.stage_draft(z), O.poa_draft(batch, z, P)), f"zmw {z}: draft differs"
        res = h.consensus(batch)
        _compare(res, _oracle(h, batch), batch)
    finally:
        h.close()


def test_stages_match_oracle(handle):
    batch = api.synth(4, 6, 900, seed=11)
    handle.upload(batch); handle.run(); handle.sync()
    for z in range(batch.n_zmw):
        d_ref = O.poa_draft(batch, z, handle.opts.max_poa_cov)
        d = handle.stage_draft(z)
        assert np.array_equal(d, d_ref), f"zmw {z}: draft differs"
        wb = handle.stage_windows(z)
        assert np.array_equal(wb, O.windows(d_ref))
        need = sorted({0, len(d)} | {int(b) - 2 for b in wb[1:-1]} | {int(b) + 2 for b in wb[1:-1]})
        r0 = int(batch.read_off[z])
        for r in range(r0, int(batch.read_off[z + 1])):
            bases, _ = batch.read(r)
            rev = (batch.flags[r] & 1) != (batch.flags[r0] & 1)
            rs_ref, v_ref, sc_ref = O.align(O.orient(bases, rev), d_ref)
            rs, v, sc = handle.stage_align(r, len(d))
            assert (v, sc) == (v_ref, sc_ref)
            if v:
                assert [int(rs[c]) for c in need] == [int(rs_ref[c]) for c in need]


def test_degenerate_inputs(handle):
    """too few passes, a garbage read, single window, empty read."""
    batch = api.synth(3, 4, 120, seed=5)
    # zmw 1: replace read 1 with random junk of the same length (must be dropped, not crash)
    r = int(batch.read_off[1]) + 1
    a, b = int(batch.base_off[r]), int(batch.base_off[r + 1])
    rng = np.random.default_rng(0)
    batch.bases[a:b] = rng.integers(0, 4, b - a, dtype=np.uint8)
    res = handle.consensus(batch)
    _compare(res, _oracle(handle, batch), batch)
    two = api.synth(2, 2, 200, seed=6)     # 2 passes < min_passes 3
    res2 = handle.consensus(two)
    assert list(res2.status) == [1, 1]
    _compare(res2, _oracle(handle, two), two)


def test_batch_split_invariance(handle):
    """results do not depend on how ZMWs are batched (the multi-GPU sharder relies on this)."""
    batch = api.synth(6, 5, 700, seed=9)
    whole = handle.consensus(batch)
    for z0, z1 in [(0, 2), (2, 6)]:
        part = handle.consensus(batch.slice(z0, z1))
        for z in range(z0, z1):
            assert np.array_equal(part.sequence(z - z0), whole.sequence(z))
            assert np.array_equal(part.raw(z - z0), whole.raw(z))
            assert part.rq[z - z0] == whole.rq[z]


def test_large_batch_takes_the_two_stream_paths(handle):
    """a batch of >= 4096 ZMWs / quads runs its POA stage as two half-batches on two streams (the second half's kernels start at a block offset) and the
    trace-back of k_align16 beside the 64-row retry: every ZMW of BOTH halves against the oracle (bench.py compares the first few thousand ZMWs of a batch,
    i.e. the first half only), and the same batch cut into pieces that stay below the threshold"""
    batch = api.synth(4608, (3, 5), (150, 420), seed=77)
    res = handle.consensus(batch)
    _compare(res, _oracle(handle, batch), batch)
    for z0, z1 in [(0, 1500), (3000, 4608)]:                 # below 4096: one stream
        part = handle.consensus(batch.slice(z0, z1))
        for z in range(z0, z1, 7):
            assert part.status[z - z0] == res.status[z] and np.array_equal(part.sequence(z - z0), res.sequence(z)) and np.array_equal(part.raw(z - z0), res.raw(z))


def test_recovers_truth_at_full_size(handle):
    """size-independent property at the BASELINE config-2 shape (10 passes x 10 kb): consensus ~= template."""
    batch = api.synth(8, 10, 10000, seed=21)
    res = handle.consensus(batch)
    assert np.isin(res.status, (0, 4)).all() and (res.status == 0).sum() >= batch.n_zmw - 1
    for z in range(batch.n_zmw):
        tpl = batch.tpl[batch.tpl_off[z]:batch.tpl_off[z + 1]]
        s = res.sequence(z)
        assert abs(len(s) - len(tpl)) <= 12
        # cheap identity proxy: 16-mers of the template present in the consensus
        def kmers(x):
            v = np.zeros(len(x) - 15, np.uint64)
            for k in range(16):
                v = v * np.uint64(4) + x[k:len(x) - 15 + k].astype(np.uint64)
            return set(v.tolist())
        kt, ks = kmers(tpl), kmers(s)
        assert len(kt & ks) / len(kt) > 0.98
        assert res.rq[z] > 0.999


@pytest.mark.parametrize("n,passes,length,seed", [
    (256, 3, 1000, 30),               # BASELINE config 1 shape: the CPU-runnable case (every ZMW ends LOW_RQ at 3 passes)
    (32, 30, 20000, 31),              # BASELINE config 4 shape: deep coverage, long template (the oracle needs ~1 core-s per ZMW here)
    (128, (3, 50), (1000, 25000), 32), # BASELINE config 5 shape: Sequel-II-like mix
])
def test_baseline_config_shapes_bit_exact(handle, n, passes, length, seed):
    import os
    batch = api.synth(n, passes, length, seed=seed)
    res = handle.consensus(batch)
    ref = api.Results.allocate(batch)
    O.consensus_batch(handle.model, handle.opts, batch, ref, nthreads=min(16, len(os.sched_getaffinity(0))))
    _compare(res, ref, batch)


def test_headline_size_matches_oracle(handle):
    """BASELINE configs[1] shape (10 passes x 10 kb) against the oracle itself, not only through properties:
    64 ZMWs bit-exact (C2-size oracle parity inside -m gpu).  The oracle runs with OpenMP over ZMWs."""
    import os
    batch = api.synth(64, 10, 10000, seed=0xC2)
    res = handle.consensus(batch)
    ref = api.Results.allocate(batch)
    O.consensus_batch(handle.model, handle.opts, batch, ref, nthreads=min(16, len(os.sched_getaffinity(0))))
    _compare(res, ref, batch)
    assert (res.status == 0).sum() >= 60


def test_top_passes_and_poa_coverage_options(built):
    o = api.default_opts(); o.top_passes = 5; o.max_poa_cov = 3
    h = api.Handle(0, opts=o)
    batch = api.synth(3, 9, 600, seed=33)
    res = h.consensus(batch)
    ref = api.Results.allocate(batch)
    O.consensus_batch(h.model, o, batch, ref)
    _compare(res, ref, batch)
    assert (res.np_ <= 5).all()
    h.close()


def test_empty_and_tiny_reads(handle):
    """a zero-length read and a ZMW of very short reads must not crash and must match the oracle"""
    batch = api.synth(2, 4, 60, seed=34)
    # make read 1 of zmw 0 empty by moving its bases to read 2
    bo = batch.base_off.copy(); bo[2] = bo[1]
    batch.base_off = bo
    res = handle.consensus(batch)
    _compare(res, _oracle(handle, batch), batch)


@pytest.mark.parametrize("kin", [0, 1])
def test_more_than_64_passes(built, kin):
    """SPEC v5 (docs/faq/accuracy-vs-passes.md:49-52: `--top-passes 0` = unlimited): up to CCSX_MAX_PASSES = 255 passes
    of a ZMW are used — k_polish and k_kinetics take them in groups of 32 (PW_MAXREADS), the draft cascade ranks all of them.  100- and 150-pass ZMWs next
    to ordinary ones, partial passes behind 70 full ones, a junk first pass (fallback backbone among > 64 passes): bit-exact against the
    oracle, np reports more than 64; a 300-pass ZMW is capped at 255"""
    o = api.default_opts(); o.top_passes = 0; o.hifi_kinetics = kin
    parts = [api.synth(1, 100, 400, seed=35), api.synth(2, 9, 700, seed=36), api.synth(1, 150, 300, seed=37), api.synth(1, 65, 500, seed=38),
             api.synth(1, 300, 200, seed=39)]
    batch = api.concat(parts)
    rng = np.random.default_rng(5)
    a, b = int(batch.base_off[0]), int(batch.base_off[1])
    batch.bases[a:b] = rng.integers(0, 4, b - a, dtype=np.uint8)        # ZMW 0: pass 0 is junk -> the fallback draft picks among 100 passes
    h = api.Handle(0, opts=o)
    try:
        res = h.consensus(batch)
        ref = api.Results.allocate(batch, kinetics=bool(kin))
        O.consensus_batch(h.model, o, batch, ref, nthreads=8)
        _compare(res, ref, batch)
        assert np.array_equal(res.np_, ref.np_) and np.array_equal(res.fn, ref.fn) and np.array_equal(res.rn, ref.rn)
        assert np.allclose(res.ec, ref.ec, atol=1e-6)
        if kin:
            for z in range(batch.n_zmw):
                assert np.array_equal(res.kinetics(z), ref.kinetics(z))
        assert res.np_[0] > 64 and res.np_[3] > 100 and res.np_[5] > 200 and res.np_[4] >= 64
    finally:
        h.close()


def test_api_misuse_is_reported_not_fatal(built):
    import ctypes as C
    L = api.lib()
    h = api.Handle(0)
    with pytest.raises(RuntimeError, match="no batch uploaded"):
        h.run()
    batch = api.synth(2, 3, 150, seed=36)
    bad = api.Batch(batch.zmw_id, batch.snr, batch.read_off.copy(), batch.base_off, batch.bases, batch.pw, batch.ipd, batch.flags)
    bad.read_off[1] = 99                                    # not monotone / inconsistent
    with pytest.raises(RuntimeError, match="read_off|n_reads"):
        h.upload(bad)
    h.upload(batch); h.run(); h.sync()
    small = api.Results.allocate(batch)
    cr = small.c_struct(); cr.seq_capacity = 10             # too small
    assert L.ccsx_download(h._h, C.byref(cr)) != 0 and b"too small" in L.ccsx_last_error()
    good = h.download()                                     # the handle stays usable
    assert (good.status >= 0).all()
    hp = C.c_void_p()
    assert L.ccsx_create(99, C.byref(h.model), C.byref(h.opts), C.byref(hp)) != 0
    h.close()


def test_fuzz_ragged_batch_bit_exact(handle):
    """200 ragged ZMWs (3-24 passes, 40-1800 bp), with corrupted reads, truncated reads, all-forward ZMWs,
    constant-base reads and flipped strand flags mixed in: every output must equal the oracle's."""
    batch = api.synth(200, (3, 24), (40, 1800), seed=4242)
    rng = np.random.default_rng(7)
    bases, flags = batch.bases, batch.flags
    for z in range(0, 200, 7):                      # junk read
        r = int(batch.read_off[z]) + int(rng.integers(0, batch.read_off[z + 1] - batch.read_off[z]))
        a, b = int(batch.base_off[r]), int(batch.base_off[r + 1])
        bases[a:b] = rng.integers(0, 4, b - a, dtype=np.uint8)
    for z in range(3, 200, 11):                     # homopolymer read
        r = int(batch.read_off[z]) + 1
        a, b = int(batch.base_off[r]), int(batch.base_off[r + 1])
        bases[a:b] = 2
    for z in range(5, 200, 13):                     # wrong strand flag on one read
        r = int(batch.read_off[z + 1]) - 1
        flags[r] ^= 1
    for z in range(1, 200, 17):                     # a block of the read replaced by junk (large insertion-like)
        r = int(batch.read_off[z]) + 2
        a, b = int(batch.base_off[r]), int(batch.base_off[r + 1])
        if b - a > 200:
            m = a + (b - a) // 2
            bases[m:m + 90] = rng.integers(0, 4, 90, dtype=np.uint8)
    res = handle.consensus(batch)
    ref = _oracle(handle, batch)
    _compare(res, ref, batch)
    assert len(set(res.status.tolist())) >= 2       # the batch exercises more than one status


def test_full_size_determinism_and_sharding(handle):
    """BASELINE config-2 shape at a bench-sized batch: two runs are byte-identical, and so is the same batch
    processed as two independent shards on two handles (what multi-GPU sharding does)."""
    import hashlib
    batch = api.synth(512, 10, 10000, seed=99)

    def digest(results, parts):
        h = hashlib.sha256()
        for res, n in zip(results, parts):
            for z in range(n):
                h.update(res.sequence(z).tobytes()); h.update(res.raw(z).tobytes()); h.update(res.rq[z].tobytes())
        return h.hexdigest()

    a = handle.consensus(batch)
    b = handle.consensus(batch)
    d1, d2 = digest([a], [512]), digest([b], [512])
    assert d1 == d2
    h2 = api.Handle(0)
    p0, p1 = batch.slice(0, 200), batch.slice(200, 512)
    handle.upload(p0); h2.upload(p1)
    handle.run(); h2.run(); handle.sync(); h2.sync()
    d3 = digest([handle.download(), h2.download()], [200, 312])
    h2.close()
    assert d3 == d1
    assert (a.status == 0).mean() > 0.99 and a.rq[a.status == 0].mean() > 0.9995


# ---- N4: HiFi kinetics (docs/faq/kinetics.md:8-18; SPEC DESIGN.md §2.9) ----------------------------------------
def _kin_handle():
    opts = api.default_opts()
    opts.hifi_kinetics = 1
    return api.Handle(0, opts=opts)


@pytest.mark.parametrize("n,passes,length,seed", [
    (6, 10, 2000, 21),
    (12, (3, 14), (150, 1500), 22),     # ragged; some ZMWs fail (too few passes) and must stay empty
    (2, 40, 500, 23),                   # deep coverage
])
def test_kinetics_bit_exact(built, n, passes, length, seed):
    batch = api.synth(n, passes, length, seed=seed)
    rng = np.random.default_rng(seed)
    batch.ipd = rng.integers(0, 256, len(batch.bases)).astype(np.uint8)          # the whole CodecV1 range
    batch.pw = np.where(rng.random(len(batch.bases)) < 0.9, batch.pw, rng.integers(0, 256, len(batch.bases))).astype(np.uint8)
    h = _kin_handle()
    try:
        res = h.consensus(batch)
        ref = api.Results.allocate(batch, kinetics=True)
        O.consensus_batch(h.model, h.opts, batch, ref, nthreads=8)
        _compare(res, ref, batch)
        assert np.array_equal(res.fn, ref.fn) and np.array_equal(res.rn, ref.rn)
        assert np.array_equal(res.fn + res.rn, res.np_)
        seen = 0
        for z in range(batch.n_zmw):
            assert np.array_equal(res.kinetics(z), ref.kinetics(z)), f"zmw {z}: kinetics differ"
            seen += int((res.kinetics(z) > 0).sum())
        assert seen > 0
    finally:
        h.close()


def test_kinetics_do_not_change_the_consensus(handle):
    batch = api.synth(5, 8, 1200, seed=41)
    plain = handle.consensus(batch)
    assert plain.kin is None and np.array_equal(plain.fn + plain.rn, plain.np_)  # pass counts come with every run
    h = _kin_handle()
    try:
        res = h.consensus(batch)
        _compare(res, plain, batch)
        # split form + base-coded kinetics: forward planes follow SEQ, reverse planes its complement
        batch.ipd = (10 + 10 * batch.bases).astype(np.uint8)
        h.upload(batch); h.run(); h.sync()
        r2 = h.download()
        for z in range(batch.n_zmw):
            s = r2.sequence(z).astype(int)
            fi, _, ri, _ = r2.kinetics(z).astype(int)
            assert (fi[fi > 0] == 10 + 10 * s[fi > 0]).all() and (ri[ri > 0] == 10 + 10 * (3 - s[ri > 0])).all()
            assert (fi > 0).mean() > 0.99 and (ri > 0).mean() > 0.99
    finally:
        h.close()


def test_kinetics_need_ipd(built):
    import ctypes as C
    batch = api.synth(2, 4, 200, seed=3)
    h = _kin_handle()
    try:
        cb = batch.c_struct()
        cb.ipd = C.POINTER(C.c_uint8)()
        assert h._L.ccsx_upload(h._h, C.byref(cb)) != 0
        assert b"ipd" in h._L.ccsx_last_error()
    finally:
        h.close()
    # and a handle without the option refuses kinetics buffers instead of leaving them unwritten
    h2 = api.Handle(0)
    try:
        h2.upload(batch); h2.run(); h2.sync()
        res = api.Results.allocate(batch, kinetics=True)
        cr = res.c_struct()
        assert h2._L.ccsx_download(h2._h, C.byref(cr)) != 0
    finally:
        h2.close()


def test_dirty_base_bytes_are_memory_safe(handle):
    """Only the low two bits of a base byte count (include/ccsx.h): garbage in the high bits must neither fault nor change
    the result; arbitrary pw bytes only select the pulse-width bin."""
    batch = api.synth(6, 7, 900, seed=91)
    clean = handle.consensus(batch)
    rng = np.random.default_rng(9)
    batch.bases = (batch.bases | (rng.integers(0, 64, len(batch.bases)) << 2)).astype(np.uint8)
    dirty = handle.consensus(batch)
    _compare(dirty, clean, batch)
    _compare(dirty, _oracle(handle, batch), batch)
    batch.pw = rng.integers(0, 256, len(batch.bases)).astype(np.uint8)
    _compare(handle.consensus(batch), _oracle(handle, batch), batch)


def test_hostile_metadata(built):
    """NaN / inf / negative / zero SNR, a ZMW without reads and a ZMW whose reads are all empty: same statuses and bytes as
    the oracle, nothing faults (one status per ZMW, the run continues: docs/faq/reports-aux-files.md:10-12)."""
    b = api.synth(8, 6, 400, seed=3)
    b.snr[1] = np.nan; b.snr[2] = np.inf; b.snr[3] = -5.0; b.snr[4] = 0.0
    ro, bo = b.read_off, b.base_off
    bases, pw, ipd, flags, nbo, nro = [], [], [], [], [0], [0]
    for z in range(8):
        for r in range(ro[z], ro[z + 1]):
            if z == 5:
                continue                                     # ZMW 5: no reads at all
            a, e = int(bo[r]), int(bo[r + 1])
            if z == 6:
                e = a                                        # ZMW 6: six empty reads
            bases.append(b.bases[a:e]); pw.append(b.pw[a:e]); ipd.append(b.ipd[a:e]); flags.append(b.flags[r]); nbo.append(nbo[-1] + e - a)
        nro.append(len(flags))
    nb = api.Batch(b.zmw_id.copy(), b.snr.copy(), np.array(nro, np.int32), np.array(nbo, np.int64), np.concatenate(bases).astype(np.uint8),
                   np.concatenate(pw).astype(np.uint8), np.concatenate(ipd).astype(np.uint8), np.array(flags, np.uint8))
    for kin in (0, 1):
        o = api.default_opts(); o.hifi_kinetics = kin; o.min_passes = 1
        h = api.Handle(0, opts=o)
        try:
            res = h.consensus(nb)
            ref = api.Results.allocate(nb, kinetics=bool(kin))
            O.consensus_batch(h.model, o, nb, ref, nthreads=4)
            assert res.status.tolist() == ref.status.tolist() == [0, 7, 0, 0, 0, 1, 2, 0]
            assert np.array_equal(res.seq_len, ref.seq_len)
            for z in range(8):
                assert np.array_equal(res.sequence(z), ref.sequence(z)) and np.array_equal(res.quals(z), ref.quals(z))
                if kin:
                    assert np.array_equal(res.kinetics(z), ref.kinetics(z))
            assert np.array_equal(np.nan_to_num(res.rq, nan=-1), np.nan_to_num(ref.rq, nan=-1))
        finally:
            h.close()


def test_pinned_batch_gives_identical_results(handle):
    batch = api.synth(5, 6, 800, seed=61)
    a = handle.consensus(batch)
    pb = batch.pinned()
    assert np.array_equal(pb.bases, batch.bases) and np.array_equal(pb.pw, batch.pw) and np.array_equal(pb.ipd, batch.ipd)
    b = handle.consensus(pb)
    _compare(b, a, batch)


def test_async_pipeline_matches_synchronous(built):
    """ccsx_submit / ccsx_wait (three batches in flight, copies under compute) give the results of the synchronous call,
    for batches of different shapes sharing the handle's slots and scratch"""
    shapes = [(6, 5, 700), (3, 9, 1500), (8, 4, 300), (2, 12, 2500), (5, 6, 900), (4, 3, 400), (6, 8, 1100)]
    batches = [api.synth(n, p, l, seed=60 + i) for i, (n, p, l) in enumerate(shapes)]
    hs = api.Handle(0)
    want = [hs.consensus(b) for b in batches]
    hs.close()
    h = api.Handle(0)
    pinned = [b.pinned() for b in batches]
    res = [api.Results.allocate(b, pinned=True) for b in batches]
    tickets, depth = [], 3
    for k in range(len(batches) + depth):
        if k >= depth:
            r = h.wait(tickets[k - depth])
            w = want[k - depth]
            assert np.array_equal(r.status, w.status) and np.array_equal(r.seq_len, w.seq_len) and np.array_equal(r.np_, w.np_)
            assert np.array_equal(r.seq_off, w.seq_off)
            for z in range(batches[k - depth].n_zmw):
                assert np.array_equal(r.sequence(z), w.sequence(z)) and np.array_equal(r.raw(z), w.raw(z))
            assert np.array_equal(r.rq, w.rq)
            t = h.ticket_timings(tickets[k - depth])
            assert t.total_ms > 0 and t.polish_workgroups == int(w.n_windows.sum())
            h.release(tickets[k - depth])
        if k < len(batches):
            tickets.append(h.submit(pinned[k], res[k]))
            assert h.poll(tickets[-1]) in (True, False)
    # a recycled ticket is reported, not undefined behaviour
    with pytest.raises(RuntimeError):
        h.wait(tickets[0])
    h.close()


def test_async_submit_rejects_small_result_buffers(built):
    h = api.Handle(0)
    big, small = api.synth(4, 5, 800, seed=70), api.synth(2, 3, 200, seed=71)
    res_small = api.Results.allocate(small)
    with pytest.raises(RuntimeError):
        h.submit(big, res_small)
    # the handle stays usable
    r = h.wait(h.submit(small, res_small))
    assert (r.status >= 0).all()
    h.close()


def test_bench_two_ranks_on_one_device(built, tmp_path):
    """the N>1 code path of bench.py (one process per rank, barrier + max-over-ranks timing, ZMW shards
    with distinct ids, no data-path collective) executes the HIP kernels before an 8-GPU node ever sees it: two ranks share
    GPU 0 through the CCSX_BENCH_DEVICE hook, the timing collectives run over gloo."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    from conftest import free_port
    env = dict(os.environ, CCSX_BENCH_DEVICE="0", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(free_port()),
           os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--zmws", "48", "--length", "2000", "--backend", "gloo",
           "--distinct", "2", "--no-cpu-baseline"]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=root)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1                                  # rank 0 only
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["scaling"] == "weak" and out["steps"] == 3
    assert out["value"] > 0 and out["success_frac"] > 0.9
    assert abs(out["value"] - 2 * 48 * 3 / (out["ms_per_step"] * 3e-3)) / out["value"] < 1e-3      # whole-job aggregate over both ranks
    # round 6: under a launcher every rank binds itself to its device's NUMA node before it allocates anything (rank 0's placement is in the line)
    node = api.lib().ccsx_device_numa_node(0)
    assert out["rank0_numa"]["numa_node"] == node and out["rank0_numa"]["thread_bound_to_node"] in (node, -1)


def test_bench_gpus_n_runs_n_workers_in_one_process(built):
    """plain `python bench.py --gpus 2` must MEAN two GPUs without a launcher and without RCCL — one process, one worker thread and one
    engine handle per device (here both on GPU 0 through CCSX_BENCH_DEVICES); per-GPU entries, aggregate = all ZMWs / the slowest worker's time"""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["CCSX_BENCH_DEVICES"] = "0,0"
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--zmws", "48", "--length", "2000", "--distinct", "2",
           "--no-cpu-baseline", "--extra", "", "--full"]        # --full: the per-worker H2D rates
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=root)
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][0])
    assert out["n_gpus"] == 2 and len(out["per_gpu"]) == 2 and [g["device"] for g in out["per_gpu"]] == [0, 0]
    slowest = max(g["ms_per_step"] for g in out["per_gpu"])
    assert abs(out["ms_per_step"] - slowest) < 1e-6 and abs(out["value"] - 2 * 48 * 3 / (slowest * 3e-3)) / out["value"] < 1e-3
    assert out["success_frac"] > 0.9 and all(g["success_frac"] > 0.9 for g in out["per_gpu"])
    # every worker reports its device's NUMA node, where its thread was bound (that node, or -1 when the platform names none / binding is off),
    # the H2D rate it gets while its neighbour uploads too, and how much of its run the kernels covered; both workers of GPU 0 sit on GPU 0's node
    node = api.lib().ccsx_device_numa_node(0)
    for g in out["per_gpu"]:
        assert g["numa_node"] == node and g["thread_bound_to_node"] in (node, -1)
        assert g["h2d_GBps"] > 0.1 and 0.0 < g["copies_hidden_frac"] <= 1.0
    if node >= 0 and os.environ.get("CCSX_NUMA", "1") != "0":
        assert all(g["thread_bound_to_node"] == node for g in out["per_gpu"])
    assert out["config"]["runtime_switches"] == "" and "two compute streams" in out["config"]["stages"]
    # the stage label says what the library DID: an override from the environment is named and changes it
    ps = subprocess.run(cmd, env={**env, "CCSX_SERIAL_STAGES": "1"}, capture_output=True, text=True, timeout=600, cwd=root)
    assert ps.returncode == 0, ps.stderr[-2000:]
    os_ = json.loads([l for l in ps.stdout.splitlines() if l.startswith("{")][0])
    assert os_["config"]["runtime_switches"] == "CCSX_SERIAL_STAGES=1" and os_["config"]["stages"].startswith("serial")
    # N = 1 keeps its line: no per-GPU block
    p1 = subprocess.run([a for a in cmd if a not in ("2",)][:2] + ["--gpus", "1"] + cmd[4:], env={k: v for k, v in env.items() if k != "CCSX_BENCH_DEVICES"},
                        capture_output=True, text=True, timeout=600, cwd=root)
    assert p1.returncode == 0, p1.stderr[-2000:]
    o1 = json.loads([l for l in p1.stdout.splitlines() if l.startswith("{")][0])
    assert o1["n_gpus"] == 1 and "per_gpu" not in o1


def test_bench_plain_run_dumps_its_last_step(built, tmp_path):
    """a plain `bench.py` run times exactly --steps steps and measures nothing its headline does not need (no CPU baseline, reference probe, other
    shapes or clocks: those are --full); --dump-outputs writes what the last timed step computed as float arrays, and that is the oracle's consensus
    of the same batch"""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "CCSX_BENCH_DEVICES")}
    d = tmp_path / "out"
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--zmws", "48", "--length", "2000", "--distinct", "2",
           "--dump-outputs", str(d)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=root)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["full"] is False and out["value"] > 0 and out["ms_per_step"] > 0
    assert abs(out["value"] - 48 * 3 / (out["ms_per_step"] * 3e-3)) / out["value"] < 1e-3
    for k in ("cpu_baseline", "extra", "reference_ccs", "gpu_clocks"):
        assert k not in out, k
    files = {f[:-4]: np.load(d / f) for f in os.listdir(d)}
    assert all(f.endswith(".npy") for f in os.listdir(d)) and sum(os.path.getsize(d / f) for f in os.listdir(d)) <= 64_000_000
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    # steps 0, 1, 2 cycle through 2 distinct batches: the last step ran batch 0 again (ZMW ids 0..47)
    batch = api.synth(48, 10, 2000, seed=0xC0FFEE, first_zmw_id=0)
    assert np.array_equal(files["zmw_id"], batch.zmw_id)
    ref = api.Results.allocate(batch)
    O.consensus_batch(api.default_model(), api.default_opts(), batch, ref, nthreads=8)
    assert np.array_equal(files["status"], ref.status) and np.array_equal(files["seq_len"], ref.seq_len) and np.array_equal(files["np"], ref.np_)
    assert np.allclose(files["rq"], ref.rq, atol=1e-6, rtol=0) and len(files["sample_zmw"]) == 48
    off = files["sample_seq_off"].astype(np.int64)
    for i, z in enumerate(files["sample_zmw"].astype(np.int64)):
        assert np.array_equal(files["seq"][off[i]:off[i + 1]], ref.sequence(z)) and np.array_equal(files["qual"][off[i]:off[i + 1]], ref.quals(z))


def test_inserted_blocks_fuzz_matches_oracle(handle):
    """passes carrying 40-200 base blocks of foreign sequence (beyond what the 64-row band can follow) must end
    in the same deliberate outcome on the GPU as in the oracle — same statuses, np, sequences, QVs — never a crash or a hang"""
    rng = np.random.default_rng(12)
    base = api.synth(12, (4, 12), (600, 2500), seed=91)
    bases, pw, ipd, off = [], [], [], [0]
    for r in range(int(base.read_off[-1])):
        a, b = int(base.base_off[r]), int(base.base_off[r + 1])
        bb, pp, ii = base.bases[a:b], base.pw[a:b], base.ipd[a:b]
        if rng.random() < 0.35:
            at, size = int(rng.integers(0, len(bb) + 1)), int(rng.integers(40, 201))
            blk = rng.integers(0, 4, size, dtype=np.uint8)
            bb = np.concatenate([bb[:at], blk, bb[at:]]); pp = np.concatenate([pp[:at], np.full(size, 2, np.uint8), pp[at:]])
            ii = np.concatenate([ii[:at], np.full(size, 5, np.uint8), ii[at:]])
        bases.append(bb); pw.append(pp); ipd.append(ii); off.append(off[-1] + len(bb))
    batch = api.Batch(base.zmw_id, base.snr, base.read_off, np.array(off, np.int64), np.concatenate(bases), np.concatenate(pw),
                      np.concatenate(ipd), base.flags, base.tpl_off, base.tpl)
    res = handle.consensus(batch)
    ref = _oracle(handle, batch)
    _compare(res, ref, batch)
    assert set(int(s) for s in res.status) <= {0, 2, 3, 4, 7}           # SUCCESS, DRAFT_FAILURE, TOO_MANY_UNUSABLE, NON_CONVERGENT, LOW_RQ
    assert (res.status == 0).sum() >= 4


def test_fallback_draft_matches_oracle(built):
    """the second draft attempt (median-length backbone, twice the passes, orientation of the new backbone) on the GPU: ZMWs whose
    pass 0 is junk, next to ZMWs that need no fallback, with and without opts.no_fallback_draft, and with kinetics"""
    rng = np.random.default_rng(21)
    batch = api.synth(12, (5, 9), (500, 1600), seed=97)
    for z in (1, 3, 4, 6, 7, 9, 10):
        r = int(batch.read_off[z])
        a, b = int(batch.base_off[r]), int(batch.base_off[r + 1])
        batch.bases[a:b] = rng.integers(0, 4, b - a, dtype=np.uint8)
    seen_rescue = False
    for nofb, kin in ((0, 0), (1, 0), (0, 1)):
        o = api.default_opts(); o.no_fallback_draft = nofb; o.hifi_kinetics = kin
        h = api.Handle(0, opts=o)
        res = h.consensus(batch)
        ref = api.Results.allocate(batch, kinetics=bool(kin))
        O.consensus_batch(h.model, o, batch, ref, nthreads=4)
        _compare(res, ref, batch)
        assert np.array_equal(res.fn, ref.fn) and np.array_equal(res.rn, ref.rn)
        if kin:
            for z in range(batch.n_zmw):
                assert np.array_equal(res.kinetics(z), ref.kinetics(z))
        if nofb:
            lost = set(np.nonzero(res.status == 3)[0].tolist())
        else:
            ok = set(np.nonzero((res.status == 0) | (res.status == 7))[0].tolist())
        h.close()
    assert len(lost) >= 2 and lost <= ok                      # what is lost without the fallback gets a consensus with it (HiFi or LOW_RQ)


@pytest.mark.gpu
def test_split_alignment_keeps_passes_with_large_blocks(handle):
    """SPEC "split alignment" on the GPU (k_rescue): passes with a 60 / 150 / 400 base foreign block fail the banded alignment, are
    split into prefix + insertion + suffix, keep serving every window (the block is trimmed in its window) — np counts them, the
    consensus equals the one without blocks, and everything matches the oracle bit for bit"""
    rng = np.random.default_rng(17)
    base = api.synth(5, 8, 2500, seed=95)
    bases, pw, ipd, off = [], [], [], [0]
    sizes = {(1, 2): 60, (1, 5): 150, (3, 0): 400, (3, 7): 60}
    for r in range(int(base.read_off[-1])):
        a, b = int(base.base_off[r]), int(base.base_off[r + 1])
        bb, pp, ii = base.bases[a:b], base.pw[a:b], base.ipd[a:b]
        z = int(np.searchsorted(base.read_off, r, side="right") - 1)
        size = sizes.get((z, r - int(base.read_off[z])))
        if size:
            at = int(rng.integers(300, len(bb) - 300))
            blk = rng.integers(0, 4, size, dtype=np.uint8)
            bb = np.concatenate([bb[:at], blk, bb[at:]]); pp = np.concatenate([pp[:at], np.full(size, 2, np.uint8), pp[at:]])
            ii = np.concatenate([ii[:at], np.full(size, 5, np.uint8), ii[at:]])
        bases.append(bb); pw.append(pp); ipd.append(ii); off.append(off[-1] + len(bb))
    batch = api.Batch(base.zmw_id, base.snr, base.read_off, np.array(off, np.int64), np.concatenate(bases), np.concatenate(pw),
                      np.concatenate(ipd), base.flags, base.tpl_off, base.tpl)
    res = handle.consensus(batch)
    _compare(res, _oracle(handle, batch), batch)
    clean = handle.consensus(base)
    assert (res.status == 0).all() and (res.np_ == 8).all()           # no pass is lost (pass 0 of ZMW 3 is even the POA backbone)
    for z in (0, 2, 4):
        assert np.array_equal(res.sequence(z), clean.sequence(z))
    for z in (1, 3):
        assert abs(int(res.seq_len[z]) - int(clean.seq_len[z])) <= 2 and res.ec[z] > 7.5


@pytest.mark.parametrize("maxins,kin", [(10, 0), (6, 1), (-1, 0)])
def test_large_insertion_trimming_matches_oracle(built, maxins, kin):
    """SPEC "trim large insertions" (docs/how-does-ccs-work.md:74-78, opts.max_insertion_size): passes with 8-30 base blocks of
    foreign sequence, trimmed in their window at thresholds 10 / 6 (with kinetics: those always see the untrimmed segment) and never:
    the GPU must reproduce the oracle bit for bit, and trimming must keep more passes per window than not trimming"""
    rng = np.random.default_rng(14)
    base = api.synth(10, (6, 12), (700, 2200), seed=93)
    bases, pw, ipd, off = [], [], [], [0]
    for r in range(int(base.read_off[-1])):
        a, b = int(base.base_off[r]), int(base.base_off[r + 1])
        bb, pp, ii = base.bases[a:b], base.pw[a:b], base.ipd[a:b]
        for _ in range(int(rng.integers(0, 3))):
            at, size = int(rng.integers(0, len(bb) + 1)), int(rng.integers(8, 31))
            blk = rng.integers(0, 4, size, dtype=np.uint8)
            bb = np.concatenate([bb[:at], blk, bb[at:]]); pp = np.concatenate([pp[:at], np.full(size, 2, np.uint8), pp[at:]])
            ii = np.concatenate([ii[:at], np.full(size, 5, np.uint8), ii[at:]])
        bases.append(bb); pw.append(pp); ipd.append(ii); off.append(off[-1] + len(bb))
    batch = api.Batch(base.zmw_id, base.snr, base.read_off, np.array(off, np.int64), np.concatenate(bases), np.concatenate(pw),
                      np.concatenate(ipd), base.flags, base.tpl_off, base.tpl)
    o = api.default_opts(); o.max_insertion_size = maxins; o.hifi_kinetics = kin
    h = api.Handle(0, opts=o)
    res = h.consensus(batch)
    ref = api.Results.allocate(batch)
    O.consensus_batch(h.model, o, batch, ref)
    h.close()
    _compare(res, ref, batch)
    if maxins > 0 and not kin:
        o2 = api.default_opts(); o2.max_insertion_size = -1
        h2 = api.Handle(0, opts=o2)
        off_ = h2.consensus(batch)
        h2.close()
        ok = (res.status == 0) & (off_.status == 0)
        assert ok.sum() >= 5 and res.ec[ok].sum() > off_.ec[ok].sum()


@pytest.mark.parametrize("passes,length,n,seed,disable", [(5, (800, 3000), 24, 301, 0), (10, (1500, 6000), 16, 302, 0), (30, (1000, 4000), 8, 303, 0),
                                                            (10, (1500, 5000), 12, 304, 1)])
def test_low_complexity_templates_bit_exact(built, passes, length, n, seed, disable):
    """VERDICT r02 item 3b / docs/faq/low-complexity.md:11-18: templates made of homopolymer runs (5-60) and 2-4-mer tandem repeats
    (20-500 bp) next to random stretches (tools/lowcx.py, a generator independent of the library's) — where the rarely taken
    kernel branches live (JMAX / JMIN caps, cycle guard, NON_CONVERGENT, band placement ties in repeats): HIP == oracle bit for
    bit at 5 / 10 / 30 passes, with the candidate filter and with --disable-heuristics"""
    import lowcx
    batch = lowcx.make(n, passes, length, seed, tpl="lowcx")
    o = api.default_opts(); o.disable_heuristics = disable
    h = api.Handle(0, opts=o)
    try:
        res = h.consensus(batch)
        ref = api.Results.allocate(batch)
        O.consensus_batch(h.model, o, batch, ref, nthreads=8)
        _compare(res, ref, batch)
        assert np.array_equal(res.np_, ref.np_) and np.array_equal(res.iters, ref.iters)
        assert ((res.status == 0) | (res.status == 7) | (res.status == 4)).sum() >= n // 2
    finally:
        h.close()


@pytest.mark.parametrize("disable", [0, 1])
def test_low_complexity_yield_and_accuracy(built, disable):
    """VERDICT r03 item 1 / docs/faq/low-complexity.md:11-18 — not only HIP == oracle but YIELD and ACCURACY on low-complexity templates:
    the data set of profiles/r03_spec_studies.txt (tpl=lowcx, 48 ZMWs, 10 x 5 kb) lost 15 of 48 ZMWs to NON_CONVERGENT under SPEC v4's
    16-row first alignment band; with SPEC v5's band-saturation retry at least 46 succeed (48 with --disable-heuristics, which aligns with
    64 rows at once), the consensus is no worse than the 64-row-only result (8608 ppm) and nearly every pass took the 64-row retry"""
    import lowcx
    batch = lowcx.make(48, 10, 5000, 50, tpl="lowcx")
    o = api.default_opts(); o.disable_heuristics = disable
    h = api.Handle(0, opts=o)
    try:
        res = h.consensus(batch)
        ok = np.nonzero(res.status == 0)[0]
        assert len(ok) >= (48 if disable else 46), np.unique(res.status, return_counts=True)
        err = sum(O.edit_distance(res.sequence(z), batch.tpl[batch.tpl_off[z]:batch.tpl_off[z + 1]]) for z in ok)
        nb = int(sum(batch.tpl_off[z + 1] - batch.tpl_off[z] for z in ok))
        assert 1e6 * err / nb <= 9000.0, (err, nb)
        assert np.array_equal(res.np_[ok], np.full(len(ok), 10))          # every pass is used: none lost to a wrong repeat phase
    finally:
        h.close()


@pytest.mark.parametrize("channel,hp_boost,seed", [(1.5, 1.0, 311), (1.0, 2.5, 312), (0.5, 1.0, 313)])
def test_off_model_error_channels_bit_exact(built, channel, hp_boost, seed):
    """reads from an error channel the parameter set was NOT matched to (rates x1.5 / x0.5, indels boosted
    2.5x inside homopolymers) — more gate failures, 64-row retries, z-score drops and polish rounds than on-model data"""
    import lowcx
    batch = lowcx.make(16, (6, 12), (1500, 5000), seed, channel=channel, hp_boost=hp_boost)
    h = api.Handle(0)
    try:
        res = h.consensus(batch)
        ref = _oracle(h, batch)
        _compare(res, ref, batch)
    finally:
        h.close()


def test_last_resort_draft_matches_oracle(built):
    """SPEC "draft cascade", third generator (pass 2: a pass is the draft itself): ZMWs whose pass 0 AND median-length pass are junk,
    next to ZMWs that need no retry, with and without kinetics; bit-exact incl. np / fn / rn and the orientation of the new backbone"""
    import test_oracle_draft as T
    batch = T._junk_backbones_batch()
    for kin in (0, 1):
        o = api.default_opts(); o.hifi_kinetics = kin
        h = api.Handle(0, opts=o)
        try:
            res = h.consensus(batch)
            ref = api.Results.allocate(batch, kinetics=bool(kin))
            O.counts_reset()
            O.consensus_batch(h.model, o, batch, ref, nthreads=4)
            assert O.counts()["third_draft"] >= 2
            _compare(res, ref, batch)
            assert np.array_equal(res.fn, ref.fn) and np.array_equal(res.rn, ref.rn) and np.array_equal(res.np_, ref.np_)
            assert ((res.status == 0) | (res.status == 7)).all()
            if kin:
                for z in range(batch.n_zmw):
                    assert np.array_equal(res.kinetics(z), ref.kinetics(z))
        finally:
            h.close()


@pytest.mark.parametrize("kin", [0, 1])
def test_partial_passes_match_oracle(built, kin):
    """SPEC "partial passes" (docs/faq/accuracy-vs-passes.md:26-29) on the GPU: k_rescue's anchored alignment of the passes that carry
    flag bit 1 (start- and end-anchored, both strands), np counts full-length passes, ec the partial ones too; with fallback-draft
    ZMWs (a junk pass 0 changes the draft's orientation, so the anchor side of the partial passes flips) and with kinetics"""
    import test_oracle_draft as T
    batch = T.partial_pass_batch(n=10, seed=56, nfull=6, length=(900, 3000))
    rng = np.random.default_rng(3)
    for z in (2, 7):                                         # junk pass 0 -> fallback draft with another backbone / orientation
        r = int(batch.read_off[z]); a, b = int(batch.base_off[r]), int(batch.base_off[r + 1])
        batch.bases[a:b] = rng.integers(0, 4, b - a, dtype=np.uint8)
    o = api.default_opts(); o.hifi_kinetics = kin
    h = api.Handle(0, opts=o)
    try:
        res = h.consensus(batch)
        ref = api.Results.allocate(batch, kinetics=bool(kin))
        O.counts_reset()
        O.consensus_batch(h.model, o, batch, ref, nthreads=4)
        assert O.counts()["partial_used"] >= 16
        _compare(res, ref, batch)
        assert np.array_equal(res.np_, ref.np_) and np.array_equal(res.fn, ref.fn) and np.array_equal(res.rn, ref.rn)
        assert np.allclose(res.ec, ref.ec, atol=1e-6)
        ok = (res.status == 0) | (res.status == 7)
        assert ok.sum() >= 8 and (res.ec[ok] > res.np_[ok] + 0.5).all()
        if kin:
            for z in range(batch.n_zmw):
                assert np.array_equal(res.kinetics(z), ref.kinetics(z))
    finally:
        h.close()
    bad = T.partial_pass_batch(n=2, seed=57)
    bad.flags[int(bad.read_off[1]) - 1] &= 1                 # a full-length pass after a partial one: refused, not misread
    h = api.Handle(0)
    try:
        with pytest.raises(RuntimeError, match="follows a partial pass"):
            h.consensus(bad)
    finally:
        h.close()


def test_scratch_grows_while_tickets_are_in_flight(built):
    """the shared POA / alignment scratch is re-allocated when a later batch needs more (longer reads, more ZMWs)
    while earlier tickets are still in flight on the other slots — every batch must still equal its synchronous result"""
    small = api.synth(64, 5, 600, seed=401)
    big = api.synth(96, 8, 6000, seed=402)                   # ~10x the vertex capacity per graph and more graphs
    mid = api.synth(80, 6, 2500, seed=403)
    seq = [small, big, small, mid, big, small]
    h = api.Handle(0)
    try:
        want = {id(b): h.consensus(b) for b in (small, mid)}      # synchronous references first, on a handle whose scratch is still small
    finally:
        h.close()
    h2 = api.Handle(0)
    try:
        want[id(big)] = h2.consensus(big)
    finally:
        h2.close()
    h = api.Handle(0)                                        # fresh handle: its scratch starts at the size of `small`
    try:
        res = [api.Results.allocate(b, pinned=True) for b in seq]
        ticks = [None] * len(seq)
        for k, b in enumerate(seq):
            if k >= 3:
                h.wait(ticks[k - 3])
            ticks[k] = h.submit(b.pinned(), res[k])
        for k in range(len(seq) - 3, len(seq)):
            h.wait(ticks[k])
        for k, b in enumerate(seq):
            w = want[id(b)]
            assert np.array_equal(res[k].status, w.status) and np.array_equal(res[k].seq_len, w.seq_len), k
            for z in range(b.n_zmw):
                assert np.array_equal(res[k].sequence(z), w.sequence(z)) and np.array_equal(res[k].quals(z), w.quals(z)), (k, z)
    finally:
        h.close()


def test_partial_passes_are_realigned_after_a_redraft(built):
    """found by tools/corruption_fuzz.py in round 3: a partial pass that was valid against the FIRST draft kept its entry rows when the
    fallback draft replaced that draft (k_rescue only looks at passes that are not valid).  Pass 0 and the two partial passes come
    from molecule B, the six other passes from molecule A: the first draft is B (most passes do not map -> fallback), the partial
    passes map to it; against the fallback draft (A) they must be aligned again and drop out."""
    A = api.synth(3, 7, 1500, seed=611)
    B = api.synth(3, 7, 1500, seed=612)
    bases, pw, ipd, off, flags = [], [], [], [0], []
    read_off = [0]
    for z in range(3):
        src = [(B, 0, None)] + [(A, q, None) for q in range(1, 7)] + [(B, 2, "head"), (B, 3, "tail")]
        for S, q, cut in src:
            r = int(S.read_off[z]) + q
            a, b = int(S.base_off[r]), int(S.base_off[r + 1])
            fl = int(S.flags[r])
            if cut == "head": b = a + (6 * (b - a)) // 10; fl |= 2
            if cut == "tail": a = b - (b - a) // 2; fl |= 2 | 4
            bases.append(S.bases[a:b]); pw.append(S.pw[a:b]); ipd.append(S.ipd[a:b]); off.append(off[-1] + (b - a)); flags.append(fl)
        read_off.append(len(flags))
    batch = api.Batch(A.zmw_id, A.snr, np.array(read_off, np.int32), np.array(off, np.int64), np.concatenate(bases), np.concatenate(pw),
                      np.concatenate(ipd), np.array(flags, np.uint8), A.tpl_off, A.tpl)
    for kin in (0, 1):
        o = api.default_opts(); o.hifi_kinetics = kin
        h = api.Handle(0, opts=o)
        try:
            res = h.consensus(batch)
            ref = api.Results.allocate(batch, kinetics=bool(kin))
            O.counts_reset()
            O.consensus_batch(h.model, o, batch, ref, nthreads=4)
            assert O.counts()["fallback"] == 3
            _compare(res, ref, batch)
            assert np.allclose(res.ec, ref.ec, atol=1e-6) and np.array_equal(res.np_, ref.np_)
            assert (res.np_ == 6).all() and (res.ec < 6.01).all()     # the B passes serve no window of the A consensus
        finally:
            h.close()


def test_corruption_fuzz_sample(built):
    """A fixed sample of tools/corruption_fuzz.py inside the suite (the 900-batch runs are in profiles/): passes damaged the way real
    subreads are — foreign blocks, missing stretches, junk, truncation, partial passes, low-complexity / off-model templates — under
    random option sets; every field bit-exact against the oracle.  Seeds 9000.. include the batch that exposed the stale partial-pass
    alignment of round 3."""
    import corruption_fuzz as F
    seen_status = np.zeros(16, np.int64)
    for k in range(28):
        batch, o, n, lmax, ncorr, npass = F.make_batch(k, 9000)
        h = api.Handle(0, opts=o)
        try:
            res = h.consensus(batch)
            ref = api.Results.allocate(batch, kinetics=bool(o.hifi_kinetics))
            O.consensus_batch(h.model, o, batch, ref, nthreads=8)
            for f in ("status", "seq_len", "np_", "iters", "fn", "rn", "rq", "ec"):
                assert np.array_equal(getattr(res, f), getattr(ref, f)), f"batch {k}: {f} differs"
            for z in range(n):
                assert np.array_equal(res.sequence(z), ref.sequence(z)) and np.array_equal(res.quals(z), ref.quals(z)) and np.array_equal(res.raw(z), ref.raw(z)), f"batch {k} zmw {z}"
                if o.hifi_kinetics: assert np.array_equal(res.kinetics(z), ref.kinetics(z)), f"batch {k} zmw {z}: kinetics"
            seen_status += np.bincount(res.status, minlength=16)[:16]
        finally:
            h.close()
    assert seen_status[0] > 100 and (seen_status[1:] > 0).sum() >= 3       # successes and at least three kinds of failure were compared


def test_double_split_matches_oracle(handle):
    """SPEC "double split" (v4) on the GPU (k_rescue): passes with three foreign blocks serve the windows before the first and after the
    last block, ec shows the gap (two blocks: the ordinary split and the band's recovery); bit-exact against the oracle, with and
    without kinetics (which see the same windows)"""
    from test_oracle_filter import _two_block_batch
    for sizes, fr, want in (((250, 250, 250), (0.2, 0.5, 0.8), "split2"), ((300, 200, 400), (0.15, 0.45, 0.75), "split2"), ((90, 140), (0.3, 0.7), "split")):
        base, batch = _two_block_batch(sizes=sizes, fr=fr)
        O.counts_reset()
        ref = _oracle(handle, batch)
        assert O.counts()[want] == 2
        res = handle.consensus(batch)
        _compare(res, ref, batch)
        assert res.status[1] == 0 and res.np_[1] >= 6 and 6.2 < res.ec[1] < 7.8
    o = api.default_opts(); o.hifi_kinetics = 1
    hk = api.Handle(0, opts=o)
    try:
        base, batch = _two_block_batch(sizes=(250, 250, 250), fr=(0.2, 0.5, 0.8))
        batch.ipd = np.random.default_rng(5).integers(0, 256, len(batch.bases)).astype(np.uint8)
        res = hk.consensus(batch)
        ref = api.Results.allocate(batch, kinetics=True)
        O.consensus_batch(hk.model, o, batch, ref, nthreads=4)
        _compare(res, ref, batch)
        for z in range(batch.n_zmw):
            assert np.array_equal(res.kinetics(z), ref.kinetics(z))
    finally:
        hk.close()


def test_reference_concordance_harness(built, tmp_path, monkeypatch):
    """bench.py's `reference_concordance` — the only code that can ever pin parity against a real `ccs` — must work on
    the day a box has one.  A stand-in reference (this repo's driver copied to another directory, so that its realpath differs from the
    product's) goes on PATH: the harness writes the synthetic subreads, times the stand-in, runs the product and compares the HiFi reads.
    A reference that fails (unknown chemistry triple, no --version) is reported in the result, it never raises."""
    import shutil, stat, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench
    bindir = tmp_path / "refbin"
    bindir.mkdir()
    shutil.copy(os.path.join(root, "ccs_amd", "bin", "ccs"), bindir / "ccs")
    monkeypatch.setenv("LD_LIBRARY_PATH", os.path.join(root, "ccs_amd") + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))   # (the copy's $ORIGIN/.. rpath is gone)
    monkeypatch.setenv("PATH", str(bindir) + os.pathsep + os.environ["PATH"])
    ref = shutil.which("ccs")
    assert ref and os.path.realpath(ref) != os.path.realpath(os.path.join(root, "ccs_amd", "bin", "ccs"))
    sample = api.synth(24, 6, 1500, seed=0xC0FFEE)
    out = bench.reference_concordance(api, np, ref, sample, 4, 5.0)
    assert out.get("error") is None and out["rc"] == 0, out
    assert out["zmws_in_both"] > 0 and out["identical_sequences"] == out["zmws_in_both"] == out["hifi_reads_ours"], out
    assert out["zmws_per_s"] > 0 and "spec" in out["version"]
    # a reference that rejects the input (here: a script that complains about the chemistry and exits 1, and knows no --version)
    bad = tmp_path / "badbin"
    bad.mkdir()
    (bad / "ccs").write_text("#!/bin/sh\necho 'Unsupported chemistries found: (101-789-500/101-826-100/5.0)' >&2\nexit 1\n")
    os.chmod(bad / "ccs", os.stat(bad / "ccs").st_mode | stat.S_IEXEC)
    out = bench.reference_concordance(api, np, str(bad / "ccs"), sample, 4, 5.0)
    assert out["rc"] == 1 and "chemistry" in out["error"] and "zmws_per_s" not in out and "rc 1" in out["version"]


def test_polish_grid_is_launched_in_pieces(built, tmp_path):
    """a grid may not exceed 2^32 threads: k_polish / k_kinetics run one 256-thread workgroup per window slot, so a batch of more than 16.7 M
    slots (16 k ZMWs of 25 kb) would silently lose its tail — the slots are launched in pieces of at most 2^24 - 256 workgroups.  CCSX_POLISH_MAX_BLOCKS forces
    pieces of 37 here (in a fresh process: the hook is read once): same results as the oracle, with and without kinetics.  CCSX_ALIGN16_MAX_SLOTS does the
    same for k_align16 / k_align16_tb, whose quads otherwise go in one launch: five scratch slots, so the 9 ZMWs' quads take several launches and the
    trace-back addresses its slots relative to each launch"""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r"""
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
from ccs_amd import api
import oracle_lib as O
for kin in (0, 1):
    o = api.default_opts(); o.hifi_kinetics = kin
    b = api.synth(9, (4, 12), (600, 2500), seed=91)
    h = api.Handle(0, opts=o)
    r = h.consensus(b)
    ref = api.Results.allocate(b, kinetics=bool(kin))
    O.consensus_batch(h.model, o, b, ref, nthreads=4)
    assert int(r.n_windows.sum()) > 300
    for z in range(b.n_zmw):
        assert r.status[z] == ref.status[z] and np.array_equal(r.sequence(z), ref.sequence(z)) and np.array_equal(r.raw(z), ref.raw(z)), z
        if kin: assert np.array_equal(r.kinetics(z), ref.kinetics(z))
    h.close()
print("pieces ok")
""" % (root, os.path.join(root, "tests"))
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, CCSX_POLISH_MAX_BLOCKS="37", CCSX_ALIGN16_MAX_SLOTS="5"), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "pieces ok" in p.stdout, p.stderr[-2000:]


def test_align16_launches_with_trace_backs_aside(built):
    """k_align16 over several launches in a batch large enough for the second stream: launch c writes scratch region c & 1, its trace-back runs on the second
    stream under launch c + 1, launch c + 2 waits for it.  CCSX_ALIGN16_MAX_SLOTS=900 cuts the 4608-ZMW batch's quads into six launches (fresh process: the
    hook is read once); every ZMW against the oracle"""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r"""
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
from ccs_amd import api
import oracle_lib as O
b = api.synth(4608, (3, 5), (150, 420), seed=78)
h = api.Handle(0)
r = h.consensus(b)
ref = api.Results.allocate(b)
O.consensus_batch(h.model, h.opts, b, ref, nthreads=8)
bad = [z for z in range(b.n_zmw) if r.status[z] != ref.status[z] or not np.array_equal(r.sequence(z), ref.sequence(z)) or not np.array_equal(r.raw(z), ref.raw(z))]
assert not bad, bad[:10]
h.close()
print("launches ok")
""" % (root, os.path.join(root, "tests"))
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, CCSX_ALIGN16_MAX_SLOTS="900"), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "launches ok" in p.stdout, p.stderr[-2000:]


@pytest.mark.parametrize("nofb", [0, 1])
def test_empty_backbone_pass(built, nofb):
    """found by tools/corruption_fuzz.py in round 4 (batch 47 of seed 11000): pass 0 of a ZMW has no bases.  SPEC: the backbone pass becomes the chain
    whatever its length; an empty backbone leaves a graph nothing can be threaded into -> DRAFT_FAILURE, and the draft cascade takes the median-length pass
    (the restatement used to take the first non-empty pass as backbone, the kernels never did).  Few and many (70) passes, with and without the cascade."""
    parts = [api.synth(1, 8, 600, seed=41), api.synth(1, 70, 300, seed=42), api.synth(1, 6, 500, seed=43)]
    batch = api.concat(parts)
    bo = batch.base_off.copy()
    for z in (0, 1):                                                   # pass 0 of ZMWs 0 and 1 loses its bases to pass 1
        r0 = int(batch.read_off[z]); bo[r0 + 1] = bo[r0]
    batch.base_off = bo
    o = api.default_opts(); o.no_fallback_draft = nofb; o.top_passes = 0; o.min_rq = 0.9
    h = api.Handle(0, opts=o)
    try:
        res = h.consensus(batch)
        ref = api.Results.allocate(batch)
        O.consensus_batch(h.model, o, batch, ref, nthreads=4)
        _compare(res, ref, batch)
        assert np.array_equal(res.np_, ref.np_)
        assert res.status[2] == 0 and (res.status[:2] == (2 if nofb else 0)).all()      # DRAFT_FAILURE without the cascade, rescued with it
    finally:
        h.close()


# ---- the two seams of the reference's block diagram (ABI v5: ccsx_draft_batch / ccsx_polish_batch; docs/img/ccs-impl.png, docs/faq/revio.md:35-53) ----
def _seam_batches():
    import golden_util as G
    yield "plain", api.synth(6, (3, 12), (300, 1500), seed=21)
    yield "c2ish", api.synth(3, 10, 3000, seed=22)
    for case in ("fallback", "lastresort", "partial", "split", "lowcx_rescue"):      # every draft generator of the cascade, partial passes, split alignment
        yield case, G.load(case)[0]


def _same_results(a, b, batch, exact=True):
    for k in ("status", "seq_len", "np_", "iters", "n_windows", "fn", "rn"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    for z in range(batch.n_zmw):
        assert np.array_equal(a.sequence(z), b.sequence(z)) and np.array_equal(a.quals(z), b.quals(z)), f"zmw {z}"
        assert np.array_equal(a.raw(z), b.raw(z)) if exact else np.allclose(a.raw(z), b.raw(z), atol=QV_TOL, rtol=0), f"zmw {z} raw QVs"
    assert np.array_equal(a.rq, b.rq) and np.array_equal(a.ec, b.ec) if exact else (np.allclose(a.rq, b.rq, atol=1e-6) and np.allclose(a.ec, b.ec, atol=1e-6))


@pytest.mark.gpu
def test_draft_seam_then_polish_seam_equals_the_fused_path(handle):
    """ccsx_polish_batch(ccsx_draft_batch(b)) == ccsx_consensus_batch(b), byte for byte, for every generator of the draft cascade"""
    for name, batch in _seam_batches():
        fused = handle.consensus(batch)
        d = handle.draft(batch)
        for z in range(batch.n_zmw):                       # the draft seam reports what the fused run's stage holds
            assert np.array_equal(d.draft(z), handle_stage_draft(handle, batch, z)), (name, z)
        split = handle.polish(batch, d)
        _same_results(split, fused, batch)
        assert (d.n_windows >= fused.n_windows).all() and ((d.status == 0) | (d.len == 0) | (d.status != 0)).all()
        ok = np.nonzero(d.status == 0)[0]
        assert np.array_equal(d.n_windows[ok], fused.n_windows[ok])
        for z in ok:
            w = d.windows(int(z))
            assert w[0] == 0 and w[-1] == d.len[z] and (np.diff(w) >= 1).all()


def handle_stage_draft(handle, batch, z):
    handle.upload(batch); handle.run(); handle.sync()
    return handle.stage_draft(z)


@pytest.mark.gpu
def test_polish_seam_on_the_oracles_draft_equals_the_oracles_polish(handle):
    """a host that drafts elsewhere: the oracle's first draft (POA of pass 0) goes through ccsx_polish_batch and through the oracle's polish seam"""
    batch = api.synth(5, (5, 10), (400, 1600), seed=31)
    d = api.Drafts.allocate(batch)
    for z in range(batch.n_zmw):
        d.set_draft(z, O.poa_draft(batch, z, handle.opts.max_poa_cov), backbone=0)
    res = handle.polish(batch, d)
    ref = O.polish_batch(handle.model, handle.opts, batch, d, api.Results.allocate(batch))
    _same_results(res, ref, batch, exact=False)
    # a draft in the orientation of a REVERSE pass (backbone 1): reverse complement of the first draft
    d2 = api.Drafts.allocate(batch)
    for z in range(batch.n_zmw):
        d2.set_draft(z, (3 - d.draft(z))[::-1].copy(), backbone=1)
    res2 = handle.polish(batch, d2)
    ref2 = O.polish_batch(handle.model, handle.opts, batch, d2, api.Results.allocate(batch))
    _same_results(res2, ref2, batch, exact=False)
    assert np.array_equal(res2.fn, res.rn) and np.array_equal(res2.rn, res.fn)


@pytest.mark.gpu
def test_qv_only_scores_the_sequence_as_given(handle):
    """CCSX_QV_ONLY (docs/faq/revio.md:35-53, "Arrow again for QVs"): no mutation is applied, one round; on a converged consensus the QVs are those of a
    polish that starts from it; bit-exact against the oracle's QV-only path"""
    batch = api.synth(4, 10, 2000, seed=41)
    fused = handle.consensus(batch)
    d = api.Drafts.allocate(batch)
    for z in range(batch.n_zmw):
        d.set_draft(z, fused.sequence(z), backbone=0)
    qv = handle.polish(batch, d, flags=api.QV_ONLY)
    ref = O.polish_batch(handle.model, handle.opts, batch, d, api.Results.allocate(batch), flags=api.QV_ONLY)
    _same_results(qv, ref, batch, exact=False)
    full = handle.polish(batch, d)
    for z in range(batch.n_zmw):
        assert np.array_equal(qv.sequence(z), fused.sequence(z)), "QV_ONLY returns the sequence it was given"
        # the windows of this run are cut from the consensus, not from the draft the fused run polished: its QVs are those of a polish that STARTS from the
        # consensus (identical wherever that polish changes nothing) and close to the fused run's own — same phred at most bases, same rq to 1e-3
        if np.array_equal(full.sequence(z), fused.sequence(z)): assert np.array_equal(qv.quals(z), full.quals(z))
        assert (qv.quals(z) == fused.quals(z)).mean() > 0.85 and abs(float(qv.rq[z]) - float(fused.rq[z])) < 1e-3
    assert (qv.iters == qv.n_windows).all()                # exactly one round per window
    # a draft with errors: QV_ONLY leaves them in and reports LOW quality there
    dz = api.Drafts.allocate(batch)
    for z in range(batch.n_zmw):
        s = fused.sequence(z).copy(); s[100] = (s[100] + 1) & 3
        dz.set_draft(z, s, backbone=0)
    bad = handle.polish(batch, dz, flags=api.QV_ONLY)
    for z in range(batch.n_zmw):
        assert bad.sequence(z)[100] == dz.draft(z)[100] and bad.quals(z)[100] <= 3 and bad.rq[z] < qv.rq[z]


@pytest.mark.gpu
def test_junk_and_missing_drafts_yield_statuses_not_errors(handle):
    batch = api.synth(6, 6, 800, seed=51)
    good = handle.draft(batch)
    rng = np.random.default_rng(5)
    d = api.Drafts.allocate(batch)
    d.set_draft(0, good.draft(0), backbone=int(good.backbone[0]))
    d.set_draft(1, rng.integers(0, 4, 700, dtype=np.uint8))                  # junk: nothing maps
    d.len[2] = 0                                                              # no draft
    d.set_draft(3, good.draft(3)); d.len[3] = int(d.seq_off[4] - d.seq_off[3]) + 5   # a length beyond the slot
    d.set_draft(4, good.draft(4)[:5])                                         # shorter than --min-length
    d.set_draft(5, (good.draft(5) | 0xF0).astype(np.uint8), backbone=99)      # high bits set, backbone out of range: masked / clamped
    res = handle.polish(batch, d)
    fused = handle.consensus(batch)
    assert res.status[0] == fused.status[0] and np.array_equal(res.sequence(0), fused.sequence(0))
    assert [api.STATUS_NAMES[int(s)] for s in res.status[1:5]] == ["TOO_MANY_UNUSABLE", "DRAFT_FAILURE", "DRAFT_FAILURE", "TOO_SHORT"]
    assert (res.seq_len[1:5] == 0).all()
    assert np.array_equal(res.sequence(5), fused.sequence(5))
    ref = O.polish_batch(handle.model, handle.opts, batch, _masked(d), api.Results.allocate(batch))
    assert np.array_equal(res.status, ref.status) and np.array_equal(res.seq_len, ref.seq_len)
    # drafts laid out for another batch are refused as a whole (an error of the call, nothing enqueued)
    other = api.Drafts.allocate(api.synth(6, 6, 900, seed=52))
    with pytest.raises(RuntimeError, match="capacity layout|another batch"):
        handle.polish(batch, other)
    assert np.array_equal(handle.consensus(batch).seq_len, fused.seq_len)    # the handle is still usable


def _masked(d):
    """the oracle's view of the same drafts: lengths beyond the slot are no draft"""
    import copy
    m = copy.deepcopy(d)
    for z in range(len(m.len)):
        if m.len[z] > m.seq_off[z + 1] - m.seq_off[z]: m.len[z] = 0
    return m


@pytest.mark.gpu
def test_seams_share_the_ticket_pipeline(handle):
    """ccsx_submit_draft / ccsx_submit_polish take tickets like ccsx_submit: three in flight, results equal the synchronous calls"""
    import ctypes as C
    L = api.lib()
    batches = [api.synth(3, 6, 700, seed=60 + k) for k in range(3)]
    drafts = [api.Drafts.allocate(b) for b in batches]
    keep, tickets = [], []
    for b, d in zip(batches, drafts):
        cb, cd, t = b.c_struct(), d.c_struct(), C.c_int64()
        assert L.ccsx_submit_draft(handle._h, C.byref(cb), C.byref(cd), C.byref(t)) == 0, L.ccsx_last_error()
        keep.append((cb, cd)); tickets.append(t.value)
    for t in tickets: assert L.ccsx_wait(handle._h, t) == 0
    results = [api.Results.allocate(b) for b in batches]
    tickets = []
    for b, d, r in zip(batches, drafts, results):
        cb, cd, cr, t = b.c_struct(), d.c_struct(), r.c_struct(), C.c_int64()
        assert L.ccsx_submit_polish(handle._h, C.byref(cb), C.byref(cd), C.byref(cr), 0, C.byref(t)) == 0, L.ccsx_last_error()
        keep.append((cb, cd, cr)); tickets.append(t.value)
    for t in tickets: assert L.ccsx_wait(handle._h, t) == 0
    for b, r in zip(batches, results):
        _same_results(r, handle.consensus(b), b)


@pytest.mark.gpu
def test_unwaited_draft_ticket_is_completed_when_its_slot_is_reused(handle):
    """four draft-seam tickets, the first never waited for: the submit that reuses its slot retires it, so its drafts' seq_off, win_off and backbone
    words (the cascade's marks masked off) are complete without a ccsx_wait"""
    import ctypes as C
    L = api.lib()
    batches = [api.synth(4, 6, 700 + 100 * k, seed=80 + k) for k in range(4)]
    want = handle.draft(batches[0])
    drafts = [api.Drafts.allocate(b) for b in batches]
    keep, tickets = [], []
    for b, d in zip(batches, drafts):
        d.seq_off[:] = -1; d.win_off[:] = -1; d.backbone[:] = -1   # (written by the engine, not left from ccsx_draft_layout)
        cb, cd, t = b.c_struct(), d.c_struct(), C.c_int64()
        assert L.ccsx_submit_draft(handle._h, C.byref(cb), C.byref(cd), C.byref(t)) == 0, L.ccsx_last_error()
        keep.append((cb, cd)); tickets.append(t.value)
    got = drafts[0]
    assert np.array_equal(got.seq_off, want.seq_off) and np.array_equal(got.win_off, want.win_off)
    assert (got.backbone < 256).all() and np.array_equal(got.backbone, want.backbone)
    assert np.array_equal(got.status, want.status) and np.array_equal(got.len, want.len) and np.array_equal(got.n_windows, want.n_windows)
    for z in range(batches[0].n_zmw):
        assert np.array_equal(got.draft(z), want.draft(z)) and np.array_equal(got.windows(z), want.windows(z)), z
    assert L.ccsx_wait(handle._h, tickets[0]) != 0 and b"recycled" in L.ccsx_last_error()
    for t in tickets[1:]: assert L.ccsx_wait(handle._h, t) == 0


@pytest.mark.gpu
def test_upload_retires_unwaited_tickets_and_recycles_slot_0(built):
    """two fused tickets on a fresh handle (slots 0 and 1), then ccsx_upload of a third batch with no wait: both tickets' outputs and timings are complete,
    slot 0's ticket is recycled, slot 1's stays valid, and the synchronous path runs the uploaded batch"""
    h = api.Handle(0)
    bs = [api.synth(5, 6, 800 + 200 * k, seed=90 + k) for k in range(3)]
    want = [h.consensus(b) for b in bs]
    res = [api.Results.allocate(b, pinned=True) for b in bs[:2]]
    for r in res: r.seq_off[:] = -1
    pinned = [b.pinned() for b in bs[:2]]
    t0, t1 = h.submit(pinned[0], res[0]), h.submit(pinned[1], res[1])
    assert (t0, t1) == (0, 1)
    h.upload(bs[2])
    for r, w, b in zip(res, want, bs):
        assert np.array_equal(r.seq_off, w.seq_off)
        _same_results(r, w, b)
    assert h.ticket_timings(t1).polish_workgroups == int(want[1].n_windows.sum())
    with pytest.raises(RuntimeError, match="recycled"):
        h.wait(t0)
    assert h.wait(t1) is res[1]
    h.run(); h.sync()
    _same_results(h.download(), want[2], bs[2])
    h.close()


@pytest.mark.gpu
def test_poll_retires_the_ticket(built):
    """the first ccsx_poll that returns 1 retires the ticket: its outputs, seq_off included, are complete without a ccsx_wait"""
    import time
    h = api.Handle(0)
    b = api.synth(5, 6, 800, seed=95)
    want = h.consensus(b)
    pb, r = b.pinned(), api.Results.allocate(b, pinned=True)
    r.seq_off[:] = -1
    t = h.submit(pb, r)
    deadline = time.monotonic() + 5.0
    while not h.poll(t):
        assert time.monotonic() < deadline, "the ticket did not complete within 5 s"
        time.sleep(0.002)
    assert np.array_equal(r.seq_off, want.seq_off)
    _same_results(r, want, b)
    assert h.ticket_timings(t).polish_workgroups == int(want.n_windows.sum())
    assert h.poll(t)
    h.close()


@pytest.mark.gpu
def test_ticket_timings_do_not_read_caller_memory(handle):
    """polish_workgroups is taken when the ticket is retired: overwriting the results afterwards does not change it"""
    b = api.synth(5, 6, 800, seed=96)
    r = api.Results.allocate(b)
    t = handle.submit(b, r)
    handle.wait(t)
    total = int(r.n_windows.sum())
    assert total > 0
    r.n_windows[:] = 0
    assert handle.ticket_timings(t).polish_workgroups == total
    handle.release(t)


@pytest.mark.gpu
def test_every_run_mode_records_every_stage_event(built):
    """a fused ticket, a draft-seam ticket, a polish-seam ticket and a ccsx_hd_batch call each leave all seven stage durations readable: the getter returns 0,
    every figure is finite and >= 0, and total_ms is no shorter than any part — every stage event was recorded, in order, on every path of the launch
    schedule.  (ccsx_hd_batch is synchronous and has no ticket: ccsx_get_timings reads its slot's events.)"""
    import ctypes as C, math
    L = api.lib()
    h = api.Handle(0)
    b = api.synth(8, 3, 500, seed=97)

    def check(tm, what):
        parts = [tm.setup_ms, tm.draft_ms, tm.align_ms, tm.queue_ms, tm.polish_ms, tm.stitch_ms]
        print(what, parts, tm.total_ms)
        assert all(math.isfinite(x) and x >= 0 for x in parts + [tm.total_ms]), (what, parts, tm.total_ms)
        assert all(tm.total_ms >= x for x in parts), (what, parts, tm.total_ms)

    def ticket(t, what):
        tm = api.Timings()
        assert L.ccsx_wait(h._h, t.value) == 0, L.ccsx_last_error()
        assert L.ccsx_ticket_timings(h._h, t.value, C.byref(tm)) == 0, L.ccsx_last_error()
        check(tm, what)

    r, d = api.Results.allocate(b), api.Drafts.allocate(b)
    cb, cr, cd, t = b.c_struct(), r.c_struct(), d.c_struct(), C.c_int64()
    assert L.ccsx_submit(h._h, C.byref(cb), C.byref(cr), C.byref(t)) == 0, L.ccsx_last_error()
    ticket(t, "fused")
    assert L.ccsx_submit_draft(h._h, C.byref(cb), C.byref(cd), C.byref(t)) == 0, L.ccsx_last_error()
    ticket(t, "draft seam")
    assert L.ccsx_submit_polish(h._h, C.byref(cb), C.byref(cd), C.byref(cr), 0, C.byref(t)) == 0, L.ccsx_last_error()
    ticket(t, "polish seam")
    h.hd(b, d)
    check(h.timings(), "ccsx_hd_batch")
    h.close()


@pytest.mark.gpu
def test_timing_origin_moves_only_while_the_handle_is_idle(built):
    """the origin of ccsx_timings.start_ms / end_ms is moved forward at a submit that finds NO slot in flight (never inside the getter, never under pending
    tickets).  CCSX_EPOCH_REBASE_MS=0 forces a move at every idle submit: times stay monotone across moves, tickets in flight keep their timings."""
    import subprocess, sys, os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r'''
import sys; sys.path.insert(0, %r)
from ccs_amd import api
h = api.Handle(0)
bs = [api.synth(8, 5, 600, seed=70 + k) for k in range(4)]
rs = [api.Results.allocate(b) for b in bs]
ends = []
t0 = h.submit(bs[0], rs[0]); h.wait(t0); a = h.ticket_timings(t0); ends.append((a.start_ms, a.end_ms)); h.release(t0)
t1 = h.submit(bs[1], rs[1])                      # the handle was idle: the origin moved here
t2 = h.submit(bs[2], rs[2])                      # one ticket in flight: no move
h.wait(t1); b = h.ticket_timings(t1); ends.append((b.start_ms, b.end_ms))
h.wait(t2); c = h.ticket_timings(t2); ends.append((c.start_ms, c.end_ms))
h.release(t1); h.release(t2)
t3 = h.submit(bs[3], rs[3]); h.wait(t3); d = h.ticket_timings(t3); ends.append((d.start_ms, d.end_ms))
assert all(e > s_ > 0 for s_, e in ends), ends
assert all(ends[k + 1][0] >= ends[k][0] for k in range(3)), ends
print("ok", ends)
''' % root
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, CCSX_EPOCH_REBASE_MS="0"), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "ok" in p.stdout, p.stderr[-1500:] + p.stdout[-500:]

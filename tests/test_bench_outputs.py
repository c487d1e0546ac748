"""bench.py --dump-outputs without a GPU: the files it writes for one batch's result buffers (the GPU test runs the whole command)."""
import ctypes
import os

import numpy as np
import pytest

from ccs_amd import api
import bench


def _fake_results(batch, kinetics):
    """result buffers of `batch` filled as a run would fill them: a consensus of up to its capacity per ZMW, seeded"""
    res = api.Results.allocate(batch, kinetics=kinetics, raw=False)
    rng = np.random.default_rng(5)
    n = batch.n_zmw
    cap = np.diff(res.seq_off)
    res.seq_len[:] = cap - rng.integers(0, 50, n)
    res.status[:] = rng.integers(0, 3, n)
    res.rq[:] = rng.random(n, dtype=np.float32); res.ec[:] = rng.random(n, dtype=np.float32) * 10
    res.np_[:] = 10; res.iters[:] = rng.integers(1, 9, n); res.n_windows[:] = cap // 200; res.fn[:] = 5; res.rn[:] = 5
    res.seq[:] = rng.integers(0, 4, len(res.seq)); res.qual[:] = rng.integers(0, 94, len(res.qual))
    if kinetics:
        res.kin[:] = rng.integers(0, 256, res.kin.shape)
    return res


@pytest.mark.parametrize("kinetics", [False, True])
def test_dump_outputs_is_a_fixed_sample_under_the_limit(built, tmp_path, kinetics):
    batch = api.synth(1600, 10, 6000, seed=0xC0FFEE)        # more per-base output than the limit allows: the sample is a strict subset
    res = _fake_results(batch, kinetics)
    a, b = tmp_path / "a", tmp_path / "b"
    total = bench.dump_outputs(np, batch, res, kinetics, str(a))
    bench.dump_outputs(np, batch, res, kinetics, str(b))
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and all(f.endswith(".npy") for f in names)
    assert total == sum(os.path.getsize(a / f) for f in names) <= bench.DUMP_BYTES
    got = {f[:-4]: np.load(a / f) for f in names}
    for f in names:                                          # same inputs, same files
        assert np.array_equal(got[f[:-4]], np.load(b / f))
    assert all(x.dtype in (np.float32, np.float64) for x in got.values())
    assert ("kinetics" in got) == kinetics
    n = batch.n_zmw
    for k, ref in (("zmw_id", batch.zmw_id), ("status", res.status), ("seq_len", res.seq_len), ("np", res.np_), ("iters", res.iters),
                   ("n_windows", res.n_windows), ("fn", res.fn), ("rn", res.rn), ("rq", res.rq), ("ec", res.ec)):
        assert len(got[k]) == n and np.array_equal(got[k], ref), k
    pick = got["sample_zmw"].astype(np.int64)
    assert 0 < len(pick) < n and np.all(np.diff(pick) > 0)
    off = got["sample_seq_off"].astype(np.int64)
    assert len(off) == len(pick) + 1 and off[-1] == len(got["seq"]) == len(got["qual"])
    for i, z in enumerate(pick):
        assert np.array_equal(got["seq"][off[i]:off[i + 1]], res.sequence(z)) and np.array_equal(got["qual"][off[i]:off[i + 1]], res.quals(z))
        if kinetics:
            assert np.array_equal(got["kinetics"][:, off[i]:off[i + 1]], res.kinetics(z))


def test_bench_synthesis_is_api_synth(built, monkeypatch):
    """the benchmark makes its page-locked batches straight from the generator's buffers: field for field what api.synth(...).pinned() holds
    (page-locked memory stood in for by host buffers: no device here)"""
    L = api.lib()
    held = {}

    def alloc(n):
        buf = (ctypes.c_uint8 * n)()
        held[ctypes.addressof(buf)] = buf
        return ctypes.addressof(buf)
    monkeypatch.setattr(L, "ccsx_alloc_pinned", alloc)
    monkeypatch.setattr(L, "ccsx_free_pinned", lambda p: held.pop(p))
    for passes, length, first, pin in ((10, 3000, 0, ("bases", "pw", "ipd")), ((3, 12), (300, 2500), 4096, ("bases", "pw"))):
        got = bench.synth_pin(api, np, bench.synth_generate(api, 64, passes, length, first), pin)
        ref = api.synth(64, passes, length, seed=0xC0FFEE, first_zmw_id=first)
        for k in ("zmw_id", "snr", "read_off", "base_off", "bases", "pw", "ipd", "flags", "tpl_off", "tpl"):
            a, b = getattr(got, k), getattr(ref, k)
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), k
        assert len(got._pinned) == len(pin) and all(p.p in held for p in got._pinned)
        assert {k for k in ("bases", "pw", "ipd") if ctypes.addressof(ctypes.c_uint8.from_buffer(getattr(got, k))) in held} == set(pin)
        del got
    assert not held

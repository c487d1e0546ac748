"""k_polish_t with DEFAULT heuristics — candidate filter and z-score gate on — against the float64 reference of tests/arrow_ref.py on the filter lab (tests/filter_lab.py),
drafts handed in through the polish seam: (a) bit-exact against the CPU restatement; (b) raw QVs per core base — a base the reference calls skipped reports its p_skip,
every other base lies inside the propagated bound, a quiet base's sum starting at p_skip: the witness that the engine skipped what the SPEC says and nothing else;
(c) cores per window; (d) usable reads per window, all passes and full-length passes (ccsx_stage_wmeta), rounds, np / ec / iters / status per ZMW; (e) byte-identical
results whatever the lab's place in a batch.  Every run asserts from the engine's own stage outputs that the planted classes occurred, and prints the three left-out
shares (python -m pytest tests/test_filter_gpu.py -m gpu -s)."""
import time

import numpy as np
import pytest

from ccs_amd import api
import filter_lab as F
import oracle_lib as O

pytestmark = pytest.mark.gpu


def _drafts(batch, drafts):
    d = api.Drafts.allocate(batch)
    for zi, t in enumerate(drafts): d.set_draft(zi, t, backbone=0)
    return d


def engine_run(batch, drafts, where, o, flags):
    """Handle.polish on `batch` with the drafts handed in; where = {lab ZMW name: index in the batch}.  Returns (results, drafts object, windows cut from the engine's
    stage outputs per lab ZMW, ccsx_stage_wmeta rows per lab ZMW)."""
    h = api.Handle(0, model=api.default_model(), opts=o)
    try:
        d = _drafts(batch, drafts)
        res = h.polish(batch, d, flags=flags)
        W_of, wm_of = {}, {}
        for z in F.lab():
            zi = where[z.name]
            assert np.array_equal(h.stage_windows(zi), O.windows(z.draft)), f"zmw {z.name}: the windows are not those the lab was built on"
            W_of[z.name] = F.cut_engine(h, batch, zi, z); wm_of[z.name] = h.stage_wmeta(zi)
    finally:
        h.close()
    return res, d, W_of, wm_of


@pytest.mark.parametrize("qv_only,max_qv,min_zscore", F.RUNS)
def test_lab_with_default_heuristics(built, qv_only, max_qv, min_zscore):
    """The lab through Handle.polish with the product's default heuristics, drafts handed in: (d) per window, (b) per base, (c) per core, the three left-out shares within
    their caps, then (a) bit for bit the CPU restatement.  Measured on an MI355X box: 0 of 80 windows ambiguous, 0 of 1 774 core bases left out, 0 of 1 203 z decisions
    undecided in every run; the first case pays about 8 s of CPU for the float64 gains, the others share them (under 2 s each)."""
    model = api.default_model(); lab = F.lab(); batch = F.batch_of(lab); o = F.opts(max_qv, min_zscore); flags = api.QV_ONLY if qv_only else 0
    where = {z.name: zi for zi, z in enumerate(lab)}
    res, d, W_of, wm_of = engine_run(batch, [z.draft for z in lab], where, o, flags)
    tag = f"{'QV_ONLY' if qv_only else 'full polish'} max_qv {max_qv} min_zscore {min_zscore}"
    O.counts_reset()
    ref = O.polish_batch(model, o, batch, d, api.Results.allocate(batch), flags=flags)
    cnt = O.counts()
    # the float64 reference on the windows, segments and dirty bits the ENGINE reports
    t0 = time.time()
    for z in lab: F.reference(model, W_of[z.name], qv_only, max_qv, min_zscore, F.caches_for(z, W_of[z.name]))
    t_ref = time.time() - t0
    # the planted classes occurred in this run
    if not qv_only:
        for z in lab:
            if (max_qv, min_zscore) == (50, -3.4): F.run_checks(z, W_of[z.name], z.checks)
            F.run_checks(z, W_of[z.name], z.zchecks.get(min_zscore, []))
    ndrop = sum(sum(w["zdrop"]) for W in W_of.values() for w in W)
    assert (ndrop > 0) == (min_zscore != 0.0) and cnt["zdrop"] == ndrop, f"{tag}: the reference drops {ndrop} (pass, window) pairs by z-score, the restatement {cnt['zdrop']}"
    # (d) per window: core length, usable reads over all passes and over the full-length passes, non-convergence, rounds
    for z in lab:
        wm = wm_of[z.name]
        assert len(wm) == len(W_of[z.name]), f"{tag} zmw {z.name}: ccsx_stage_wmeta reports {len(wm)} windows"
        for wi, w in enumerate(W_of[z.name]):
            if w["amb"] or w["z_und"]: continue
            want = (len(w["core"]), w["last"]["n_use"], w["last"]["n_full"], int(w["last"]["nonconv"]), w["rounds"])
            assert tuple(int(x) for x in wm[wi]) == want, f"{tag} zmw {z.name} ({z.cls}) window {wi}: (core, usable, usable full-length, non-convergent, rounds) {tuple(int(x) for x in wm[wi])}, reference {want}"
    # (b), (c) and the per-ZMW fields
    S = F.compare_run(res, where, W_of, qv_only, max_qv, tag, core_len=lambda name, wi: int(wm_of[name][wi][0]))
    F.assert_caps(S, W_of, tag + f" (float64 reference {t_ref:.1f} s)")
    # (a) bit for bit the CPU restatement (last: the messages above name ZMW, class, window and column; this one names the ZMW)
    for zi, z in enumerate(lab):
        assert res.status[zi] == ref.status[zi] and np.array_equal(res.sequence(zi), ref.sequence(zi)) and np.array_equal(res.raw(zi), ref.raw(zi)), f"{tag} zmw {z.name} ({z.cls}): differs from the CPU restatement"
        assert (res.np_[zi], res.iters[zi], res.n_windows[zi]) == (ref.np_[zi], ref.iters[zi], ref.n_windows[zi]) and res.ec[zi] == ref.ec[zi] and res.rq[zi] == ref.rq[zi], f"{tag} zmw {z.name}: np / ec / iters / rq differ from the CPU restatement"


def _concat(parts):
    """(batch, drafts) of [(Batch, [drafts])] in this order"""
    cat = lambda xs: np.ascontiguousarray(np.concatenate(xs))
    nr = np.cumsum([0] + [int(b.read_off[-1]) for b, _ in parts]); nb = np.cumsum([0] + [int(b.base_off[-1]) for b, _ in parts]); n = sum(b.n_zmw for b, _ in parts)
    batch = api.Batch(np.arange(n, dtype=np.int32), cat([b.snr for b, _ in parts]), cat([[0]] + [b.read_off[1:] + nr[k] for k, (b, _) in enumerate(parts)]).astype(np.int32),
                      cat([[0]] + [b.base_off[1:] + nb[k] for k, (b, _) in enumerate(parts)]).astype(np.int64), cat([b.bases for b, _ in parts]), cat([b.pw for b, _ in parts]),
                      cat([b.ipd for b, _ in parts]), cat([b.flags for b, _ in parts]))
    return batch, [t for _, ds in parts for t in ds]


def test_results_do_not_depend_on_the_place_in_the_batch(built):
    """(e) the lab reversed, and interleaved with plain api.synth ZMWs: every lab ZMW's sequence, QVs and per-ZMW fields byte-identical across the runs"""
    lab = F.lab(); o = F.opts()
    single = [(F.batch_of([z]), [z.draft]) for z in lab]
    syn = []
    for k in range(5):
        b = api.synth(1, (4, 9), (150, 700), seed=90 + k)
        syn.append((b, [O.poa_draft(b, 0)]))
    orders = {"straight": [("L", k) for k in range(len(lab))], "reversed": [("L", k) for k in reversed(range(len(lab)))],
              "interleaved": [x for k in range(len(lab)) for x in ([("L", k)] + ([("S", k // 3)] if k % 3 == 0 and k // 3 < len(syn) else []))]}
    got = {}
    for name, order in orders.items():
        batch, drafts = _concat([single[k] if kind == "L" else syn[k] for kind, k in order])
        h = api.Handle(0, model=api.default_model(), opts=o)
        try: res = h.polish(batch, _drafts(batch, drafts))
        finally: h.close()
        got[name] = {lab[k].name: (res.sequence(i).tobytes(), res.raw(i).tobytes(), res.qual[res.seq_off[i]:res.seq_off[i] + res.seq_len[i]].tobytes(), int(res.status[i]), int(res.np_[i]),
                                   float(res.ec[i]), float(res.rq[i]), int(res.iters[i])) for i, (kind, k) in enumerate(order) if kind == "L"}
    assert len(got["interleaved"]) == len(lab) and sum(1 for kind, _ in orders["interleaved"] if kind == "S") == len(syn)
    for name in ("reversed", "interleaved"):
        for z in lab:
            assert got[name][z.name] == got["straight"][z.name], f"zmw {z.name} ({z.cls}): results of the {name} batch differ from those of the lab batch"


def test_tandem_flag_switches_the_filter_off_for_one_zmw(built):
    """(f) three lab ZMWs through the fused path (the engine's own drafts: their passes are clean enough that the POA draft is the planted one) with the tandem-repeat
    switch at 10 bases: the middle one (a period-2 tract of 12: tandem_len 12) is flagged and must equal the reference with NO evidence, its unflagged neighbours
    (tandem_len 0) the reference with the filter.  max_qv 93, where p_skip of 8 and more passes is not hidden by the floor."""
    model = api.default_model(); by = {z.name: z for z in F.lab()}; zs = [by["g11_13"], by["g12_tracts"], by["masks"]]
    batch = F.batch_of(zs); o = F.opts(93, -3.4)
    h = api.Handle(0, model=model, opts=o)
    try:
        res, tl, _ = h.consensus_extras(batch, tandem=True, min_tandem_repeat_length=10)
        assert [int(x) for x in tl] == [0, 12, 0], f"tandem_len {tl}"
        W_of = {z.name: F.cut_engine(h, batch, zi, z) for zi, z in enumerate(zs)}; wm_of = {z.name: h.stage_wmeta(zi) for zi, z in enumerate(zs)}
    finally:
        h.close()
    for z in zs: F.reference(model, W_of[z.name], False, 93, -3.4, F.caches_for(z, W_of[z.name]), filtered=(z.name != "g12_tracts"))
    assert not any(any(w["last"]["skipped"]) or any(w["last"]["quiet"]) for w in W_of["g12_tracts"]) and all(sum(w["last"]["skipped"]) > 15 for z in (zs[0], zs[2]) for w in W_of[z.name])
    S = F.compare_run(res, {z.name: zi for zi, z in enumerate(zs)}, W_of, False, 93, "tandem switch at 10", core_len=lambda name, wi: int(wm_of[name][wi][0]), zmws=zs)
    assert S["ambiguous"] == 0 and S["left_out"] <= 0.02 * S["bases"] and S["skipped"] > 0 and S["bases"] == sum(len(z.draft) for z in zs)

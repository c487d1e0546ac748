"""The heteroduplex finder's kernels (k_hd_pile, k_hd_indel, k_hd_verdict; DESIGN.md §2 "Heteroduplex rule") at their limits: every planted batch of
tests/hd_lab.py through ccsx_hd_batch on the supplied drafts, against the plain reference (tests/hd_plain.py: exact Fisher test, written from the rule's text) and
against the restatement (tests/hd_ref.py) on the engine's own stage outputs.  The census of the plain reference must show the limit the batch is named for before
anything is compared.  tests/test_hd_plain.py does the same on the oracle's stages, without a GPU."""
import numpy as np
import pytest

from ccs_amd import api
import hd_lab
import hd_plain
import hd_ref

FIELDS = ("column", "kind", "alt", "fwd_alt", "fwd_n", "rev_alt", "rev_n")


def engine_reports(rep):
    return [dict(verdict=int(rep.verdict[z]), n_sub=int(rep.n_sub_sites[z]), n_indel=int(rep.n_indel_sites[z]), min_p=float(rep.min_p[z]),
                 sites=[dict({f: int(s[f]) for f in FIELDS}, p=float(s["p"])) for s in rep.site_list(z)]) for z in range(len(rep.verdict))]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(hd_lab.BATCHES))
def test_batch_at_its_limit(built, name):
    """one handle, every option set of the batch: ccsx_hd_batch, the engine's stages, the plain reference's census, then engine = plain = restatement"""
    lab = hd_lab.BATCHES[name]()
    h = api.Handle(0, opts=hd_lab.engine_opts(lab))
    try:
        d = hd_lab.drafts_of(lab)
        got, stage = [], None
        for kw in lab.opt_sets:
            rep = h.hd(lab.batch, d, hd_lab.hd_opts(kw))
            if stage is None:                                   # (the stages do not depend on the finder's options)
                stage = hd_ref.collect_stage(h, lab.batch, rep.status, d.backbone)
            assert [int(s) for s in rep.status] == [Z.status for Z in stage]
            got.append(engine_reports(rep))
    finally:
        h.close()
    for z, (t, _) in enumerate(lab.drafts):
        assert stage[z].status != 0 or np.array_equal(stage[z].draft, t), z
    used = hd_lab.used_records(stage)
    both = [hd_plain.hd_zmws(stage, hd_lab.ref_opts(kw)) for kw in lab.opt_sets]
    plain, cens = [r for r, _ in both], [c for _, c in both]
    hd_lab.check_census(name, lab, cens, plain)
    for k, kw in enumerate(lab.opt_sets):
        ref = hd_ref.hd_zmws(used, hd_lab.ref_opts(kw))
        keep = [z for z in range(lab.batch.n_zmw) if name != "noisy_small" or not hd_plain.borderline(cens[k][z])]
        pick = lambda r: [r[z] for z in keep]
        diffs = dict(engine_vs_plain=hd_lab.differences(pick(got[k]), pick(plain[k])), engine_vs_restatement=hd_lab.differences(pick(got[k]), pick(ref)),
                     restatement_vs_plain=hd_lab.differences(pick(ref), pick(plain[k])))
        assert not any(diffs.values()), (name, kw, {a: v[:3] for a, v in diffs.items() if v})


@pytest.mark.gpu
def test_fused_path_reports_the_same_at_the_limits(built):
    """ccsx_consensus_hd without the split against ccsx_hd_batch on ccsx_draft_batch's drafts, field for field, on the planted batches (tests/test_hd_fused.py
    asserts it on natural data); the seam's report against the plain reference on those drafts as well, so that both paths are held to the rule here"""
    h = api.Handle(0)
    try:
        for name in ("segment_rows", "site_lists", "indel_spans"):
            lab = hd_lab.BATCHES[name]()
            d, stage = h.draft(lab.batch), None
            for kw in lab.opt_sets:
                o = hd_lab.hd_opts(kw)
                _, fused, _, _ = h.consensus_hd(lab.batch, o, split=False)
                seam = h.hd(lab.batch, d, o)
                assert np.array_equal(fused.status, seam.status), (name, kw)
                if stage is None:                               # (the stages do not depend on the finder's options)
                    stage = hd_ref.collect_stage(h, lab.batch, seam.status, d.backbone)
                plain, cens = hd_plain.hd_zmws(stage, hd_lab.ref_opts(kw))
                keep = [z for z, c in enumerate(cens) if not hd_plain.borderline(c)]       # (the engine's own drafts: the plants are not pinned, a tie may occur)
                assert len(keep) >= lab.batch.n_zmw - 1
                assert hd_lab.differences([engine_reports(seam)[z] for z in keep], [plain[z] for z in keep]) == [], (name, kw)
                assert hd_lab.differences(engine_reports(fused), engine_reports(seam), rel=0.0) == [], (name, kw)
                assert (seam.n_sub_sites.sum() + seam.n_indel_sites.sum()) > 0, (name, kw)
    finally:
        h.close()

"""The pileup summary (sa sm sx of docs/faq/bam-output.md:25-27; DESIGN.md §2 "Pileup summary"): the CPU restatement on hand-made cases, the C ABI,
and on an MI355X exact parity of the planes with the restatement, no effect on any other output, the ticketed form, a batch at scale and the CLI."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from ccs_amd import api
import bam_util
import pileup_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CCS = os.path.join(ROOT, "ccs_amd", "bin", "ccs")
T = np.array([0, 1, 2, 3] * 7, np.uint8)          # 28 columns; no base repeats its neighbour, so every single edit has one best alignment


def rc(s):
    return (3 - np.asarray(s, np.uint8)[::-1]).astype(np.uint8)


def _one_window(reads, tpl=T, cs=2, ce=26, ref_strand=0):
    """planes of a one-window ZMW: reads = [(native bases, flags)], each pass's segment is the whole read"""
    z = pileup_ref.Zmw([np.asarray(tpl, np.uint8)], [(cs, ce)], ref_strand,
                       [(np.asarray(b, np.uint8), fl, True, np.array([0, len(b)])) for b, fl in reads])
    return pileup_ref.pileup_zmws([z])[0]


# ---------------------------------------------------------------- CPU: the restatement
def test_identical_segments_match_everywhere():
    cov, sm, sx = _one_window([(T, 0)] * 5 + [(rc(T), 1)] * 3)
    assert len(cov) == 24 and (cov == 8).all() and (sm == 8).all() and (sx == 0).all()


def test_a_substitution_and_a_deletion_land_on_their_column():
    sub = T.copy(); sub[10] = 0                                  # G -> A at column 10
    cov, sm, sx = _one_window([(sub, 0)])
    assert (cov == 1).all() and sx.tolist() == [int(c == 10) for c in range(2, 26)] and (sm + sx == 1).all()
    dele = np.delete(T, 13)                                      # column 13 has no read base
    cov, sm, sx = _one_window([(dele, 0)])
    assert (cov == 1).all() and (sx == 0).all() and sm.tolist() == [int(c != 13) for c in range(2, 26)]
    ins = np.insert(T, 7, 3)                                     # an inserted base is no outcome of any column
    cov, sm, sx = _one_window([(ins, 0)])
    assert (cov == 1).all() and (sm == 1).all() and (sx == 0).all()


def test_a_reverse_strand_segment_maps_to_the_mirrored_column():
    sub = T.copy(); sub[5] = 3                                   # the reverse-strand read carries a substitution at forward column 5
    cov, sm, sx = _one_window([(rc(sub), 1)])
    assert (cov == 1).all() and sx.tolist() == [int(c == 5) for c in range(2, 26)]
    rows = pileup_ref.diag_rows([rc(sub).astype(np.int64)], [rc(T).astype(np.int64)])[0]
    assert rows[len(T) - 1 - 5] == len(T) - 1 - 5               # (read-oriented column J-1-j holds the read row of that base)
    cov, sm, sx = _one_window([(sub, 1)], ref_strand=1)          # the strand reference decides the orientation, not the flag alone
    assert sx.tolist() == [int(c == 5) for c in range(2, 26)]


def test_empty_and_unusable_segments():
    z = pileup_ref.Zmw([T], [(2, 26)], 0, [(T, 0, True, np.array([4, 4])),           # empty segment: coverage only
                                           (T, 0, True, np.array([0, len(T)])),
                                           (T, 0, False, np.array([0, len(T)])),     # not valid: no coverage
                                           (np.tile(T, 3), 0, True, np.array([0, 84]))])   # longer than 63 rows: not a segment
    cov, sm, sx = pileup_ref.pileup_zmws([z])[0]
    assert (cov == 2).all() and (sm == 1).all() and (sx == 0).all()


def test_two_windows_concatenate_their_cores():
    t0, t1 = T[:24], T[20:]
    z = pileup_ref.Zmw([t0, t1], [(0, 22), (2, 8)], 0, [(T, 0, True, np.array([0, 18, 22, 28]))])
    cov, sm, sx = pileup_ref.pileup_zmws([z])[0]
    assert len(cov) == 28 and (cov == 1).all() and (sm == 1).all()


def test_run_length_encoding_round_trip():
    rng = np.random.default_rng(5)
    for n in (0, 1, 7, 500):
        v = np.repeat(rng.integers(0, 256, n), rng.integers(1, 30, n)).astype(np.uint8)
        sa = api.rle(v)
        assert sa.dtype == np.uint32 and int(sa[0::2].sum()) == len(v) and (sa[0::2] > 0).all()
        assert (sa[1::2][1:] != sa[1::2][:-1]).all()             # runs are maximal
        assert np.array_equal(api.unrle(sa), v)


def test_pileup_struct_and_versions(built, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ccsx.h"\nint main(void){printf("%zu %zu\\n", sizeof(ccsx_pileup), '
                   'offsetof(ccsx_pileup, mismatches));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == [C.sizeof(api.CPileup), api.CPileup.mismatches.offset]
    L = api.lib()
    assert L.ccsx_pileup_rule_version() == 1 and L.ccsx_spec_version() == 8 and L.ccsx_abi_version() == 6
    b = api.synth(2, 4, 300, seed=1)
    res = api.Results.allocate(b)
    pl = api.Pileup.allocate(res)
    cb, cr, cp = b.c_struct(), res.c_struct(), pl.c_struct()
    assert cp.seq_capacity == len(res.seq)
    assert L.ccsx_consensus_pileup(None, C.byref(cb), C.byref(cr), C.byref(cp)) < 0 and b"null argument" in L.ccsx_last_error()
    t = C.c_int64()
    assert L.ccsx_submit_pileup(None, C.byref(cb), C.byref(cr), None, C.byref(t)) < 0 and b"null argument" in L.ccsx_last_error()


def test_cli_pileup_summary_is_an_option(built, tmp_path):
    """--pileup-summary is known to the driver; without a GPU the run fails like any other run, not as an unknown option"""
    usage = subprocess.run([CCS, "--help"], capture_output=True, text=True, timeout=60).stderr
    assert "--pileup-summary" in usage
    if api.device_count() > 0:
        return
    bam = tmp_path / "s.subreads.bam"
    subprocess.run([CCS, "--write-synthetic", "2,3,150,1", str(bam)], check=True, capture_output=True, timeout=120)
    p = subprocess.run([CCS, "--pileup-summary", str(bam), str(tmp_path / "o.bam")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 1 and "no gfx950 GPU" in p.stderr and "unknown option" not in p.stderr


# ---------------------------------------------------------------- GPU
def _parity(h, batch, zmws=None):
    res, pl = h.consensus_pileup(batch)
    zs = list(range(batch.n_zmw)) if zmws is None else list(zmws)
    ref = pileup_ref.pileup_zmws(pileup_ref.collect_stage(h, batch, zs))
    for z, (cov, sm, sx) in zip(zs, ref):
        if res.seq_len[z] == 0:
            assert len(cov) == 0 and len(pl.cov(z)) == 0, z
            continue
        assert np.array_equal(pl.cov(z), cov), z
        assert np.array_equal(pl.sm(z), sm), z
        assert np.array_equal(pl.sx(z), sx), z
    return res, pl


@pytest.mark.gpu
def test_pileup_parity_with_the_restatement(built):
    import hd_synth
    import lowcx
    sets = {
        "both_strands": api.synth(24, 8, 1500, seed=61),
        "partial": hd_synth.make(16, (2, 8), (600, 2500), seed=62, k_sub=2, partial=True)[0],
        "groups_of_32": api.synth(3, 70, 500, seed=63),
        "lowcx": lowcx.make(16, 10, 1500, seed=64, tpl="lowcx"),
        "failed": api.concat([api.synth(4, 2, 800, seed=65), api.synth(4, 6, 800, seed=66), api.synth(2, 6, 12, seed=67)]),
    }
    for kin in (0, 1):
        opts = api.default_opts(); opts.hifi_kinetics = kin
        h = api.Handle(0, opts=opts)
        for name, b in sets.items():
            res, pl = _parity(h, b)
            ok = res.status == 0
            assert ok.any() or name == "failed", name
            if name == "failed":
                assert (~ok[:4]).all() and ok[4:8].any()
        h.close()
    # a 255-pass ZMW: coverage reaches 255 and nothing wraps
    opts = api.default_opts(); opts.top_passes = 0
    h = api.Handle(0, opts=opts)
    b = api.synth(1, 255, 300, seed=68)
    res, pl = _parity(h, b)
    assert res.status[0] == 0 and pl.cov(0).max() > 200 and (pl.sm(0).astype(int) + pl.sx(0) <= pl.cov(0)).all()
    h.close()


@pytest.mark.gpu
def test_pileup_changes_nothing_else(built):
    b = api.concat([api.synth(24, 8, 1200, seed=71), api.synth(8, (2, 40), (300, 3000), seed=72)])
    fields = ("status", "seq_len", "seq", "qual", "raw_qv", "rq", "np_", "ec", "iters", "n_windows", "fn", "rn")
    for kin in (0, 1):
        opts = api.default_opts(); opts.hifi_kinetics = kin
        h = api.Handle(0, opts=opts)
        plain = h.consensus(b)
        res, pl = h.consensus_pileup(b)
        for f in fields:
            assert np.array_equal(getattr(plain, f), getattr(res, f)), (kin, f)
        if kin:
            for z in range(b.n_zmw):
                assert np.array_equal(plain.kinetics(z), res.kinetics(z)), z
        for z in range(b.n_zmw):                                   # the consensus is the concatenation of the cores the planes describe
            assert len(pl.cov(z)) == res.seq_len[z] and int(pl.sa(z)[0::2].sum()) == res.seq_len[z]
        h.close()


@pytest.mark.gpu
def test_submit_pileup_equals_the_synchronous_call(built):
    batches = [api.synth(16, 6 + k, 900, seed=80 + k) for k in range(5)]
    h = api.Handle(0)
    want = [h.consensus_pileup(b) for b in batches]
    tickets, outs = [], []
    for b in batches:                                              # five tickets on three slots: tickets 0 and 1 are retired by slot reuse
        res = api.Results.allocate(b, pinned=True)
        pl = api.Pileup.allocate(res, pinned=True)
        tickets.append(h.submit(b, res, pileup=pl)); outs.append((res, pl))
    for t in tickets[2:]:
        while not h.poll(t):
            pass
    for (res, pl), (wres, wpl), b in zip(outs, want, batches):
        for z in range(b.n_zmw):
            assert np.array_equal(res.sequence(z), wres.sequence(z))
            assert np.array_equal(pl.cov(z), wpl.cov(z)) and np.array_equal(pl.sm(z), wpl.sm(z)) and np.array_equal(pl.sx(z), wpl.sx(z)), z
    # a plain submit on a slot that carried planes writes none
    res = api.Results.allocate(batches[0], pinned=True)
    h.wait(h.submit(batches[0], res))
    assert all(np.array_equal(res.sequence(z), want[0][0].sequence(z)) for z in range(batches[0].n_zmw))
    h.close()


@pytest.mark.gpu
def test_several_polish_launches(built, tmp_path):
    """the planes do not depend on how the window slots are cut into launches (CCSX_POLISH_MAX_BLOCKS: a test hook of the library)"""
    b = api.synth(48, 8, 2000, seed=91)
    h = api.Handle(0)
    res, pl = _parity(h, b, range(0, 48, 6))
    h.close()
    out = tmp_path / "p.npz"
    code = ("import sys; sys.path.insert(0, %r); import numpy as np; from ccs_amd import api\n"
            "b = api.synth(48, 8, 2000, seed=91); h = api.Handle(0); r, p = h.consensus_pileup(b)\n"
            "np.savez(%r, seq=r.seq, cov=p.coverage, sm=p.matches, sx=p.mismatches); h.close()\n") % (ROOT, str(out))
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, CCSX_POLISH_MAX_BLOCKS="40"), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    got = np.load(out)
    for z in range(b.n_zmw):
        o, n = int(res.seq_off[z]), int(res.seq_len[z])
        for k, want in (("seq", res.seq), ("cov", pl.coverage), ("sm", pl.matches), ("sx", pl.mismatches)):
            assert np.array_equal(got[k][o:o + n], want[o:o + n]), (z, k)


@pytest.mark.gpu
def test_pileup_at_scale(built):
    b = api.synth(16384, 10, 10000, seed=41)
    h = api.Handle(0)
    res, pl = h.consensus_pileup(b)
    assert (res.status == 0).mean() > 0.95
    for z in range(0, b.n_zmw, 97):
        if res.seq_len[z] == 0:
            continue
        cov, sm, sx = pl.cov(z).astype(int), pl.sm(z).astype(int), pl.sx(z).astype(int)
        assert (sm + sx <= cov).all() and cov.max() <= 10 and (sm.mean() > 0.8 * cov.mean())
    # coverage is constant over each window's core
    for z in range(0, 64):
        if res.seq_len[z] == 0:
            continue
        tpl, meta, _, _ = h.stage_polished(z)
        cov, p = pl.cov(z), 0
        for w, (J, cs, ce) in enumerate(meta):
            assert (cov[p:p + ce - cs] == cov[p]).all(), (z, w)
            assert np.array_equal(res.sequence(z)[p:p + ce - cs], tpl[w, cs:ce]), (z, w)   # the sequence is the templates' cores
            p += ce - cs
        assert p == res.seq_len[z]
    ref = pileup_ref.pileup_zmws(pileup_ref.collect_stage(h, b, range(16)))
    for z, (cov, sm, sx) in zip(range(16), ref):
        assert np.array_equal(pl.cov(z), cov) and np.array_equal(pl.sm(z), sm) and np.array_equal(pl.sx(z), sx), z
    h.close()


def _ccs(*args, check=True):
    return subprocess.run([CCS, *map(str, args)], capture_output=True, text=True, check=check, timeout=600)


@pytest.mark.gpu
def test_cli_pileup_summary(built, tmp_path):
    bam = tmp_path / "s.subreads.bam"
    _ccs("--write-synthetic", "9,8,700,37", bam)
    batch = api.synth(9, 8, 700, seed=37, first_zmw_id=1000)
    h = api.Handle(0)
    res, pl = h.consensus_pileup(batch)
    h.close()
    ok = [z for z in range(9) if res.status[z] == 0]
    out, plain = tmp_path / "p.hifi.bam", tmp_path / "n.hifi.bam"
    _ccs(bam, out, "--pileup-summary", "--suppress-reports", "--batch-size", 4, "--gpus", "0,0", "--workers-per-gpu", 2)
    _ccs(bam, plain, "--suppress-reports")
    _, recs = bam_util.read_bam(out)
    assert len(recs) == len(ok) > 0
    for rec, z in zip(recs, ok):
        t = rec["tags"]
        assert np.array_equal(rec["seq"], res.sequence(z))
        assert t["sa"].dtype == np.uint32 and np.array_equal(t["sa"], pl.sa(z))
        assert np.array_equal(t["sm"], pl.sm(z)) and np.array_equal(t["sx"], pl.sx(z))
    # the three tags are the records' last: without them the records are byte for byte those of a run without the flag
    _, raw = bam_util.read_bam_raw_records(out)
    _, raw0 = bam_util.read_bam_raw_records(plain)
    assert len(raw) == len(raw0)
    for r, r0, rec in zip(raw, raw0, recs):
        n, nsa = len(rec["seq"]), len(rec["tags"]["sa"])
        tail = (8 + 4 * nsa) + 2 * (8 + n)
        assert r[4:-tail] == r0[4:] and int.from_bytes(r[:4], "little") - tail == int.from_bytes(r0[:4], "little")
    # with --by-strand, --hifi-kinetics and --qv-binning: every strand record carries its own planes
    both = tmp_path / "s.hifi.bam"
    _ccs(bam, both, "--pileup-summary", "--by-strand", "--hifi-kinetics", "--qv-binning", "--min-rq", 0.9, "--suppress-reports")
    _, recs2 = bam_util.read_bam(both)
    assert len(recs2) > 0
    for r in recs2:
        t = r["tags"]
        n = len(r["seq"])
        assert len(t["sm"]) == len(t["sx"]) == len(t["ip"]) == n and int(t["sa"][0::2].sum()) == n
        cov = api.unrle(t["sa"]).astype(int)
        assert (t["sm"].astype(int) + t["sx"] <= cov).all() and cov.max() <= 8

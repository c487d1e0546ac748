"""The cell-tag rule on the CPU (DESIGN.md §2 "Cell-tag rule"): the restatement's candidates against the brute force from the definition, its table against the
library's, ccsx_cell_reads_host against tests/cell_ref.py on the limit set (on poisoned planes, and again with the reads in reverse order), the tie to the cDNA
rule, the structs against the header, and every refusal of ccsx_cell_check and of the whitelist's builder."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from ccs_amd import api
import cdna_ref
import cell_ref as R
from test_cdna_ref import _bad_sets_and_opts, _mk_opts, _set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = R.limit_cases()
NAMES = [c[0] for c in CASES]
LISTED = [i for i, c in enumerate(CASES) if c[5] is not None]


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


def poisoned(n):
    """a report whose every byte is 0xA5: what the rule does not write shows"""
    rep = api.CellReport.allocate(n)
    for k in R.FIELDS:
        getattr(rep, k).view(np.uint8)[...] = 0xA5
    return rep


def test_the_candidates_equal_the_bruteforce_on_random_fields():
    """fields 0, 1 and 2 edits away from a member of a dense whitelist (4 000 of the 65 536 8-mers: strangers are reached all the time), with and without indels
    and the base behind the field"""
    rng = np.random.default_rng(11)
    wl = np.array(R.whitelist(rng, 4000, 8), np.int64)
    index = {tuple(w.tolist()): k for k, w in enumerate(wl)}
    seen = set()
    for _ in range(1500):
        f = list(wl[rng.integers(0, len(wl))])
        for _ in range(int(rng.integers(0, 3))):
            kind, i = rng.integers(0, 3), int(rng.integers(0, len(f)))
            if kind == 0:
                f[i] = int(rng.integers(0, 4))
            elif kind == 1:
                del f[i]
            else:
                f.insert(i, int(rng.integers(0, 4)))
        f = (f + rng.integers(0, 4, 9).tolist())[:9]
        raw, nxt, indels = tuple(int(v) for v in f[:8]), int(f[8]) if rng.random() < 0.7 else None, int(rng.random() < 0.7)
        got = R.correct(raw, nxt, indels, index)
        assert got == R.correct_brute(raw, nxt, indels, wl), (raw, nxt, indels)
        seen.add((got[0], got[3]))
    assert seen >= {(R.EXACT, 0), (R.CORRECTED, 1), (R.CORRECTED, 2), (R.CORRECTED, 3), (R.AMBIGUOUS, 0), (R.ABSENT, 0)}


@pytest.mark.parametrize("i", LISTED, ids=[NAMES[i] for i in LISTED])
def test_the_restatement_equals_the_bruteforce_on_the_limit_set(i):
    name, S, roles, o, d, wl, reads = CASES[i]
    assert R.diff(R.cell_reads(S, roles, reads, d, wl, brute=True, **o), R.expected(i)) == [], name


def test_the_limit_set_holds_what_it_is_for():
    E = {name: R.expected(i) for i, name in enumerate(NAMES)}
    for n in (1, 2, 1000, 4096):
        w = E[f"wl{n}"]
        assert w["tag"].tolist() == [R.EXACT] * 4 + [R.CORRECTED] * 6 + [R.ABSENT] * 2 and w["bc"][:4].tolist() == [0, 0, n - 1, n - 1] and (w["bc"][4:10] == n // 2).all()
        assert (w["strand"] == [0, 1] * 6).all() and (w["cls"] == R.FULL_LENGTH).all() and (w["tag_clip"] == 28).all() and (w["polya_len"] == 30).all()
    assert R.n_slots(4096) == 8192 and R.n_slots(1) == 64 and R.n_slots(32) == 64 and R.n_slots(33) == 128
    assert (E["raw"]["tag"] == R.RAW).all() and (E["raw"]["bc"] == -1).all() and (E["raw"]["bc_raw"] == E["wl4096"]["bc_raw"]).all()
    w = E["wl_AT"]
    assert w["bc_raw"][:4].tolist() == [0, 0, 0xFFFFFFFF, 0xFFFFFFFF] and w["bc"].tolist() == [0, 0, 1, 1] * 2
    for name, n, home in (("run8", 8, 5), ("run70", 70, 100), ("wrap8", 8, 61)):
        wl = CASES[NAMES.index("table_" + name)][5]
        t = R.table_of(wl)
        taken = np.flatnonzero(t)
        assert sorted(taken.tolist()) == sorted((home + k) % len(t) for k in range(n)) and (R.first_slot([R.pack(x) for x in wl], len(t)) == home).all()
        w = E["table_" + name]
        assert w["tag"].tolist() == [R.EXACT] * 4 + [R.CORRECTED] * 4 + [R.ABSENT] * 2 and w["bc"][:8].tolist() == [0, 0, n - 1, n - 1] * 2
    w = E["kinds"]
    assert w["kind"][0::2].tolist() == [1, 1, 1, 2, 2, 1, 3, 3, 1] and w["shift"][0::2].tolist() == [0, 0, 0, -1, -1, 0, 1, 1, 0] and (w["bc"] == 20).all()
    assert w["tag_clip"][0::2].tolist() == [28, 28, 28, 27, 27, 28, 29, 29, 28]
    w = E["kinds_noindels"]
    assert w["tag"][0::2].tolist() == [R.CORRECTED] * 3 + [R.ABSENT] * 2 + [R.CORRECTED] + [R.ABSENT] * 2 + [R.CORRECTED] and (w["shift"] == 0).all()
    w = E["homopolymer"]
    assert w["kind"].tolist() == [1, 1, 2, 2, 0, 0] and w["shift"].tolist() == [0, 0, -1, -1, 0, 0] and w["bc"].tolist() == [3, 3, 0, 0, -1, -1]
    w = E["ambiguous"]
    assert (w["tag"] == R.AMBIGUOUS).all() and (w["bc"] == 4).all() and (w["bc_hi"] == 31).all() and (w["shift"] == 0).all()
    for name in NAMES:
        if name.startswith("design_"):
            w, d = E[name], CASES[NAMES.index(name)][4]
            assert (w["strand"] == [0, 1] * (len(w["strand"]) // 2)).all() and (w["cls"] == R.FULL_LENGTH).all(), name
            if d["bc_len"] == 0:
                assert (w["tag"] == R.RAW).all() and (w["tag_clip"] == d["umi_len"]).all()
            elif d["bc_len"] == 16:
                assert w["tag"][0] == R.EXACT and (w["tag"][2:] == R.CORRECTED).all() and w["shift"][4:].tolist() == [-1, -1, 1, 1], (name, w["tag"], w["shift"])
            else:                                                   # (8 bases: a lost or a gained base may reach a second barcode of the four)
                assert w["tag"][0] == R.EXACT and w["tag"][2] == R.CORRECTED and np.isin(w["tag"][4:], (R.CORRECTED, R.AMBIGUOUS)).all(), (name, w["tag"])
    for s in (0, 1):
        w = E[f"lengths_s{s}"]
        assert w["tag"][0::2].tolist() == [R.NONE, R.EXACT, R.EXACT, R.ABSENT, R.CORRECTED, R.NONE, R.CORRECTED, R.CORRECTED]
        assert w["shift"][0::2].tolist() == [0, 0, 0, 0, 1, 0, -1, 1] and w["cls"][0::2].tolist() == [R.SHORT] * 2 + [R.FULL_LENGTH] + [R.SHORT] * 4 + [R.FULL_LENGTH]
        assert w["tag_clip"][8] == 29 and w["end"][8] == 0                                     # T + 1 bases, the shift takes the last: ins_len' = 0
    a, c = E["polya_shift_A"], E["polya_shift_C"]
    assert a["shift"].tolist() == c["shift"].tolist() == [0, 0, 0, 0, -1, -1, 1, 1, -1, -1] * 2
    assert a["cls"][:10].tolist() == [R.FULL_LENGTH] * 10 and c["cls"][8:10].tolist() == [R.NO_TAIL] * 2 and a["cls"][18:].tolist() == [R.FULL_LENGTH] * 2
    assert a["polya_len"][:8].tolist() == c["polya_len"][:8].tolist() == [20] * 8               # the shift is the molecule's: the scan starts at the tail
    assert a["polya_len"][8] == 22 and c["polya_len"][8] == 0     # the wrong shift leaves the UMI's last two bases to the scan: x A . tail, or x C . tail
    w = E["internal_in_fields"]
    assert w["cls"].tolist() == [R.FULL_LENGTH] * 2 + [R.CONCATEMER] * 2 and w["n_internal"].tolist() == [0, 0, 1, 1]
    w = E["classes"]
    assert w["cls"].tolist() == [0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 4, 4] and (w["tag"][:12] == R.NONE).all() and (w["bc"][:12] == -1).all()
    w = E["sizes"]
    assert [len(r) for r in CASES[NAMES.index("sizes")][6]][:3] == [0, 24, 3001] and w["tested"][0] == 0 and w["tag"].tolist() == [0, 0, 3, 3, 2, 2]
    assert [len(CASES[NAMES.index(n)][6]) for n in ("n0", "n1", "n257")] == [0, 1, 257]


def test_the_table_and_the_slot_equal_the_restatement(built):
    rng = np.random.default_rng(5)
    keys = rng.integers(0, 1 << 32, 200, dtype=np.uint64)
    for slots in (64, 256, 1 << 24):
        assert [api.cell_slot(int(k), slots) for k in keys] == R.first_slot(keys, slots).tolist()
    for i in LISTED:
        wl = CASES[i][5]
        if len(wl) <= 1000:
            w = api.CellWhitelist(wl)
            assert w.table.tolist() == R.table_of(wl).tolist(), NAMES[i]
            w.close()


@pytest.mark.parametrize("i", range(len(CASES)), ids=NAMES)
def test_the_host_rule_equals_the_restatement(built, i):
    name, S, roles, o, d, wl, reads = CASES[i]
    pset, w = api.CdnaPrimers.from_codes(S, roles), api.CellWhitelist(wl) if wl is not None else None
    rep = api.cell_reads_host(pset, list(reads), _design(d), w, _opts(o), poisoned(len(reads)))
    assert R.diff(rep, R.expected(i)) == [], (name, R.diff(rep, R.expected(i)))
    rep = api.cell_reads_host(pset, list(reads)[::-1], _design(d), w, _opts(o), poisoned(len(reads)))
    assert R.diff(rep, R.reversed_order(R.expected(i))) == [], (name, "reversed", R.diff(rep, R.reversed_order(R.expected(i))))


@pytest.mark.parametrize("side", [0, 1])
def test_without_the_fields_the_cdna_planes_are_the_cdna_rule_on_the_cut_reads(built, side):
    """the tie to the existing rule: molecules that carry no fields, under a design of T = 28 bases and no whitelist; the cDNA planes equal ccsx_cdna_reads_host on
    the same reads with the T bases behind the tag end's primer cut out (coordinates behind the cut moved by T)"""
    rng = np.random.default_rng(31 + side)
    S = R.random_set(rng, 2, [25])
    pset, d = api.CdnaPrimers.from_codes(S, [0, 1]), dict(R.DESIGN, side=side)
    shapes = ((150, 30), (90, 0), (60, 25), (300, 40), (40, 30))
    reads = R.both([cdna_ref.mol(S[0], S[1], R.body(rng, n), t) for n, t in shapes])          # no fields: the rule takes 28 bases of the insert or of the tail
    reads += R.both([R.cmol(d, S[0], S[1], R.body(rng, n), R.rand(rng, 16), R.rand(rng, 12), t) for n, t in shapes])   # 28 bases that are nobody's barcode
    o = _opts(dict(R.DEFAULTS, window=25))                         # (the windows hold the primers alone: the cut changes no window)
    got = api.cell_reads_host(pset, reads, _design(d), None, o)
    cut, moved = [], []
    for z, c in enumerate(reads):
        e_t = 0 if int(got.strand[z]) == side else 1
        assert got.tag[z] == R.RAW and got.tag_clip[z] == 28 and got.clip[z].tolist() == [25, 25]
        cut.append(np.concatenate([c[:25], c[25 + 28:]]) if e_t == 0 else np.concatenate([c[: len(c) - 25 - 28], c[len(c) - 25:]]))
        moved.append(28 if e_t == 0 else 0)
    want = api.cdna_reads_host(pset, cut, o)
    moved = np.array(moved)
    for k in cdna_ref.FIELDS:
        w = getattr(want, k).copy()
        if k in ("start", "end"):
            w = np.where(want.cls >= cdna_ref.CONCATEMER, w + moved, w)
        if k == "first_internal":
            w = np.where(w >= 0, w + moved, w)
        assert np.array_equal(getattr(got, k), w), (k, getattr(got, k), w)
    assert set(want.cls.tolist()) >= {cdna_ref.FULL_LENGTH, cdna_ref.NO_TAIL, cdna_ref.SHORT}


def test_structs_match_the_header(built, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ccsx.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %d %d %d\\n", '
                   'sizeof(ccsx_cell_design), offsetof(ccsx_cell_design, indels), offsetof(ccsx_cell_design, reserved), sizeof(ccsx_cell_report), '
                   'offsetof(ccsx_cell_report, tag), offsetof(ccsx_cell_report, umi), offsetof(ccsx_cell_report, tag_clip), CCSX_CELL_MAX_FIELD, '
                   'CCSX_CELL_MAX_WHITELIST, CCSX_CELL_ABSENT);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    D, Rp = api.CellDesign, api.CCellReport
    assert got == [C.sizeof(D), D.indels.offset, D.reserved.offset, C.sizeof(Rp), Rp.tag.offset, Rp.umi.offset, Rp.tag_clip.offset, api.CELL_MAX_FIELD,
                   api.CELL_MAX_WHITELIST, api.CELL_ABSENT]
    assert got[0] == 32 and got[3] == C.sizeof(api.CCdnaReport) + 8 * 8
    L = api.lib()
    assert L.ccsx_cell_rule_version() == 1 and L.ccsx_abi_version() == 6 and L.ccsx_spec_version() == 8 and L.ccsx_cdna_rule_version() == 1
    d = api.CellDesign.default()
    assert {k: getattr(d, k) for k in R.DESIGN} == R.DESIGN and list(d.reserved) == [0, 0, 0]
    assert R.CELL_PLANES == api.CELL_PLANES and len(api.CELL_NAMES) == 6


def test_the_whitelist_builder_refuses(built):
    L = api.lib()
    codes = np.zeros((4, 16), np.uint8)
    codes[:, 0] = [0, 1, 2, 1]
    p = codes.ctypes.data_as(C.POINTER(C.c_uint8))
    for args, msg in (((None, 4, 16), "null codes"), ((p, 0, 16), "n outside 1 .. 2^23"), ((p, (1 << 23) + 1, 16), "n outside 1 .. 2^23"),
                      ((p, 4, 0), "bc_len outside 1 .. 16"), ((p, 4, 17), "bc_len outside 1 .. 16"), ((p, 4, 16), "barcodes 1 and 3 are the same")):
        assert not L.ccsx_cell_whitelist_create(*args) and msg.encode() in L.ccsx_last_error(), (msg, L.ccsx_last_error())
    codes[3, 0] = 4
    assert not L.ccsx_cell_whitelist_create(p, 4, 16) and b"barcode 3: code above 3" in L.ccsx_last_error()
    with pytest.raises(RuntimeError, match="barcodes 0 and 2 are the same"):
        api.CellWhitelist(["ACGTACGT", "ACGTACGA", "acgtacgt"])
    with pytest.raises(ValueError, match="bc_len = 8"):
        api.CellWhitelist(["ACGTACGT", "ACGT"])
    assert L.ccsx_cell_whitelist_info(None, None, None, None, None) < 0 and b"null whitelist" in L.ccsx_last_error()
    L.ccsx_cell_whitelist_destroy(None)


@pytest.mark.parametrize("entry", ["ccsx_cell_reads_host", "ccsx_cell_reads"])
def test_the_calls_refuse_bad_arguments(built, entry):
    """one check, ccsx_cell_check, for both forms: everything ccsx_cdna_check refuses, then the design, the whitelist and the report; no handle is needed to be
    refused, and with valid arguments the handle is what is missing"""
    L = api.lib()
    reads = [np.zeros(30, np.uint8), np.zeros(0, np.uint8)]
    wl8 = api.CellWhitelist(["ACGTACGT"])

    def call(pset=None, opts=None, design=None, wl=None, rep=None, null=(), poke=None, poke_rep=None):
        args, _, keep = api._cell_reads_args(pset if pset is not None else _set([16, 16]), opts, design, wl, reads, rep)
        args = list(args)
        for k in null:
            args[k] = None
        if poke:
            poke(keep)
        if poke_rep:
            poke_rep(keep[5])
        return getattr(L, entry)(*(([None] if entry == "ccsx_cell_reads" else []) + args))

    def design(**kw):
        return _design({**R.DESIGN, **kw})

    for msg, s, kw in _bad_sets_and_opts():
        assert call(s, _mk_opts(kw)) < 0 and msg.encode() in L.ccsx_last_error() and entry.encode() in L.ccsx_last_error(), (msg, L.ccsx_last_error())
    assert call(null=(0,)) < 0 and b"null cdna set" in L.ccsx_last_error()
    assert call(null=(8,)) < 0 and b"null cell report" in L.ccsx_last_error()
    assert call(null=(2,)) < 0 and b"null cell design" in L.ccsx_last_error()
    assert call(rep=api.CellReport.allocate(3)) < 0 and b"sized for another batch" in L.ccsx_last_error()
    for kw in (dict(umi_len=0, bc_len=0),):
        assert call(design=design(**kw)) < 0 and b"umi_len + bc_len must be at least 1" in L.ccsx_last_error()
    for kw in (dict(umi_len=17), dict(bc_len=17), dict(umi_len=-1), dict(bc_len=-1)):
        assert call(design=design(**kw)) < 0 and b"a field length outside 0 .. 16" in L.ccsx_last_error(), kw
    for kw in (dict(side=2), dict(side=-1), dict(bc_first=2), dict(indels=2), dict(indels=-1)):
        assert call(design=design(**kw)) < 0 and b"side, bc_first and indels are 0 or 1" in L.ccsx_last_error(), kw
    for k in range(3):
        d = design()
        d.reserved[k] = 1
        assert call(design=d) < 0 and b"cell design: reserved must be 0" in L.ccsx_last_error()
    assert call(wl=wl8) < 0 and b"the whitelist's barcodes have 8 bases, the design's 16" in L.ccsx_last_error()
    for k in api.CdnaReport.FIELDS:
        assert call(poke_rep=lambda r, k=k: setattr(r.cdna, k, None)) < 0 and b"cdna report arrays missing" in L.ccsx_last_error(), k
    for k in api.CELL_PLANES:
        assert call(poke_rep=lambda r, k=k: setattr(r, k, None)) < 0 and b"cell report arrays missing" in L.ccsx_last_error(), k
    for k in (4, 5, 6):
        assert call(null=(k,)) < 0 and b"null argument" in L.ccsx_last_error(), k

    def neg(keep):
        keep[3][0] = -1
    assert call(poke=neg) < 0 and b"read 0: negative seq_off" in L.ccsx_last_error()
    for d, w in ((design(), None), (design(umi_len=16, bc_len=16, side=0, bc_first=0, indels=0), None), (design(umi_len=0, bc_len=8), wl8), (design(umi_len=1, bc_len=0), None)):
        rc = call(design=d, wl=w)
        if entry == "ccsx_cell_reads":
            assert rc < 0 and b"null argument" in L.ccsx_last_error(), L.ccsx_last_error()
        else:
            assert rc == 0, L.ccsx_last_error()

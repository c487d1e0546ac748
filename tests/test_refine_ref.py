"""The polisher hand-back without a GPU (DESIGN.md §2 "Polisher hand-back"): the exports, the table of error probabilities, the structs against the header, and
the numpy restatement of the rule (tests/refine_ref.py) against its brute force on every code of the table."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

import refine_ref as R
from ccs_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ccsx_refine_tiles_init", "ccsx_refine_rule_version", "ccsx_refine_perr", "ccsx_refine_batch", "ccsx_submit_refine")


def test_exports_and_rule_version(built):
    L = api.lib()
    assert set(NAMES) <= set(api.EXPORTS) and all(hasattr(L, k) for k in NAMES)
    assert L.ccsx_refine_rule_version() == 1 and L.ccsx_abi_version() == 6 and L.ccsx_spec_version() == 8
    t = api.CRefineTiles()
    C.memset(C.byref(t), 0xff, C.sizeof(t))
    L.ccsx_refine_tiles_init(C.byref(t))
    assert (t.n_tiles, t.stride, t.reserved0, t.tile_zmw, t.new_qual, list(t.reserved)) == (0, 128, 0, None, None, [0, 0])
    codes = [api.REFINE_SKIPPED, api.REFINE_RESCORED, api.REFINE_REFINED, api.REFINE_BAD_TILE, api.REFINE_BAD_ORDER, api.REFINE_BAD_SYMBOL, api.REFINE_TOO_LONG,
             api.REFINE_EMPTY, api.REFINE_BAD_BACKBONE, api.REFINE_BAD_LIST]
    assert codes == [R.SKIPPED, R.RESCORED, R.REFINED, R.BAD_TILE, R.BAD_ORDER, R.BAD_SYMBOL, R.TOO_LONG, R.EMPTY, R.BAD_BACKBONE, R.BAD_LIST] == [0, 1, 2] + list(range(-1, -8, -1))
    assert sorted(api.REFINE_CODE_NAMES) == sorted(codes)


def test_perr_table(built):
    L = api.lib()
    for q in range(94):
        assert L.ccsx_refine_perr(q) == math.floor(10 ** (-q / 10) * 2 ** 32 + 0.5), q
    assert L.ccsx_refine_perr(0) == 2 ** 32 and L.ccsx_refine_perr(-1) == 0 and L.ccsx_refine_perr(94) == 0
    assert api.refine_perr_table().dtype == np.uint64 and int(api.refine_perr_table()[10]) == 429496730


def test_structs_match_the_header(built, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ccsx.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d %d %d %d %d %d %d\\n", '
                   'sizeof(ccsx_refine_tiles), offsetof(ccsx_refine_tiles, stride), offsetof(ccsx_refine_tiles, tile_zmw), offsetof(ccsx_refine_tiles, new_len), '
                   'offsetof(ccsx_refine_tiles, new_qual), offsetof(ccsx_refine_tiles, reserved), sizeof(ccsx_refine_report), offsetof(ccsx_refine_report, code), '
                   'offsetof(ccsx_refine_report, rq_merged), offsetof(ccsx_refine_report, qual_merged), sizeof(ccsx_results), '
                   'CCSX_REFINE_SKIPPED, CCSX_REFINE_RESCORED, CCSX_REFINE_REFINED, CCSX_REFINE_BAD_TILE, CCSX_REFINE_BAD_ORDER, CCSX_REFINE_BAD_SYMBOL, '
                   'CCSX_REFINE_TOO_LONG, CCSX_REFINE_EMPTY, CCSX_REFINE_BAD_BACKBONE, CCSX_REFINE_BAD_LIST);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    T, Q = api.CRefineTiles, api.CRefineReport
    assert got[:11] == [C.sizeof(T), T.stride.offset, T.tile_zmw.offset, T.new_len.offset, T.new_qual.offset, T.reserved.offset, C.sizeof(Q), Q.code.offset,
                        Q.rq_merged.offset, Q.qual_merged.offset, C.sizeof(api.CResults)]
    assert got[0] == 80 and got[6] == 48
    assert got[11:] == [0, 1, 2, -1, -2, -3, -4, -5, -6, -7]


# ---------------------------------------------------------------- the restatement against the brute force
U = 8


def as_arrays(tiles):
    m = len(tiles)
    a = dict(tile_zmw=np.array([t[0] for t in tiles], np.int64), tile_start=np.array([t[1] for t in tiles], np.int64), tile_len=np.array([t[2] for t in tiles], np.int64),
             new_len=np.array([t[3] for t in tiles], np.int64), new_seq=np.zeros((m, U), np.uint8), new_qual=np.zeros((m, U), np.uint8))
    for g, t in enumerate(tiles):
        a["new_seq"][g, :len(t[4])], a["new_qual"][g, :len(t[5])] = t[4], t[5]
    return a


def both(bases, quals, caps, passes, backbone, tiles):
    perr = R.perr_table()
    off = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
    seq, qual = np.zeros(off[-1], np.uint8), np.zeros(off[-1], np.uint8)
    for z in range(len(bases)):
        seq[off[z]:off[z] + len(bases[z])], qual[off[z]:off[z] + len(bases[z])] = bases[z], quals[z]
    a = R.refine(off, [len(b) for b in bases], seq, qual, passes, backbone, as_arrays(tiles), U, perr)
    b = R.brute(bases, quals, caps, passes, backbone, tiles, U, [int(x) for x in perr])
    assert a["code"].tolist() == b["code"] and a["n_applied"].tolist() == b["n_applied"] and int(a["counts"][2]) == b["violations"]
    assert int(a["counts"][0]) == b["code"].count(2) and int(a["counts"][1]) == sum(b["n_applied"])
    for z in range(len(bases)):
        assert a["drafts"][z].tolist() == b["drafts"][z] and a["quals"][z].tolist() == b["quals"][z], z
        k = len(b["drafts"][z])
        want = np.float32(1.0 - b["sums"][z] / 4294967296.0 / k) if k else np.float32(0)
        assert a["rq_merged"][z].tobytes() == want.tobytes(), z
    return a


def molecule(rng, n):
    return rng.integers(0, 4, n).tolist(), rng.integers(0, 94, n).tolist()


def test_every_code_against_the_brute_force(built):
    rng = np.random.default_rng(5)
    mol = [molecule(rng, n) for n in (20, 20, 20, 20, 20, 20, 0, 20, 20, 3, 20)]
    bases, quals = [m[0] for m in mol], [m[1] for m in mol]
    caps = [24] * 11
    caps[9] = 3
    passes = [5] * 11
    backbone = [0, 4, 0, 0, 0, 0, 0, -1, 5, 0, 0]
    row = lambda k, s=1, q=30: ([s] * k, [q] * k)
    tiles = [
        (0, 0, 3, 3, *row(3)), (0, 3, 2, 0, [], []), (0, 5, 1, 5, *row(5, 2, 93)), (0, 17, 3, 4, *row(4, 3, 0)),   # REFINED: at 0, adjacent, deletion, growth, ending at L
        # ZMW 1: no tile (RESCORED)
        (2, 4, 2, 2, *row(2)), (2, 19, 2, 1, *row(1)),                         # BAD_TILE: start + len > L
        (3, 4, 4, 2, *row(2)), (3, 7, 2, 2, *row(2)),                          # BAD_ORDER: starts inside its predecessor
        (4, 4, 4, 3, [0, 1, 4], [0, 0, 0]),                                    # BAD_SYMBOL: code 4 at the last read entry
        (5, 2, 1, 6, *row(6)),                                                 # TOO_LONG: 20 + 5 > 24
        (6, 0, 1, 1, *row(1)),                                                 # SKIPPED: L = 0, its tile ignored
        (7, 0, 1, 1, *row(1)),                                                 # SKIPPED: backbone -1
        (8, 0, 1, 1, *row(1)),                                                 # BAD_BACKBONE
        (9, 0, 3, 0, [], []),                                                  # EMPTY: L' = 0
        (10, 5, 2, 2, [0, 1, 9], [5, 93, 94]),                                 # REFINED: the bad symbol lies beyond new_len
    ]
    a = both(bases, quals, caps, passes, backbone, tiles)
    assert a["code"].tolist() == [2, 1, -1, -2, -3, -4, 0, 0, -6, -5, 2] and a["counts"].tolist() == [2, 5, 0]
    assert a["new_len"].tolist() == [23, 20, 20, 20, 20, 20, 0, 0, 0, 3, 20]      # 20 + 0 - 2 + 4 + 1
    # the class with the smallest number wins: a ZMW with a bad tile, a tile out of order and a bad symbol; then one with the latter two
    t2 = [(0, 4, 4, 2, *row(2)), (0, 6, 30, 1, [7], [0]), (1, 4, 4, 2, *row(2)), (1, 6, 2, 1, [0], [94])]
    assert both(bases[:2], quals[:2], caps[:2], passes[:2], [0, 0], t2)["code"].tolist() == [-1, -2]
    # L' = C exactly is accepted, qual 94 refused, new_len above the stride and below 0 are bad tiles
    assert both(bases[:1], quals[:1], [24], [5], [0], [(0, 2, 1, 5, *row(5))])["code"].tolist() == [2]
    assert both(bases[:1], quals[:1], [24], [5], [0], [(0, 2, 1, 2, [0, 0], [0, 94])])["code"].tolist() == [-3]
    assert both(bases[:1], quals[:1], [40], [5], [0], [(0, 2, 1, U + 1, *row(U))])["code"].tolist() == [-1]
    assert both(bases[:1], quals[:1], [40], [5], [0], [(0, 2, 1, -1, [], [])])["code"].tolist() == [-1]
    # the list's order: one tile_zmw below its predecessor, one equal to n_zmw -> two violations, -7 for every staged ZMW, the others keep their codes
    bad = [tiles[4], tiles[0], (11, 0, 1, 1, *row(1))]
    a = both(bases, quals, caps, passes, backbone, bad)
    assert a["counts"].tolist() == [0, 0, 2] and a["code"].tolist() == [-7, -7, -7, -7, -7, -7, 0, 0, -6, -7, -7]
    assert all(a["drafts"][z].tolist() == bases[z] for z in (0, 2))

"""The two CPU references of the polisher hand-off (tests/handoff_ref.py) on hand-made windows whose cells are written out here, and against each other on
random segments.  No GPU."""
import numpy as np
import pytest

import handoff_ref as H

TPL = [0, 1, 3, 2, 0, 2, 1, 3]                    # ACTGAGCT: no repeated neighbour, not its own reverse complement
RC = [0, 2, 1, 3, 1, 0, 2, 3]                     # its reverse complement
INS_FWD = [0, 1, 3, 2, 1, 1, 0, 2, 1, 3]          # ACTG + CC + AGCT
INS_RC = [0, 2, 1, 3, 2, 2, 1, 0, 2, 3]           # the same read as a pass on the opposite strand sees it


def seq(a, n):
    return [a + r for r in range(n)]


# name -> (core, segment in the pass's own orientation, st, pw, ip, expected cells of the core)
CASES = {
    "forward, every base matches": ((2, 6), TPL, 0, seq(1, 8), None, [[3, 3, 0, 0], [2, 4, 0, 0], [0, 5, 0, 0], [2, 6, 0, 0]]),
    "forward, a mismatch keeps its column": ((2, 6), [0, 1, 3, 1, 0, 2, 1, 3], 0, seq(1, 8), None, [[3, 3, 0, 0], [1, 4, 0, 0], [0, 5, 0, 0], [2, 6, 0, 0]]),
    "forward, column 3 deleted": ((2, 6), [0, 1, 3, 0, 2, 1, 3], 0, seq(10, 7), None, [[3, 12, 0, 0], [4, 0, 0, 0], [0, 13, 0, 0], [2, 14, 0, 0]]),
    "forward, two bases inserted before column 4": ((2, 6), INS_FWD, 0, seq(20, 10), seq(100, 10),
                                                    [[3, 22, 102, 0], [2, 23, 103, 0], [0, 26, 106, 2], [2, 27, 107, 0]]),
    "opposite strand, every base matches": ((2, 6), RC, 1, seq(30, 8), None, [[3, 35, 0, 0], [2, 34, 0, 0], [0, 33, 0, 0], [2, 32, 0, 0]]),
    "opposite strand, two bases inserted before column 4": ((2, 6), INS_RC, 1, seq(40, 10), seq(50, 10),
                                                            [[3, 47, 57, 0], [2, 46, 56, 0], [0, 43, 53, 2], [2, 42, 52, 0]]),
    "forward, two leading bases before column 0": ((0, 4), [2, 2] + TPL, 0, seq(60, 10), None, [[0, 62, 0, 2], [1, 63, 0, 0], [3, 64, 0, 0], [2, 65, 0, 0]]),
    "forward, the walk reaches row 0 with two columns left": ((0, 4), TPL[2:], 0, seq(70, 6), None, [[4, 0, 0, 0], [4, 0, 0, 0], [3, 70, 0, 0], [2, 71, 0, 0]]),
    "an empty segment is usable": ((2, 6), [], 0, [], None, [[4, 0, 0, 0]] * 4),
    "64 bases are not": ((2, 6), [(7 * i + i // 3) & 3 for i in range(64)], 0, seq(1, 64), None, [[5, 0, 0, 0]] * 4),
}


@pytest.mark.parametrize("name", list(CASES))
def test_hand_made_windows(name):
    (cs, ce), seg, st, pw, ip, want = CASES[name]
    want = np.array(want, np.uint8)
    brute = H.brute_window_cells(TPL, cs, ce, seg, st, pw, ip)
    assert np.array_equal(brute, want), (name, brute.tolist())
    z, passes, kin = H.single_window(TPL, cs, ce, [(seg, st, pw, ip)])
    got = H.zmw_cells([z], [passes], [kin])[0]
    assert got.shape == (1, ce - cs, 4) and np.array_equal(got[0], want), (name, got.tolist())


def test_rows_and_tiles_of_a_hand_made_batch():
    """two ZMWs of one window each, the second pass of the first invalid; tiles of 16 over consensus lengths 4 and 0"""
    (cs, ce), seg, st, pw, ip, want = CASES["forward, column 3 deleted"]
    z, _, kin = H.single_window(TPL, cs, ce, [(seg, st, pw, ip), (TPL, 0, seq(1, 8), None), (RC, 1, seq(30, 8), None)])
    z.reads[1] = z.reads[1][:2] + (False,) + z.reads[1][3:]
    empty = H.Zmw([], [], 0, [])
    quals = [np.array([10, 20, 30, 40], np.uint8), np.zeros(0, np.uint8)]
    out = H.handoff_batch([z, empty], quals, [kin, []], 16, 3, 26, 5)
    assert out["counts"].tolist() == [1, 1]                                    # 100 < 26 x 4
    assert (out["tile_zmw"][0], out["tile_start"][0], out["tile_len"][0], out["tile_qsum"][0], out["tile_rows"][0]) == (0, 0, 4, 100, 2)
    assert out["row_pass"].tolist() == [[0, 2, 255]] and out["row_strand"].tolist() == [[0, 1, 0]]
    c = out["cells"][0]
    assert np.array_equal(c[0, :4], np.array(want, np.uint8)) and np.array_equal(c[1, :4], np.array(CASES["opposite strand, every base matches"][5], np.uint8))
    assert (c[2, :, 0] == 5).all() and (c[:, 4:, 0] == 5).all() and not c[:, :, 1:][c[:, :, 0] >= 4].any()
    assert H.handoff_batch([z, empty], quals, [kin, []], 16, 3, 25, 5)["counts"].tolist() == [1, 0]      # 100 < 25 x 4 is false
    assert H.handoff_batch([z, empty], quals, [kin, []], 16, 3, 94, 0)["counts"].tolist() == [1, 1]      # selected, but no room: nothing written
    assert len(H.handoff_batch([z, empty], quals, [kin, []], 16, 3, 94, 0)["tile_zmw"]) == 0


def test_restatement_and_brute_force_agree_on_random_segments():
    rng = np.random.default_rng(11)
    n_ins = n_del = n_lead = n_unusable = n_rev = 0
    for _ in range(300):
        J = int(rng.integers(4, 32))
        tpl = rng.integers(0, 4, J)
        cs = int(rng.integers(0, 3)); ce = int(rng.integers(max(cs + 1, J - 3), J + 1))
        st = int(rng.integers(0, 2))
        read = []
        for b in tpl:                                                          # the template through a noisy channel, in SEQ orientation
            u = rng.random()
            if u < 0.08:
                continue
            read.append(int(b) if u > 0.16 else int(rng.integers(0, 4)))
            while rng.random() < 0.12:
                read.append(int(rng.integers(0, 4)))
        if rng.random() < 0.1:
            read = list(rng.integers(0, 4, int(rng.integers(20, 60)))) + read      # a long insertion
        if rng.random() < 0.25:
            read = list(rng.integers(0, 4, int(rng.integers(1, 4)))) + read        # a few leading bases
        read = np.array(read[:70], np.int64)
        seg = (3 - read[::-1]) if st else read
        pw = rng.integers(1, 256, len(seg)); ip = rng.integers(0, 256, len(seg)) if rng.random() < 0.7 else None
        brute = H.brute_window_cells(tpl, cs, ce, seg, st, pw, ip)
        z, passes, kin = H.single_window(tpl, cs, ce, [(seg, st, pw, ip)])
        got = H.zmw_cells([z], [passes], [kin])[0][0]
        assert np.array_equal(got, brute), (tpl.tolist(), seg.tolist(), st, got.tolist(), brute.tolist())
        n_ins += int((brute[:, 3] > 0).any()); n_del += int((brute[:, 0] == 4).any()); n_unusable += int((brute[:, 0] == 5).any())
        n_lead += int(brute[0, 0] < 4 and brute[0, 3] > 0 and cs == 0); n_rev += st
    assert min(n_ins, n_del, n_lead, n_unusable, n_rev) >= 5, (n_ins, n_del, n_lead, n_unusable, n_rev)

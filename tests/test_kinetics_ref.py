"""tests/kinetics_ref.py (the plain restatement of DESIGN.md §2 "HiFi kinetics" and of the stitch) against the second independent implementation, the oracle,
before it judges the kernels in tests/test_kinetics_gpu.py; and the `rq` tolerance of that module, measured here.  CPU only.

rq: over the oracle's results for every batch of tests/kinetics_lab.py the largest |(1 - rq_oracle) - (1 - rq_ref)| / (1 - rq_ref) is 1.358e-3 (rq_ref rebuilt in
float64 from the oracle's float32 raw_qv; it is the float32 rounding of rq itself: 1.36e-8 on a 1 - rq of 1e-5, a ZMW whose every base sits at the Q50 cap).  kinetics_lab.RQ_DEV_MEASURED holds
it rounded up to 1.36e-3; the GPU tests allow 4 x that x (1 - rq_ref) + one float32 ulp of rq."""
from fractions import Fraction

import numpy as np
import pytest

import handoff_ref as H
import kinetics_lab as Lab
import kinetics_ref as K
import oracle_lib as O
from ccs_amd import api
from pileup_ref import Read, Zmw


def rc(t):
    return (3 - np.asarray(t, np.uint8)[::-1]).astype(np.uint8)


# ---------------------------------------------------------------- the codec
def test_codec_against_the_oracle(built):
    assert [K.dec(c) for c in range(256)] == [O.codec_decode(c) for c in range(256)]
    assert [K.enc(f) for f in range(1201)] == [O.codec_encode(f) for f in range(1201)]
    assert K.enc(-3) == 0 == O.codec_encode(-3) and K.enc(5000) == 255 == O.codec_encode(5000)


def test_codec_boundaries_by_hand():
    assert (K.dec(63), K.dec(64), K.dec(65)) == (63, 64, 66)
    assert (K.dec(127), K.dec(128), K.dec(129)) == (190, 192, 196)
    assert (K.dec(191), K.dec(192), K.dec(193)) == (444, 448, 456)
    assert K.dec(255) == 952
    assert [K.enc(f) for f in (62, 63, 64, 65, 66, 67)] == [62, 63, 64, 65, 65, 66]              # 65 lies between 64 and 66: up
    assert [K.enc(f) for f in (189, 190, 191, 192, 193, 194, 195, 196)] == [127, 127, 128, 128, 128, 129, 129, 129]   # 191: 190 | 192 up; 194: 192 | 196 up
    assert [K.enc(f) for f in (444, 445, 446, 447, 448, 451, 452, 453)] == [191, 191, 192, 192, 192, 192, 193, 193]   # 446: 444 | 448 up; 452: 448 | 456 up
    assert [K.enc(f) for f in (943, 944, 947, 948, 951, 952, 953, 956, 1200, 10 ** 6)] == [254, 254, 254, 255, 255, 255, 255, 255, 255, 255]
    assert all(K.enc(K.dec(c)) == c for c in range(256))
    for f in range(953):                                                                       # nearest, and of two nearest the upper
        c = K.enc(f)
        d = abs(K.dec(c) - f)
        assert d == min(abs(v - f) for v in K.DEC) and (c == 255 or abs(K.dec(c + 1) - f) > d), f


def test_mean_rounds_halves_up():
    ks = list(range(0, 70)) + list(range(188, 194)) + list(range(442, 450)) + list(range(940, 953))
    for n in range(1, 256):
        for k in ks:
            half = (2 * k + 1) * n                                                             # sum / n = k + 1/2  <=>  2 sum = (2 k + 1) n
            for s in {half // 2 - 1, half // 2, half // 2 + 1, (half + 1) // 2, k * n, k * n + 1}:
                if s < 0:
                    continue
                q = Fraction(s, n) + Fraction(1, 2)
                assert K.mean_frames(s, n) == q.numerator // q.denominator, (s, n)
    k = np.arange(953, dtype=np.int64)                                                         # every k + 1/2 up to 952, every n: quotient and remainder
    for n in range(1, 256):
        half = (2 * k + 1) * n
        for s in (half // 2 - 1, half // 2, half // 2 + 1, (half + 1) // 2, k * n, k * n + n - 1):
            s = s[s >= 0]
            q, r = np.divmod(s, n)
            assert np.array_equal(K.mean_frames(s, n), q + (2 * r >= n)), n
    assert K.mean_code(0, 0) == 0 and K.mean_code(255 * 952, 255) == 255 and K.mean_code(3, 2) == 2 and K.mean_code(5, 4) == 1


# ---------------------------------------------------------------- per-read sums on hand-made windows
def mutate(rng, T, rate):
    out = []
    for b in T:
        u = rng.random()
        if u < rate / 3:
            continue
        if u < 2 * rate / 3:
            out.append(int(rng.integers(0, 4)))
        out.append(int((b + rng.integers(1, 4)) & 3) if rng.random() < rate / 3 else int(b))
    return np.array(out, np.uint8)


def sized(rng, r, n):
    return np.concatenate([r[:n], rng.integers(0, 4, max(0, n - len(r)), dtype=np.uint8)]).astype(np.uint8)


def hand_made_cases(rng):
    """(J, forward template, cs, ce, strand, read in its own orientation, kind)"""
    out = []
    for J in (1, 2, 31, 32):
        for st in (0, 1):
            for n in sorted({0, 1, J - 1, J, J + 1, 31, 32, 62, 63}):
                for kind in ("match", "mismatch", "lead_ins", "trail_ins", "rand5", "rand30"):
                    t = rng.integers(0, 4, J, dtype=np.uint8)
                    cs, ce = (int(rng.choice([0, 2])), int(rng.choice([J, J - 2]))) if J > 4 else (int(rng.integers(0, J)), J)
                    T = rc(t) if st else t
                    k = min(3, n)
                    if kind == "match":
                        r = np.resize(T, n)
                    elif kind == "mismatch":
                        r = (np.resize(T, n) + rng.integers(1, 4, n)) & 3
                    elif kind == "lead_ins":
                        r = np.concatenate([np.full(k, (T[0] + 2) & 3), np.resize(T, n - k)])
                    elif kind == "trail_ins":
                        r = np.concatenate([np.resize(T, n - k), np.full(k, (T[(n - k - 1) % J] + 2) & 3)])
                    else:
                        r = sized(rng, mutate(rng, T, 0.05 if kind == "rand5" else 0.30), n)
                    out.append((J, t, cs, ce, st, r.astype(np.uint8), kind))
            if J >= 31:                                                  # the core's edges, in the read's orientation (both strands: both forward edges)
                t = np.resize(np.array([0, 1, 2, 3], np.uint8), J)       # no base repeats its neighbour: every single edit has one best alignment
                T = rc(t) if st else t
                for cs, ce in ((2, J - 2), (0, J), (3, J - 7)):
                    a, b = (J - ce, J - cs) if st else (cs, ce)
                    for kind, r in (("del_first", np.delete(T, a)), ("del_last", np.delete(T, b - 1)), ("del_both", np.delete(T, [a, b - 1])),
                                    ("ins_edges", np.insert(T, [a, b], [(T[a] + 2) & 3, (T[b - 1] + 2) & 3])),
                                    ("ins_inside_edges", np.insert(T, [a + 1, b - 1], [(T[a] + 2) & 3, (T[b - 1] + 2) & 3]))):
                        out.append((J, t, cs, ce, st, r.astype(np.uint8), kind))
    return out


def brute_sums(T, r, ipd, pw, st):
    """sums over forward columns from the explicit path of handoff_ref.brute_path (a plain Python DP with its own trace-back)"""
    J = len(T)
    s = np.zeros((3, J), np.int64)
    for e in H.brute_path(r, T):
        if e[0] == "M" and int(r[e[1]]) == int(T[e[2]]):
            jf = J - 1 - e[2] if st else e[2]
            s[0, jf] += K.dec(ipd[e[1]]); s[1, jf] += K.dec(pw[e[1]]); s[2, jf] += 1
    return s


def test_read_sums_against_the_oracle_at_the_limits(built):
    """J = 32 is one column more than a window can have (CCSX_JMAX = 31, the size of the oracle's matrices), so those cases are held to the brute force of
    tests/handoff_ref.py instead; J <= 31 to orc_kinetics_read, and a sample of them to the brute force as well"""
    rng = np.random.default_rng(2024)
    cases = hand_made_cases(rng)
    zmws = []
    for J, t, cs, ce, st, r, kind in cases:
        n = len(r)
        zmws.append(Zmw([t], [(cs, ce)], 0, [Read(r, st, True, np.array([0, n]), rng.integers(0, 256, n).astype(np.uint8), rng.integers(0, 256, n).astype(np.uint8))]))
    sums = K.kinetics_sums(zmws)
    seen = set()
    for q, ((J, t, cs, ce, st, r, kind), z, sz) in enumerate(zip(cases, zmws, sums)):
        rd = z.reads[0]
        T = rc(t) if st else t
        got = sz[0][st]
        assert not sz[0][1 - st].any() and not got[:, :cs].any() and not got[:, ce:].any(), (J, kind)     # the pass's own strand, core columns only
        if J <= 31:
            want = np.array(O.kinetics_read(T, r, rd.ipd, rd.pw, st), np.int64)
            assert np.array_equal(got[:, cs:ce], want[:, cs:ce]), (J, len(r), st, kind)
        if J == 32 or q % 7 == 0:
            assert np.array_equal(got[:, cs:ce], brute_sums(T, r, rd.ipd, rd.pw, st)[:, cs:ce]), (J, len(r), st, kind)
        seen.add((J, len(r), st)); seen.add(kind)
    assert len(cases) > 400
    assert all((J, n, st) in seen for J in (1, 2, 31, 32) for st in (0, 1) for n in (0, 1, J - 1, J, J + 1, 31, 32, 62, 63))
    assert {"match", "mismatch", "lead_ins", "trail_ins", "rand5", "rand30", "del_first", "del_last", "ins_edges"} <= seen


def test_reads_add_up_per_strand_and_groups_do_not_matter():
    """70 passes on one window: the sums are those of the passes one by one, on the strand (flags ^ flags[backbone]) & 1"""
    rng = np.random.default_rng(7)
    t = rng.integers(0, 4, 26, dtype=np.uint8)
    reads = []
    for p in range(70):
        fl = int(rng.integers(0, 2))
        r = mutate(rng, rc(t) if fl else t, 0.1)
        reads.append(Read(r, fl | (2 if p >= 66 else 0), p != 5, np.array([0, len(r)]), rng.integers(0, 256, len(r)).astype(np.uint8), rng.integers(0, 256, len(r)).astype(np.uint8)))
    for ref in (0, 1):
        z = Zmw([t], [(2, 24)], ref, reads)
        whole = K.kinetics_sums([z])[0][0]
        parts = sum(sz[0] for sz in K.kinetics_sums([Zmw([t], [(2, 24)], ref, [rd]) for rd in reads]))
        assert np.array_equal(whole, parts) and (ref or (whole[0, 2, 2:24].min() > 5 and whole[1, 2, 2:24].min() > 5))
        first64 = K.kinetics_sums([z], keep=lambda zi, p: p < 64)[0][0]
        assert not np.array_equal(first64, whole)
        flipped = [Read(rd[0], rd[1] ^ ref, rd[2], rd[3], rd.ipd, rd.pw) for rd in reads]
        assert np.array_equal(K.kinetics_sums([Zmw([t], [(2, 24)], 0, flipped)])[0][0], whole)      # a reverse backbone swaps the roles of the two flag values, nothing else
        codes = K.kinetics_zmws([z])[0]
        assert codes.shape == (4, 22) and codes[0, 3] == K.mean_code(whole[0, 0, 5], whole[0, 2, 5]) and codes[3, 0] == K.mean_code(whole[1, 1, 2], whole[1, 2, 2])
        assert K.strand_counts(z) == (sum(1 for rd in reads[:66] if rd[2] and (rd[1] ^ ref) & 1 == 0), sum(1 for rd in reads[:66] if rd[2] and (rd[1] ^ ref) & 1))
    c = K.census([Zmw([t], [(2, 24)], 0, reads)])
    assert c["invalid_pass"] == 1 and c["passes_above_64"] == 6 and c["partial_segments"] == 4 and c["core_not_19"] == 1 and c["opposite_segments"] > 20


# ---------------------------------------------------------------- the stitch on hand-made windows
T26 = np.resize(np.array([0, 1, 2, 3], np.uint8), 26)


def windows(meta):
    """nw windows of T26 with core [2, 2 + len) and the given (core length, used_all, used_full, non-convergent, rounds)"""
    return [T26] * len(meta), [(2, 2 + m[0]) for m in meta], np.array(meta, np.int64).reshape(len(meta), 5)


def opts(min_rq=0.99):
    o = api.default_opts()
    o.min_rq = min_rq
    return o


def test_stitch_by_hand(built):
    tp, co, wm = windows([(22, 8, 7, 0, 1), (20, 9, 8, 0, 2), (22, 8, 8, 0, 1), (5, 7, 7, 0, 3)])
    raw = np.full(69, 30.0, np.float32); raw[:3] = (10.49999, 10.5, 49.500004)
    r = K.stitch_zmw(tp, co, wm, raw, opts(0.998))
    assert r["seq_len"] == 69 and np.array_equal(r["seq"], np.concatenate([T26[2:24], T26[2:22], T26[2:24], T26[2:7]]))
    assert r["qual"][:4].tolist() == [10, 11, 50, 30] and r["n_windows"] == 4 and r["iters"] == 7
    assert r["np"] == 7 and r["ec"] == np.float32(8.0)                   # used_full 7, 8, 8, 7: a tie, the smaller count
    assert abs(r["rq_ref"] - (1 - (66 * 1e-3 + 10 ** -1.049999 + 10 ** -1.05 + 10 ** -4.9500004) / 69)) < 1e-9 and r["status"] == K.LOW_RQ
    assert K.stitch_zmw(tp, co, wm, np.full(69, 30.0, np.float32), opts(0.998))["status"] == K.SUCCESS
    # the mode: most windows first, then the smaller count; a window nothing reached (used_full 0) counts like any other
    for full, want in (([5, 5, 6, 6, 6], 6), ([0, 0, 9, 9, 3], 0), ([0, 4, 4], 4), ([255], 255), ([3, 2, 1], 1)):
        tp, co, wm = windows([(10, f + 1, f, 0, 1) for f in full])
        r = K.stitch_zmw(tp, co, wm, np.full(10 * len(full), 40.0, np.float32), opts())
        assert r["np"] == want and r["ec"] == np.float32(sum(f + 1 for f in full) / len(full)) and r["status"] == K.SUCCESS
    assert K.stitch_zmw(*windows([(10, 1, 1, 0, 1), (10, 1, 1, 0, 1), (10, 2, 2, 0, 1)]), np.full(30, 40.0, np.float32), opts())["ec"] == np.float32(4.0 / 3.0)
    # the order of the statuses when two hold: EMPTY_WINDOW, NON_CONVERGENT, LOW_RQ, SUCCESS
    bad = np.full(30, 3.0, np.float32)
    assert K.stitch_zmw(*windows([(10, 5, 5, 0, 1), (10, 5, 5, 1, 8), (10, 5, 5, 0, 1)]), bad, opts())["status"] == K.NON_CONVERGENT
    assert K.stitch_zmw(*windows([(10, 5, 5, 0, 1)] * 3), bad, opts())["status"] == K.LOW_RQ
    r = K.stitch_zmw(*windows([(0, 5, 5, 1, 8), (0, 5, 5, 0, 1)]), np.zeros(0, np.float32), opts())
    assert r["status"] == K.EMPTY_WINDOW and r["seq_len"] == 0 and r["rq_ref"] == 0.0 and r["n_windows"] == 2 and r["iters"] == 9
    r = K.stitch_zmw([], [], np.zeros((0, 5)), np.zeros(0, np.float32), opts())
    assert r["status"] == K.EMPTY_WINDOW and r["seq_len"] == 0 and r["ec"] == 0 and r["np"] == 0
    # a ZMW that failed before the stitch reports nothing but its status
    r = K.stitch_zmw([], [], np.zeros((0, 5)), np.zeros(0, np.float32), opts(), pre_status=3)
    assert (r["status"], r["seq_len"], r["n_windows"], r["iters"], float(r["ec"]), r["rq_ref"]) == (3, 0, 0, 0, 0.0, 0.0)


# ---------------------------------------------------------------- rq: the reference against the oracle on the GPU tests' batches
@pytest.fixture(scope="module")
def oracle_runs(built):
    out = {}
    for name, make in Lab.BATCHES.items():
        b = make()
        o = Lab.kin_opts(**Lab.OPTS.get(name, {}))
        out[name] = (b, O.consensus_batch(api.default_model(), o, b, api.Results.allocate(b, kinetics=True), nthreads=8))
    return out


def test_rq_deviation_on_the_gpu_batches(oracle_runs):
    worst, n = 0.0, 0
    for name, (b, res) in oracle_runs.items():
        for z in range(b.n_zmw):
            if res.seq_len[z] == 0:
                continue
            ref = 1.0 - float(np.mean(10.0 ** (-res.raw(z).astype(np.float64) / 10.0)))
            dev = abs((1.0 - float(res.rq[z])) - (1.0 - ref)) / (1.0 - ref)
            worst, n = max(worst, dev), n + 1
            assert abs(float(res.rq[z]) - ref) <= Lab.rq_bound(ref), (name, z)
    print(f"rq: largest relative deviation of 1 - rq over {n} ZMWs {worst:.3e}; bound 4 x {Lab.RQ_DEV_MEASURED:.1e} x (1 - rq) + 1 ulp")
    assert n > 30 and 0.25 * Lab.RQ_DEV_MEASURED < worst <= Lab.RQ_DEV_MEASURED          # the constant is the measured value, rounded up


def test_min_rq_of_the_low_rq_test_leaves_no_zmw_out(oracle_runs):
    b, res = oracle_runs["low_rq"]
    ref = [1.0 - float(np.mean(10.0 ** (-res.raw(z).astype(np.float64) / 10.0))) for z in range(b.n_zmw) if res.seq_len[z] > 0]
    assert len(ref) == b.n_zmw
    assert all(abs(r - Lab.MIN_RQ_LOW) > 4 * Lab.rq_bound(r) for r in ref), ref
    assert sum(r < Lab.MIN_RQ_LOW for r in ref) >= 2 and sum(r > Lab.MIN_RQ_LOW for r in ref) >= 2, ref
    o = Lab.kin_opts(min_rq=Lab.MIN_RQ_LOW)
    low = O.consensus_batch(api.default_model(), o, b, api.Results.allocate(b, kinetics=True), nthreads=8)
    assert [int(s) for s in low.status] == [K.LOW_RQ if r < Lab.MIN_RQ_LOW else K.SUCCESS for r in ref]


def test_base_coded_kinetics_on_the_oracle_follow_the_backbone(oracle_runs):
    """the planes' strands are those of the backbone: on the strand_reference batch (pass 0 reverse; a backbone that is not pass 0) the oracle's forward planes
    carry the code of SEQ's base — the statement tests/test_kinetics_gpu.py makes of the engine"""
    b = Lab.strand_reference()
    b.ipd = (10 + 10 * b.bases).astype(np.uint8)
    res = O.consensus_batch(api.default_model(), Lab.kin_opts(), b, api.Results.allocate(b, kinetics=True), nthreads=8)
    assert res.status[6] == 0 and res.np_[6] < res.fn[6] + res.rn[6] == 10          # np is the mode over windows of the passes the polish used, fn + rn the aligned passes
    for z in (0, 1, 2, 3, 5, 6):
        assert res.seq_len[z] > 0
        s, (fi, _, ri, _) = res.sequence(z).astype(int), res.kinetics(z).astype(int)
        assert (fi[fi > 0] == 10 + 10 * s[fi > 0]).all() and (ri[ri > 0] == 10 + 10 * (3 - s[ri > 0])).all() and (fi > 0).mean() > 0.9
        assert (ri > 0).mean() > 0.9 if z != 1 else not ri.any()          # (every aligned pass of ZMW 1 is on its backbone's strand)

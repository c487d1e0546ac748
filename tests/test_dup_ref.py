"""The duplicate rule on the CPU (DESIGN.md §2 "Duplicate rule"): the restatement of tests/dup_ref.py against its brute force on the whole limit set; the library's
two host calls against the restatement, signature byte for byte and report field for field; the hash, the defaults DESIGN.md states, the layout of the
signature; every error of the call.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ccs_amd import api
import dup_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = R.limit_cases()
IDS = [c[0] for c in CASES]


def _opts(o=None, **kw):
    x = api.dup_opts_default()
    for k, v in {**(o or {}), **kw}.items():
        setattr(x, k, v)
    return x


def _poisoned(n):
    rep = api.DupReport.allocate(n)
    for k in R.FIELDS:
        getattr(rep, k).view(np.uint8)[...] = 0xA5
    return rep


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_restatement_equals_the_brute_force(i):
    _, o, reads, group, score = CASES[i]
    assert R.diff(R.brute(reads, o, group, score), R.expected(i)[1]) == []


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_host_calls_equal_the_restatement(built, i):
    _, o, reads, group, score = CASES[i]
    want_sig, want = R.expected(i)
    sig = api.dup_sign_host(reads, _opts(o))
    assert sig.dtype == R.SIG_DTYPE and sig.tobytes() == want_sig.tobytes()
    rep = api.dup_cluster_host(sig, group, score, _opts(o), _poisoned(len(reads)))
    assert R.diff(rep, want) == [], R.diff(rep, want)


def test_reads_with_gaps_and_out_of_order(built):
    i = IDS.index("untested_mixed_in")
    reads = CASES[i][2]
    layout = R.with_gaps(reads, np.random.default_rng(5))
    assert api.dup_sign_host(layout, _opts(CASES[i][1])).tobytes() == R.expected(i)[0].tobytes()


def test_score_null_is_score_zero(built):
    i = IDS.index("score_tied_largest")
    sig = R.expected(i)[0]
    a, b = api.dup_cluster_host(sig), api.dup_cluster_host(sig, score=np.zeros(len(sig), np.int32), group=np.zeros(len(sig), np.int32))
    assert R.diff(a, {k: getattr(b, k) for k in R.FIELDS}) == [] and a.rep.tolist() == [0, 0, 0, 0]


def test_hash_defaults_and_layout(built):
    L = api.lib()
    assert L.ccsx_dup_rule_version() == 1
    x = np.array([0, 1, 2, 0xFFFFFFFF, 0x12345678, 0xDEADBEEF] + np.random.default_rng(1).integers(0, 1 << 32, 200).tolist(), np.uint64)
    assert [L.ccsx_dup_hash(int(v)) for v in x] == R.hash32(x).tolist()
    src = open(os.path.join(ROOT, "ccs_amd", "csrc", "dup_core.h")).read()
    consts = {k: int(v.rstrip("u"), 0) for k, v in re.findall(r"#define CCSX_DUP_HASH_(\w+)\s+(\w+)", src)}
    assert consts == dict(M1=R.M1, M2=R.M2, S1=R.S1, S2=R.S2, S3=R.S3)
    # a bijection: the finaliser's inverse brings every value back
    def inv(h):
        h ^= h >> 16; h = (h * pow(R.M2, -1, 1 << 32)) & 0xFFFFFFFF
        h ^= (h >> 13) ^ (h >> 26); h = (h * pow(R.M1, -1, 1 << 32)) & 0xFFFFFFFF
        return h ^ (h >> 16)
    assert [inv(int(h)) for h in R.hash32(x)] == x.tolist()
    # the defaults are the ones DESIGN.md states
    o = api.dup_opts_default()
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    m = re.search(r"Defaults of the duplicate rule: window (\d+),\s+kmer (\d+),\s+max_dist_pct (\d+),\s+max_len_diff_pct (\d+)", text)
    assert m and (o.window, o.kmer, o.max_dist_pct, o.max_len_diff_pct) == tuple(int(v) for v in m.groups())
    assert C.sizeof(api.DupOpts) == 16 and api.DUP_SIG_DTYPE.itemsize == 48 and api.DUP_SIG_DTYPE == R.SIG_DTYPE
    assert (api.DUP_MAX_BUCKET, api.DUP_UNTESTED, api.DUP_TESTED, api.DUP_OVERFLOW) == (R.MAX_BUCKET, R.UNTESTED, R.TESTED, R.OVERFLOW)


def _sign_raw(L, o, seq, off, ln, n, sig):
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t)) if a is not None else None
    return L.ccsx_dup_sign_reads_host(C.byref(o) if o is not None else None, p(seq, C.c_uint8), p(off, C.c_int64), p(ln, C.c_int32), n,
                                      sig.ctypes.data_as(C.c_void_p) if sig is not None else None)


def _cluster_raw(L, o, sig, group, score, n, crep):
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None
    return L.ccsx_dup_cluster_host(C.byref(o) if o is not None else None, sig.ctypes.data_as(C.c_void_p) if sig is not None else None, p(group), p(score), n,
                                   C.byref(crep) if crep is not None else None)


def test_every_error_of_the_calls(built):
    L = api.lib()
    err = lambda: L.ccsx_last_error().decode()
    seq, off, ln = np.zeros(100, np.uint8), np.array([0, 40], np.int64), np.array([40, 60], np.int32)
    sig = np.zeros(2, api.DUP_SIG_DTYPE)
    assert _sign_raw(L, None, seq, off, ln, 2, sig) == 0 and sig["window"].tolist() == [32, 32]     # (opts NULL: the defaults)
    good = sig.copy()
    # options out of range, kmer > window
    for kw in (dict(window=15), dict(window=65), dict(kmer=7), dict(kmer=17), dict(window=16, kmer=16, max_dist_pct=31), dict(max_dist_pct=-1),
               dict(max_len_diff_pct=21), dict(max_len_diff_pct=-1), dict(window=16, kmer=17), dict(window=10, kmer=8)):
        assert _sign_raw(L, _opts(**kw), seq, off, ln, 2, sig) == -1 and "ccsx_dup_sign_reads_host: duplicate options out of range" in err(), kw
        rep = api.DupReport.allocate(2)
        assert _cluster_raw(L, _opts(**kw), good, None, None, 2, rep.c_struct()) == -1 and "ccsx_dup_cluster_host: duplicate options out of range" in err(), kw
    assert _sign_raw(L, _opts(window=16, kmer=16), seq, off, ln, 2, sig) == 0
    # null arguments, n, seq_off
    for args in ((None, off, ln, 2, sig), (seq, None, ln, 2, sig), (seq, off, None, 2, sig), (seq, off, ln, 2, None)):
        assert _sign_raw(L, None, *args) == -1 and "null argument" in err(), args
    assert _sign_raw(L, None, seq, off, ln, -1, sig) == -1 and "n must be >= 0" in err()
    assert _sign_raw(L, None, seq, off, ln, api.DUP_MAX_READS + 1, sig) == -1 and "CCSX_DUP_MAX_READS" in err()
    assert _sign_raw(L, None, seq, np.array([0, -1], np.int64), ln, 2, sig) == -1 and "negative seq_off" in err()
    assert _sign_raw(L, None, None, None, None, 0, None) == 0                                         # (nothing to sign needs nothing)
    # the cluster call
    rep = api.DupReport.allocate(2)
    assert _cluster_raw(L, None, good, None, None, 2, rep.c_struct()) == 0
    assert _cluster_raw(L, None, None, None, None, 2, rep.c_struct()) == -1 and "null argument" in err()
    assert _cluster_raw(L, None, good, None, None, 2, None) == -1 and "null argument" in err()
    assert _cluster_raw(L, None, good, None, None, -1, rep.c_struct()) == -1 and "n must be >= 0" in err()
    assert _cluster_raw(L, None, good, None, None, api.DUP_MAX_READS + 1, rep.c_struct()) == -1 and "CCSX_DUP_MAX_READS" in err()
    other = good.copy(); other["window"][1] = 16
    assert _cluster_raw(L, None, other, None, None, 2, rep.c_struct()) == -1 and "signature 1: taken with another window" in err()
    assert _cluster_raw(L, None, good, np.array([0, -1], np.int32), None, 2, rep.c_struct()) == -1 and "read 1: negative group" in err()
    assert _cluster_raw(L, None, good, None, None, 2, api.DupReport.allocate(3).c_struct()) == -1 and "sized for another n" in err()
    for k in R.FIELDS:
        c = rep.c_struct()
        setattr(c, k, C.POINTER(C.c_int32)())
        assert _cluster_raw(L, None, good, None, None, 2, c) == -1 and "report arrays missing" in err(), k
    empty = api.DupReport.allocate(0)
    assert _cluster_raw(L, None, None, None, None, 0, empty.c_struct()) == 0
    # an untested signature (window 0) beside tested ones is no error
    other = good.copy(); other["window"][0] = 0
    assert _cluster_raw(L, None, other, None, None, 2, rep.c_struct()) == 0 and rep.status.tolist() == [R.UNTESTED, R.TESTED]

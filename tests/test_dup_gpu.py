"""The k_dup_* kernels on an MI355X (DESIGN.md §2 "Duplicate rule", §4): Handle.dup_sign and Handle.dup_cluster against tests/dup_ref.py on the whole limit set,
signature byte for byte and report field for field on poisoned planes, and again with the reads in reverse order (the expectation computed on the reversed
input: the tie to the smallest index moves); the same partition into sets under three seeded permutations; two runs byte for byte; score NULL as score 0; reads
with gaps in seq; a ticket in flight during the calls completes with its own results."""
import numpy as np
import pytest

from ccs_amd import api
import dup_ref as R

pytestmark = pytest.mark.gpu
CASES = R.limit_cases()
IDS = [c[0] for c in CASES]
RES_FIELDS = ("status", "seq_len", "rq", "np_", "ec", "iters", "n_windows", "fn", "rn")


@pytest.fixture(scope="module")
def handle(built):
    h = api.Handle(0)
    yield h
    h.close()


def _opts(o):
    x = api.dup_opts_default()
    for k, v in o.items():
        setattr(x, k, v)
    return x


def _poisoned(n):
    rep = api.DupReport.allocate(n)
    for k in R.FIELDS:
        getattr(rep, k).view(np.uint8)[...] = 0xA5
    return rep


def _run(handle, o, reads, group, score):
    sig = handle.dup_sign(reads, _opts(o))
    return sig, handle.dup_cluster(sig, group, score, _opts(o), _poisoned(len(reads)))


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_sign_and_cluster_equal_the_restatement_on_the_limit_set(handle, i):
    name, o, reads, group, score = CASES[i]
    want_sig, want = R.expected(i)
    sig, rep = _run(handle, o, reads, group, score)
    assert sig.tobytes() == want_sig.tobytes(), name
    assert R.diff(rep, want) == [], (name, R.diff(rep, want))
    rev = lambda v: None if v is None else list(v)[::-1]
    rsig, rrep = _run(handle, o, reads[::-1], rev(group), rev(score))
    want_rsig, want_rev = R.mark(reads[::-1], o, rev(group), rev(score))
    assert rsig.tobytes() == want_rsig.tobytes() and R.diff(rrep, want_rev) == [], (name, "reversed", R.diff(rrep, want_rev))


@pytest.mark.parametrize("name", ["random_257", "random_4097", "W64_k8", "chain_by_distance", "bucket_of_512", "untested_mixed_in", "chain_of_300_by_length"])
def test_the_partition_is_the_same_under_permutations(handle, name):
    i = IDS.index(name)
    _, o, reads, group, score = CASES[i]
    want = R.partition(R.expected(i)[1])
    for seed in (1, 2, 3):
        perm = np.random.default_rng(seed).permutation(len(reads))
        pick = lambda v: None if v is None else [v[z] for z in perm]
        _, rep = _run(handle, o, [reads[z] for z in perm], pick(group), pick(score))
        assert R.partition({k: getattr(rep, k) for k in R.FIELDS}, perm) == want, (name, seed)


def test_two_runs_give_equal_bytes(handle):
    i = IDS.index("random_4097")
    _, o, reads, group, score = CASES[i]
    a, b = _run(handle, o, reads, group, score), _run(handle, o, reads, group, score)
    assert a[0].tobytes() == b[0].tobytes()
    for k in R.FIELDS:
        assert getattr(a[1], k).tobytes() == getattr(b[1], k).tobytes(), k


def test_score_null_is_score_zero_and_mark_duplicates_chains_the_calls(handle):
    i = IDS.index("score_tied_largest")
    _, o, reads, _, _ = CASES[i]
    sig = handle.dup_sign(reads, _opts(o))
    a = handle.dup_cluster(sig, None, None, _opts(o), _poisoned(len(reads)))
    b = handle.dup_cluster(sig, np.zeros(len(reads), np.int32), np.zeros(len(reads), np.int32), _opts(o), _poisoned(len(reads)))
    assert R.diff(a, {k: getattr(b, k) for k in R.FIELDS}) == [] and a.rep.tolist() == [0, 0, 0, 0]
    i = IDS.index("groups_split_equal_reads")
    _, o, reads, group, score = CASES[i]
    assert R.diff(handle.mark_duplicates(reads, group, score, _opts(o)), R.expected(i)[1]) == []


def test_reads_with_gaps_and_out_of_order(handle):
    i = IDS.index("untested_mixed_in")
    layout = R.with_gaps(CASES[i][2], np.random.default_rng(5))
    assert handle.dup_sign(layout, _opts(CASES[i][1])).tobytes() == R.expected(i)[0].tobytes()


def test_errors_launch_nothing_and_the_handle_runs_on(handle):
    i = IDS.index("identical_x3")
    _, o, reads, _, _ = CASES[i]
    sig = handle.dup_sign(reads, _opts(o))
    with pytest.raises(RuntimeError, match="ccsx_dup_sign_reads: duplicate options out of range"):
        handle.dup_sign(reads, _opts(dict(window=16, kmer=17)))
    with pytest.raises(RuntimeError, match="ccsx_dup_cluster: signature 0: taken with another window"):
        handle.dup_cluster(sig, None, None, _opts(dict(window=64)))
    with pytest.raises(RuntimeError, match="ccsx_dup_cluster: read 1: negative group"):
        handle.dup_cluster(sig, [0, -1, 0, 0])
    with pytest.raises(RuntimeError, match="sized for another n"):
        handle.dup_cluster(sig, report=api.DupReport.allocate(3))
    assert len(handle.dup_sign([])) == 0 and len(handle.dup_cluster(np.zeros(0, api.DUP_SIG_DTYPE)).rep) == 0
    assert R.diff(handle.dup_cluster(sig, None, None, _opts(o)), R.expected(i)[1]) == []


def test_a_ticket_in_flight_completes_with_its_own_results(handle):
    """the calls stage nothing: a ticket submitted before them completes with the results of a plain run"""
    b = api.synth(n_zmw=6, passes=5, length=600, seed=11)
    plain = handle.consensus(b)
    res = api.Results.allocate(b, pinned=True)
    t = handle.submit(b.pinned(), res)
    i = IDS.index("random_257")
    _, o, reads, group, score = CASES[i]
    sig, rep = _run(handle, o, reads, group, score)
    assert sig.tobytes() == R.expected(i)[0].tobytes() and R.diff(rep, R.expected(i)[1]) == []
    handle.wait(t)
    handle.release(t)
    for f in RES_FIELDS:
        assert getattr(res, f).tobytes() == getattr(plain, f).tobytes(), f
    for z in range(b.n_zmw):
        assert np.array_equal(res.sequence(z), plain.sequence(z)) and np.array_equal(res.quals(z), plain.quals(z)), z

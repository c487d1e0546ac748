"""ZMWs whose final drafts put the k-mer scan that k_fold and k_control share at its edges.  A 256-thread workgroup splits a draft's npos = L - 14 15-mer positions
into contiguous ranges of ceil(npos / 256): below 256 positions most threads own nothing, just above 256 the last owning thread's range is cut short and the
threads behind it are empty, at a multiple of 256 every range is full.  The insert lengths, seeds and passes below were chosen on the CPU with the oracle
(oracle_lib.poa_draft) so that the drafts have exactly these lengths; the tests assert on the engine's own drafts that every class is present."""
import numpy as np

from ccs_amd import api

# (insert length, seed, passes) -> the oracle's draft has npos = 16, 85, 255 | 258, 267, 513 | 256, 512
ZMWS = ((30, 9000, 5), (100, 9002, 7), (268, 9003, 8), (272, 9001, 6), (278, 9003, 8), (528, 9000, 5), (270, 9001, 6), (526, 9000, 5))
CLASSES = ("below 256", "above 256, no multiple", "multiple of 256")


def batch() -> api.Batch:
    import adapter_synth
    parts = []
    for length, seed, passes in ZMWS:
        rng = np.random.default_rng(seed)
        parts.append(adapter_synth.from_templates([rng.integers(0, 4, length, dtype=np.uint8)], [passes], rng))
    return api.concat(parts)


def assert_every_class(draft_lengths) -> None:
    """draft_lengths: the final drafts of the TESTED ZMWs.  At least one in each class of npos"""
    npos = [int(L) - 14 for L in draft_lengths if L >= 15]
    got = {CLASSES[0 if p < 256 else 2 if p % 256 == 0 else 1] for p in npos}
    assert got == set(CLASSES) and any(256 < p < 300 for p in npos), sorted(npos)[:16]   # (just above 256: ranges of two positions, half the threads empty)

"""The ZMWs of the representative tests on the GPU: inserts of 200 - 600 bases, a few dozen ZMWs, every status the engine reaches by construction.
  polished      five passes over one template: the neighbours nothing of which may change
  few           0 or 1 full-length pass with 0 - 4 partial ones (prefixes and suffixes of further passes over the template): TOO_FEW_PASSES at min_passes 2;
                the ZMW of (0, 0) has no pass at all
  unrelated     2 and 4 full-length passes of unrelated random sequence: no draft generator finds a draft that most of them map to, TOO_MANY_UNUSABLE after the
                cascade (tests/test_represent_ref.py checks that on the CPU oracle)
batch() returns (api.Batch, kind per ZMW)."""
from __future__ import annotations

import numpy as np

import lowcx
import represent_ref as R

SEED = 23


def rc(x):
    return (3 - np.asarray(x, np.uint8)[::-1]).astype(np.uint8)


def zmws(seed=SEED):
    rng = np.random.default_rng(seed)
    out, kinds = [], []

    def passes_over(t, k, first_rev=0):
        ps = []
        for q in range(k):
            b, _ = lowcx.sequence_read(rng, t)
            rev = (q + first_rev) & 1
            ps.append((rc(b) if rev else b, rev))
        return ps

    def partial(t, q):
        b, _ = lowcx.sequence_read(rng, t)
        cut = int(rng.integers(len(b) // 4, 3 * len(b) // 4))
        at_end, rev = q & 1, (q >> 1) & 1                            # bit 2: the adapter is at the pass's end, so the pass is the tail of a whole one
        native = rc(b) if rev else b
        return (native[len(native) - cut:] if at_end else native[:cut], R.PARTIAL | (4 if at_end else 0) | rev)

    tpl = lambda: rng.integers(0, 4, int(rng.integers(200, 601))).astype(np.uint8)
    for k in range(3):
        out.append(passes_over(tpl(), 5, k & 1)); kinds.append("polished")
    for nf in (0, 1):
        for npart in range(5):
            t = tpl()
            out.append(passes_over(t, nf, npart & 1) + [partial(t, q) for q in range(npart)]); kinds.append("few")
    for k in range(3):
        out.append(passes_over(tpl(), 5, k & 1)); kinds.append("polished")
    for nf in (2, 4, 2, 4):
        out.append([(tpl(), q & 1) for q in range(nf)]); kinds.append("unrelated")
    out.append(passes_over(tpl(), 6)); kinds.append("polished")
    return out, kinds


def batch(seed=SEED):
    z, kinds = zmws(seed)
    return R.make_batch(z, seed=seed + 1), kinds

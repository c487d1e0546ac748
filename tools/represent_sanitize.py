#!/usr/bin/env python3
"""Run the representative rule of k_represent under AddressSanitizer + UBSan on the CPU: a stand-alone program (tools/represent_sanitize/main.cpp, its own main,
no Python in the process) around ccsx_represent_host, over every batch of the tests' limit set (tests/represent_ref.py) under the four combinations of
subread_fallback and kinetics with the planes the restatement expects, plus seeded random batches of its own.  CPU only.
Usage: tools/represent_sanitize.py [--keep DIR]"""
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from host_sanitize import build_and_run  # noqa: E402
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import represent_ref as R  # noqa: E402


def write_cases(f) -> None:
    for i, (_, zmws, top, status, drafts) in enumerate(R.limit_cases()):
        for fb in (0, 1):
            for kin in (0, 1):
                b = R.make_batch(zmws, seed=5, high_bits=bool(i & 1))
                want = R.poisoned_results(b, kinetics=True)
                cls, pas = R.apply(b, top, status, drafts, want, fb, kin)
                dseq = np.concatenate([np.asarray(d, np.uint8) for d in drafts] + [np.zeros(0, np.uint8)])
                f.write(struct.pack("<8q", b.n_zmw, len(b.flags), len(b.bases), len(dseq), len(want.seq), top, fb, kin))
                for a, dt in ((b.read_off, np.int32), (b.base_off, np.int64), (b.flags, np.uint8), (b.bases, np.uint8), (b.pw, np.uint8), (b.ipd, np.uint8),
                              (status, np.int32), ([len(d) for d in drafts], np.int32), (dseq, np.uint8), (cls, np.int32), (pas, np.int32),
                              (want.seq_len, np.int32), (want.rq, np.float32), (want.ec, np.float32), (want.seq, np.uint8), (want.qual, np.uint8),
                              (want.raw_qv, np.float32), (want.kin[0], np.uint8), (want.kin[1], np.uint8)):
                    f.write(np.ascontiguousarray(a, dt).tobytes())


if __name__ == "__main__":
    sys.exit(build_and_run("represent", write_cases))

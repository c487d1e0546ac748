#!/usr/bin/env python3
"""Run the duplicate rule of the k_dup_* kernels under AddressSanitizer + UBSan on the CPU: a stand-alone program (tools/dup_sanitize/main.cpp, its own main, no
Python in the process) around ccsx_dup_sign_reads_host, ccsx_dup_cluster_host and their argument checks, over every case of the tests' limit set
(tests/dup_ref.py) with the signatures and the report the restatement expects, plus seeded random cases of its own.  CPU only.
Usage: tools/dup_sanitize.py [--keep DIR]"""
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from host_sanitize import build_and_run  # noqa: E402
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dup_ref as R  # noqa: E402


def write_cases(f) -> None:
    for i, (_, o, reads, group, score) in enumerate(R.limit_cases()):
        n = len(reads)
        f.write(struct.pack("<7i", n, *(o[k] for k in R.DEFAULTS), group is not None, score is not None))
        for r in reads:
            f.write(struct.pack("<i", len(r)) + np.asarray(r, np.uint8).tobytes())
        if group is not None:
            f.write(np.asarray(group, np.int32).tobytes())
        if score is not None:
            f.write(np.asarray(score, np.int32).tobytes())
        sig, want = R.expected(i)
        f.write(sig.tobytes())
        for k in R.FIELDS:
            f.write(np.ascontiguousarray(want[k], np.int32).tobytes())


if __name__ == "__main__":
    sys.exit(build_and_run("dup", write_cases))

#!/usr/bin/env python3
"""Run the cDNA rule of k_cdna under AddressSanitizer + UBSan on the CPU: a stand-alone program (tools/cdna_sanitize/main.cpp, its own main, no Python in the
process) around ccsx_cdna_reads_host and ccsx_cdna_check, over every set and read of the tests' limit set (tests/cdna_ref.py) with the report the restatement
expects, plus seeded random sets and reads of its own.  CPU only.  Usage: tools/cdna_sanitize.py [--keep DIR]"""
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from host_sanitize import build_and_run  # noqa: E402
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cdna_ref as R  # noqa: E402


def write_cases(f) -> None:
    for i, (_, S, roles, o, reads) in enumerate(R.limit_cases()):
        f.write(struct.pack("<10i", len(S), len(reads), *(o[k] for k in R.DEFAULTS)))
        for p, role in zip(S, roles):
            f.write(struct.pack("<2i", len(p), role) + np.asarray(p, np.uint8).tobytes())
        for r in reads:
            f.write(struct.pack("<i", len(r)) + np.asarray(r, np.uint8).tobytes())
        want = R.expected(i)
        for k in R.FIELDS:
            f.write(np.ascontiguousarray(want[k], np.int32).tobytes())


if __name__ == "__main__":
    sys.exit(build_and_run("cdna", write_cases))

#!/usr/bin/env python3
"""Run the cell-tag rule of k_cell under AddressSanitizer + UBSan on the CPU: a stand-alone program (tools/cell_sanitize/main.cpp, its own main, no Python in the
process) around ccsx_cell_reads_host, the whitelist's builder and ccsx_cell_check, over every case of the tests' limit set (tests/cell_ref.py) with the report the
restatement expects, plus seeded random cases of its own.  CPU only.  Usage: tools/cell_sanitize.py [--keep DIR]"""
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from host_sanitize import build_and_run  # noqa: E402
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cell_ref as R  # noqa: E402


def write_cases(f) -> None:
    for i, (_, S, roles, o, d, wl, reads) in enumerate(R.limit_cases()):
        f.write(struct.pack("<16i", len(S), len(reads), *(o[k] for k in R.DEFAULTS), *(d[k] for k in R.DESIGN), -1 if wl is None else len(wl)))
        for p, role in zip(S, roles):
            f.write(struct.pack("<2i", len(p), role) + np.asarray(p, np.uint8).tobytes())
        for w in wl or ():
            f.write(np.asarray(w, np.uint8).tobytes())
        for r in reads:
            f.write(struct.pack("<i", len(r)) + np.asarray(r, np.uint8).tobytes())
        want = R.expected(i)
        for k in R.FIELDS:
            f.write(np.ascontiguousarray(want[k]).astype("<u4" if want[k].dtype == np.uint32 else "<i4").tobytes())


if __name__ == "__main__":
    sys.exit(build_and_run("cell", write_cases))

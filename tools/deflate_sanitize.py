#!/usr/bin/env python3
"""Run the DEFLATE encoder of k_deflate under AddressSanitizer + UBSan on the CPU, judged by the project's own decoder: a stand-alone program
(tools/deflate_sanitize/main.cpp, its own main, no Python in the process) over every input of tests/deflate_ref.py plus seeded random inputs of its own.
Encode, decode, compare; the CRC; out_cap == out_len and out_len - 1.  CPU only.  Usage: tools/deflate_sanitize.py [--keep DIR]"""
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from host_sanitize import build_and_run  # noqa: E402
sys.path.insert(0, os.path.join(ROOT, "tests"))
import deflate_ref as R  # noqa: E402


def write_cases(f) -> None:
    cases = [d for _, d in R.all_cases()]
    ccs = os.path.join(ROOT, "ccs_amd", "bin", "ccs")
    if os.path.exists(ccs):
        cases.append(R.synthetic_bam_slice(ccs))
    for d in cases:
        f.write(struct.pack("<q", len(d)) + d)


if __name__ == "__main__":
    sys.exit(build_and_run("deflate", write_cases))

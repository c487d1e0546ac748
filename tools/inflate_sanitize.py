#!/usr/bin/env python3
"""Run the DEFLATE decoder of k_inflate under AddressSanitizer + UBSan on the CPU: a stand-alone program (tools/inflate_sanitize/main.cpp, its own main, no
Python in the process) over every valid, corrupt and flipped stream of tests/inflate_ref.py, plus its own bit-flip loop.  Run this before the corrupt list goes
to a GPU.  Usage: tools/inflate_sanitize.py [--keep DIR]"""
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from host_sanitize import build_and_run  # noqa: E402
sys.path.insert(0, os.path.join(ROOT, "tests"))
import inflate_ref as R  # noqa: E402


def write_cases(f) -> None:
    cases = [(s, len(d), R.OK, d) for _, s, d in R.valid_cases() + R.fuzz_cases() + R.limit_cases()]
    cases += [(s, n, -1 if want is None else want, b"") for _, s, n, want in R.corrupt_cases()]
    cases += [(s, n, -1, b"") for s, n in R.flip_cases(n=4000)]
    for s, n, want, d in cases:
        f.write(struct.pack("<qqqq", len(s), n, want, len(d)) + s + d)


if __name__ == "__main__":
    sys.exit(build_and_run("inflate", write_cases))

#!/usr/bin/env python3
"""Run the DEFLATE decoder of k_inflate under AddressSanitizer + UBSan on the CPU: a stand-alone program (tools/inflate_sanitize/main.cpp, its own main, no
Python in the process) over every valid, corrupt and flipped stream of tests/inflate_ref.py, plus its own bit-flip loop.  Run this before the corrupt list goes
to a GPU.  Usage: tools/inflate_sanitize.py [--keep DIR]"""
import os
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import inflate_ref as R  # noqa: E402


def main() -> int:
    keep = sys.argv[sys.argv.index("--keep") + 1] if "--keep" in sys.argv else None
    work = keep or tempfile.mkdtemp(prefix="inflate_sanitize_")
    os.makedirs(work, exist_ok=True)
    cases = [(s, len(d), R.OK, d) for _, s, d in R.valid_cases() + R.fuzz_cases()]
    cases += [(s, n, -1 if want is None else want, b"") for _, s, n, want in R.corrupt_cases()]
    cases += [(s, n, -1, b"") for s, n in R.flip_cases(n=4000)]
    path = os.path.join(work, "cases.bin")
    with open(path, "wb") as f:
        for s, n, want, d in cases:
            f.write(struct.pack("<qqqq", len(s), n, want, len(d)) + s + d)
    exe = os.path.join(work, "inflate_sanitize")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "ccs_amd", "csrc"), os.path.join(ROOT, "tools", "inflate_sanitize", "main.cpp"),
                           "-o", exe])
    return subprocess.call([exe, path])


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Run the DEFLATE encoder of k_deflate under AddressSanitizer + UBSan on the CPU, judged by the project's own decoder: a stand-alone program
(tools/deflate_sanitize/main.cpp, its own main, no Python in the process) over every input of tests/deflate_ref.py plus seeded random inputs of its own.
Encode, decode, compare; the CRC; out_cap == out_len and out_len - 1.  CPU only.  Usage: tools/deflate_sanitize.py [--keep DIR]"""
import os
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import deflate_ref as R  # noqa: E402


def main() -> int:
    keep = sys.argv[sys.argv.index("--keep") + 1] if "--keep" in sys.argv else None
    work = keep or tempfile.mkdtemp(prefix="deflate_sanitize_")
    os.makedirs(work, exist_ok=True)
    cases = [d for _, d in R.all_cases()]
    ccs = os.path.join(ROOT, "ccs_amd", "bin", "ccs")
    if os.path.exists(ccs):
        cases.append(R.synthetic_bam_slice(ccs))
    path = os.path.join(work, "cases.bin")
    with open(path, "wb") as f:
        for d in cases:
            f.write(struct.pack("<q", len(d)) + d)
    exe = os.path.join(work, "deflate_sanitize")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "ccs_amd", "csrc"), os.path.join(ROOT, "tools", "deflate_sanitize", "main.cpp"),
                           "-o", exe])
    return subprocess.call([exe, path])


if __name__ == "__main__":
    sys.exit(main())

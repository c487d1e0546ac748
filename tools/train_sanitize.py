#!/usr/bin/env python3
"""Run the host path of the model training — the counting rule of train_core.h through ccsx_train_pair_host, and the fitter — under AddressSanitizer + UBSan on
the CPU: a stand-alone program (tools/train_sanitize/main.cpp, its own main, no Python in the process, no device).  Usage: tools/train_sanitize.py [--keep DIR]
[--pairs N]"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main() -> int:
    keep = sys.argv[sys.argv.index("--keep") + 1] if "--keep" in sys.argv else None
    pairs = sys.argv[sys.argv.index("--pairs") + 1] if "--pairs" in sys.argv else "20000"
    work = keep or tempfile.mkdtemp(prefix="train_sanitize_")
    os.makedirs(work, exist_ok=True)
    exe = os.path.join(work, "train_sanitize")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ccs_amd", "csrc"),
                           os.path.join(ROOT, "tools", "train_sanitize", "main.cpp"), "-o", exe])
    return subprocess.call([exe, pairs])


if __name__ == "__main__":
    sys.exit(main())

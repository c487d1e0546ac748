#!/usr/bin/env python3
"""Run the host path of the model training — the counting rule of train_core.h through ccsx_train_pair_host, and the fitter — under AddressSanitizer + UBSan on
the CPU: a stand-alone program (tools/train_sanitize/main.cpp, its own main, no Python in the process, no device).  Usage: tools/train_sanitize.py [--keep DIR]
[--pairs N]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from host_sanitize import build_and_run  # noqa: E402


if __name__ == "__main__":
    pairs = sys.argv[sys.argv.index("--pairs") + 1] if "--pairs" in sys.argv else "20000"
    sys.exit(build_and_run("train", flags=["-ffp-contract=off"], args=[pairs]))

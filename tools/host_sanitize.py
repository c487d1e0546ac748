"""What the *_sanitize.py scripts share: the work directory (--keep DIR keeps it), the case file, the AddressSanitizer + UBSan build of the stand-alone program
tools/<name>_sanitize/main.cpp (its own main, no Python in the process, CPU only) and its run."""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_and_run(name: str, write_cases=None, flags=(), args=()) -> int:
    """write_cases(f): writes the cases into the open binary file whose path becomes the program's first argument (None: no case file); flags: further
    compiler flags; args: further arguments of the program.  Returns the program's exit status"""
    keep = sys.argv[sys.argv.index("--keep") + 1] if "--keep" in sys.argv else None
    work = keep or tempfile.mkdtemp(prefix=name + "_sanitize_")
    os.makedirs(work, exist_ok=True)
    run = [os.path.join(work, name + "_sanitize")]
    if write_cases is not None:
        run.append(os.path.join(work, "cases.bin"))
        with open(run[1], "wb") as f:
            write_cases(f)
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", *flags, "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "ccs_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tools", name + "_sanitize", "main.cpp"), "-o", run[0]])
    return subprocess.call(run + list(args))

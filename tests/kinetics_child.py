"""A fresh process for tests/test_kinetics_gpu.py::test_launch_pieces: the named batch of tests/kinetics_lab.py through ccsx_consensus_pileup on a handle with
opts.hifi_kinetics, under whatever CCSX_POLISH_MAX_BLOCKS the parent set (the library reads it once per process).  Prints `sha <sha256 of the results>`."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
from ccs_amd import api  # noqa: E402
import kinetics_lab as Lab  # noqa: E402

name = sys.argv[1]
b = Lab.BATCHES[name]()
h = api.Handle(0, opts=Lab.kin_opts(**Lab.OPTS.get(name, {})))
res, pile = h.consensus_pileup(b)
print("sha", hashlib.sha256(Lab.result_bytes(res)).hexdigest(), "windows", int(res.n_windows.sum()))
h.close()

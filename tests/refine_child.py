"""A fresh process for tests/test_refine_gpu.py: torch opens the GPU before the engine does (the two share one HIP runtime only in that order), the tile list
of test_device_resident_tiles lives in torch tensors on the handle's GPU, and the hand-back runs through the synchronous and the ticketed form.  Prints
`sha <form> <sha256 of results and report>` lines."""
import hashlib
import os
import sys

import torch

torch.cuda.init()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from ccs_amd import api  # noqa: E402
import test_refine_gpu as t  # noqa: E402

h = api.Handle(0, opts=t.lab_opts())
lab = t.Lab(h)
tiles = t.tiles_of(t.child_rows(lab), device=h.device)
assert tiles.on_device and tiles.new_seq.is_cuda and tiles.n_tiles > 20
res, rep = h.refine(lab.batch, lab.base, tiles, lab.backbone)
print("sha sync", hashlib.sha256(t.res_bytes(res) + t.rep_bytes(rep)).hexdigest())
b = lab.batch.pinned()
res2, rep2 = api.Results.allocate(b, pinned=True), api.RefineReport.allocate(b, pinned=True)
tk = h.submit_refine(b, lab.base, tiles, lab.backbone, res2, rep2)
h.wait(tk)
h.release(tk)
print("sha ticket", hashlib.sha256(t.res_bytes(res2) + t.rep_bytes(rep2)).hexdigest())
h.close()

"""A fresh process for tests/test_handoff_gpu.py.  `device`: torch opens the GPU before the engine does (the two share one HIP runtime only in that order), the
hand-off lands in torch tensors through the synchronous and the ticketed form; `pieces`: a host destination, for a run under CCSX_POLISH_MAX_BLOCKS.  Prints
`sha <what> <sha256 of the written slots>` lines for the batch and options of BATCH / OPTS."""
import hashlib
import os
import sys

mode = sys.argv[1]
if mode == "device":
    import torch
    torch.cuda.init()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from ccs_amd import api  # noqa: E402
import test_handoff_gpu as t  # noqa: E402

b = api.synth(*t.CHILD_BATCH[0], seed=t.CHILD_BATCH[1])
o = t.hopts(*t.CHILD_OPTS)
h = api.Handle(0)
if mode == "device":
    _, ho = h.consensus_handoff(b, opts=o, device=True)
    assert ho.on_device and ho.cells.is_cuda and ho.tile(0)["cells"].shape[0] == o.max_rows
    host = ho.host()
    n = ho.n_tiles
    on_gpu = int((ho.cells[:n, :, :, 0] < 4).sum().item())            # a consumer on the same GPU reads the tensor where it is
    assert on_gpu == int((host.cells[:n, :, :, 0] < 4).sum()) > 0
    print("sha sync", hashlib.sha256(t.ho_bytes(ho)).hexdigest())
    ho2 = api.Handoff.allocate(b, None, o, device=h.device)
    res = api.Results.allocate(b, pinned=True)
    tk = h.submit(b.pinned(), res, handoff=ho2)
    h.wait(tk)
    h.release(tk)
    print("sha ticket", hashlib.sha256(t.ho_bytes(ho2)).hexdigest())
else:
    _, ho = h.consensus_handoff(b, opts=o)
    print("sha sync", hashlib.sha256(t.ho_bytes(ho)).hexdigest())
h.close()

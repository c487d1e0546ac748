#!/usr/bin/env python3
"""What the training counts cost (ccsx_train_batch, k_train) beside the polish of the same batch.  Default: 4096 ZMWs x 10 passes x 10 kb of api.synth, the fused
consensus handed back as drafts.  Per round the stage times of ccsx_timings (the training stage sits where the polish stage does: polish_ms is k_train with its
memsets) and the wall time of the synchronous call; the pairs and bases counted.  Writes every line it prints to --out (profiles/train_bench.txt).
    python tools/train_bench.py [--zmws N --passes P --length L --rounds R --out FILE]
For a kernel trace: rocprofv3 --kernel-trace --stats -d OUT -- python tools/train_bench.py --rounds 1"""
import argparse
import os
import sys
import time

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
from ccs_amd import api  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--zmws", type=int, default=4096)
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--length", type=int, default=10000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(R, "profiles", "train_bench.txt"))
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    b = api.synth(a.zmws, a.passes, a.length, seed=1)
    h = api.Handle(0)
    say(f"train_bench: {a.zmws} ZMWs x {a.passes} passes x {a.length} bases; library abi {api.lib().ccsx_abi_version()} spec {api.lib().ccsx_spec_version()} "
        f"train rule {api.lib().ccsx_train_rule_version()}; runtime switches '{api.lib().ccsx_runtime_switches().decode()}'")
    d0 = h.draft(b)
    res = h.consensus(b)
    t = h.timings()
    say(f"consensus of the batch: draft {t.draft_ms:.1f} ms, align {t.align_ms:.1f} ms, polish {t.polish_ms:.1f} ms, total {t.total_ms:.1f} ms; "
        f"{int((res.status == 0).sum())} ZMWs succeed, {int(res.n_windows.sum())} windows")
    d = api.Drafts.allocate(b)
    for z in range(b.n_zmw):
        if res.status[z] == 0:
            d.set_draft(z, res.sequence(z), backbone=int(d0.backbone[z]))
    first = None
    for r in range(a.rounds):
        t0 = time.perf_counter()
        tc = h.train_counts(b, d)
        wall = (time.perf_counter() - t0) * 1e3
        t = h.timings()
        pairs, bases = int(tc.n_pairs.sum()), int(tc.n_bases.sum())
        say(f"round {r}: k_train stage {t.polish_ms:.1f} ms ({pairs / max(t.polish_ms, 1e-9) / 1e3:.2f} M pairs/s), draft-in + cascade {t.align_ms + t.draft_ms:.1f} ms, "
            f"kernels {t.total_ms:.1f} ms, call {wall:.1f} ms; {pairs} pairs counted, {int(tc.n_gated.sum())} gated, {bases} bases, "
            f"log2-likelihood per base {tc.loglik.sum() / 65536.0 / max(bases, 1):.5f}")
        key = [getattr(tc, k).tobytes() for k, _, _ in api.TrainCounts.PLANES]
        if first is None:
            first = key
        elif key != first:
            say("round differs from round 0: the counts are NOT reproducible")
            return 1
    ok = tc.status == 0
    say(f"events per ZMW (mean over {int(ok.sum())}): match {tc.match[ok].sum() / 2.0 ** 32 / ok.sum():.1f}, stay {tc.stay[ok].sum() / 2.0 ** 32 / ok.sum():.1f}, "
        f"deletion {tc.del_[ok].sum() / 2.0 ** 32 / ok.sum():.1f}; all rounds bit-identical")
    fit, rep = api.Fitter(h.model).add(tc, b.snr).finish()
    say(f"fitter on these counts: contexts kept {rep.contexts_kept}, SNR range {rep.snr_lo:.3f} .. {rep.snr_hi:.3f}, largest parameter change {rep.max_change:.4f}")
    h.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

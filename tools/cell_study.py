#!/usr/bin/env python3
"""The study behind the `indels` default of the cell-tag rule and the advice on dense whitelists (DESIGN.md §2 "Cell-tag rule", §7), on the CPU: molecules
5p . insert . A x 30 . rc(barcode . UMI) . rc(3p) (the default design), every second one reverse complemented, each with a barcode planted from the whitelist
and a random UMI, are sequenced into 3, 6 and 10 passes (tools/lowcx.py, the numpy channel), the oracle makes their consensus, and the host rule
(ccsx_cell_reads_host) reads the tags.  Whitelists of 4096, 2^16 and 2^20 random 16-mers, with `indels` 0 and 1.  Per configuration: the shares exact /
corrected / ambiguous / absent of the reads that reach the tag, the share called (exact or corrected) to a barcode that was not planted, and how many UMIs come
out as planted among the reads called to the planted barcode.  A second table takes the channel out: random 16-mers that are nobody's barcode against the
same whitelists, the share that reaches a stranger — the whitelist's density alone.
    python tools/cell_study.py [--out profiles/cell_study.txt]"""
import argparse
import os
import sys

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tools"))
sys.path.insert(0, os.path.join(R, "tests"))
from ccs_amd import api  # noqa: E402
import adapter_synth  # noqa: E402
import cell_ref as REF  # noqa: E402
import oracle_lib  # noqa: E402

M, SEED, N_MOL, INSERT, B, U = 25, 8100, 192, (300, 501), 16, 12
SIZES = (4096, 1 << 16, 1 << 20)
N_STRANGERS = 20000


def whitelist(rng, n) -> np.ndarray:
    keys = np.unique(rng.integers(0, 1 << 32, n + n // 4, dtype=np.uint64))
    rng.shuffle(keys)
    return ((keys[:n, None] >> (2 * (B - 1 - np.arange(B, dtype=np.uint64)))[None, :]) & np.uint64(3)).astype(np.uint8)


def consensus(tpls, passes, rng):
    b = adapter_synth.from_templates(tpls, [passes] * len(tpls), rng)
    res = api.Results.allocate(b)
    oracle_lib.consensus_batch(api.default_model(), api.default_opts(), b, res, nthreads=min(16, os.cpu_count() or 1))
    return [res.sequence(z).copy() if res.seq_len[z] > 0 else np.zeros(0, np.uint8) for z in range(b.n_zmw)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(R, "profiles", "cell_study.txt"))
    a = ap.parse_args()
    rng = np.random.default_rng(SEED)
    p5, p3 = REF.random_set(rng, 2, [M])
    pset = api.CdnaPrimers.from_codes([p5, p3], [0, 1])
    lists = {n: whitelist(rng, n) for n in SIZES}
    objs = {n: api.CellWhitelist(w) for n, w in lists.items()}
    d0 = api.CellDesign.default()
    lines = [f"cell tags: two random {M}-mers as 5' and 3' primer, the default design ({U} U, {B} B at the 3' primer, the barcode next to it); per pass count {N_MOL} molecules "
             f"with inserts of {INSERT[0]}-{INSERT[1] - 1} bases and a tail of 30 A, a barcode planted from the whitelist and a random UMI, every second molecule reverse "
             f"complemented; tools/lowcx.py channel, oracle consensus, ccsx_cell_reads_host; seed {SEED}", f"shipped default: indels {d0.indels}", "",
             "passes  whitelist  indels   reads at the tag   exact   corrected   ambiguous   absent   called to a barcode not planted   UMI as planted (of the reads called to the planted)"]
    total = {}
    for passes in (3, 6, 10):
        per = {}
        for n in SIZES:                                              # (the same molecules but for the planted barcodes, which are the whitelist's)
            mrng = np.random.default_rng(SEED + passes)
            planted = mrng.integers(0, n, N_MOL)
            umis = [REF.rand(mrng, U) for _ in range(N_MOL)]
            tpls = [REF.cmol(REF.DESIGN, p5, p3, REF.body(mrng, int(mrng.integers(*INSERT))), lists[n][planted[z]], umis[z]) for z in range(N_MOL)]
            tpls = [REF.rc(t) if z & 1 else t for z, t in enumerate(tpls)]
            reads = consensus(tpls, passes, mrng)
            for indels in (0, 1):
                d = api.CellDesign.default()
                d.indels = indels
                rep = api.cell_reads_host(pset, reads, d, objs[n])
                at = rep.tag != api.CELL_NONE
                called = at & ((rep.tag == api.CELL_EXACT) | (rep.tag == api.CELL_CORRECTED))
                wrong = called & (rep.bc != planted)
                right = called & (rep.bc == planted)
                umi_ok = sum(1 for z in np.flatnonzero(right) if int(rep.umi[z]) == REF.pack(umis[z]))
                row = [int(at.sum())] + [int((rep.tag[at] == t).sum()) for t in (api.CELL_EXACT, api.CELL_CORRECTED, api.CELL_AMBIGUOUS, api.CELL_ABSENT)] + \
                      [int(wrong.sum()), umi_ok, int(right.sum())]
                per[(n, indels)] = row
                t = total.setdefault((n, indels), [0] * 8)
                for k, v in enumerate(row):
                    t[k] += v
                lines.append(f"{passes:6d}  {n:9d}  {indels:6d}   {row[0]:17d}   {row[1]:5d}   {row[2]:9d}   {row[3]:9d}   {row[4]:6d}   {row[5]:31d}   {row[6]} of {row[7]}"
                             + ("   <- shipped" if indels == d0.indels else ""))
        lines.append("")
    lines.append("all pass counts together: shares of the reads at the tag")
    for (n, indels), t in total.items():
        s = max(t[0], 1)
        lines.append(f"  whitelist {n:7d} indels {indels}: exact {100 * t[1] / s:5.1f} %, corrected {100 * t[2] / s:5.1f} %, ambiguous {100 * t[3] / s:5.1f} %, absent {100 * t[4] / s:5.1f} %, "
                     f"called to a barcode not planted {100 * t[5] / s:5.2f} % ({t[5]} of {t[0]}); UMI as planted {t[6]} of {t[7]}" + ("   <- shipped" if indels == d0.indels else ""))
    lines += ["", f"the whitelist's density alone: {N_STRANGERS} random 16-mers that are no member, behind an exact 3' primer; the share whose candidates reach a member (called), or two",
              "whitelist  indels   candidates   called to a stranger   ambiguous   expected called = candidates x n / 4^16"]
    srng = np.random.default_rng(SEED + 1)
    fields = srng.integers(0, 4, (N_STRANGERS, B)).astype(np.uint8)
    ins = REF.body(srng, 60)
    reads = [REF.cmol(REF.DESIGN, p5, p3, ins, fields[z], REF.rand(srng, U)) for z in range(N_STRANGERS)]
    o = api.cdna_opts_default()
    for n in SIZES:
        member = set(map(bytes, lists[n]))
        keep = np.array([bytes(f) not in member for f in fields])
        for indels in (0, 1):
            d = api.CellDesign.default()
            d.indels = indels
            rep = api.cell_reads_host(pset, reads, d, objs[n], o)
            k = int(keep.sum())
            cand = 3 * B + (5 * B if indels else 0)
            lines.append(f"{n:9d}  {indels:6d}   {cand:10d}   {100 * int((rep.tag[keep] == api.CELL_CORRECTED).sum()) / k:19.2f} %   {100 * int((rep.tag[keep] == api.CELL_AMBIGUOUS).sum()) / k:7.2f} %   "
                         f"{100 * cand * n / 4.0 ** B:6.2f} %")
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()

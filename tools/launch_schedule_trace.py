#!/usr/bin/env python3
"""Does a change to the launch schedule (ccsx_launch_all) leave the sequence of HIP calls of a batch as it was?

    python tools/launch_schedule_trace.py --parent DIR [--new DIR] [--dir OUT] [--out profiles/launch_schedule_trace.txt]

DIR is a built tree of the parent commit (git worktree add DIR HEAD~1, then python __graft_entry__.py there); --new defaults to this tree.  For each tree one
scripted process runs under `rocprofv3 --hip-trace --kernel-trace` (no counters), once with a clean environment and once with CCSX_POLISH_MAX_BLOCKS=40
CCSX_ALIGN16_MAX_SLOTS=64 (the polish stage and the alignment cascade in pieces).  The process (`--batches`) puts one batch of 4608 ZMWs of short reads —
enough for the two-stream POA round and the trace-backs aside — through every run mode: fused with kinetics, pileup, tandem repeats and the heteroduplex
split; fused with the same extras and the three draft screens (the finder and the screens are not combined in one call); the draft seam; the polish seam;
ccsx_hd_batch.

From each trace comes the ordered list of hipLaunchKernel*, hipEventRecord, hipStreamWaitEvent and hipMemsetAsync calls, streams and events renamed by order of
first appearance, a launch with its kernel, grid (threads), workgroup size and LDS bytes as dispatched.  The lists of the two trees must be identical.  The
output file holds the verdict, each list's length and SHA-256, and the new tree's lists with repeated runs of lines folded.  --skip-trace reads the traces
already in --dir.  Exit status 0 = identical."""
import argparse
import glob
import hashlib
import os
import shutil
import sqlite3
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENVS = {"clean": {}, "pieces": {"CCSX_POLISH_MAX_BLOCKS": "40", "CCSX_ALIGN16_MAX_SLOTS": "64"}}
CALLS = ("hipLaunchKernel", "hipExtLaunchKernel", "hipModuleLaunchKernel", "hipExtModuleLaunchKernel", "hipEventRecord", "hipStreamWaitEvent", "hipMemsetAsync")


def batches(root):
    """the scripted process"""
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tools"))
    from ccs_amd import api
    import control_synth
    opts = api.default_opts()
    opts.hifi_kinetics = 1
    h = api.Handle(0, opts=opts)
    b = api.synth(4608, (3, 5), (150, 420), seed=77)
    h.consensus_hd(b, split=True, tandem=True, pileup=True)
    h.consensus_control(b, api.ControlSeq.from_string(control_synth.TEST_CONTROL), fold=True, adapters=api.AdapterSet.default(), tandem=True, pileup=True)
    d = h.draft(b)
    res = h.polish(b, d)
    rep = h.hd(b, d)
    print("batches done:", int((res.status == 0).sum()), "of", b.n_zmw, "ZMWs polished,", int((rep.verdict != 0).sum()), "tested by the finder", flush=True)
    h.close()


def trace(root, env_name, out_dir):
    """one profiled process; returns the directory of its trace"""
    d = os.path.join(out_dir, env_name)
    os.makedirs(d, exist_ok=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("CCSX_")}
    env.update(ENVS[env_name])
    cmd = ["timeout", "-k", "10", "420", shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3", "--hip-trace", "--kernel-trace", "--output-format", "rocpd", "-d", d, "-o", "trace", "--",
           sys.executable, os.path.abspath(__file__), "--batches", root]
    print("+", " ".join(cmd), flush=True)
    subprocess.run(cmd, env=env, check=True)     # (a failed or timed-out process ends the whole run: nothing more is started on the device)
    return d


def call_list(trace_dir):
    """the ordered calls of one trace as lines"""
    dbs = sorted(glob.glob(os.path.join(trace_dir, "**", "*.db"), recursive=True))
    if len(dbs) != 1:
        raise SystemExit(f"{trace_dir}: expected one rocpd database, found {dbs}")
    db = sqlite3.connect(dbs[0])
    marks = ",".join("?" * len(CALLS))
    regions = db.execute(f"SELECT id, name, stack_id FROM regions WHERE name IN ({marks}) ORDER BY start, id", CALLS).fetchall()
    args = {}
    for rid, name, value in db.execute("SELECT id, name, value FROM region_args"):
        args.setdefault(rid, {})[name] = value
    kernels = {}
    for corr, name, sid, gx, gy, gz, wx, wy, wz, lds in db.execute(
            "SELECT stack_id, name, stream_id, grid_x, grid_y, grid_z, workgroup_x, workgroup_y, workgroup_z, lds_size FROM kernels"):
        kernels.setdefault(corr, []).append((name, sid, f"grid {gx}x{gy}x{gz} wg {wx}x{wy}x{wz} lds {lds}"))   # (a hipMemsetAsync may dispatch several fill kernels)
    names = {}

    def alias(kind, value):
        if value is None:
            return kind + "?"
        return names.setdefault((kind, value), f"{kind}{sum(1 for k in names if k[0] == kind)}")

    lines = []
    for rid, name, corr in regions:
        a = args.get(rid, {})
        stream = alias("stream", a["stream"]) if "stream" in a else None
        if "Launch" in name:
            if len(kernels.get(corr, ())) != 1:
                raise SystemExit(f"{trace_dir}: {name} (correlation {corr}) has {len(kernels.get(corr, ()))} kernel dispatches")
            k = kernels[corr][0]
            lines.append(f"{name} {k[0]} {k[2]} {stream or alias('queue', k[1])}")
        elif name == "hipMemsetAsync":
            lines.append(f"{name} {a.get('sizeBytes', a.get('count', '?'))} bytes of {a.get('value', '?')} {stream or 'stream?'}")
        else:
            lines.append(f"{name} {alias('event', a.get('event'))} {stream or 'stream?'}")
    if not lines:
        raise SystemExit(f"{trace_dir}: no calls in the trace")
    return lines


def folded(lines, max_period=32):
    """consecutive repeats of a block of up to max_period lines as one block with a count"""
    out, i = [], 0
    while i < len(lines):
        best = (1, 1)
        for p in range(1, min(max_period, (len(lines) - i) // 2) + 1):
            r = 1
            while lines[i + r * p:i + (r + 1) * p] == lines[i:i + p]:
                r += 1
            if r > 1 and p * r > best[0] * best[1]:
                best = (p, r)
        p, r = best
        if r == 1:
            out.append(lines[i])
        else:
            out.append(f"{r} times:")
            out += ["    " + x for x in lines[i:i + p]]
        i += p * r
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", metavar="ROOT", help="run the scripted process on the tree ROOT (what the profiler is given)")
    ap.add_argument("--parent", help="built tree of the parent commit")
    ap.add_argument("--new", default=HERE, help="built tree of the new commit (default: this one)")
    ap.add_argument("--dir", default="launch_schedule_traces", help="where the traces go")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "launch_schedule_trace.txt"))
    ap.add_argument("--skip-trace", action="store_true", help="the traces are in --dir already")
    a = ap.parse_args()
    if a.batches:
        return batches(os.path.abspath(a.batches))
    if not a.parent:
        ap.error("--parent is needed")
    trees = {"parent": os.path.abspath(a.parent), "new": os.path.abspath(a.new)}
    report, same = [], True
    for env_name, env in ENVS.items():
        lists = {}
        for which, root in trees.items():
            d = os.path.join(a.dir, which)
            lists[which] = call_list(os.path.join(d, env_name) if a.skip_trace else trace(root, env_name, d))
        digest = {w: hashlib.sha256("\n".join(x).encode()).hexdigest() for w, x in lists.items()}
        equal = lists["parent"] == lists["new"]
        same = same and equal
        report.append(f"== environment: {' '.join(f'{k}={v}' for k, v in env.items()) or 'clean'}")
        for w in trees:
            report.append(f"{w:6s} {len(lists[w])} calls, sha256 {digest[w]}")
        report.append("IDENTICAL" if equal else "DIFFERENT")
        if not equal:
            n = next((i for i, (x, y) in enumerate(zip(lists["parent"], lists["new"])) if x != y), min(len(lists["parent"]), len(lists["new"])))
            report.append(f"first difference at call {n}:")
            report += [f"  parent: {x}" for x in lists["parent"][n:n + 5]] + [f"  new:    {x}" for x in lists["new"][n:n + 5]]
        report.append("the new tree's calls in order:")
        report += ["  " + x for x in folded(lists["new"])]
        report.append("")
    report.insert(0, "verdict: the parent's and the new tree's call sequences are " + ("IDENTICAL in both environments" if same else "DIFFERENT") + "\n")
    with open(a.out, "w") as f:
        f.write("\n".join(report))
    print(report[0], "->", a.out)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())

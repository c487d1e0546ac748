"""`ccs --gpu-inflate`: the BGZF blocks of IN are inflated by k_inflate.  Every output byte, every error text and every exit code is what it is without the flag."""
import gzip
import os
import subprocess

import pytest

import bam_util  # noqa: F401  (the tests' directory is importable: same check as the other CLI tests)
from ccs_amd import api

CCS = os.path.join(os.path.dirname(api.LIB_PATH), "bin", "ccs")


def _run(*args):
    return subprocess.run([CCS, *map(str, args)], capture_output=True, text=True, timeout=600)


def _outputs(out):
    p = str(out)[:-len(".bam")]
    files = {"bam": str(out), "pbi": str(out) + ".pbi", "report": p + ".ccs_report.txt", "metrics": p + ".zmw_metrics.json.gz"}
    got = {}
    for k, f in files.items():
        raw = open(f, "rb").read()
        got[k] = gzip.decompress(raw) if k == "metrics" else raw
    return got


def test_help_names_the_flag(built):
    p = _run("--help")
    assert p.returncode == 0 and "--gpu-inflate" in p.stderr


def test_flag_is_ignored_with_host_only_when_no_device_is_present(built, tmp_path):
    if api.device_count() > 0:
        pytest.skip("a device is present: the flag is used")
    bam = tmp_path / "s.subreads.bam"
    assert _run("--write-synthetic", "12,4,500,5", bam).returncode == 0
    p = _run("--host-only", "--gpu-inflate", "--log-level", "INFO", bam)
    assert p.returncode == 0 and "--gpu-inflate ignored" in p.stderr and "12 ZMWs read" in p.stdout


@pytest.fixture(scope="module")
def subreads(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_inflate")
    bam = d / "s.subreads.bam"
    assert _run("--write-synthetic", "48,6,1500,7", bam).returncode == 0       # several BGZF blocks per ZMW, more than one slab with the kinetics tags
    return bam


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [(), ("--chunk", "2/3"), ("--hifi-kinetics",)], ids=["plain", "chunk-2-of-3", "hifi-kinetics"])
def test_outputs_are_byte_identical(subreads, tmp_path, extra):
    off, on = tmp_path / "off" / "o.bam", tmp_path / "on" / "o.bam"
    os.makedirs(off.parent)
    os.makedirs(on.parent)
    a = _run(subreads, off, *extra)
    b = _run(subreads, on, "--gpu-inflate", "--log-level", "INFO", *extra)
    assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
    assert "--gpu-inflate: " in b.stderr                                        # the flag was used, not ignored
    x, y = _outputs(off), _outputs(on)
    assert len(x["bam"]) > 1000
    for k in x:
        assert x[k] == y[k], k


@pytest.mark.gpu
def test_broken_inputs_fail_as_without_the_flag(subreads, tmp_path):
    raw = bytearray(open(subreads, "rb").read())
    blocks, at = [], 0
    while at < len(raw):
        size = (raw[at + 16] | (raw[at + 17] << 8)) + 1
        blocks.append((at, size))
        at += size
    assert len(blocks) > 4
    flipped = bytearray(raw)
    s, n = blocks[len(blocks) // 2]
    flipped[s + 18 + (n - 26) // 2] ^= 0x04                                     # one bit in the middle of a payload
    cut = raw[:blocks[-2][0] + blocks[-2][1] // 2]                              # the last data block (the one before the EOF marker) cut in half
    for name, data in (("flipped", flipped), ("truncated", cut)):
        bad = tmp_path / f"{name}.subreads.bam"
        open(bad, "wb").write(bytes(data))
        res = []
        for flag in ((), ("--gpu-inflate",)):
            out = tmp_path / f"{name}{len(flag)}.bam"
            p = _run(bad, out, *flag)
            res.append((p.returncode, p.stderr.strip().splitlines()[-1]))
            assert not os.path.exists(out), name
        assert res[0] == res[1], (name, res)
        assert res[0][0] == 1 and "BGZF" in res[0][1], (name, res)

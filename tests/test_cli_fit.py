"""ccs --fit-model OUT.json IN.subreads.bam (DESIGN.md §2 "Model training"): the mode's usage errors, and on an MI355X a small synthetic BAM fitted for two
iterations: the json loads, carries the header's chemistry triple and the name fit-<start>, every iteration logs one INFO line, and two runs of one iteration
chained through the file of the first (--model-file) give the parameters of one run of two iterations."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from ccs_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CCS = os.path.join(ROOT, "ccs_amd", "bin", "ccs")


@pytest.mark.parametrize("extra", [["out.bam"], ["--fail-reads", "f.bam"], ["--by-strand"], ["out.fastq.gz"], ["--gpus", "0,1"], ["--fit-iterations", "0"],
                                   ["--fit-degree", "4"], ["--control", "c.fasta"], ["--gpu-inflate"], ["--metrics-json", "m.gz"], ["--report-json", "r.json"],
                                   ["--hifi-summary-json", "h.json"], ["--report-file", "r.txt"], ["--pileup-summary"], ["--qv-binning"], ["--hifi-kinetics"],
                                   ["--min-tandem-repeat-length", "500"], ["--suppress-reports"], ["--chunk", "1/2"]])
def test_usage_errors(built, tmp_path, extra):
    p = subprocess.run([CCS, "--fit-model", "m.json", "in.bam", *extra], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert p.returncode == 2 and "--fit-model" in p.stderr and not os.path.exists(tmp_path / "m.json")


def test_option_is_documented(built):
    usage = subprocess.run([CCS, "--help"], capture_output=True, text=True, timeout=60).stderr
    for o in ("--fit-model", "--fit-iterations", "--fit-min-rq", "--fit-max-zmws", "--fit-degree"): assert o in usage


def test_a_missing_input_writes_no_json(built, tmp_path):
    p = subprocess.run([CCS, "--fit-model", "m.json", "nothing.bam"], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert p.returncode == 1 and not os.path.exists(tmp_path / "m.json")


@pytest.mark.gpu
def test_fit_model_on_a_synthetic_bam(built, tmp_path):
    bam, out = tmp_path / "s.subreads.bam", tmp_path / "fit.json"
    subprocess.run([CCS, "--write-synthetic", "24,8,1500,5", bam], check=True, capture_output=True, timeout=120)
    p = subprocess.run([CCS, "--fit-model", out, bam, "--fit-iterations", "2", "--fit-min-rq", "0.99", "--fit-max-zmws", "20", "--log-level", "INFO"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = re.findall(r"--fit-model iteration (\d+): (\d+) ZMWs used, (\d+) pairs, (\d+) gated, log2-likelihood per base (-?[\d.]+), largest parameter change ([\d.e+-]+)", p.stderr)
    assert [int(l[0]) for l in lines] == [1, 2] and all(0 < int(l[1]) <= 20 and int(l[2]) > 1000 for l in lines), p.stderr[-2000:]
    text = open(out).read()
    j = json.loads(text)
    fit = api.model_from_json(text)
    start = api.default_model()
    assert fit.name == b"fit-" + start.name and j["ConsensusModelVersion"] == "ccsx-1"
    assert "101-789-500" in text and "101-826-100" in text and "5.0.0" in text and bytes(fit)[32:] != bytes(start)[32:]
    assert start.snr_lo <= fit.snr_lo <= fit.snr_hi <= start.snr_hi
    for key in ("em_match", "em_branch", "em_stick"):
        rows = np.array(getattr(fit, key), np.float64)
        assert np.all(rows > 0) and np.all(np.abs(rows.sum(1) - 1.0) <= 4 * 2.0 ** -23)
    # the second iteration ran with the first one's model: its likelihood is the higher one
    assert float(lines[1][4]) > float(lines[0][4]), lines
    # one iteration more = a start from the file of one iteration less
    p1 = subprocess.run([CCS, "--fit-model", tmp_path / "one.json", bam, "--fit-iterations", "1", "--fit-min-rq", "0.99", "--fit-max-zmws", "20"], capture_output=True, text=True, timeout=300)
    assert p1.returncode == 0, p1.stderr[-2000:]
    p2 = subprocess.run([CCS, "--fit-model", tmp_path / "two.json", bam, "--fit-iterations", "1", "--fit-min-rq", "0.99", "--fit-max-zmws", "20", "--model-file", tmp_path / "one.json"],
                        capture_output=True, text=True, timeout=300)
    assert p2.returncode == 0, p2.stderr[-2000:]
    two = api.model_from_json(open(tmp_path / "two.json").read())
    assert two.name == b"fit-fit-" + start.name and bytes(two)[32:] == bytes(fit)[32:]

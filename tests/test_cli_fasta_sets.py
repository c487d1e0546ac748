"""The FASTA files of `ccs --adapters`, `--barcodes`, `--segment-adapters` and `--control` go through one reader (ccs_main.cpp load_fasta_set): the same
malformed file gives exit 2 and the same message under each option, with the option's own limits and the record named as `record k (>name)`; a well-formed
file with CRLF line ends, trailing blanks and lower case is read, and the run goes on to its next usage check.  No GPU: every run ends in parse()."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CCS = os.path.join(ROOT, "ccs_amd", "bin", "ccs")
# option: (what else the command line needs, records of a well-formed file, fewest and most bases of a record)
OPTIONS = {"--adapters": (["--fail-reads", "f.bam"], 1, 16, 64), "--barcodes": ([], 1, 8, 64), "--segment-adapters": ([], 2, 8, 64),
           "--control": ([], 1, 64, 4096)}


def _seq(n, shift=0):
    return "".join("ACGT"[(i * 7 + i // 3 + shift) % 4] for i in range(n))


def _run(tmp_path, option, path, *more):
    p = subprocess.run([CCS, "in.bam", "out.bam", *OPTIONS[option][0], option, path, *more], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    return p.returncode, p.stderr


def _records(option, last):
    """a well-formed file's records but for the last one, whose sequence lines are `last`"""
    _, n, lo, _ = OPTIONS[option]
    return "".join(f">rec{k + 1} first records\n{_seq(lo, k)}\n" for k in range(n - 1)) + f">rec{n} the last one\n" + last


@pytest.mark.parametrize("option", list(OPTIONS))
def test_malformed_files_are_refused_alike(built, tmp_path, option):
    _, n, lo, hi = OPTIONS[option]
    where = f"record {n} (>rec{n} the last one): "
    cases = {"empty.fa": ("", "no FASTA record"),
             "early.fa": (_seq(lo) + "\n>late\n" + _seq(lo) + "\n", "sequence before the first '>' line"),
             "other.fa": (_records(option, _seq(lo - 1) + "\nN\n"), where + "'N' is not one of ACGT"),
             "long.fa": (_records(option, _seq(hi - 3) + "\n" + _seq(4) + "\n"), where + f"more than {hi} bases"),
             "short.fa": (_records(option, _seq(lo - 1) + "\n"), where + f"{lo - 1} bases, fewer than {lo}")}
    for name, (text, tail) in cases.items():
        (tmp_path / name).write_text(text)
    cases["missing.fa"] = (None, "cannot open the file")
    for name, (_, tail) in cases.items():
        rc, err = _run(tmp_path, option, name)
        assert rc == 2 and f"ccs: {option} {name}: {tail}\n" in err, (name, err)


@pytest.mark.parametrize("option", list(OPTIONS))
def test_names_are_cut_at_60_characters(built, tmp_path, option):
    _, n, lo, _ = OPTIONS[option]
    name = ">" + "x" * 80
    (tmp_path / "cut.fa").write_text(_records(option, "").replace(f">rec{n} the last one", name) + _seq(lo - 1) + "\n")
    rc, err = _run(tmp_path, option, "cut.fa")
    assert rc == 2 and f"record {n} ({name[:60]}): {lo - 1} bases" in err, err


@pytest.mark.parametrize("option", list(OPTIONS))
def test_too_many_records(built, tmp_path, option):
    _, _, lo, _ = OPTIONS[option]
    most = {"--adapters": 8, "--barcodes": 384, "--segment-adapters": 33, "--control": 1}[option]
    (tmp_path / "many.fa").write_text("".join(f">r{k + 1}\n{_seq(lo, k)}\n" for k in range(most + 1)))
    rc, err = _run(tmp_path, option, "many.fa")
    tail = "more than one record" if most == 1 else f"more than {most} records"
    assert rc == 2 and f"ccs: {option} many.fa: record {most + 1} (>r{most + 1}): {tail}\n" in err, err


def test_an_array_needs_two_adapters(built, tmp_path):
    (tmp_path / "one.fa").write_text(">only\n" + _seq(25) + "\n")
    rc, err = _run(tmp_path, "--segment-adapters", "one.fa")
    assert rc == 2 and "ccs: --segment-adapters one.fa: record 1 (>only): the only record, an array has at least 2 adapters\n" in err, err


@pytest.mark.parametrize("option", list(OPTIONS))
def test_crlf_blanks_and_lower_case_are_read(built, tmp_path, option):
    """the file is accepted: the run ends at the next usage check behind the four readers, with that check's message alone"""
    _, n, lo, hi = OPTIONS[option]
    text = "\r\n".join(f">rec{k + 1}  \r\n{_seq(lo, k).lower()} \t\r\n\r\n{_seq(hi - lo, k + 1)}" for k in range(n)) + "\r\n"
    (tmp_path / "good.fa").write_bytes(text.encode())
    rc, err = _run(tmp_path, option, "good.fa", "--coverage-block", "5")
    assert rc == 2 and "--coverage-filters" in err and "good.fa" not in err, err

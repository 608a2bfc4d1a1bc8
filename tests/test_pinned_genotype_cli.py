"""CPU: bin/DipGenie rejects a bad --pinned-genotype-margins / --pinned-genotype-table before it needs a device."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

PINS = ["--pins", "p.pins"]                              # (never opened: the checks below come first)


@pytest.mark.parametrize("option", ["--pinned-genotype-margins", "--pinned-genotype-table"])
@pytest.mark.parametrize("extra,word", [
    (lambda o: ["-p2", "-R4", o, "m.tsv"], b"--pins"), (lambda o: ["-p2", "-R4", o + "=m.tsv"], b"--pins"),                 # without --pins
    (lambda o: ["-p2", "-R4", o, "m.tsv", "--genotype-table", "t.tsv"], b"--pins"),
    (lambda o: ["-p1", o, "m.tsv"] + PINS, b"-p2"), (lambda o: ["-p1", "-R4", o + "=m.tsv"] + PINS, b"-p2"),
    (lambda o: ["-p2", "-R4", o, ""] + PINS, b"file name"), (lambda o: ["-p2", "-R4", o + "="] + PINS, b"file name"), (lambda o: ["-p2", "-R4"] + PINS + [o], b"file name"),
    (lambda o: ["-p2", "-R4", o, "m.tsv", "--gpus", "2"] + PINS, b"--gpus"), (lambda o: ["-p2", "-R4", "--gpus=2", o + "=m.tsv"] + PINS, b"--gpus"),
])
def test_cli_rejects_bad_pinned_genotype_options_before_any_device_call(built_hip, tmp_path, option, extra, word):
    """exit status 1, a message that names the option, no FASTA and no FILE -- on a machine without a GPU too: the check comes before
    the device (and before the pins file is opened)"""
    out = tmp_path / "o.fa"
    p = subprocess.run([built_hip, "-k11", "-w5", "-g", os.path.join(ROOT, "tests", "golden", "e2e", "bub_a.gfa"), "-r", os.path.join(ROOT, "tests", "golden", "e2e", "bub_a.fa"),
                        "-o", str(out), *extra(option)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=tmp_path)
    assert p.returncode == 1, (p.returncode, p.stderr)
    assert option.encode() in p.stderr and word in p.stderr and b"no CPU fallback" not in p.stderr, p.stderr
    assert p.stdout == b"" and not out.exists() and os.listdir(tmp_path) == []


def test_without_pins_the_message_names_both_options(built_hip, tmp_path):
    p = subprocess.run([built_hip, "-k11", "-w5", "-g", os.path.join(ROOT, "tests", "golden", "e2e", "bub_a.gfa"), "-r", os.path.join(ROOT, "tests", "golden", "e2e", "bub_a.fa"),
                        "-o", str(tmp_path / "o.fa"), "--pinned-genotype-table", "t.tsv"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=tmp_path)
    assert p.returncode == 1 and b"--pinned-genotype-margins" in p.stderr and b"--pinned-genotype-table" in p.stderr and b"--pins" in p.stderr, p.stderr
    assert os.listdir(tmp_path) == []


def test_usage_names_the_options(built_hip):
    p = subprocess.run([built_hip], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 1 and b"--pinned-genotype-margins FILE" in p.stderr and b"--pinned-genotype-table FILE" in p.stderr

"""CPU: bin/DipGenie rejects a bad --genotype-table before it needs a device."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.mark.parametrize("extra,word", [
    (["-p1", "--genotype-table", "t.tsv"], b"-p2"), (["-p1", "-R4", "--genotype-table=t.tsv"], b"-p2"),
    (["-p2", "-R4", "--genotype-table", ""], b"file name"), (["-p2", "-R4", "--genotype-table="], b"file name"), (["-p2", "-R4", "--genotype-table"], b"file name"),
    (["-p2", "-R4", "--genotype-table", "t.tsv", "--gpus", "2"], b"--gpus"), (["-p2", "-R4", "--gpus=2", "--genotype-table=t.tsv"], b"--gpus"),
    (["-p2", "-R4", "--genotype-margins", "m.tsv", "--genotype-table", ""], b"file name"),
])
def test_cli_rejects_bad_genotype_table_before_any_device_call(built_hip, tmp_path, extra, word):
    """exit status 1, a message that names the option, no FASTA and no FILE -- on a machine without a GPU too: the check comes before
    the device"""
    out = tmp_path / "o.fa"
    p = subprocess.run([built_hip, "-k11", "-w5", "-g", os.path.join(ROOT, "tests", "golden", "e2e", "bub_a.gfa"), "-r", os.path.join(ROOT, "tests", "golden", "e2e", "bub_a.fa"),
                        "-o", str(out), *extra], stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=tmp_path)
    assert p.returncode == 1, (p.returncode, p.stderr)
    assert b"--genotype-table" in p.stderr and word in p.stderr and b"no CPU fallback" not in p.stderr, p.stderr
    assert p.stdout == b"" and not out.exists() and not (tmp_path / "t.tsv").exists() and os.listdir(tmp_path) == []


def test_usage_names_the_option(built_hip):
    p = subprocess.run([built_hip], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 1 and b"--genotype-table FILE" in p.stderr and b"--genotype-margins FILE" in p.stderr

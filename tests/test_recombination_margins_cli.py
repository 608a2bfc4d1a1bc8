"""CPU: bin/DipGenie rejects a bad --recombination-margins before it needs a device, and the bindings export the call."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.mark.parametrize("extra,word", [
    (["-p1", "--recombination-margins", "m.tsv"], b"-p2"), (["-p1", "-R4", "--recombination-margins=m.tsv"], b"-p2"),
    (["-p2", "-R4", "--recombination-margins", ""], b"file name"), (["-p2", "-R4", "--recombination-margins="], b"file name"), (["-p2", "-R4", "--recombination-margins"], b"file name"),
    (["-p2", "-R4", "--recombination-margins", "m.tsv", "--gpus", "2"], b"--gpus"), (["-p2", "-R4", "--gpus=2", "--recombination-margins=m.tsv"], b"--gpus"),
    (["-p2", "-R4", "--recombination-margins", "m.tsv", "--pins", "p.tsv"], b"--pins"), (["-p2", "-R4", "--pins=p.tsv", "--recombination-margins=m.tsv"], b"--pins"),
])
def test_cli_rejects_bad_recombination_margins_before_any_device_call(built_hip, tmp_path, extra, word):
    """exit status 1, a message that names the option, no FASTA and no FILE -- on a machine without a GPU too: the check comes before
    the device (and before the file of --pins is opened)"""
    out = tmp_path / "o.fa"
    p = subprocess.run([built_hip, "-k11", "-w5", "-g", os.path.join(ROOT, "tests", "golden", "e2e", "bub_a.gfa"), "-r", os.path.join(ROOT, "tests", "golden", "e2e", "bub_a.fa"),
                        "-o", str(out), *extra], stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=tmp_path)
    assert p.returncode == 1, (p.returncode, p.stderr)
    assert b"--recombination-margins" in p.stderr and word in p.stderr and b"no CPU fallback" not in p.stderr, p.stderr
    assert p.stdout == b"" and not out.exists() and not (tmp_path / "m.tsv").exists() and os.listdir(tmp_path) == []


def test_usage_names_the_option(built_hip):
    p = subprocess.run([built_hip], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 1 and b"--recombination-margins FILE" in p.stderr


def test_bindings_export_the_call():
    from dipgenie_amd import capi
    for name in ("dg_dp_recombination_margins", "dg_dp_get_recombination_stats"):
        assert name in capi.SYMBOLS and hasattr(capi.lib, name)
    assert callable(capi.Context.dp_recombination_margins) and callable(capi.Context.dp_recombination_stats)
    assert capi.RECOMBINATION_MARGIN.itemsize == 64
    assert capi.RECOMBINATION_MARGIN.names == ("level", "value", "from1", "from2", "to1", "to2")

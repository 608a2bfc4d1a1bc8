"""CPU: bin/DipGenie rejects a bad --budget-recombination-margins before it needs a device."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.mark.parametrize("extra,word", [
    (["-p2", "-R4", "--budget-recombination-margins", "m.tsv"], b"needs --budgets"), (["-p2", "-R4", "--budget-recombination-margins=m.tsv"], b"needs --budgets"),
    (["-p1", "--budgets", "all", "--budget-recombination-margins", "m.tsv"], b"-p2"), (["-p1", "-R4", "--budget-recombination-margins=m.tsv"], b"-p2"),
    (["-p2", "-R4", "--budgets", "all", "--budget-recombination-margins", ""], b"file name"), (["-p2", "-R4", "--budgets=all", "--budget-recombination-margins="], b"file name"),
    (["-p2", "-R4", "--budgets", "0,2", "--budget-recombination-margins"], b"file name"),
    (["-p2", "-R4", "--budgets", "all", "--budget-recombination-margins", "m.tsv", "--gpus", "2"], b"--gpus"), (["-p2", "-R4", "--gpus=2", "--budgets=all", "--budget-recombination-margins=m.tsv"], b"--gpus"),
    (["-p2", "-R4", "--budgets", "all", "--budget-recombination-margins", "m.tsv", "--pins", "pins.tsv"], b"--pins"),
    (["-p2", "-R4", "--pins=pins.tsv", "--budgets=all", "--budget-recombination-margins=m.tsv"], b"--pins"),
    (["-p2", "-R256", "--budgets", "all", "--budget-recombination-margins", "m.tsv"], b"257 limits"),       # one device call takes 256 queries
    (["-p2", "-R300", "--budget-recombination-margins=m.tsv", "--budgets=" + ",".join(str(r) for r in range(257))], b"257 limits"),
])
def test_cli_rejects_bad_budget_recombination_margins_before_any_device_call(built_hip, tmp_path, extra, word):
    """exit status 1, a message that names the option, no FASTA and no FILE -- on a machine without a GPU too: the check comes before
    the device (and before the --pins file, which does not exist, is read)"""
    out = tmp_path / "o.fa"
    p = subprocess.run([built_hip, "-k11", "-w5", "-g", os.path.join(ROOT, "tests", "golden", "e2e", "bub_a.gfa"), "-r", os.path.join(ROOT, "tests", "golden", "e2e", "bub_a.fa"),
                        "-o", str(out), *extra], stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=tmp_path)
    assert p.returncode == 1, (p.returncode, p.stderr)
    assert b"--budget-recombination-margins" in p.stderr and word in p.stderr and b"no CPU fallback" not in p.stderr, p.stderr
    assert p.stdout == b"" and not out.exists() and not (tmp_path / "m.tsv").exists() and os.listdir(tmp_path) == []


def test_usage_names_the_option(built_hip):
    p = subprocess.run([built_hip], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 1 and b"--budget-recombination-margins FILE" in p.stderr


def test_the_binding_and_the_header_name_the_call(built_hip):
    from dipgenie_amd import capi
    for name in ("dg_dp_recombination_margins_budgets", "dg_dp_get_recombination_budget_stats"):
        assert name in capi.SYMBOLS and hasattr(capi.lib, name)
        assert name + "(" in open(os.path.join(ROOT, "include", "dipgenie_hip.h")).read()
    assert callable(capi.Context.dp_recombination_margins_budgets) and callable(capi.Context.dp_recombination_budget_stats)
    assert "recombination_margins_budgets" not in open(os.path.join(ROOT, "include", "dipgenie_run.h")).read()      # the run interface does not get it

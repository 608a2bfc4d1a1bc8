"""CPU: the per-budget fixture (tests/golden/budgets.json, the reference run once per -R r) is what the host pipeline behind the
oracle answers for -R r; and bin/DipGenie rejects a bad --budgets before it needs a device."""
import hashlib
import json
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CASES = json.load(open(os.path.join(HERE, "golden", "e2e.json")))
BUDGETS = json.load(open(os.path.join(HERE, "golden", "budgets.json")))
SPREAD = [("bub_c", 0), ("bub_c", 3), ("bub_c", 7), ("bub_e", 1), ("bub_e", 6), ("bub_e", 10), ("bub_g", 0), ("bub_g", 5), ("bub_g", 12),
          ("bub_g", 17), ("c5s", 0), ("c5s", 9), ("c5s", 31)]


def test_fixture_shape():
    assert {n: b["R"] for n, b in BUDGETS.items()} == {"bub_c": 8, "bub_e": 10, "bub_g": 18, "c5s": 32}
    assert sum(len(b["rows"]) for b in BUDGETS.values()) == 72          # 9 + 11 + 19 + 33: every r = 0..R of the four panels
    for name, b in BUDGETS.items():
        assert [row["r"] for row in b["rows"]] == list(range(b["R"] + 1))
        last = b["rows"][b["R"]]
        assert (last["dp_value"], last["fasta_md5"]) == (CASES[name]["dp_value"], CASES[name]["fasta_md5"])      # r = R is e2e.json's run
        values = [row["dp_value"] for row in b["rows"] if not row.get("unreachable")]
        assert values == sorted(values)


@pytest.mark.parametrize("name,r", SPREAD)
def test_host_pipeline_behind_the_oracle_reproduces_the_fixture(name, r, built_cpu, tmp_path):
    c, want = CASES[name], BUDGETS[name]["rows"][r]
    out, js = tmp_path / "o.fa", tmp_path / "o.json"
    args = [a if not a.startswith("-R") else f"-R{r}" for a in c["args"]]
    p = subprocess.run([built_cpu, "-q", "-t4"] + args + ["-g", os.path.join(ROOT, c["gfa"]), "-r", os.path.join(ROOT, c["reads"]), "-o", str(out), "-J", str(js)],
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    if want.get("unreachable"):
        assert p.returncode != 0 or not out.exists()
        return
    assert p.returncode == 0
    summ = json.load(open(js))
    assert {k: summ[k] for k in ("dp_value", "r1", "r2", "len1", "len2")} == {k: want[k] for k in ("dp_value", "r1", "r2", "len1", "len2")}
    assert hashlib.md5(open(out, "rb").read()).hexdigest() == want["fasta_md5"]


@pytest.mark.parametrize("extra,word", [
    (["-p1", "--budgets", "all"], b"-p2"), (["-p2", "-R4", "--budgets", "0,5"], b"above -R"), (["-p2", "-R4", "--budgets", "-1"], b"not a recombination limit"),
    (["-p2", "-R4", "--budgets", "1,x"], b"not a recombination limit"), (["-p2", "-R4", "--budgets=2,,3"], b"not a recombination limit"),
    (["-p2", "-R4", "--budgets", ""], b"not a recombination limit"), (["-p2", "-R4", "--budget-table", "t.tsv"], b"--budgets"),
])
def test_cli_rejects_bad_budgets_before_any_device_call(built_hip, tmp_path, extra, word):
    """exit status 1, a message that names the option, no FASTA -- on a machine without a GPU too: the check comes before the device"""
    out = tmp_path / "o.fa"
    p = subprocess.run([built_hip, "-k11", "-w5", "-g", os.path.join(ROOT, "tests", "golden", "e2e", "bub_a.gfa"), "-r", os.path.join(ROOT, "tests", "golden", "e2e", "bub_a.fa"),
                        "-o", str(out), *extra], stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=tmp_path)
    assert p.returncode == 1, (p.returncode, p.stderr)
    assert b"--budgets" in p.stderr and word in p.stderr and b"no CPU fallback" not in p.stderr, p.stderr
    assert p.stdout == b"" and not out.exists() and not (tmp_path / "t.tsv").exists()

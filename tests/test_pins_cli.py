"""CPU: bin/DipGenie rejects a bad --pins before it needs a device: the refused combinations with exit status 1, a malformed FILE with
exit status 2."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _run(built_hip, tmp_path, extra):
    out = tmp_path / "o.fa"
    p = subprocess.run([built_hip, "-k11", "-w5", "-g", os.path.join(ROOT, "tests", "golden", "e2e", "bub_a.gfa"), "-r", os.path.join(ROOT, "tests", "golden", "e2e", "bub_a.fa"),
                        "-o", str(out), *extra], stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=tmp_path)
    assert p.stdout == b"" and not out.exists() and b"no CPU fallback" not in p.stderr, p.stderr
    return p


@pytest.mark.parametrize("extra,word", [
    (["-p1", "--pins", "f.pins"], b"-p2"), (["-p2", "--pins", ""], b"file name"), (["-p2", "--pins="], b"file name"), (["-p2", "--pins"], b"file name"),
    (["-p2", "--pins", "f.pins", "--gpus", "2"], b"--gpus"), (["-p2", "--shard-transport=host", "--pins=f.pins"], b"--gpus"),
    (["-p2", "--pins", "f.pins", "--site-margins", "s.tsv"], b"--site-margins"), (["-p2", "--genotype-margins=m.tsv", "--pins", "f.pins"], b"--genotype-margins"),
    (["-p2", "--pins", "f.pins", "--genotype-table", "t.tsv"], b"--genotype-table"),
])
def test_cli_refuses_pins_beside_what_it_does_not_go_with(built_hip, tmp_path, extra, word):
    (tmp_path / "f.pins").write_text("1\t.\t.\n")
    p = _run(built_hip, tmp_path, extra)
    assert p.returncode == 1 and b"[E::main] --pins" in p.stderr and word in p.stderr, (p.returncode, p.stderr)
    assert os.listdir(tmp_path) == ["f.pins"]


@pytest.mark.parametrize("text,line,word", [
    ("1\t2\n", 1, b"columns"), ("1\t2\t3\t4\t5\n", 1, b"columns"), ("# fine\n\n1\t.\t.\n1 2 3\n", 4, b"columns"), ("1\t.\t.\n.\t2\t3\n", 2, b"level"),
    ("1\t-2\t3\n", 1, b"vertex id"), ("1\t2\t3x\n", 1, b"vertex id"), ("1\t2\t3\tREQUIRE\n", 1, b"kind"), ("1\t2\t3\trequire\n1\t2\t3\tforbid-unordered\n", 2, b"kind"),
    ("1\t2\t\n", 1, b"columns"), ("1\t99999999999\t3\n", 1, b"vertex id"),
])
def test_cli_ends_with_status_2_on_a_malformed_pins_file(built_hip, tmp_path, text, line, word):
    (tmp_path / "f.pins").write_text(text)
    p = _run(built_hip, tmp_path, ["-p2", "--pins", "f.pins"])
    assert p.returncode == 2 and b"--pins: line %d:" % line in p.stderr and word in p.stderr, (p.returncode, p.stderr)
    assert os.listdir(tmp_path) == ["f.pins"]


def test_a_missing_pins_file_and_the_usage(built_hip, tmp_path):
    p = _run(built_hip, tmp_path, ["-p2", "--pins", "nowhere.pins"])
    assert p.returncode == 2 and b"--pins: cannot open nowhere.pins" in p.stderr
    u = subprocess.run([built_hip], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert u.returncode == 1 and b"--pins FILE" in u.stderr

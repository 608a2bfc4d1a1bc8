"""-m gpu: bin/DipGenie --objective-table FILE on the committed end-to-end cases of tests/test_gpu_site_margins_cli.py: FILE holds
what Context.dp_answer_objectives answers on the dumped graph, the -J summary lists the same rows, and a run without the option
writes the same FASTA files, standard output and budget table, and a summary without `objectives`."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from dipgenie_amd import capi
from objective_model import as_rows
from paths_model import NEG_INF

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CASES = json.load(open(os.path.join(HERE, "golden", "e2e.json")))
HEADER = "r dp_value objective hom_shared hom_single het_single het_both".split()


def _cli(cli, case, tmp, extra):
    """one run writing tmp/o.fa (+ .R<r>), tmp/o.json and, with --budget-table, tmp/b.tsv (stdout names the FASTA's path: every run
    of a test uses the same one); returns the process, {file name: bytes} of what it wrote and the summary -- the files are removed"""
    out, js = tmp / "o.fa", tmp / "o.json"
    p = subprocess.run([cli, "-t8"] + case["args"] + ["-g", os.path.join(ROOT, case["gfa"]), "-r", os.path.join(ROOT, case["reads"]), "-o", str(out), "-J", str(js), *extra],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    summ = json.load(open(js)) if js.exists() else None
    files = {}
    for f in sorted(tmp.iterdir()):
        if f.name.startswith("o.fa") or f.name in ("o.json", "b.tsv"):
            if f.name != "o.json":
                files[f.name] = f.read_bytes()
            os.remove(f)
    return p, files, summ


@pytest.mark.parametrize("name,budgets", [("toy1_p2", "all"), ("bub_a", "all"), ("bub_a", None), ("bub_c", "0,3,8")])
def test_objective_table_is_what_the_library_answers(built_hip, gpu_ctx, tmp_path, name, budgets):
    c = CASES[name]
    pre = tmp_path / "dump"
    common = ["--budgets", budgets, "--budget-table", str(tmp_path / "b.tsv")] if budgets else []
    p, files, summ = _cli(built_hip, c, tmp_path, common + ["--objective-table", str(tmp_path / "t.tsv"), "-D", str(pre)])
    assert p.returncode == 0, p.stderr
    p0, files0, summ0 = _cli(built_hip, c, tmp_path, common)
    assert p0.returncode == 0, p0.stderr
    # FASTA files, stdout and the budget table: byte for byte
    assert hashlib.md5(files["o.fa"]).hexdigest() == c["fasta_md5"]
    assert files == files0 and ("b.tsv" in files) == bool(budgets)
    assert p.stdout == p0.stdout
    # -J: the objectives key only (and the stage's wall time)
    assert "objectives" not in summ0 and "objective_table" not in summ0["stages"] and "objective_table" in summ["stages"]
    assert set(summ) == set(summ0) | {"objectives"}
    for key in summ0:
        if key not in ("stages", "dp_forward_ms", "dp_traceback_ms"):
            assert summ[key] == summ0[key], key
    # FILE against the library on the dumped graph
    g = capi.DpGraphArrays.load(str(pre) + ".dpg")
    listed = [g.R] if budgets is None else list(range(g.R + 1)) if budgets == "all" else [int(b) for b in budgets.split(",")]
    gpu_ctx.dp_load_graph(g)
    gpu_ctx.dp_run_budgets(listed)
    values = gpu_ctx.dp_budget_values()
    want = as_rows(gpu_ctx.dp_answer_objectives(listed))
    assert values[g.R] == c["dp_value"]
    lines = open(tmp_path / "t.tsv").read().split("\n")
    assert lines[-1] == "" and lines[0].split("\t") == HEADER
    rows = [ln.split("\t") for ln in lines[1:-1]]
    assert [int(r[0]) for r in rows] == listed
    entries = []
    for row, b, rec in zip(rows, listed, want):
        assert len(row) == 7
        if values[b] == NEG_INF:
            assert row[1:] == ["."] * 6 and (rec == -1).all()
            entries.append(dict(r=b, dp_value=None, objective=None, hom_shared=None, hom_single=None, het_single=None, het_both=None))
            continue
        assert [int(x) for x in row[1:]] == [values[b], rec[0] + rec[2], *rec], (b, row, rec)
        entries.append(dict(r=b, dp_value=int(values[b]), objective=int(rec[0] + rec[2]), hom_shared=int(rec[0]), hom_single=int(rec[1]),
                            het_single=int(rec[2]), het_both=int(rec[3])))
    assert summ["objectives"] == entries
    assert (want >= 0).any()
    # (the graph objective at -R beside the summary's obj, which is counted from anchors inside the copied stretches: printed, never compared)
    print(f"{name}: graph objective at -R {entries[-1]['objective'] if listed[-1] == g.R else None}, obj {summ['obj']}")


@pytest.mark.parametrize("extra", [["-p1", "--objective-table", "t.tsv"], ["--objective-table"], ["--objective-table="]])
def test_bad_arguments_end_the_run_before_any_output(built_hip, tmp_path, extra):
    c = CASES["toy1_p2"]
    extra = [str(tmp_path / x) if x == "t.tsv" else x for x in extra]
    args = [a for a in c["args"] if not (a.startswith("-p") and "-p1" in extra)]
    out, js = tmp_path / "o.fa", tmp_path / "o.json"
    p = subprocess.run([built_hip, "-t8"] + args + ["-g", os.path.join(ROOT, c["gfa"]), "-r", os.path.join(ROOT, c["reads"]), "-o", str(out), "-J", str(js), *extra],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 1, (p.returncode, p.stderr)
    assert b"--objective-table" in p.stderr and p.stdout == b""
    assert list(tmp_path.iterdir()) == []

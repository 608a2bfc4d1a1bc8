"""-m gpu: bin/DipGenie --budgets all --budget-genotype-margins FILE on the smallest committed end-to-end case of the --genotype-margins
tests: FASTA, stdout and the --budgets outputs are those of a run without the option, the rows of FILE with r == R are the
--genotype-margins file of the same run, the rows of another r are what Context.dp_genotype_margins answers on the dumped graph for
dp_answer_paths(r), and the -J summary counts what FILE holds."""
import glob
import hashlib
import os

import numpy as np
import pytest

from dipgenie_amd import capi
from paths_model import NEG_INF
from test_gpu_genotype_margins_cli import HEADER
from test_gpu_site_margins_cli import CASES, _cli

pytestmark = pytest.mark.gpu


def _budget_outputs(tmp):
    """the files --budgets writes beside the FASTA (<fasta>.R<r>) and the --budget-table, by name"""
    return {os.path.basename(f): open(f, "rb").read() for f in sorted(glob.glob(str(tmp / "o.fa.R*")) + glob.glob(str(tmp / "t.tsv")))}


def test_budget_genotype_margins_file(built_hip, gpu_ctx, tmp_path):
    c = CASES["bub_a"]
    pre = tmp_path / "dump"
    common = ["--budgets", "all", "--budget-table", str(tmp_path / "t.tsv")]
    p, fasta, summ = _cli(built_hip, c, tmp_path, common + ["--budget-genotype-margins", str(tmp_path / "f.tsv"), "--genotype-margins", str(tmp_path / "g.tsv"), "-D", str(pre)])
    assert p.returncode == 0, p.stderr
    with_option = _budget_outputs(tmp_path)
    for f in with_option:
        os.remove(tmp_path / f)
    p0, fasta0, summ0 = _cli(built_hip, c, tmp_path, common + ["--genotype-margins", str(tmp_path / "g0.tsv")])
    assert p0.returncode == 0, p0.stderr
    assert hashlib.md5(fasta).hexdigest() == c["fasta_md5"] and fasta0 == fasta
    assert p.stdout == p0.stdout
    assert len(with_option) >= 3 and "t.tsv" in with_option and _budget_outputs(tmp_path) == with_option
    assert open(tmp_path / "g.tsv").read() == open(tmp_path / "g0.tsv").read()
    assert "budget_genotype_margins" not in summ0 and "budget_genotype_margins" not in summ0["stages"]
    assert set(summ) == set(summ0) | {"budget_genotype_margins"} and "budget_genotype_margins" in summ["stages"]
    for key in summ0:
        if key not in ("stages", "dp_forward_ms", "dp_traceback_ms", "genotype_margins"):
            assert summ[key] == summ0[key], key
    drop = lambda d: {k: v for k, v in d.items() if k != "wall_s"}
    assert drop(summ["genotype_margins"]) == drop(summ0["genotype_margins"])
    # FILE: the header of --genotype-margins behind r; rows in the order of the list, levels ascending
    g = capi.DpGraphArrays.load(str(pre) + ".dpg")
    cls = np.fromfile(str(pre) + ".cls", np.int32)
    L, R = g.n_levels, g.R
    lines = open(tmp_path / "f.tsv").read().split("\n")
    assert lines[-1] == "" and lines[0].split("\t") == ["r"] + HEADER
    rows = [ln.split("\t") for ln in lines[1:-1]]
    assert all(len(row) == 15 and "" not in row for row in rows)
    gpu_ctx.dp_load_graph(g)
    gpu_ctx.dp_run_budgets(range(R + 1))
    planes = gpu_ctx.dp_budget_values()
    fit = [r for r in range(R + 1) if planes[r] != NEG_INF]
    assert R in fit and len(fit) >= 2
    assert [(int(row[0]), int(row[1])) for row in rows] == [(r, l) for r in fit for l in range(1, L - 1)]
    dp_values = {b["r"]: b["dp_value"] for b in summ["budgets"]}
    for row in rows:
        assert int(row[8]) == dp_values[int(row[0])] == planes[int(row[0])]
    # r == R: the --genotype-margins file of the same run
    top = ["\t".join(row[1:]) for row in rows if int(row[0]) == R]
    assert top == open(tmp_path / "g.tsv").read().split("\n")[1:-1]
    # another r: what the one-budget call answers for that limit's answer
    other = fit[0] if fit[0] != R else fit[1]
    levels, best = gpu_ctx.dp_genotype_margins(gpu_ctx.dp_answer_paths(other), other, cls)
    assert best == planes[other]
    got = [row for row in rows if int(row[0]) == other]
    want_stats = {}
    for r in fit:
        want_stats[r] = dict(r=r, with_alternative=0, margin0=0, min_positive_margin=None)
    for i, row in enumerate(got):
        rec = levels[0, 1 + i]
        assert (int(row[2]), int(row[5]), int(row[8])) == (rec["vertex1"], rec["vertex2"], rec["value"]), (i, row)
        if rec["alt_vertex1"] < 0:
            assert row[9:] == ["."] * 6 and rec["alt_value"] == NEG_INF
        else:
            margin = int(rec["value"]) - int(rec["alt_value"])
            assert (int(row[9]), int(row[11]), int(row[13]), int(row[14])) == (rec["alt_vertex1"], rec["alt_vertex2"], rec["alt_value"], margin), (i, row)
    # -J counts what FILE holds, per limit
    for row in rows:
        st = want_stats[int(row[0])]
        if row[14] == ".":
            continue
        margin = int(row[14])
        assert margin >= 0
        st["with_alternative"] += 1
        st["margin0"] += margin == 0
        if margin > 0:
            st["min_positive_margin"] = margin if st["min_positive_margin"] is None else min(st["min_positive_margin"], margin)
    bm = summ["budget_genotype_margins"]
    assert bm["budgets"] == [want_stats[r] for r in fit] and bm["segments"] == 1 and bm["wall_s"] > 0
    assert sum(st["with_alternative"] for st in want_stats.values()) >= 1
    top_stats = {k: v for k, v in want_stats[R].items() if k != "r"}
    assert top_stats == {k: summ["genotype_margins"][k] for k in top_stats}


def test_a_list_is_answered_in_its_order(built_hip, tmp_path):
    c = CASES["bub_a"]
    p, fasta, summ = _cli(built_hip, c, tmp_path, ["--budgets", "all", "--budget-genotype-margins", str(tmp_path / "all.tsv")])
    assert p.returncode == 0, p.stderr
    everything = [ln.split("\t") for ln in open(tmp_path / "all.tsv").read().split("\n")[1:-1]]
    R = max(int(row[0]) for row in everything)
    listed = [str(R), "0", str(R - 1)]
    p, fasta2, summ2 = _cli(built_hip, c, tmp_path, ["--budgets", ",".join(listed), "--budget-genotype-margins", str(tmp_path / "some.tsv")])
    assert p.returncode == 0 and fasta2 == fasta, p.stderr
    some = [ln.split("\t") for ln in open(tmp_path / "some.tsv").read().split("\n")[1:-1]]
    have = {row[0] for row in everything}
    assert some == [row for r in listed if r in have for row in everything if row[0] == r]
    assert [b["r"] for b in summ2["budget_genotype_margins"]["budgets"]] == [int(r) for r in listed if r in have]

"""-m gpu: bin/DipGenie --genotype-margins FILE on committed end-to-end cases: FASTA and stdout are those of a run without the option,
FILE has one row per inner level whose value is the run's DP value and whose fields are what Context.dp_genotype_margins answers on the
dumped graph with the dumped allele classes for the run's own answer, and the -J summary counts what FILE holds."""
import hashlib
import json
import os

import numpy as np
import pytest

from dipgenie_amd import capi
from paths_model import NEG_INF
from test_gpu_site_margins_cli import CASES, _cli

pytestmark = pytest.mark.gpu

HEADER = "level vertex1 panel_hap1 segment1 vertex2 panel_hap2 segment2 value alt_vertex1 alt_segment1 alt_vertex2 alt_segment2 alt_value margin".split()


@pytest.mark.parametrize("name", ["bub_a", "bub_c"])
def test_genotype_margins_file_is_what_the_library_answers(built_hip, gpu_ctx, tmp_path, name):
    c = CASES[name]
    pre = tmp_path / "dump"
    p, fasta, summ = _cli(built_hip, c, tmp_path, ["--genotype-margins", str(tmp_path / "g.tsv"), "-D", str(pre)])
    assert p.returncode == 0, p.stderr
    p0, fasta0, summ0 = _cli(built_hip, c, tmp_path, [])
    assert p0.returncode == 0, p0.stderr
    assert hashlib.md5(fasta).hexdigest() == c["fasta_md5"] and fasta0 == fasta
    assert p.stdout == p0.stdout
    assert "genotype_margins" not in summ0 and "genotype_margins" not in summ0["stages"]
    assert set(summ) == set(summ0) | {"genotype_margins"}
    for key in summ0:
        if key not in ("stages", "dp_forward_ms", "dp_traceback_ms"):
            assert summ[key] == summ0[key], key
    # FILE against the library on the dumped graph with the dumped classes
    g = capi.DpGraphArrays.load(str(pre) + ".dpg")
    cls = np.fromfile(str(pre) + ".cls", np.int32)
    L, R = g.n_levels, g.R
    assert cls.shape == (g.n_vertices,)
    gpu_ctx.dp_load_graph(g)
    gpu_ctx.dp_run()
    levels, best = gpu_ctx.dp_genotype_margins(gpu_ctx.dp_answer_paths(R), R, cls)
    assert best == c["dp_value"] == summ["dp_value"]
    lines = open(tmp_path / "g.tsv").read().split("\n")
    assert lines[-1] == "" and lines[0].split("\t") == HEADER
    rows = [ln.split("\t") for ln in lines[1:-1]]
    assert len(rows) == L - 2
    stats = dict(with_alternative=0, margin0=0, min_positive_margin=None)
    for i, row in enumerate(rows):
        rec = levels[0, 1 + i]
        assert len(row) == 14 and "" not in row and int(row[0]) == 1 + i
        assert (int(row[1]), int(row[4]), int(row[7])) == (rec["vertex1"], rec["vertex2"], rec["value"]), (i, row)
        assert int(row[7]) == summ["dp_value"]
        if rec["alt_vertex1"] < 0:
            assert row[8:] == ["."] * 6 and rec["alt_value"] == NEG_INF
            continue
        margin = int(rec["value"]) - int(rec["alt_value"])
        assert (int(row[8]), int(row[10]), int(row[12]), int(row[13])) == (rec["alt_vertex1"], rec["alt_vertex2"], rec["alt_value"], margin), (i, row)
        assert margin >= 0 and {cls[rec["alt_vertex1"]], cls[rec["alt_vertex2"]]} != {cls[rec["vertex1"]], cls[rec["vertex2"]]}
        stats["with_alternative"] += 1
        stats["margin0"] += margin == 0
        if margin > 0:
            stats["min_positive_margin"] = margin if stats["min_positive_margin"] is None else min(stats["min_positive_margin"], margin)
    gm = summ["genotype_margins"]
    assert {k: gm[k] for k in stats} == stats and gm["segments"] == 1 and gm["wall_s"] > 0
    assert stats["with_alternative"] >= 1


def test_it_goes_with_site_margins_and_budgets(built_hip, gpu_ctx, tmp_path):
    c = CASES["bub_a"]
    p, fasta, summ = _cli(built_hip, c, tmp_path, ["--genotype-margins", str(tmp_path / "g.tsv")])
    both, fasta2, summ2 = _cli(built_hip, c, tmp_path, ["--genotype-margins", str(tmp_path / "g2.tsv"), "--site-margins", str(tmp_path / "m.tsv"), "--budgets", "all"])
    assert p.returncode == 0 and both.returncode == 0, (p.stderr, both.stderr)
    assert hashlib.md5(fasta2).hexdigest() == c["fasta_md5"] and fasta2 == fasta
    assert open(tmp_path / "g.tsv").read() == open(tmp_path / "g2.tsv").read()
    assert {"genotype_margins", "site_margins", "budgets"} <= set(summ2)
    drop = lambda d: {k: v for k, v in d.items() if k != "wall_s"}
    assert drop(summ2["genotype_margins"]) == drop(summ["genotype_margins"])

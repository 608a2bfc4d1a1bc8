"""-m gpu: bin/DipGenie --phase-margins FILE on committed end-to-end cases: FASTA and stdout are those of a run without the option,
FILE has one row per pair of neighbouring het levels of the run's own answer with what Context.dp_phase_margins answers on the dumped
graph with the dumped allele classes, every cis_value is the run's DP value, and the -J summary counts what FILE holds.  A case whose
answer has fewer than two het levels still compares the header-only file: the test prints how many rows each case gave."""
import hashlib

import numpy as np
import pytest

from dipgenie_amd import capi
from paths_model import NEG_INF
from test_gpu_site_margins_cli import CASES, _cli

pytestmark = pytest.mark.gpu

HEADER = "level_a level_b vertex1_a segment1_a vertex2_a segment2_a vertex1_b segment1_b vertex2_b segment2_b cis_value trans_value trans_vertex1 trans_vertex2 margin".split()


@pytest.mark.parametrize("name", ["toy1_p2", "bub_a", "bub_c"])
def test_phase_margins_file_is_what_the_library_answers(built_hip, gpu_ctx, tmp_path, name):
    c = CASES[name]
    pre = tmp_path / "dump"
    p, fasta, summ = _cli(built_hip, c, tmp_path, ["--phase-margins", str(tmp_path / "p.tsv"), "-D", str(pre)])
    assert p.returncode == 0, p.stderr
    p0, fasta0, summ0 = _cli(built_hip, c, tmp_path, [])
    assert p0.returncode == 0, p0.stderr
    assert hashlib.md5(fasta).hexdigest() == c["fasta_md5"] and fasta0 == fasta
    assert p.stdout == p0.stdout
    assert "phase_margins" not in summ0 and "phase_margins" not in summ0["stages"]
    assert set(summ) == set(summ0) | {"phase_margins"}
    for key in summ0:
        if key not in ("stages", "dp_forward_ms", "dp_traceback_ms"):
            assert summ[key] == summ0[key], key
    # FILE against the library on the dumped graph with the dumped classes
    g = capi.DpGraphArrays.load(str(pre) + ".dpg")
    cls = np.fromfile(str(pre) + ".cls", np.int32)
    R = g.R
    assert cls.shape == (g.n_vertices,)
    gpu_ctx.dp_load_graph(g)
    gpu_ctx.dp_run()
    called = gpu_ctx.dp_answer_paths(R)
    records, best = gpu_ctx.dp_phase_margins(called, R, cls)
    het = gpu_ctx.dp_phase_stats()["het_levels"]
    assert best == c["dp_value"] == summ["dp_value"]
    assert het == int((cls[called[0]] != cls[called[1]]).sum()) and len(records) == max(het - 1, 0)
    lines = open(tmp_path / "p.tsv").read().split("\n")
    assert lines[-1] == "" and lines[0].split("\t") == HEADER
    rows = [ln.split("\t") for ln in lines[1:-1]]
    assert len(rows) == len(records)
    stats = dict(het_levels=het, records=len(records), with_alternative=0, margin0=0, min_positive_margin=None)
    for row, rec in zip(rows, records):
        a, e = int(rec["level_a"]), int(rec["level_b"])
        assert len(row) == 15 and "" not in row and (int(row[0]), int(row[1])) == (a, e)
        assert [int(row[x]) for x in (2, 4, 6, 8)] == [called[0, a], called[1, a], called[0, e], called[1, e]]
        assert int(row[10]) == rec["cis_value"] == summ["dp_value"]
        if rec["trans_vertex1"] < 0:
            assert row[11:] == ["."] * 4 and rec["trans_value"] == NEG_INF
            continue
        margin = int(rec["cis_value"]) - int(rec["trans_value"])
        assert [int(x) for x in row[11:]] == [rec["trans_value"], rec["trans_vertex1"], rec["trans_vertex2"], margin] and margin >= 0
        assert (cls[rec["trans_vertex1"]], cls[rec["trans_vertex2"]]) == (cls[called[1, a]], cls[called[0, a]])
        stats["with_alternative"] += 1
        stats["margin0"] += margin == 0
        if margin > 0:
            stats["min_positive_margin"] = margin if stats["min_positive_margin"] is None else min(stats["min_positive_margin"], margin)
    pm = summ["phase_margins"]
    assert {k: pm[k] for k in stats} == stats and pm["segments"] == 1 and pm["wall_s"] > 0
    print(f"{name}: het levels {het}, rows {len(rows)}, with a reachable trans {stats['with_alternative']}")


def test_it_goes_with_the_other_margin_options_and_budgets(built_hip, gpu_ctx, tmp_path):
    c = CASES["bub_a"]
    p, fasta, summ = _cli(built_hip, c, tmp_path, ["--phase-margins", str(tmp_path / "p.tsv")])
    extra = ["--phase-margins", str(tmp_path / "p2.tsv"), "--site-margins", str(tmp_path / "m.tsv"), "--genotype-margins", str(tmp_path / "g.tsv"),
             "--genotype-table", str(tmp_path / "t.tsv"), "--budgets", "all"]
    every, fasta2, summ2 = _cli(built_hip, c, tmp_path, extra)
    without, fasta3, summ3 = _cli(built_hip, c, tmp_path, [x.replace("g.tsv", "g3.tsv").replace("t.tsv", "t3.tsv").replace("m.tsv", "m3.tsv") for x in extra[2:]])
    assert p.returncode == 0 and every.returncode == 0 and without.returncode == 0, (p.stderr, every.stderr, without.stderr)
    assert hashlib.md5(fasta2).hexdigest() == c["fasta_md5"] and fasta2 == fasta == fasta3 and every.stdout == without.stdout
    assert open(tmp_path / "p.tsv").read() == open(tmp_path / "p2.tsv").read()
    for a, b in (("g.tsv", "g3.tsv"), ("t.tsv", "t3.tsv"), ("m.tsv", "m3.tsv")):      # the other files are what they are without the option
        assert open(tmp_path / a).read() == open(tmp_path / b).read()
    assert {"phase_margins", "genotype_margins", "genotype_table", "site_margins", "budgets"} <= set(summ2) and set(summ2) == set(summ3) | {"phase_margins"}
    drop = lambda d: {k: v for k, v in d.items() if k != "wall_s"}
    assert drop(summ2["phase_margins"]) == drop(summ["phase_margins"])
    for key in ("genotype_margins", "genotype_table", "site_margins"):
        assert drop(summ2[key]) == drop(summ3[key])
    assert summ2["budgets"] == summ3["budgets"]


@pytest.mark.parametrize("extra,word", [(["--gpus", "2"], b"--gpus"), (["--pins", "p.tsv"], b"--pins")])
def test_it_is_refused_with_gpus_and_pins(built_hip, tmp_path, extra, word):
    p, fasta, summ = _cli(built_hip, CASES["bub_a"], tmp_path, ["--phase-margins", str(tmp_path / "p.tsv"), *extra])
    assert p.returncode == 1 and b"--phase-margins" in p.stderr and word in p.stderr, (p.returncode, p.stderr)
    assert fasta is None and summ is None and not (tmp_path / "p.tsv").exists()

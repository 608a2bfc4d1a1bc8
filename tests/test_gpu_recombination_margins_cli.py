"""-m gpu: bin/DipGenie --recombination-margins FILE on committed end-to-end cases: FASTA and stdout are those of a run without the
option, FILE has one row per transition with what Context.dp_recombination_margins answers on the dumped graph for the run's own answer,
every value is the run's DP value, the called crossovers add up to the run's r1 + r2, and the -J summary counts what FILE holds.
toy1_p2 spends 1 + 1 crossovers, bub_a none (no breakpoint), bub_c 3 + 5."""
import hashlib

import pytest

from dipgenie_amd import capi
from paths_model import PathModel
from test_gpu_site_margins_cli import CASES, _cli

pytestmark = pytest.mark.gpu

HEADER = ("level vertex1_from segment1_from vertex1_to segment1_to w1 vertex2_from segment2_from vertex2_to segment2_to w2 s_called value value_s0 value_s1 value_s2 "
          "alt_s alt_value margin alt_from1 alt_to1 alt_from2 alt_to2").split()
CROSSOVERS = {"toy1_p2": (1, 1), "bub_a": (0, 0), "bub_c": (3, 5)}


@pytest.mark.parametrize("name", sorted(CROSSOVERS))
def test_recombination_margins_file_is_what_the_library_answers(built_hip, gpu_ctx, tmp_path, name):
    c = CASES[name]
    pre = tmp_path / "dump"
    p, fasta, summ = _cli(built_hip, c, tmp_path, ["--recombination-margins", str(tmp_path / "r.tsv"), "-D", str(pre)])
    assert p.returncode == 0, p.stderr
    p0, fasta0, summ0 = _cli(built_hip, c, tmp_path, [])
    assert p0.returncode == 0, p0.stderr
    assert hashlib.md5(fasta).hexdigest() == c["fasta_md5"] and fasta0 == fasta
    assert p.stdout == p0.stdout
    assert "recombination_margins" not in summ0 and "recombination_margins" not in summ0["stages"]
    assert set(summ) == set(summ0) | {"recombination_margins"}
    for key in summ0:
        if key not in ("stages", "dp_forward_ms", "dp_traceback_ms"):
            assert summ[key] == summ0[key], key
    # FILE against the library on the dumped graph
    g = capi.DpGraphArrays.load(str(pre) + ".dpg")
    m = PathModel(g)
    R = g.R
    gpu_ctx.dp_load_graph(g)
    gpu_ctx.dp_run()
    called = gpu_ctx.dp_answer_paths(R)
    records, out, best = gpu_ctx.dp_recombination_margins(R, called[None])
    score = gpu_ctx.dp_score_paths(called[None])[0]
    assert best == c["dp_value"] == summ["dp_value"]
    assert (int(score["r1"]), int(score["r2"])) in (CROSSOVERS[name], CROSSOVERS[name][::-1]) and int(score["r1"]) + int(score["r2"]) == summ["r1"] + summ["r2"]
    lines = open(tmp_path / "r.tsv").read().split("\n")
    assert lines[-1] == "" and lines[0].split("\t") == HEADER
    rows = [ln.split("\t") for ln in lines[1:-1]]
    assert len(rows) == len(records) == g.n_levels - 1
    stats = dict(transitions=len(rows), called_recombinations=0, breakpoints_margin0=0, min_positive_breakpoint_margin=None, co_optimal_elsewhere=0)
    for l, (row, rec) in enumerate(zip(rows, records)):
        assert len(row) == len(HEADER) and "" not in row and int(row[0]) == l == rec["level"]
        hops = [(int(called[h, l]), int(called[h, l + 1])) for h in range(2)]
        assert [int(row[x]) for x in (1, 3, 6, 8)] == [hops[0][0], hops[0][1], hops[1][0], hops[1][1]]
        w = [m.succ[u][v] for u, v in hops]
        s_called, value = int(out[0, l, 0]), int(out[0, l, 1])
        assert [int(row[5]), int(row[10])] == w and int(row[11]) == sum(w) == s_called
        assert int(row[12]) == value == summ["dp_value"] == rec["value"][s_called]
        assert row[13:16] == [str(rec["value"][s]) if rec["from1"][s] >= 0 else "." for s in range(3)]
        others = [s for s in range(3) if s != s_called and rec["from1"][s] >= 0]
        stats["called_recombinations"] += s_called
        if not others:
            assert row[16:] == ["."] * 7
            continue
        alt = max(others, key=lambda s: (rec["value"][s], -s))              # ties to the smaller s
        margin = value - int(rec["value"][alt])
        assert [int(x) for x in row[16:]] == [alt, rec["value"][alt], margin, rec["from1"][alt], rec["to1"][alt], rec["from2"][alt], rec["to2"][alt]] and margin >= 0
        if s_called > 0 and margin == 0:
            stats["breakpoints_margin0"] += 1
        if s_called > 0 and margin > 0:
            stats["min_positive_breakpoint_margin"] = margin if stats["min_positive_breakpoint_margin"] is None else min(stats["min_positive_breakpoint_margin"], margin)
        if s_called == 0 and rec["value"][alt] == summ["dp_value"]:
            stats["co_optimal_elsewhere"] += 1
    assert stats["called_recombinations"] == sum(CROSSOVERS[name])
    rm = summ["recombination_margins"]
    assert {k: rm[k] for k in stats} == stats and rm["segments"] == 1 and rm["wall_s"] > 0
    print(f"{name}: transitions {len(rows)}, summary {stats}")


def test_it_goes_with_the_other_margin_options_and_budgets(built_hip, gpu_ctx, tmp_path):
    c = CASES["bub_c"]
    p, fasta, summ = _cli(built_hip, c, tmp_path, ["--recombination-margins", str(tmp_path / "r.tsv")])
    extra = ["--recombination-margins", str(tmp_path / "r2.tsv"), "--site-margins", str(tmp_path / "m.tsv"), "--genotype-margins", str(tmp_path / "g.tsv"),
             "--genotype-table", str(tmp_path / "t.tsv"), "--phase-margins", str(tmp_path / "p.tsv"), "--budgets", "all"]
    every, fasta2, summ2 = _cli(built_hip, c, tmp_path, extra)
    renamed = [x.replace("g.tsv", "g3.tsv").replace("t.tsv", "t3.tsv").replace("m.tsv", "m3.tsv").replace("p.tsv", "p3.tsv") for x in extra[2:]]
    without, fasta3, summ3 = _cli(built_hip, c, tmp_path, renamed)
    assert p.returncode == 0 and every.returncode == 0 and without.returncode == 0, (p.stderr, every.stderr, without.stderr)
    assert hashlib.md5(fasta2).hexdigest() == c["fasta_md5"] and fasta2 == fasta == fasta3 and every.stdout == without.stdout
    assert open(tmp_path / "r.tsv").read() == open(tmp_path / "r2.tsv").read()
    for a, b in (("g.tsv", "g3.tsv"), ("t.tsv", "t3.tsv"), ("m.tsv", "m3.tsv"), ("p.tsv", "p3.tsv")):      # the other files are what they are without the option
        assert open(tmp_path / a).read() == open(tmp_path / b).read()
    assert set(summ2) == set(summ3) | {"recombination_margins"}
    drop = lambda d: {k: v for k, v in d.items() if k != "wall_s"}
    assert drop(summ2["recombination_margins"]) == drop(summ["recombination_margins"])
    for key in ("genotype_margins", "genotype_table", "site_margins", "phase_margins"):
        assert drop(summ2[key]) == drop(summ3[key])
    assert summ2["budgets"] == summ3["budgets"]


@pytest.mark.parametrize("extra,word", [(["--gpus", "2"], b"--gpus"), (["--pins", "p.tsv"], b"--pins")])
def test_it_is_refused_with_gpus_and_pins(built_hip, tmp_path, extra, word):
    p, fasta, summ = _cli(built_hip, CASES["bub_a"], tmp_path, ["--recombination-margins", str(tmp_path / "r.tsv"), *extra])
    assert p.returncode == 1 and b"--recombination-margins" in p.stderr and word in p.stderr, (p.returncode, p.stderr)
    assert fasta is None and summ is None and not (tmp_path / "r.tsv").exists()

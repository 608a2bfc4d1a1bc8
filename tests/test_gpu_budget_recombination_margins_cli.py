"""-m gpu: bin/DipGenie --budgets all --budget-recombination-margins FILE on committed end-to-end cases: FASTA, stdout and the --budgets
outputs are those of a run without the option, the rows of FILE with r == R are the --recombination-margins file of the same run, the
rows of every r are the --recombination-margins file of a separate run with -R r, and the -J summary counts what FILE holds."""
import hashlib
import os

import pytest

from test_gpu_budget_phase_margins_cli import _budget_outputs, _rows
from test_gpu_recombination_margins_cli import HEADER
from test_gpu_site_margins_cli import CASES, _cli

pytestmark = pytest.mark.gpu

COUNTS = ("transitions", "called_recombinations", "breakpoints_margin0", "min_positive_breakpoint_margin", "co_optimal_elsewhere")


@pytest.mark.parametrize("name", ["bub_a", "toy1_p2"])
def test_budget_recombination_margins_file(built_hip, tmp_path, name):
    c = CASES[name]
    R = int([a for a in c["args"] if a.startswith("-R")][0][2:])
    common = ["--budgets", "all"]
    p, fasta, summ = _cli(built_hip, c, tmp_path, common + ["--budget-recombination-margins", str(tmp_path / "f.tsv"), "--recombination-margins", str(tmp_path / "p.tsv")])
    assert p.returncode == 0, p.stderr
    with_option = _budget_outputs(tmp_path)
    for f in with_option:
        os.remove(tmp_path / f)
    p0, fasta0, summ0 = _cli(built_hip, c, tmp_path, common + ["--recombination-margins", str(tmp_path / "p0.tsv")])
    assert p0.returncode == 0, p0.stderr
    assert hashlib.md5(fasta).hexdigest() == c["fasta_md5"] and fasta0 == fasta
    assert p.stdout == p0.stdout
    assert len(with_option) >= 2 and _budget_outputs(tmp_path) == with_option
    assert open(tmp_path / "p.tsv").read() == open(tmp_path / "p0.tsv").read()
    assert "budget_recombination_margins" not in summ0 and "budget_recombination_margins" not in summ0["stages"]
    assert set(summ) == set(summ0) | {"budget_recombination_margins"} and "budget_recombination_margins" in summ["stages"]
    for key in summ0:
        if key not in ("stages", "dp_forward_ms", "dp_traceback_ms", "recombination_margins"):
            assert summ[key] == summ0[key], key
    drop = lambda d: {k: v for k, v in d.items() if k != "wall_s"}
    assert drop(summ["recombination_margins"]) == drop(summ0["recombination_margins"])
    # FILE: the header of --recombination-margins behind r; limits in the order of the list, levels ascending
    header, rows = _rows(tmp_path / "f.tsv")
    assert header == ["r"] + HEADER and all(len(row) == 1 + len(HEADER) and "" not in row for row in rows)
    fit = [b["r"] for b in summ["budgets"] if b["dp_value"] is not None]
    assert R in fit and len(fit) >= 2
    dp_values = {b["r"]: b["dp_value"] for b in summ["budgets"]}
    order = [int(row[0]) for row in rows]
    assert order == sorted(order) and set(order) == set(fit)
    for row in rows:
        assert int(row[13]) == dp_values[int(row[0])]                     # the answer's hops are worth the run's DP value at its limit
    # r == R: the --recombination-margins file of the same run
    assert [row[1:] for row in rows if int(row[0]) == R] == _rows(tmp_path / "p.tsv")[1]
    # every r: the --recombination-margins file of a separate run with -R r
    want_stats = []
    for r in fit:
        pr, fasta_r, summ_r = _cli(built_hip, c, tmp_path, ["-R", str(r), "--recombination-margins", str(tmp_path / f"p{r}.tsv")])
        assert pr.returncode == 0, pr.stderr
        assert summ_r["dp_value"] == dp_values[r]
        assert [row[1:] for row in rows if int(row[0]) == r] == _rows(tmp_path / f"p{r}.tsv")[1], r
        want_stats.append(dict(r=r, **{k: summ_r["recombination_margins"][k] for k in COUNTS}))
    # -J: per limit what FILE holds (the counts of each separate run), and the call's statistics
    br = summ["budget_recombination_margins"]
    assert br["budgets"] == want_stats and br["segments"] == 1 and br["wall_s"] > 0 and set(br) == {"budgets", "segments", "wall_s"}
    assert sum(st["transitions"] for st in want_stats) == len(rows) >= 2
    print(f"{name}: limits {fit}, rows {len(rows)}, crossovers per limit {[st['called_recombinations'] for st in want_stats]}")


def test_a_list_is_answered_in_its_order_beside_the_other_options(built_hip, tmp_path):
    c = CASES["bub_a"]
    p, fasta, summ = _cli(built_hip, c, tmp_path, ["--budgets", "all", "--budget-recombination-margins", str(tmp_path / "all.tsv")])
    assert p.returncode == 0, p.stderr
    everything = _rows(tmp_path / "all.tsv")[1]
    R = max(int(row[0]) for row in everything)
    listed = [str(R), "0", str(R - 1)]
    extra = ["--budgets", ",".join(listed), "--site-margins", str(tmp_path / "m.tsv"), "--genotype-margins", str(tmp_path / "g.tsv"), "--budget-genotype-margins", str(tmp_path / "bg.tsv"),
             "--budget-phase-margins", str(tmp_path / "bp.tsv")]
    p, fasta2, summ2 = _cli(built_hip, c, tmp_path, extra + ["--budget-recombination-margins", str(tmp_path / "some.tsv")])
    assert p.returncode == 0 and fasta2 == fasta, p.stderr
    p3, fasta3, summ3 = _cli(built_hip, c, tmp_path, [x.replace("m.tsv", "m3.tsv").replace("bg.tsv", "bg3.tsv").replace("bp.tsv", "bp3.tsv").replace("g.tsv", "g3.tsv") for x in extra])
    assert p3.returncode == 0 and fasta3 == fasta and p3.stdout == p.stdout, p3.stderr
    some = _rows(tmp_path / "some.tsv")[1]
    have = {row[0] for row in everything}
    assert some == [row for r in listed if r in have for row in everything if row[0] == r] and len(some) >= 2
    assert [b["r"] for b in summ2["budget_recombination_margins"]["budgets"]] == [int(r) for r in listed if int(r) in {b["r"] for b in summ["budget_recombination_margins"]["budgets"]}]
    for a, b in (("m.tsv", "m3.tsv"), ("g.tsv", "g3.tsv"), ("bg.tsv", "bg3.tsv"), ("bp.tsv", "bp3.tsv")):      # the other files are what they are without the option
        assert open(tmp_path / a).read() == open(tmp_path / b).read()
    assert set(summ2) == set(summ3) | {"budget_recombination_margins"}

"""-m gpu: every recombination budget 0..R from one diploid DP pass (dg_dp_run_budgets, bin/DipGenie --budgets).

The library against the oracle solved once per budget (value, s_het, both edge lists), in every lattice mode and with both chain
walkers; argument errors; the CLI against the reference's recorded answers per budget (tests/golden/budgets.json); MHC-24 by
properties and against separate -R runs of the same binary."""
import copy
import hashlib
import json
import os
import random
import subprocess

import numpy as np
import pytest

import graphgen
import oracle_py as orc
from dipgenie_amd import capi, synth

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CASES = json.load(open(os.path.join(HERE, "golden", "e2e.json")))
BUDGETS = json.load(open(os.path.join(HERE, "golden", "budgets.json")))
NEG_INF = -(2 ** 31) // 4

GRAPHS = {
    0: {}, 1: dict(max_width=30, n_levels=40, R=6), 2: dict(max_width=12, n_levels=120, R=12, p_w1=0.1),
    3: dict(max_width=40, n_levels=300, R=12, p_w1=0.3, p_colour=0.4), 4: dict(max_width=5, n_levels=12, R=30, p_w1=0.5),
    5: dict(p_w1=0.9, R=18), 6: dict(max_width=30, n_levels=60, R=18, p_w1=0.3, p_colour=0.5),
    7: dict(max_width=60, n_levels=30, R=32, p_w1=0.6), 8: dict(max_width=20, n_levels=2500, R=6, p_w1=0.05),
    9: dict(max_width=70, n_levels=10, R=4, extra_edges=3.0), 11: dict(n_levels=2, R=2),
    12: dict(max_width=12, n_levels=1200, R=8, p_w1=0.03, p_colour=0.5),
}
_ORACLE = {}


def graph(q):
    return graphgen.random_levelized(9900 + q, **GRAPHS[q])


def oracle_per_budget(q):
    """the oracle on the same arrays with g.R = r, for r = 0..R: keys (value, s_het, p1, p2)"""
    if q not in _ORACLE:
        g = graph(q)
        keys = []
        for r in range(g.R + 1):
            gr = copy.copy(g)
            gr.R = r
            ref = orc.dp_solve(gr)
            keys.append((ref["value"], ref["s_het"], tuple(ref["p1"]), tuple(ref["p2"])))
        _ORACLE[q] = keys
    return _ORACLE[q]


def test_library_every_budget_equals_the_oracle(gpu_ctx):
    n_entries = n_unreachable = n_rich = 0
    for q in GRAPHS:
        g = graph(q)
        want = oracle_per_budget(q)
        gpu_ctx.dp_load_graph(g)
        outs = gpu_ctx.dp_run_budgets(range(g.R + 1))
        assert len(outs) == g.R + 1
        for r, out in enumerate(outs):
            assert out.key() == want[r], (q, r, out.key(), want[r])
        assert list(gpu_ctx.dp_budget_values()) == [w[0] for w in want], q
        assert gpu_ctx.dp_run().key() == want[g.R], q                     # a plain run afterwards: the answer at R
        assert list(gpu_ctx.dp_budget_values()) == [w[0] for w in want], q
        n_entries += g.R + 1
        n_unreachable += sum(1 for w in want if w[0] == NEG_INF)
        for w in want:
            if w[0] == NEG_INF:
                assert w[2] == () and w[3] == ()
        n_rich += len({w[0] for w in want if w[0] != NEG_INF}) >= 3
    # against a vacuous test: most budgets are reachable and most graphs answer differently at different budgets
    print(f"entries {n_entries}, unreachable {n_unreachable}, graphs with >= 3 distinct reachable values {n_rich}")
    assert n_entries == 163 and 4 * n_unreachable <= n_entries and n_rich >= 8, (n_entries, n_unreachable, n_rich)


@pytest.mark.parametrize("lean", [1, 0])
@pytest.mark.parametrize("plane_limit", [1, 0])
@pytest.mark.parametrize("mode", ["chunked", "segmented"])
def test_every_lattice_mode_every_walker(gpu_ctx, mode, plane_limit, lean):
    for q in (3, 8, 12):
        g = graph(q)
        want = oracle_per_budget(q)
        cells = int(orc.dp_solve(g)["cells"])
        cut = {"lattice_chunk_cells": max(2, cells // 5)} if mode == "chunked" else {"segment_cells": max(1, cells // 7)}
        with gpu_ctx.dp_options(lean_chain=lean, plane_limit=plane_limit, **cut):
            gpu_ctx.dp_load_graph(g)
            rnd = random.Random(q)
            full = list(range(g.R + 1))
            rnd.shuffle(full)
            for subset in (full, [g.R], [0], [g.R, 0, g.R // 2]):
                outs = gpu_ctx.dp_run_budgets(subset)
                t = gpu_ctx.dp_timing()
                if mode == "chunked":
                    assert t.n_chunks > 1, (q, t.n_chunks)
                else:
                    assert t.n_segments > 1, (q, t.n_segments)
                for r, out in zip(subset, outs):
                    assert out.key() == want[r], (q, mode, plane_limit, lean, subset, r)
                assert list(gpu_ctx.dp_budget_values()) == [w[0] for w in want], (q, mode)


def test_errors_leave_the_context_usable(gpu_ctx):
    g = graph(6)
    want = oracle_per_budget(6)
    fresh = capi.Context(0)
    try:
        with pytest.raises(capi.DgError, match="no graph loaded"):
            fresh.dp_run_budgets([0])
    finally:
        fresh.close()
    gpu_ctx.dp_load_graph(g)
    for bad in ([g.R + 1], [-1], [3, 5, 3], [], [0, g.R + 7]):
        with pytest.raises(capi.DgError, match="dg_dp_run_budgets"):
            gpu_ctx.dp_run_budgets(bad)
        assert gpu_ctx.dp_run().key() == want[g.R], bad
    # a result whose edge buffers are too small for its budget
    res, bufs = capi.make_result(g.R)
    arr = (capi.DpResult * 1)(res)
    b = np.asarray([g.R], np.int32)
    assert capi.lib.dg_dp_run_budgets(gpu_ctx.h, b.ctypes.data, 1, arr) != 0 and b"cap" in capi.lib.dg_last_error()
    assert gpu_ctx.dp_run().key() == want[g.R]
    assert [o.key() for o in gpu_ctx.dp_run_budgets([2, g.R])] == [want[2], want[g.R]]
    # a damaged lattice: dg_dp_run_budgets fails as dg_dp_run does
    with gpu_ctx.dp_options(test_poison_level=g.n_levels - 1, test_poison_byte=0xFF):
        gpu_ctx.dp_load_graph(g)
        with pytest.raises(capi.DgError, match="corrupt|disagree"):
            gpu_ctx.dp_run()
        with pytest.raises(capi.DgError, match="(corrupt|disagree).*budget"):
            gpu_ctx.dp_run_budgets(range(g.R + 1))
    gpu_ctx.dp_load_graph(g)
    assert gpu_ctx.dp_run().key() == want[g.R]


def _cli(binary, case, out, extra=(), R=None):
    args = [a if R is None or not a.startswith("-R") else f"-R{R}" for a in case["args"]]
    cmd = [binary, "-t4"] + args + ["-g", os.path.join(ROOT, case["gfa"]), "-r", os.path.join(ROOT, case["reads"]), "-o", str(out), *extra]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return p.stdout


def _table(path):
    return [line.split("\t") for line in open(path).read().splitlines()]


@pytest.mark.parametrize("name", list(BUDGETS))
def test_cli_budgets_equal_the_reference(built_hip, gpu_ctx, tmp_path, name):
    c, gold = CASES[name], BUDGETS[name]
    R = gold["R"]
    out, tsv, js = tmp_path / "out.fa", tmp_path / "t.tsv", tmp_path / "o.json"
    plain = _cli(built_hip, c, tmp_path / "plain.fa")
    stdout = _cli(built_hip, c, out, extra=("--budgets", "all", "--budget-table", str(tsv), "-J", str(js)))
    assert stdout == plain.replace(str(tmp_path / "plain.fa").encode(), str(out).encode())      # (the line that names the -o file)
    assert hashlib.md5(open(out, "rb").read()).hexdigest() == c["fasta_md5"]
    assert open(out, "rb").read() == open(tmp_path / "plain.fa", "rb").read()
    rows = _table(tsv)
    summ = json.load(open(js))["budgets"]
    assert len(rows) == len(summ) == R + 1 == len(gold["rows"])
    for r, (row, g, s) in enumerate(zip(rows, gold["rows"], summ)):
        extra_file = tmp_path / f"out.fa.R{r}"
        if g.get("unreachable"):
            assert row == [str(r)] + ["NA"] * 5 and not extra_file.exists() and s["dp_value"] is None, (name, r)
            continue
        assert row == [str(r)] + [str(g[k]) for k in ("dp_value", "r1", "r2", "len1", "len2")], (name, r, row, g)
        assert {k: s[k] for k in ("r", "dp_value", "r1", "r2", "len1", "len2")} == {k: g[k] for k in ("r", "dp_value", "r1", "r2", "len1", "len2")}
        fa = open(out if r == R else extra_file, "rb").read()
        assert hashlib.md5(fa).hexdigest() == g["fasta_md5"], (name, r)
    assert not (tmp_path / f"out.fa.R{R}").exists()


def test_cli_budget_subset_writes_only_the_listed_files(built_hip, gpu_ctx, tmp_path):
    c, gold = CASES["bub_c"], BUDGETS["bub_c"]
    out, tsv = tmp_path / "out.fa", tmp_path / "t.tsv"
    _cli(built_hip, c, out, extra=("--budgets", "0,3", "--budget-table", str(tsv)))
    assert sorted(os.listdir(tmp_path)) == ["out.fa", "out.fa.R0", "out.fa.R3", "t.tsv"]
    assert hashlib.md5(open(out, "rb").read()).hexdigest() == c["fasta_md5"]
    rows = _table(tsv)
    assert [row[0] for row in rows] == ["0", "3"]
    for row in rows:
        g = gold["rows"][int(row[0])]
        assert row[1:] == [str(g[k]) for k in ("dp_value", "r1", "r2", "len1", "len2")]
        assert hashlib.md5(open(tmp_path / f"out.fa.R{row[0]}", "rb").read()).hexdigest() == g["fasta_md5"]


def test_cli_budgets_mhc24(built_hip, gpu_ctx, tmp_path):
    """MHC-24 (the bench workload), -R18 --budgets all: budget 18 is the reference's answer (e2e.json), the value is
    non-decreasing in the budget, and budgets 0 and 9 equal separate -R 0 / -R 9 runs of the same binary byte for byte"""
    c = CASES["mhc24_p2"]
    gfa, reads, _ = synth.ensure_mhc24(str(tmp_path / "mhc24"))
    case = dict(c, gfa=os.path.relpath(gfa, ROOT), reads=os.path.relpath(reads, ROOT))
    out, tsv, js = tmp_path / "out.fa", tmp_path / "t.tsv", tmp_path / "o.json"
    _cli(built_hip, case, out, extra=("--budgets", "all", "--budget-table", str(tsv), "-J", str(js)))
    summ = json.load(open(js))
    print("MHC-24, 19 budgets: dp_traceback_ms", summ["dp_traceback_ms"], "dp_forward_ms", summ["dp_forward_ms"])
    assert hashlib.md5(open(out, "rb").read()).hexdigest() == c["fasta_md5"] == "cd13930ac90651b7e441506c1ecd4514"
    rows = _table(tsv)
    assert [row[0] for row in rows] == [str(r) for r in range(19)]
    assert rows[18][1:4] == ["331848", "10", "8"] and (summ["dp_value"], summ["r1"], summ["r2"]) == (331848, 10, 8)
    values = [int(row[1]) for row in rows if row[1] != "NA"]
    assert values == sorted(values) and all(row[1] != "NA" for row in rows[[row[1] != "NA" for row in rows].index(True):])
    for r in (0, 9):
        sep, sj = tmp_path / f"sep{r}.fa", tmp_path / f"sep{r}.json"
        _cli(built_hip, case, sep, extra=("-J", str(sj)), R=r)
        s = json.load(open(sj))
        assert rows[r][1:] == [str(s[k]) for k in ("dp_value", "r1", "r2", "len1", "len2")], (r, rows[r], s)
        assert open(tmp_path / f"out.fa.R{r}", "rb").read() == open(sep, "rb").read(), r

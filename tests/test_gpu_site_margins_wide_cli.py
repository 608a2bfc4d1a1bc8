"""-m gpu: bin/DipGenie --site-margins FILE --wide-levels on c5s, the committed case that --site-margins alone refuses (widest level
771, R = 32: 25,443 cells): the run goes to its end, the FASTA is the golden one, and FILE holds what Context.dp_call_margins
answers on the dumped graph with the dumped allele classes under partner_wide = 1 and, the same records, under partner_wide = 2 --
the two routes on a real panel graph: the answer's own partner budgets, 32 - 18 and 32 - 14, fit the LDS."""
import hashlib

import numpy as np
import pytest

from dipgenie_amd import capi
from paths_model import NEG_INF
from test_gpu_site_margins_cli import CASES, HEADER, _cli

pytestmark = pytest.mark.gpu


def test_c5s_runs_to_the_end(built_hip, gpu_ctx, tmp_path):
    c = CASES["c5s"]
    pre = tmp_path / "dump"
    p, fasta, summ = _cli(built_hip, c, tmp_path, ["--site-margins", str(tmp_path / "m.tsv"), "--wide-levels", "-D", str(pre)])
    assert p.returncode == 0, p.stderr
    p0, fasta0, summ0 = _cli(built_hip, c, tmp_path, [])
    assert p0.returncode == 0, p0.stderr
    assert hashlib.md5(fasta).hexdigest() == c["fasta_md5"] and fasta0 == fasta
    assert p.stdout == p0.stdout
    assert set(summ) == set(summ0) | {"site_margins"} and summ["site_margins"]["wall_s"] > 0
    g = capi.DpGraphArrays.load(str(pre) + ".dpg")
    cls = np.fromfile(str(pre) + ".cls", np.int32)
    L, R = g.n_levels, g.R
    widest = int(np.diff(g.level_off).max())
    assert cls.shape == (g.n_vertices,) and (widest, R) == (771, 32) and widest * (R + 1) > 16384
    gpu_ctx.dp_load_graph(g)
    gpu_ctx.dp_run()
    with gpu_ctx.dp_options(partner_wide=1):
        levels, paths = gpu_ctx.dp_call_margins(R, cls, want_paths=True)
        route1 = gpu_ctx.dp_partner_route()
    with gpu_ctx.dp_options(partner_wide=2):
        forced, _ = gpu_ctx.dp_call_margins(R, cls)
        route2 = gpu_ctx.dp_partner_route()
    r = gpu_ctx.dp_score_paths(paths[None])[0]
    bmax = R - min(int(r["r1"]), int(r["r2"]))
    assert sorted((int(r["r1"]), int(r["r2"]))) == sorted((c["r1"], c["r2"]))
    assert route1 == (1, widest * (bmax + 1)) and route2 == (2, widest * (bmax + 1))     # 771 x 19: the queries fit the LDS, the budget does not
    assert np.array_equal(forced, levels)
    assert c["dp_value"] == 728 and (levels["value"] == 728).all()
    lines = open(tmp_path / "m.tsv").read().split("\n")
    assert lines[-1] == "" and lines[0].split("\t") == HEADER
    rows = [ln.split("\t") for ln in lines[1:-1]]
    assert len(rows) == 2 * (L - 2)
    n_alt = 0
    for i, row in enumerate(rows):
        l, h = 1 + i // 2, i % 2
        rec = levels[h, l]
        assert len(row) == 10 and (int(row[0]), int(row[1])) == (l, h + 1)
        assert (int(row[2]), int(row[5]), int(row[6])) == (rec["vertex"], rec["value"], rec["alt_vertex"]), (l, h, row)
        if rec["alt_vertex"] < 0:
            assert row[9] == "." and rec["alt_value"] == NEG_INF
            continue
        assert int(row[9]) == int(rec["value"]) - int(rec["alt_value"]) >= 0 and cls[rec["alt_vertex"]] != cls[rec["vertex"]]
        n_alt += 1
    assert n_alt >= 1 and n_alt == sum(st["with_alternative"] for st in summ["site_margins"]["haplotypes"])


def test_wide_levels_needs_site_margins(built_hip, tmp_path):
    """status 1 before any device call, the message names both options, no output of any kind"""
    p, fasta, summ = _cli(built_hip, CASES["toy1_p2"], tmp_path, ["--wide-levels"])
    assert p.returncode == 1, (p.returncode, p.stderr)
    assert b"--wide-levels" in p.stderr and b"--site-margins" in p.stderr and p.stdout == b""
    assert fasta is None and summ is None

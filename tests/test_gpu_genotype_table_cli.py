"""-m gpu: bin/DipGenie --genotype-table FILE on committed end-to-end cases: FILE parses, per level its rows are sorted by genotype,
one of them is the answer's and one is worth the DP value; it agrees with the --genotype-margins file of the same run and with what
Context.dp_genotype_table answers on the dumped graph; the margins file, the FASTA and stdout are those of a run without the option;
the -J summary counts what FILE holds."""
import hashlib

import numpy as np
import pytest

from dipgenie_amd import capi
from test_gpu_site_margins_cli import CASES, _cli

pytestmark = pytest.mark.gpu

HEADER = "level vertex1 segment1 vertex2 segment2 value delta called".split()


def _parse(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and lines[0].split("\t") == HEADER
    rows = [ln.split("\t") for ln in lines[1:-1]]
    assert all(len(r) == 8 and "" not in r for r in rows)
    return rows


@pytest.mark.parametrize("name", ["bub_a", "bub_c"])
def test_genotype_table_file(built_hip, gpu_ctx, tmp_path, name):
    c = CASES[name]
    pre = tmp_path / "dump"
    p, fasta, summ = _cli(built_hip, c, tmp_path, ["--genotype-table", str(tmp_path / "t.tsv"), "--genotype-margins", str(tmp_path / "g.tsv"), "-D", str(pre)])
    assert p.returncode == 0, p.stderr
    p1, fasta1, summ1 = _cli(built_hip, c, tmp_path, ["--genotype-margins", str(tmp_path / "g1.tsv")])
    p0, fasta0, summ0 = _cli(built_hip, c, tmp_path, [])
    p2, fasta2, summ2 = _cli(built_hip, c, tmp_path, ["--genotype-table", str(tmp_path / "t2.tsv"), "-D", str(tmp_path / "dump2")])
    assert p1.returncode == 0 and p0.returncode == 0 and p2.returncode == 0, (p1.stderr, p0.stderr, p2.stderr)
    # everything else is what it is without the option
    assert hashlib.md5(fasta).hexdigest() == c["fasta_md5"] and fasta0 == fasta == fasta1 == fasta2
    assert p.stdout == p0.stdout == p1.stdout == p2.stdout
    assert open(tmp_path / "g.tsv", "rb").read() == open(tmp_path / "g1.tsv", "rb").read()
    assert open(tmp_path / "t.tsv", "rb").read() == open(tmp_path / "t2.tsv", "rb").read()
    assert open(str(pre) + ".cls", "rb").read() == open(str(tmp_path / "dump2") + ".cls", "rb").read()
    assert set(summ) == set(summ1) | {"genotype_table"} and set(summ2) == set(summ0) | {"genotype_table"}
    assert "genotype_table" not in summ1["stages"] and "genotype_table" in summ["stages"] and "genotype_margins" not in summ2["stages"]
    drop = lambda d: {k: v for k, v in d.items() if k != "wall_s"}
    assert drop(summ["genotype_margins"]) == drop(summ1["genotype_margins"]) and drop(summ["genotype_table"]) == drop(summ2["genotype_table"])
    for key in summ0:
        if key not in ("stages", "dp_forward_ms", "dp_traceback_ms"):
            assert summ[key] == summ0[key] == summ2[key], key
    # FILE by itself
    g = capi.DpGraphArrays.load(str(pre) + ".dpg")
    cls = np.fromfile(str(pre) + ".cls", np.int32)
    L, R, V = g.n_levels, g.R, summ["dp_value"]
    rows = _parse(tmp_path / "t.tsv")
    margins = [ln.split("\t") for ln in open(tmp_path / "g.tsv").read().split("\n")[1:-1]]
    assert len(margins) == L - 2
    by_level = {}
    for r in rows:
        by_level.setdefault(int(r[0]), []).append(r)
    assert sorted(by_level) == list(range(1, L - 1)) and [int(r[0]) for r in rows] == sorted(int(r[0]) for r in rows)
    recount = dict(entries=len(rows), levels_with_choice=0, co_optimal_levels=0, max_per_level=0)
    for l in range(1, L - 1):
        lv = [(int(r[1]), int(r[3]), int(r[5]), int(r[6]), int(r[7])) for r in by_level[l]]
        a0, e0 = int(g.level_off[l]), int(g.level_off[l + 1])
        assert all(a0 <= v1 <= v2 < e0 for v1, v2, _, _, _ in lv)
        genos = [tuple(sorted((int(cls[v1]), int(cls[v2])))) for v1, v2, _, _, _ in lv]
        assert genos == sorted(set(genos)), (l, genos)                      # ascending (class1, class2), each genotype once
        assert all(delta == V - value and delta >= 0 for _, _, value, delta, _ in lv) and any(delta == 0 for _, _, _, delta, _ in lv)
        assert sorted(called for _, _, _, _, called in lv) == [0] * (len(lv) - 1) + [1]
        # against the margins row of the level: the called genotype and its value, the best other row is the alternative
        m = margins[l - 1]
        assert int(m[0]) == l
        mine = next(x for x in lv if x[4] == 1)
        assert genos[lv.index(mine)] == tuple(sorted((int(cls[int(m[1])]), int(cls[int(m[4])])))) and mine[2] == int(m[7]) == V
        others = sorted((-value, v1, v2) for v1, v2, value, _, called in lv if not called)
        if others:
            assert (others[0][1], others[0][2], -others[0][0]) == (int(m[8]), int(m[10]), int(m[12])), (l, others[0], m)
        else:
            assert m[8:] == ["."] * 6
        recount["levels_with_choice"] += len(lv) >= 2
        recount["co_optimal_levels"] += sum(delta == 0 for _, _, _, delta, _ in lv) >= 2
        recount["max_per_level"] = max(recount["max_per_level"], len(lv))
    gt = summ["genotype_table"]
    assert {k: gt[k] for k in recount} == recount and gt["wall_s"] > 0 and set(gt) == set(recount) | {"wall_s"}
    assert recount["levels_with_choice"] >= 1
    # FILE against the library on the dumped graph with the dumped classes
    gpu_ctx.dp_load_graph(g)
    off, entries, best = gpu_ctx.dp_genotype_table(R, cls)
    assert best == V == c["dp_value"]
    inner = entries[off[1]:off[L - 1]]
    assert len(inner) == len(rows)
    assert [(int(r[1]), int(r[3]), int(r[5])) for r in rows] == list(zip(inner["vertex1"].tolist(), inner["vertex2"].tolist(), inner["value"].tolist()))

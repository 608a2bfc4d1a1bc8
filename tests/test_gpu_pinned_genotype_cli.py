"""-m gpu: bin/DipGenie --pins FILE --pinned-genotype-table FILE --pinned-genotype-margins FILE on a committed end-to-end case.  An
alternative genotype of the --genotype-table file, pinned: at its level the pinned table's called row is that genotype, with delta 0
and the value the unpinned table lists for it, which is the pinned run's dp_value; both files are what the library answers on the dumped
graph with the dumped classes for the pinned answer's cells; one pass serves both files; a pin set nothing satisfies leaves the headers
alone."""
import numpy as np
import pytest

from dipgenie_amd import capi
from paths_model import NEG_INF
from test_gpu_genotype_table_cli import HEADER, _parse
from test_gpu_site_margins_cli import CASES, _cli

pytestmark = pytest.mark.gpu

MARGINS_HEADER = "level vertex1 panel_hap1 segment1 vertex2 panel_hap2 segment2 value alt_vertex1 alt_segment1 alt_vertex2 alt_segment2 alt_value margin".split()


def _margins(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and lines[0].split("\t") == MARGINS_HEADER
    return [ln.split("\t") for ln in lines[1:-1]]


@pytest.mark.parametrize("name", ["bub_a", "bub_c"])
def test_pinned_genotype_files(built_hip, gpu_ctx, tmp_path, name):
    c = CASES[name]
    pre = tmp_path / "dump"
    pt, fasta_t, summ_t = _cli(built_hip, c, tmp_path, ["--genotype-table", str(tmp_path / "t.tsv"), "-D", str(pre)])
    assert pt.returncode == 0, pt.stderr
    V = summ_t["dp_value"]
    g = capi.DpGraphArrays.load(str(pre) + ".dpg")
    cls = np.fromfile(str(pre) + ".cls", np.int32)
    L, R = g.n_levels, g.R
    rows = [(int(r[0]), int(r[1]), int(r[3]), int(r[5]), int(r[6]), int(r[7])) for r in _parse(tmp_path / "t.tsv")]   # level, vertex1, vertex2, value, delta, called
    # the alternative that costs most (the choice of tests/test_gpu_cli_pins.py)
    others = sorted((r for r in rows if r[5] == 0 and r[3] != NEG_INF), key=lambda r: (-r[4], r[0], r[1], r[2]))
    assert others and others[0][4] > 0
    level, v1, v2, value, delta, _ = others[0]
    pins_file = tmp_path / "row.pins"
    pins_file.write_text(f"{level}\t{v1}\t{v2}\n")
    pins = capi.genotype_pins(level, v1, v2)

    both = ["--pins", str(pins_file), "--pinned-genotype-table", str(tmp_path / "pt.tsv"), "--pinned-genotype-margins", str(tmp_path / "pm.tsv"), "-D", str(tmp_path / "dump2")]
    p, fasta, summ = _cli(built_hip, c, tmp_path, both)
    assert p.returncode == 0, p.stderr
    p0, fasta0, summ0 = _cli(built_hip, c, tmp_path, ["--pins", str(pins_file)])
    p1, fasta1, summ1 = _cli(built_hip, c, tmp_path, ["--pins", str(pins_file), "--pinned-genotype-table", str(tmp_path / "pt1.tsv")])
    p2, fasta2, summ2 = _cli(built_hip, c, tmp_path, ["--pins", str(pins_file), "--pinned-genotype-margins=" + str(tmp_path / "pm2.tsv")])
    assert p0.returncode == 0 and p1.returncode == 0 and p2.returncode == 0, (p0.stderr, p1.stderr, p2.stderr)
    # everything else is what --pins alone gives; one pass serves both files
    assert fasta == fasta0 == fasta1 == fasta2 and p.stdout == p0.stdout == p1.stdout == p2.stdout
    assert open(tmp_path / "pt.tsv", "rb").read() == open(tmp_path / "pt1.tsv", "rb").read() and open(tmp_path / "pm.tsv", "rb").read() == open(tmp_path / "pm2.tsv", "rb").read()
    assert set(summ) == set(summ0) | {"pinned_genotype_table", "pinned_genotype_margins"} and set(summ1) == set(summ0) | {"pinned_genotype_table"}
    assert set(summ2) == set(summ0) | {"pinned_genotype_margins"} and "genotype_table" not in summ and "genotype_margins" not in summ
    assert "pinned_genotype_table" in summ["stages"] and "pinned_genotype_margins" in summ["stages"] and "pinned_genotype_margins" not in summ1["stages"]
    assert open(str(tmp_path / "dump2") + ".cls", "rb").read() == cls.tobytes()
    for key in summ0:
        if key not in ("stages", "dp_forward_ms", "dp_traceback_ms"):
            assert summ[key] == summ0[key], key
    drop = lambda d: {k: v for k, v in d.items() if k != "wall_s"}
    assert drop(summ["pinned_genotype_table"]) == drop(summ1["pinned_genotype_table"]) and drop(summ["pinned_genotype_margins"]) == drop(summ2["pinned_genotype_margins"])
    assert set(summ["pinned_genotype_table"]) == set(summ_t["genotype_table"])                # the fields of the unpinned objects
    assert set(summ["pinned_genotype_margins"]) == {"with_alternative", "margin0", "min_positive_margin", "segments", "wall_s"}

    # the pinned -J value is the unpinned table's entry of the pinned genotype; at its level the called row is that genotype, delta 0
    assert summ["dp_value"] == value == V - delta and summ["pins"]["satisfied"] is True
    prow = [(int(r[0]), int(r[1]), int(r[3]), int(r[5]), int(r[6]), int(r[7])) for r in _parse(tmp_path / "pt.tsv")]
    at = [r for r in prow if r[0] == level]
    assert at == [(level, min(v1, v2), max(v1, v2), value, 0, 1)], at      # both orders required: the level's only genotype
    by_level = {}
    for r in prow:
        by_level.setdefault(r[0], []).append(r)
    assert sorted(by_level) == list(range(1, L - 1))
    recount = dict(entries=len(prow), levels_with_choice=0, co_optimal_levels=0, max_per_level=0)
    for l, lv in by_level.items():
        assert all(r[4] == value - r[3] and r[4] >= 0 for r in lv) and any(r[4] == 0 for r in lv) and sorted(r[5] for r in lv) == [0] * (len(lv) - 1) + [1]
        recount["levels_with_choice"] += len(lv) >= 2
        recount["co_optimal_levels"] += sum(r[4] == 0 for r in lv) >= 2
        recount["max_per_level"] = max(recount["max_per_level"], len(lv))
    assert drop(summ["pinned_genotype_table"]) == recount
    # every pinned row is a row of the unpinned table, worth at most what it is worth there
    geno = lambda r: (r[0],) + tuple(sorted((int(cls[r[1]]), int(cls[r[2]]))))
    free_g = {geno(r): r[3] for r in rows}
    assert all(geno(r) in free_g and r[3] <= free_g[geno(r)] for r in prow) and len(prow) <= len(rows)

    # both files against the library on the dumped graph: the called cells are the pinned run's answer
    gpu_ctx.dp_load_graph(g)
    assert gpu_ctx.dp_run_pinned(pins)[0].value == value
    paths = gpu_ctx.dp_answer_paths(R)
    off, entries, best, levels = gpu_ctx.dp_genotype_table_pinned(pins, R, cls, paths)
    assert best == value
    inner = entries[off[1]:off[L - 1]]
    assert [(r[1], r[2], r[3]) for r in prow] == list(zip(inner["vertex1"].tolist(), inner["vertex2"].tolist(), inner["value"].tolist()))
    margins = _margins(tmp_path / "pm.tsv")
    assert len(margins) == L - 2
    count = dict(with_alternative=0, margin0=0, min_positive_margin=None)
    for l in range(1, L - 1):
        m, rec = margins[l - 1], levels[0, l]
        assert (int(m[0]), int(m[1]), int(m[4]), int(m[7])) == (l, rec["vertex1"], rec["vertex2"], rec["value"]) and rec["value"] == value, (l, m, rec)
        if rec["alt_vertex1"] >= 0:
            assert (int(m[8]), int(m[10]), int(m[12]), int(m[13])) == (rec["alt_vertex1"], rec["alt_vertex2"], rec["alt_value"], rec["value"] - rec["alt_value"]), (l, m, rec)
            margin = int(m[13])
            count["with_alternative"] += 1
            count["margin0"] += margin == 0
            if margin > 0 and (count["min_positive_margin"] is None or margin < count["min_positive_margin"]):
                count["min_positive_margin"] = margin
        else:
            assert m[8:] == ["."] * 6
    assert margins[level - 1][8:] == ["."] * 6           # the pinned level has no other genotype
    assert {k: summ["pinned_genotype_margins"][k] for k in count} == count and summ["pinned_genotype_margins"]["segments"] == 1


def test_an_unsatisfiable_pin_set_leaves_the_headers(built_hip, tmp_path):
    c = CASES["bub_a"]
    pins_file = tmp_path / "none.pins"
    pins_file.write_text("1\t.\t.\tforbid\n")
    p, fasta, summ = _cli(built_hip, c, tmp_path, ["--pins", str(pins_file), "--pinned-genotype-table", str(tmp_path / "pt.tsv"), "--pinned-genotype-margins", str(tmp_path / "pm.tsv")])
    assert p.returncode == 0, p.stderr
    assert open(tmp_path / "pt.tsv").read() == "\t".join(HEADER) + "\n" and open(tmp_path / "pm.tsv").read() == "\t".join(MARGINS_HEADER) + "\n"
    assert {k: v for k, v in summ["pinned_genotype_table"].items() if k != "wall_s"} == dict(entries=0, levels_with_choice=0, co_optimal_levels=0, max_per_level=0)
    gm = summ["pinned_genotype_margins"]
    assert (gm["with_alternative"], gm["margin0"], gm["min_positive_margin"]) == (0, 0, None)

"""-m gpu: bin/DipGenie --site-margins FILE on committed end-to-end cases: the FASTA is the golden one, FILE holds what
Context.dp_call_margins answers on the dumped graph with the dumped allele classes, the -J summary counts what FILE holds, and a run
without the option writes the same FASTA and a summary without site_margins.  (Widest level x (R + 1) of the cases, from the dumped
graphs: toy1_p2 15 x 3, bub_a 25 x 5, bub_c 65 x 9 -- a level wider than one wave; c5s 771 x 33 is beyond the 16,384 cells.)"""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from dipgenie_amd import capi
from paths_model import NEG_INF

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CASES = json.load(open(os.path.join(HERE, "golden", "e2e.json")))
HEADER = "level hap vertex panel_hap segment value alt_vertex alt_panel_hap alt_segment margin".split()


def _cli(cli, case, tmp, extra):
    """one run writing tmp/o.fa and tmp/o.json (stdout names the FASTA's path: every run of a test uses the same one);
    returns the process, the FASTA's bytes and the summary (None where the file was not written) -- the files are removed"""
    out, js = tmp / "o.fa", tmp / "o.json"
    p = subprocess.run([cli, "-t8"] + case["args"] + ["-g", os.path.join(ROOT, case["gfa"]), "-r", os.path.join(ROOT, case["reads"]), "-o", str(out), "-J", str(js), *extra],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    fasta = open(out, "rb").read() if out.exists() else None
    summ = json.load(open(js)) if js.exists() else None
    for f in (out, js):
        if f.exists():
            os.remove(f)
    return p, fasta, summ


@pytest.mark.parametrize("name", ["toy1_p2", "bub_a", "bub_c"])
def test_site_margins_file_is_what_the_library_answers(built_hip, gpu_ctx, tmp_path, name):
    c = CASES[name]
    pre = tmp_path / "dump"
    p, fasta, summ = _cli(built_hip, c, tmp_path, ["--site-margins", str(tmp_path / "m.tsv"), "-D", str(pre)])
    assert p.returncode == 0, p.stderr
    p0, fasta0, summ0 = _cli(built_hip, c, tmp_path, [])
    assert p0.returncode == 0, p0.stderr
    assert hashlib.md5(fasta).hexdigest() == c["fasta_md5"] and fasta0 == fasta
    assert p.stdout == p0.stdout
    assert "site_margins" not in summ0 and "site_margins" not in summ0["stages"]
    assert set(summ) == set(summ0) | {"site_margins"}
    for key in summ0:
        if key not in ("stages", "dp_forward_ms", "dp_traceback_ms"):
            assert summ[key] == summ0[key], key
    # FILE against the library on the dumped graph with the dumped classes
    g = capi.DpGraphArrays.load(str(pre) + ".dpg")
    cls = np.fromfile(str(pre) + ".cls", np.int32)
    L, R = g.n_levels, g.R
    assert cls.shape == (g.n_vertices,) and int(np.diff(g.level_off).max()) * (R + 1) <= 16384
    assert len(set(cls.tolist())) < g.n_vertices          # some vertices share an allele
    gpu_ctx.dp_load_graph(g)
    gpu_ctx.dp_run()
    levels, _ = gpu_ctx.dp_call_margins(R, cls)
    assert (levels["value"] == c["dp_value"]).all()
    lines = open(tmp_path / "m.tsv").read().split("\n")
    assert lines[-1] == "" and lines[0].split("\t") == HEADER
    rows = [ln.split("\t") for ln in lines[1:-1]]
    assert len(rows) == 2 * (L - 2)
    stats = [dict(with_alternative=0, margin0=0, min_positive_margin=None) for _ in range(2)]
    for i, row in enumerate(rows):
        l, h = 1 + i // 2, i % 2
        rec = levels[h, l]
        assert len(row) == 10 and (int(row[0]), int(row[1])) == (l, h + 1)
        assert (int(row[2]), int(row[5]), int(row[6])) == (rec["vertex"], rec["value"], rec["alt_vertex"]), (l, h, row)
        assert "" not in row and (rec["alt_vertex"] >= 0 or (row[7], row[8]) == (".", "."))
        if rec["alt_vertex"] < 0:
            assert row[9] == "." and rec["alt_value"] == NEG_INF
            continue
        margin = int(rec["value"]) - int(rec["alt_value"])
        assert int(row[9]) == margin >= 0 and cls[rec["alt_vertex"]] != cls[rec["vertex"]]
        st = stats[h]
        st["with_alternative"] += 1
        st["margin0"] += margin == 0
        if margin > 0:
            st["min_positive_margin"] = margin if st["min_positive_margin"] is None else min(st["min_positive_margin"], margin)
    sm = summ["site_margins"]
    assert sm["haplotypes"] == stats and sm["wall_s"] > 0
    assert sum(st["with_alternative"] for st in stats) >= 1


def test_the_cell_cap_ends_the_run_before_the_dp(built_hip, gpu_ctx, tmp_path):
    """c5s: widest level 771, R = 32 -- status 1, the message names the option and both numbers, no FASTA, no FILE, no summary"""
    p, fasta, summ = _cli(built_hip, CASES["c5s"], tmp_path, ["--site-margins", str(tmp_path / "m.tsv")])
    assert p.returncode == 1, (p.returncode, p.stderr)
    assert b"--site-margins" in p.stderr and b"771" in p.stderr and b"33" in p.stderr, p.stderr
    assert fasta is None and summ is None and not (tmp_path / "m.tsv").exists()

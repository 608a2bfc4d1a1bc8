"""-m gpu: bin/DipGenie --pins FILE on a committed end-to-end case.  A row of the --genotype-table file that is not the call, pasted
into FILE, gives the pair of haplotypes that realises it: the -J summary's dp_value is the row's value, the pins are satisfied, the
FASTA is another one; forbidding the called genotype gives what Context.dp_run_pinned answers on the dumped graph; --budgets reads the
pinned run out per limit; a malformed FILE or an id outside its level ends the run with status 2 and no FASTA; the refused
combinations are usage errors; without the option every output is what it was."""
import hashlib

import pytest

from dipgenie_amd import capi
from paths_model import NEG_INF
from test_gpu_genotype_table_cli import _parse
from test_gpu_site_margins_cli import CASES, _cli

pytestmark = pytest.mark.gpu


def _pins(tmp, name, text):
    path = tmp / name
    path.write_text(text)
    return ["--pins", str(path)]


def test_pins_file(built_hip, gpu_ctx, tmp_path):
    c = CASES["bub_a"]
    pre = tmp_path / "dump"
    p0, fasta0, summ0 = _cli(built_hip, c, tmp_path, [])
    pt, fasta_t, summ_t = _cli(built_hip, c, tmp_path, ["--genotype-table", str(tmp_path / "t.tsv"), "-D", str(pre)])
    assert p0.returncode == 0 and pt.returncode == 0, (p0.stderr, pt.stderr)
    # without --pins: the golden FASTA, and no word of pins in the summary
    assert hashlib.md5(fasta0).hexdigest() == c["fasta_md5"] and fasta_t == fasta0 and "pins" not in summ0 and "pins" not in summ_t
    V = summ0["dp_value"]
    assert V == c["dp_value"]
    g = capi.DpGraphArrays.load(str(pre) + ".dpg")
    R = g.R
    rows = [(int(r[0]), int(r[1]), int(r[3]), int(r[5]), int(r[6]), int(r[7])) for r in _parse(tmp_path / "t.tsv")]   # level, vertex1, vertex2, value, delta, called
    # a row beside the call, finite: the one that costs most (among equals the lowest level, then the smallest ids).  A co-optimal row
    # may be another anchor of the sequence the call already spells -- the rows of delta 0 of this case are, and leave the FASTA as it
    # is --; the row furthest from the call goes through an allele that the call does not carry
    others = sorted((r for r in rows if r[5] == 0 and r[3] != NEG_INF), key=lambda r: (-r[4], r[0], r[1], r[2]))
    assert others, "no genotype beside the call on any level"
    assert others[0][4] > 0
    level, v1, v2, value, delta, _ = others[0]
    assert delta == V - value

    # the row, pasted in: the pair of haplotypes that realises it
    p1, fasta1, summ1 = _cli(built_hip, c, tmp_path, _pins(tmp_path, "row.pins", f"# level\tvertex1\tvertex2\n{level}\t{v1}\t{v2}\n") + ["--budgets", "all", "--budget-table", str(tmp_path / "b.tsv")])
    assert p1.returncode == 0, p1.stderr
    assert summ1["dp_value"] == value
    assert summ1["pins"] == dict(rows=1, pins=1 if v1 == v2 else 2, levels=1, pairs_as_singles=summ1["pins"]["pairs_as_singles"], satisfied=True)
    assert fasta1 is not None and fasta1 != fasta0
    gpu_ctx.dp_load_graph(g)
    outs = gpu_ctx.dp_run_pinned(capi.genotype_pins(level, v1, v2), range(R + 1))
    assert outs[R].value == value
    paths = gpu_ctx.dp_answer_paths(R)
    assert {int(paths[0][level]), int(paths[1][level])} == {v1, v2}
    assert [b["dp_value"] for b in summ1["budgets"]] == [None if o.value == NEG_INF else o.value for o in outs]     # <-o>.R<r>, --budget-table: the pinned answers
    for r, o in enumerate(outs):
        assert (tmp_path / f"o.fa.R{r}").exists() == (o.value != NEG_INF and r != R), r
    # the ordered kinds are one pin each
    text = f"{level}\t{v1}\t{v2}\trequire-ordered\n" + (f"{level}\t{v2}\t{v1}\tforbid-ordered # the mirror\n" if v1 != v2 else "")
    p2, fasta2, summ2 = _cli(built_hip, c, tmp_path, _pins(tmp_path, "ord.pins", text))
    assert p2.returncode == 0 and summ2["pins"]["rows"] == summ2["pins"]["pins"] == text.count("\n") and summ2["pins"]["levels"] == 1, p2.stderr
    assert summ2["dp_value"] == value and summ2["pins"]["satisfied"] is True

    # forbidding the called genotype's cell: the best other answer, as the library gives it on the dumped graph
    c1, c2 = next((r[1], r[2]) for r in rows if r[0] == level and r[5] == 1)
    want = gpu_ctx.dp_run_pinned(capi.genotype_pins(level, c1, c2, capi.PIN_FORBID))[0].value
    best_other = max(r[3] for r in rows if r[0] == level and r[5] == 0)
    assert best_other <= want <= V
    p3, fasta3, summ3 = _cli(built_hip, c, tmp_path, _pins(tmp_path, "forbid.pins", f"{level}\t{c1}\t{c2}\tforbid\n"))
    assert p3.returncode == 0 and summ3["dp_value"] == want and summ3["pins"]["satisfied"] is True, p3.stderr

    # a malformed FILE, an id outside its level: status 2 before the DP, no FASTA
    a0, a1 = int(g.level_off[level]), int(g.level_off[level + 1])
    for text, word in ((f"{level}\t{v1}\n", b"columns"), (f"{level}\tx\t{v2}\n", b"vertex id"), (f"{level} {v1} {v2}\n", b"columns"), (f"{level}\t{v1}\t{v2}\tmaybe\n", b"kind"),
                       (f"-1\t{v1}\t{v2}\n", b"level"), (f"{level}\t{v1}\t{a1}\n", b"not on level"), (f"{level}\t{a0 - 1}\t.\n", b"not on level"), (f"0\t0\t0\n", b"outside 1.."),
                       (f"{g.n_levels - 1}\t.\t.\n", b"outside 1..")):
        pb, fasta_b, summ_b = _cli(built_hip, c, tmp_path, _pins(tmp_path, "bad.pins", text))
        assert pb.returncode == 2 and b"--pins: line 1" in pb.stderr and word in pb.stderr and fasta_b is None and summ_b is None, (text, pb.returncode, pb.stderr)
    pm, fasta_m, _ = _cli(built_hip, c, tmp_path, ["--pins", str(tmp_path / "missing.pins")])
    assert pm.returncode == 2 and b"cannot open" in pm.stderr and fasta_m is None

    # refused beside the options that describe the unconstrained DP, and beside --gpus: usage errors
    ok = _pins(tmp_path, "row.pins", f"{level}\t{v1}\t{v2}\n")
    for extra, word in ((["--site-margins", "s.tsv"], b"--site-margins"), (["--genotype-margins", "m.tsv"], b"--genotype-margins"), (["--genotype-table", "t.tsv"], b"--genotype-table"),
                        (["--gpus", "2"], b"--gpus"), (["-p1"], b"-p2")):
        pr, fasta_r, summ_r = _cli(built_hip, c, tmp_path, ok + extra)
        assert pr.returncode == 1 and b"[E::main] --pins" in pr.stderr and word in pr.stderr and fasta_r is None and summ_r is None, (extra, pr.stderr)
    pe, fasta_e, _ = _cli(built_hip, c, tmp_path, ["--pins", ""])
    assert pe.returncode == 1 and b"--pins needs a file name" in pe.stderr and fasta_e is None

"""-m gpu: bin/DipGenie --tag-reads FILE on committed end-to-end cases: FILE holds, per read in input order, what
Context.sketch_tag_reads answers against the two sequences of the written FASTA (and what the model answers), the -J summary counts the
tags, and a run without the option writes the same FASTA and standard output and a summary without `read_tags`."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import tag_model as tm

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CASES = json.load(open(os.path.join(HERE, "golden", "e2e.json")))
HEADER = "read length n_min only_1 only_2 both tag".split()


def _fasta(path):
    """(name, sequence) per record: the name ends at the first white space, the lines of a sequence are joined"""
    recs = []
    for ln in open(path, "rb").read().split(b"\n"):
        ln = ln.rstrip(b"\r")
        if ln.startswith(b">"):
            recs.append([ln[1:].split()[0].decode() if ln[1:].split() else "", b""])
        elif recs:
            recs[-1][1] += ln
    return [(n, s) for n, s in recs]


def _cli(cli, case, tmp, extra):
    out, js = tmp / "o.fa", tmp / "o.json"
    p = subprocess.run([cli, "-t8"] + case["args"] + ["-g", os.path.join(ROOT, case["gfa"]), "-r", os.path.join(ROOT, case["reads"]), "-o", str(out), "-J", str(js), *extra],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    summ = json.load(open(js)) if js.exists() else None
    files = {}
    for f in sorted(tmp.iterdir()):
        if f.name != "o.json":
            files[f.name] = f.read_bytes()
        os.remove(f)
    return p, files, summ


@pytest.mark.parametrize("name", ["toy1_p2", "bub_a", "bub_c"])
def test_tag_file_is_what_the_library_and_the_model_answer(built_hip, gpu_ctx, tmp_path, name):
    c = CASES[name]
    k, w = (int(next(a for a in c["args"] if a.startswith(f))[2:]) for f in ("-k", "-w"))
    common = ["--budgets", "all", "--budget-table", str(tmp_path / "b.tsv"), "--objective-table", str(tmp_path / "ob.tsv")]
    p, files, summ = _cli(built_hip, c, tmp_path, common + ["--tag-reads", str(tmp_path / "t.tsv")])
    assert p.returncode == 0, p.stderr
    p0, files0, summ0 = _cli(built_hip, c, tmp_path, common)
    assert p0.returncode == 0, p0.stderr
    # FASTA files, stdout, the budget and objective tables: byte for byte
    assert hashlib.md5(files["o.fa"]).hexdigest() == c["fasta_md5"]
    table = files.pop("t.tsv")
    assert files == files0 and "b.tsv" in files and "ob.tsv" in files and "t.tsv" not in files0
    assert p.stdout == p0.stdout
    # -J: the read_tags key only (and the stage's wall time)
    assert "read_tags" not in summ0 and "tag_reads" not in summ0["stages"] and "tag_reads" in summ["stages"]
    assert set(summ) == set(summ0) | {"read_tags"} and set(summ["stages"]) == set(summ0["stages"]) | {"tag_reads"}
    for key in summ0:
        if key not in ("stages", "dp_forward_ms", "dp_traceback_ms"):
            assert summ[key] == summ0[key], key
    # FILE: header, one row per read in input order with the reader's names and lengths
    (tmp_path / "o.fa").write_bytes(files["o.fa"])
    (_, s1), (_, s2) = _fasta(tmp_path / "o.fa")
    reads = _fasta(os.path.join(ROOT, c["reads"]))
    lines = table.decode().split("\n")
    assert lines[-1] == "" and lines[0].split("\t") == HEADER
    rows = [ln.split("\t") for ln in lines[1:-1]]
    assert all(len(r) == 7 for r in rows)
    assert [r[0] for r in rows] == [n for n, _ in reads] and [int(r[1]) for r in rows] == [len(s) for _, s in reads]
    # counts: the library on the sequences read back from the FASTA, and the model
    ha, hb = gpu_ctx.sketch_haplotype(s1, k, w)[0], gpu_ctx.sketch_haplotype(s2, k, w)[0]
    seqs = [s for _, s in reads]
    lib = gpu_ctx.sketch_tag_reads(seqs, k, w, ha, hb)
    want = tm.tag_reads(seqs, k, w, ha, hb)
    got = np.array([[int(x) for x in r[2:6]] for r in rows], np.int32).reshape(len(rows), 4)
    assert np.array_equal(lib, want) and np.array_equal(got, want)
    tags = [int(r[6]) for r in rows]
    assert tags == [tm.tag_of(a, b) for _, a, b, _ in want]
    rt = summ["read_tags"]
    assert set(rt) == {"reads", "hap1", "hap2", "tie", "no_evidence"}
    assert rt["reads"] == len(reads) == rt["hap1"] + rt["hap2"] + rt["tie"] + rt["no_evidence"]
    assert rt["hap1"] == tags.count(1) and rt["hap2"] == tags.count(2)
    assert rt["tie"] == int(((want[:, 1] == want[:, 2]) & (want[:, 1] > 0)).sum()) and rt["no_evidence"] == int(((want[:, 1] == 0) & (want[:, 2] == 0)).sum())
    assert want[:, 0].sum() > 0
    print(f"{name}: {rt}")

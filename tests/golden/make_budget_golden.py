#!/usr/bin/env python3
"""Regenerates tests/golden/budgets.json from the REAL reference (run in the build container only, beside make_golden.py).

The reference binary under oracle/_ref/ is run on four small panels of e2e.json once per recombination limit r = 0..R; per r the
file records what the run answered: dp_value, r1, r2, len1, len2 and the md5 of its FASTA (recorded results only).  A limit the
reference cannot answer (no path with so few recombinations: it leaves without a FASTA) is recorded as {"unreachable": true}.
Usage: python tests/golden/make_budget_golden.py
"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

PANELS = {"bub_c": 8, "bub_e": 10, "bub_g": 18, "c5s": 32}       # name in e2e.json -> its -R


def main():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "ref"])
    cases = json.load(open(os.path.join(HERE, "e2e.json")))
    out = {}
    for name, R in PANELS.items():
        c = cases[name]
        assert f"-R{R}" in c["args"], (name, c["args"])
        rows = []
        for r in range(R + 1):
            args = [a if not a.startswith("-R") else f"-R{r}" for a in c["args"]]
            try:
                d = mg.run_ref(os.path.join(ROOT, c["gfa"]), os.path.join(ROOT, c["reads"]), args, threads=8 if name == "c5s" else 4)
                rows.append(dict(r=r, **{k: d[k] for k in ("dp_value", "r1", "r2", "len1", "len2", "fasta_md5")}))
            except (subprocess.CalledProcessError, FileNotFoundError, KeyError):
                rows.append(dict(r=r, unreachable=True))
            print(name, rows[-1], flush=True)
        assert {k: rows[R][k] for k in ("dp_value", "fasta_md5")} == {k: c[k] for k in ("dp_value", "fasta_md5")}, name   # r = R is e2e.json's run
        out[name] = dict(R=R, args=c["args"], rows=rows)
    json.dump(out, open(os.path.join(HERE, "budgets.json"), "w"), indent=1)


if __name__ == "__main__":
    main()

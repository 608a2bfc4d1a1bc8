#!/usr/bin/env python3
"""Call margins of the run's own answer on a dumped graph, with dp_answer_paths and dp_call_margins.

usage: call_margins.py GRAPH.dpg [--budget b] [--classes FILE.cls] [--wide {0,1,2}]

Runs the sweep (dp_run_budgets of the one budget; default: the graph's R), takes the answer as a pair of paths, checks it with
dp_score_paths against the plane's value, and asks dp_call_margins for both haplotypes: per level the called vertex and the best
vertex of another class (FILE.cls: raw int32 per vertex, as bin/DipGenie --site-margins -D writes it; without it every vertex is its
own class).  Prints, per haplotype, the levels with an alternative, the levels with margin 0 (the reads cannot tell the called
allele from another one there, given the other haplotype), the smallest positive margin, and the wall time of the one
dp_call_margins call.  --wide w sets option partner_wide: 0 (default) the level state stays in LDS and a graph beyond 16,384 cells (widest level x
(budget + 1)) is refused, 1 such a call keeps it in device memory, 2 every call does (A/B timing); the route taken is printed.  Exit status 1 if dp_score_paths of the answer paths disagrees with the plane."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dipgenie_amd import capi

NEG_INF = -(2 ** 31) // 4


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("graph")
    ap.add_argument("--budget", type=int, default=None)
    ap.add_argument("--classes", default=None)
    ap.add_argument("--wide", type=int, choices=(0, 1, 2), default=0, help="option partner_wide: level state in device memory never / beyond the LDS limit / always")
    a = ap.parse_args()
    g = capi.DpGraphArrays.load(a.graph)
    b = g.R if a.budget is None else a.budget
    cls = np.fromfile(a.classes, np.int32) if a.classes else None
    widest = int(np.diff(g.level_off).max())
    print(f"{a.graph}: {g.n_levels} levels, {g.n_vertices} vertices, widest level {widest}, R = {g.R}, budget {b}")
    ctx = capi.Context(0)
    ctx.dp_set_option("partner_wide", a.wide)
    ctx.dp_load_graph(g)
    out = ctx.dp_run_budgets([b])[0]
    plane = int(ctx.dp_budget_values()[b])
    paths = ctx.dp_answer_paths(b)
    if plane == NEG_INF:
        print(f"no pair of paths fits budget {b}: nothing to call")
        return 0
    score = ctx.dp_score_paths(paths[None])[0]
    print(f"answer: value {plane}, s_het {out.s_het}, recombinations {int(score['r1'])} + {int(score['r2'])}")
    if (int(score["value"]), int(score["s_het"])) != (plane, out.s_het) or score["r1"] + score["r2"] > b:
        print(f"FAILED: dp_score_paths of the answer paths gives value {int(score['value'])}, s_het {int(score['s_het'])}, the plane holds {plane}, {out.s_het}")
        return 1
    t0 = time.perf_counter()
    levels, _ = ctx.dp_call_margins(b, cls)
    wall = time.perf_counter() - t0
    route, cells = ctx.dp_partner_route()
    ctx.close()
    print("hap\tlevels_with_alternative\tmargin0_levels\tmin_positive_margin")
    for h in range(2):
        inner = levels[h, 1:-1]
        has = inner["alt_vertex"] >= 0
        margin = (inner["value"].astype(np.int64) - inner["alt_value"])[has]
        positive = margin[margin > 0]
        print(f"{h + 1}\t{int(has.sum())}\t{int((margin == 0).sum())}\t{int(positive.min()) if positive.size else '-'}")
    print(f"2 haplotypes, {g.n_levels} levels each: one dp_call_margins call took {wall * 1e3:.1f} ms wall "
          f"(partner_wide {a.wide}: {cells} cells per level state, in {'device memory' if route == 2 else 'LDS'})")
    return 0


if __name__ == "__main__":
    sys.exit(main())

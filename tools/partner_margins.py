#!/usr/bin/env python3
"""Per-level margins of the best partner on a dumped graph, with dp_partner_marginals.

usage: partner_margins.py GRAPH.dpg [--starts N] [--seed S] [--p-w0 P] [--wide {0,1,2}]

Samples N start paths p as partner_ascent.py does (a weight-0 out-edge with probability P wherever one exists, so that the starts
fit the budget), takes each start's best partner within R - r(p) with dp_best_partners, and asks dp_partner_marginals for the same
queries in one call: per level the vertex the best partner passes through, what the best partner through another vertex is worth,
and so the margin of the call at that site.  Prints, per start, the value, the number of levels with margin 0 (the data cannot tell
two vertices apart there), the smallest positive margin, the number of levels without any alternative, and the wall time of the one
dp_partner_marginals call.  --wide w sets option partner_wide: 0 (default) the level state stays in LDS and a graph beyond 16,384 cells (widest level x
(budget + 1)) is refused, 1 such a call keeps it in device memory, 2 every call does (A/B timing); the route taken is printed.  Exit status 1 if a level's best_value differs from the partner's value, or if the marginal of a vertex
on the partner path differs from it."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dipgenie_amd import capi
from optimality_audit import NEG_INF, sample_paths


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("graph")
    ap.add_argument("--starts", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--p-w0", type=float, default=1.0)
    ap.add_argument("--wide", type=int, choices=(0, 1, 2), default=0, help="option partner_wide: level state in device memory never / beyond the LDS limit / always")
    a = ap.parse_args()
    g = capi.DpGraphArrays.load(a.graph)
    R = g.R
    ctx = capi.Context(0)
    ctx.dp_set_option("partner_wide", a.wide)
    ctx.dp_load_graph(g)
    print(f"{a.graph}: {g.n_levels} levels, {g.n_vertices} vertices, widest level {int(np.diff(g.level_off).max())}, R = {R}")
    rng = np.random.default_rng(a.seed)
    cur = sample_paths(g, rng, a.starts, a.p_w0)
    # r of the starts comes from a first call (r1); a start beyond R gets budget 0 there and is dropped
    rec0, _ = ctx.dp_best_partners(cur, np.zeros(len(cur), np.int32), want_paths=False)
    keep = rec0["r1"] <= R
    if not keep.any():
        raise SystemExit(f"none of the {a.starts} sampled starts has r <= {R}: raise --p-w0 or --starts")
    start_id = np.flatnonzero(keep)
    cur, budgets = cur[keep], (R - rec0["r1"][keep]).astype(np.int32)
    n = len(cur)
    rec, partner = ctx.dp_best_partners(cur, budgets)
    t0 = time.perf_counter()
    levels, values = ctx.dp_partner_marginals(cur, budgets, want_vertices=True)
    wall = time.perf_counter() - t0
    route, cells = ctx.dp_partner_route()
    print(f"partner_wide {a.wide}: {cells} cells per level state, in {'device memory' if route == 2 else 'LDS'}")
    ctx.close()
    n_bad = 0
    print("start\tbudget\tvalue\tmargin0_levels\tmin_positive_margin\tlevels_without_alternative")
    for i in range(n):
        value = int(rec["value"][i])
        off_level = np.flatnonzero(levels["best_value"][i] != value)
        if off_level.size:
            n_bad += 1
            print(f"start {start_id[i]}: best_value {int(levels['best_value'][i][off_level[0]])} at level {off_level[0]} differs from the partner's value {value}")
        if value == NEG_INF:
            print(f"{start_id[i]}\t{budgets[i]}\tunreachable\t-\t-\t-")
            continue
        on_path = values[i][partner[i]]
        off_path = np.flatnonzero(on_path != value)
        if off_path.size:
            n_bad += 1
            print(f"start {start_id[i]}: the marginal of partner vertex {int(partner[i][off_path[0]])} (level {off_path[0]}) is {int(on_path[off_path[0]])}, the partner's value {value}")
        has2 = levels["second_vertex"][i] >= 0
        margin = (levels["best_value"][i].astype(np.int64) - levels["second_value"][i])[has2]
        positive = margin[margin > 0]
        print(f"{start_id[i]}\t{budgets[i]}\t{value}\t{int((margin == 0).sum())}\t{int(positive.min()) if positive.size else '-'}\t{int((~has2).sum())}")
    print(f"{n} queries, {g.n_levels} levels each: one dp_partner_marginals call took {wall * 1e3:.1f} ms wall")
    if n_bad:
        print(f"FAILED: {n_bad} disagreements with dp_best_partners")
        return 1
    print("ok: every level's best_value and every vertex of the partner path hold the partner's value")
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Coordinate ascent on a dumped graph with dp_best_partners: fix one path, take its best partner, swap, repeat.

usage: partner_ascent.py GRAPH.dpg [--starts N] [--seed S] [--p-w0 P] [--wide {0,1,2}]

Runs dp_run_budgets(all budgets 0..R), samples N start paths p with r(p) <= R (a weight-0 out-edge with probability P wherever one
exists, so that the starts fit the budget), then repeats q <- partner(p, R - r(p)), p <- partner(q, R - r(q)), ... for all starts at
once, one dp_best_partners call per round, until no start's value rises any more.  Every round is exact, so the value of a start
never falls, and a pair with r1 + r2 recombinations never beats that plane of the sweep: either is exit status 1.  Prints, per
start, the rounds, the final value, r1, r2 and the gap to plane R.  --wide w sets option partner_wide: 0 (default) the level state
stays in LDS and a graph beyond 16,384 cells (widest level x (budget + 1)) is refused, 1 such a call keeps it in device memory, 2
every call does (A/B timing)."""
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
    ap.add_argument("--max-rounds", type=int, default=64)
    ap.add_argument("--wide", type=int, choices=(0, 1, 2), default=0, help="option partner_wide: level state in device memory never / beyond the LDS limit / always")
    a = ap.parse_args()
    g = capi.DpGraphArrays.load(a.graph)
    R = g.R
    ctx = capi.Context(0)
    ctx.dp_set_option("partner_wide", a.wide)
    ctx.dp_load_graph(g)
    ctx.dp_run_budgets(range(R + 1))
    planes = ctx.dp_budget_values().astype(np.int64)
    print(f"{a.graph}: {g.n_levels} levels, {g.n_vertices} vertices, R = {R}; plane R of the sweep: {'unreachable' if planes[R] == NEG_INF else planes[R]}")
    rng = np.random.default_rng(a.seed)
    cur = sample_paths(g, rng, a.starts, a.p_w0)
    # r of the starts comes from the first call (r1); a start beyond R gets budget 0 there and is dropped
    rec0, _ = ctx.dp_best_partners(cur, np.zeros(len(cur), np.int32), want_paths=False)
    keep = rec0["r1"] <= R
    if not keep.any():
        raise SystemExit(f"none of the {a.starts} sampled starts has r <= {R}: raise --p-w0 or --starts")
    start_id = np.flatnonzero(keep)
    cur, r_cur = cur[keep], rec0["r1"][keep].astype(np.int64)
    n = len(cur)
    value = np.full(n, NEG_INF, np.int64)
    final = np.zeros((n, 3), np.int64)                   # value, r1, r2 of the last round that answered
    rounds = np.zeros(n, np.int64)
    live = np.ones(n, bool)
    n_fell = n_over = 0
    t_calls = 0.0
    for rnd in range(a.max_rounds):
        idx = np.flatnonzero(live)
        if not idx.size:
            break
        t0 = time.perf_counter()
        rec, partner = ctx.dp_best_partners(cur[idx], (R - r_cur[idx]).astype(np.int32))
        t_calls += time.perf_counter() - t0
        for j, i in enumerate(idx):
            v = int(rec["value"][j])
            if v == NEG_INF:                             # no partner within the budget this start leaves
                live[i] = False
                continue
            rounds[i] += 1
            if v < value[i]:
                n_fell += 1
                print(f"start {start_id[i]} round {rounds[i]}: the value fell from {value[i]} to {v}")
            if v > planes[rec["r1"][j] + rec["r2"][j]]:
                n_over += 1
                print(f"start {start_id[i]} round {rounds[i]}: value {v} with r1 + r2 = {rec['r1'][j] + rec['r2'][j]} beats that plane ({planes[rec['r1'][j] + rec['r2'][j]]})")
            final[i] = (v, rec["r1"][j], rec["r2"][j])
            if v <= value[i]:
                live[i] = False                          # the value stopped rising
                continue
            value[i] = v
            cur[i], r_cur[i] = partner[j], rec["r2"][j]  # swap: the partner is the given path of the next round
    ctx.close()
    print("start\trounds\tvalue\tr1\tr2\tgap_to_plane_R")
    for i in range(n):
        if value[i] == NEG_INF:
            print(f"{start_id[i]}\t0\tunreachable\t{r_cur[i]}\t-\t-")
        else:
            print(f"{start_id[i]}\t{rounds[i]}\t{final[i, 0]}\t{final[i, 1]}\t{final[i, 2]}\t{planes[R] - final[i, 0]}")
    done = value != NEG_INF
    if done.any():
        print(f"best of {int(done.sum())} starts: {int(value[done].max())}, gap to plane {R}: {int(planes[R] - value[done].max())}; "
              f"{int(rounds.sum())} queries in {t_calls * 1e3:.1f} ms of dp_best_partners calls")
    if n_fell or n_over:
        print(f"FAILED: {n_fell} rounds lowered the value, {n_over} values beat their plane")
        return 1
    print("ok: no round lowered a value, no value beats its plane")
    return 0


if __name__ == "__main__":
    sys.exit(main())

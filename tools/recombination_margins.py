#!/usr/bin/env python3
"""Recombination margins of the run's own answer on a dumped graph, with dp_answer_paths and dp_recombination_margins, or of the
answers at several budgets with dp_recombination_margins_budgets.

usage: recombination_margins.py GRAPH.dpg [--budget b] [--state-bytes N] [--check N] [--seed S]

Runs the sweep (dp_run_budgets of the one budget; default: the graph's R), takes the answer as a pair of paths and asks
dp_recombination_margins for it: per transition the best pair of paths that spends 0, 1 or 2 crossovers there, and what the answer's
own two hops are worth.  --state-bytes N sets option joint_state_bytes, the bound of the forward states of one segment.  Prints the
wall time of the call and its statistics (transitions, edge and finish launches, segments, levels swept forward twice, peak bytes
reserved, launches in all) beside the wall time of dp_genotype_margins on the answer in the same process (each call once, the
recombination call first: what a first call costs is in its time), and the summary: the crossovers the answer spends, its breakpoints
(transitions where it spends one) with margin 0 -- the best pair that spends another number there is worth as much -- the smallest
positive breakpoint margin, and the transitions without a crossover where a pair that spends one is worth the run's value (co-optimal
elsewhere).  --check N recomputes N sampled reachable (transition, s) entries with dp_run_pinned: require-ordered pins on
(from1, from2) at l and (to1, to2) at l + 1.  Exit status 1 if a called value differs from the run's plane, the called crossovers do
not add up to dp_score_paths' r1 + r2, a margin is negative or a recomputed value disagrees.

usage: recombination_margins.py GRAPH.dpg --budgets all|a,b,c [--singles] [--state-bytes N]

Runs dp_run_budgets on the listed budgets (all: 0..R) and then ONE dp_recombination_margins_budgets call on the answers of the budgets
somebody fits, each at its own budget.  Prints the call's wall time and statistics (queries, distinct budgets, transitions, edge and
finish launches, segments, levels swept forward twice, peak bytes, launches) and one line per budget: the crossovers its answer spends,
its breakpoints with margin 0 and the smallest positive breakpoint margin.  Exit status 1 if a called value differs from the plane at
its budget.  --singles also runs one dp_recombination_margins call per budget in the same process, compares every record and
called_out word with the one call's, and prints both walls."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dipgenie_amd import capi

NEG_INF = -(2 ** 31) // 4


def breakpoints(values, s_called, value):
    """-> (has, margin, alt_s): per transition whether another s is reachable, called value minus the best other value[s], and that s
    (argmax: among equals the smaller)"""
    others = np.where(np.arange(3)[None, :] == s_called[:, None], NEG_INF, values)
    alt_s = others.argmax(axis=1)
    alt = others[np.arange(len(values)), alt_s]
    return alt != NEG_INF, value - alt, alt_s


def budgets_main(a, g):
    """--budgets: one dp_recombination_margins_budgets call on the answers of dp_run_budgets"""
    listed = list(range(g.R + 1)) if a.budgets == "all" else [int(x) for x in a.budgets.split(",")]
    widths = np.diff(g.level_off).astype(np.int64)
    print(f"{a.graph}: {g.n_levels} levels, {g.n_vertices} vertices, widest level {int(widths.max())}, R = {g.R}, budgets {listed}")
    ctx = capi.Context(0)
    ctx.dp_set_option("joint_state_bytes", a.state_bytes)
    ctx.dp_load_graph(g)
    ctx.dp_run_budgets(listed)
    planes = ctx.dp_budget_values().copy()
    fit = [b for b in listed if planes[b] != NEG_INF]
    if not fit:
        print("no pair of paths fits any listed budget: nothing to call")
        ctx.close()
        return 0
    called = np.stack([ctx.dp_answer_paths(b).copy() for b in fit])
    t0 = time.perf_counter()
    records, out, best = ctx.dp_recombination_margins_budgets(fit, called)
    wall = time.perf_counter() - t0
    st = ctx.dp_recombination_budget_stats()
    print(f"one dp_recombination_margins_budgets call took {wall:.3f} s wall: {st['queries']} queries, {st['distinct_budgets']} distinct budgets, {st['transitions']} transitions, "
          f"{st['edge_launches']} edge launches, {st['finish_launches']} finish launches, {st['segments']} segments (joint_state_bytes {ctx.dp_get_option('joint_state_bytes')}), "
          f"{st['levels_twice']} levels swept forward twice, peak {st['peak_bytes'] / 1e9:.3f} GB reserved, {st['launches']} launches")
    failed = False
    for q, b in enumerate(fit):
        s_called, value = out[q, :, 0].astype(np.int64), out[q, :, 1].astype(np.int64)
        has, margin, _ = breakpoints(records[q]["value"].astype(np.int64), s_called, value)
        brk = s_called > 0
        positive = margin[brk & has & (margin > 0)]
        print(f"  budget {b}: value {int(best[q])}, {int(s_called.sum())} crossovers at {int(brk.sum())} transitions, margin 0 on {int((brk & has & (margin == 0)).sum())}, "
              f"smallest positive breakpoint margin {int(positive.min()) if positive.size else '-'}")
        if best[q] != planes[b] or (value != planes[b]).any():
            print(f"FAILED: budget {b}: the run's plane holds {int(planes[b])}, best_value is {int(best[q])}, {int((value != planes[b]).sum())} transitions of the answer have another value")
            failed = True
    if a.singles:
        walls = []
        for q, b in enumerate(fit):
            t0 = time.perf_counter()
            r1, o1, v1 = ctx.dp_recombination_margins(b, called[q:q + 1])
            walls.append(time.perf_counter() - t0)
            if v1 != best[q] or r1.tobytes() != records[q].tobytes() or not np.array_equal(o1[0], out[q]):
                print(f"FAILED: budget {b}: the one-budget call answers otherwise")
                failed = True
        print(f"{len(fit)} dp_recombination_margins calls took {sum(walls):.3f} s wall together ({', '.join(f'{b}: {w:.3f}' for b, w in zip(fit, walls))}), "
              f"{ctx.dp_recombination_stats()['launches']} launches the last; the one call {wall:.3f} s: ratio {wall / sum(walls):.3f}")
    ctx.close()
    return 1 if failed else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("graph")
    ap.add_argument("--budget", type=int, default=None)
    ap.add_argument("--budgets", default=None, help="all, or budgets separated by commas: one dp_recombination_margins_budgets call")
    ap.add_argument("--singles", action="store_true", help="with --budgets: also one dp_recombination_margins call per budget, compared and timed")
    ap.add_argument("--state-bytes", type=int, default=0, help="option joint_state_bytes (<= 0: the default)")
    ap.add_argument("--check", type=int, default=0, help="(transition, s) entries recomputed with dp_run_pinned")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    g = capi.DpGraphArrays.load(a.graph)
    if a.budgets is not None:
        return budgets_main(a, g)
    b = g.R if a.budget is None else a.budget
    widths = np.diff(g.level_off).astype(np.int64)
    print(f"{a.graph}: {g.n_levels} levels, {g.n_vertices} vertices, widest level {int(widths.max())}, R = {g.R}, budget {b}, "
          f"forward states of all levels {4 * int((widths ** 2).sum()) * (b + 1) / 1e9:.3f} GB")
    ctx = capi.Context(0)
    ctx.dp_set_option("joint_state_bytes", a.state_bytes)
    ctx.dp_load_graph(g)
    ctx.dp_run_budgets([b])
    plane = int(ctx.dp_budget_values()[b])
    if plane == NEG_INF:
        print(f"no pair of paths fits budget {b}: nothing to call")
        ctx.close()
        return 0
    paths = ctx.dp_answer_paths(b)
    t0 = time.perf_counter()
    records, out, best = ctx.dp_recombination_margins(b, paths[None])
    wall = time.perf_counter() - t0
    st = ctx.dp_recombination_stats()
    t0 = time.perf_counter()
    ctx.dp_genotype_margins(paths, b)
    wall_gm = time.perf_counter() - t0
    gs = ctx.dp_genotype_stats()
    print(f"one dp_recombination_margins call took {wall:.3f} s wall: {st['transitions']} transitions, {st['edge_launches']} edge launches, {st['finish_launches']} finish launches, "
          f"{st['segments']} segments (joint_state_bytes {ctx.dp_get_option('joint_state_bytes')}), {st['levels_twice']} levels swept forward twice, peak {st['peak_bytes'] / 1e9:.3f} GB "
          f"reserved, {st['launches']} launches")
    print(f"one dp_genotype_margins call on the same answer took {wall_gm:.3f} s wall ({gs['n_segments']} segments, {gs['launches']} launches, peak {gs['peak_bytes'] / 1e9:.3f} GB): "
          f"ratio {wall / wall_gm:.3f}")
    s_called, value = out[0, :, 0].astype(np.int64), out[0, :, 1].astype(np.int64)
    vals = records["value"].astype(np.int64)
    has, margin, alt_s = breakpoints(vals, s_called, value)
    alt = value - margin
    brk = s_called > 0
    positive = margin[brk & has & (margin > 0)]
    score = ctx.dp_score_paths(paths[None])[0]
    print(f"value {best}; the answer spends {int(s_called.sum())} crossovers ({int(score['r1'])} + {int(score['r2'])}) at {int(brk.sum())} transitions: margin 0 on "
          f"{int((brk & has & (margin == 0)).sum())} of them, smallest positive breakpoint margin {int(positive.min()) if positive.size else '-'}; "
          f"co-optimal elsewhere: {int(((s_called == 0) & has & (alt == plane)).sum())} transitions without a crossover where a pair that spends one is worth the value; "
          f"reachable s = 1 on {int((vals[:, 1] != NEG_INF).sum())}, s = 2 on {int((vals[:, 2] != NEG_INF).sum())} transitions")
    for l in np.flatnonzero(brk).tolist():
        print(f"  breakpoint at level {l}: s_called {int(s_called[l])}, values {vals[l].tolist()}, best other s {int(alt_s[l]) if has[l] else '-'}, margin {int(margin[l]) if has[l] else '-'}")
    failed = False
    if best != plane or (value != plane).any() or (s_called < 0).any():
        print(f"FAILED: the run's plane holds {plane}, best_value is {best}, {int((value != plane).sum())} transitions of the answer have another value")
        failed = True
    if s_called.sum() != int(score["r1"]) + int(score["r2"]):
        print(f"FAILED: the called hops spend {int(s_called.sum())} crossovers, dp_score_paths counts {int(score['r1'])} + {int(score['r2'])}")
        failed = True
    if (margin[has] < 0).any() or (vals.max(axis=1) != plane).any():
        print(f"FAILED: {int((margin[has] < 0).sum())} negative margins, {int((vals.max(axis=1) != plane).sum())} transitions whose best value is not the plane")
        failed = True
    if a.check:
        rng = np.random.default_rng(a.seed)
        entries = np.argwhere(vals != NEG_INF)
        for l, s in entries[rng.choice(len(entries), min(a.check, len(entries)), replace=False)].tolist():
            r = records[l]
            cells = ((l, r["from1"][s], r["from2"][s]), (l + 1, r["to1"][s], r["to2"][s]))
            pins = [(lvl, int(i), int(j), capi.PIN_REQUIRE) for lvl, i, j in cells if 0 < lvl < g.n_levels - 1]      # the first and the last level hold one cell
            got = ctx.dp_run_pinned(pins, [b])[0].value
            if got != r["value"][s]:
                print(f"FAILED: level {l}, s = {s}: value is {int(r['value'][s])}, dp_run_pinned gives {got}")
                failed = True
        print(f"{min(a.check, len(entries))} entries recomputed with dp_run_pinned")
    ctx.close()
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())

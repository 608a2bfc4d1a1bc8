#!/usr/bin/env python3
"""Genotype margins of the run's own answer on a dumped graph, with dp_answer_paths and dp_genotype_margins.

usage: genotype_margins.py GRAPH.dpg [--budget b | --budgets all|a,b,c [--singles]] [--classes FILE.cls] [--state-bytes N]

Runs the sweep (dp_run_budgets of the one budget; default: the graph's R), takes the answer as a pair of paths and asks
dp_genotype_margins for it: per level the called cell's through-value and the best cell of another genotype with both haplotypes
free (FILE.cls: raw int32 per vertex, as bin/DipGenie --genotype-margins -D writes it; without it every vertex is its own class).
--state-bytes N sets option joint_state_bytes, the bound of the forward states of one segment.  Prints the wall time of the one call
and its statistics (segments, levels swept forward twice, peak bytes reserved, launches), the inner levels with margin 0 and the
smallest positive margin, and -- where dp_call_margins can hold the graph -- the levels where the joint margin is smaller than both
conditional margins.  Exit status 1 if a value differs from the run's plane, a margin is negative, or a joint margin exceeds a
conditional one.

--budgets all|a,b,c: the sweep answers every listed budget (dp_run_budgets), and ONE dp_genotype_margins_budgets call describes the
answers of all budgets that have one, each at its own budget.  Prints that call's wall time and statistics and one summary line per
budget; exit status 1 if a value differs from the run's plane at its budget or a margin is negative.  --singles also times one
dp_genotype_margins call per budget (the route without the call) and fails if a record differs."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dipgenie_amd import capi

NEG_INF = -(2 ** 31) // 4
BIG = 2 ** 40                                           # the margin of a level without an alternative


def summary(inner):
    """an inner-level record array [levels] -> (levels with another genotype, margins int64 with BIG where there is none)"""
    has = inner["alt_vertex1"] >= 0
    return has, np.where(has, inner["value"].astype(np.int64) - inner["alt_value"], BIG)


def run_budgets(ctx, g, budgets, cls, singles):
    ctx.dp_run_budgets(budgets)
    planes = ctx.dp_budget_values()
    fit = [b for b in budgets if planes[b] != NEG_INF]
    for b in budgets:
        if b not in fit:
            print(f"budget {b}: no pair of paths fits: nothing to call")
    if not fit:
        return 0
    called = np.stack([ctx.dp_answer_paths(b) for b in fit])
    t0 = time.perf_counter()
    levels, best = ctx.dp_genotype_margins_budgets(called, fit, cls)
    wall = time.perf_counter() - t0
    stats = ctx.dp_genotype_stats()
    print(f"one dp_genotype_margins_budgets call for {len(fit)} budgets (largest {max(fit)}) took {wall:.3f} s wall: {stats['n_segments']} segments "
          f"(joint_state_bytes {ctx.dp_get_option('joint_state_bytes')}), {stats['levels_twice']} levels swept forward twice, peak {stats['peak_bytes'] / 1e9:.3f} GB reserved, "
          f"{stats['launches']} launches")
    failed = False
    for q, b in enumerate(fit):
        has, joint = summary(levels[q, 1:-1])
        positive = joint[has & (joint > 0)]
        print(f"budget {b}: value {int(best[q])}; inner levels {joint.size}, with another genotype {int(has.sum())}, margin 0 on {int((joint == 0).sum())}, "
              f"smallest positive margin {int(positive.min()) if positive.size else '-'}")
        if best[q] != planes[b] or (levels["value"][q] != planes[b]).any():
            print(f"FAILED: budget {b}: the run's plane holds {int(planes[b])}, best_value is {int(best[q])}, {int((levels['value'][q] != planes[b]).sum())} levels have another value")
            failed = True
        if (joint < 0).any():
            print(f"FAILED: budget {b}: {int((joint < 0).sum())} levels have a negative margin")
            failed = True
    if singles:
        total, launches, peak = 0.0, 0, 0
        for q, b in enumerate(fit):
            t0 = time.perf_counter()
            one, V = ctx.dp_genotype_margins(called[q], b, cls)
            dt = time.perf_counter() - t0
            st = ctx.dp_genotype_stats()
            total, launches, peak = total + dt, launches + st["launches"], max(peak, st["peak_bytes"])
            print(f"budget {b}: one dp_genotype_margins call took {dt:.3f} s wall: {st['n_segments']} segments, peak {st['peak_bytes'] / 1e9:.3f} GB reserved, {st['launches']} launches")
            if V != best[q] or not np.array_equal(one[0], levels[q]):
                print(f"FAILED: budget {b}: the one-budget call answers differently")
                failed = True
        print(f"{len(fit)} one-budget calls took {total:.3f} s wall together ({launches} launches, largest peak {peak / 1e9:.3f} GB); the one call {wall:.3f} s")
    return 1 if failed else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("graph")
    ap.add_argument("--budget", type=int, default=None)
    ap.add_argument("--budgets", default=None, help="all, or budgets separated by commas: one dp_genotype_margins_budgets call for all of them")
    ap.add_argument("--singles", action="store_true", help="with --budgets: also one dp_genotype_margins call per budget, timed")
    ap.add_argument("--classes", default=None)
    ap.add_argument("--state-bytes", type=int, default=0, help="option joint_state_bytes (<= 0: the default)")
    a = ap.parse_args()
    g = capi.DpGraphArrays.load(a.graph)
    b = g.R if a.budget is None else a.budget
    cls = np.fromfile(a.classes, np.int32) if a.classes else None
    widths = np.diff(g.level_off).astype(np.int64)
    print(f"{a.graph}: {g.n_levels} levels, {g.n_vertices} vertices, widest level {int(widths.max())}, R = {g.R}, budget {b}, "
          f"forward states of all levels {4 * int((widths ** 2).sum()) * (b + 1) / 1e9:.3f} GB")
    ctx = capi.Context(0)
    ctx.dp_set_option("joint_state_bytes", a.state_bytes)
    ctx.dp_load_graph(g)
    if a.budgets is not None:
        budgets = list(range(g.R + 1)) if a.budgets == "all" else sorted({int(x) for x in a.budgets.split(",")})
        rc = run_budgets(ctx, g, budgets, cls, a.singles)
        ctx.close()
        return rc
    ctx.dp_run_budgets([b])
    plane = int(ctx.dp_budget_values()[b])
    paths = ctx.dp_answer_paths(b)
    if plane == NEG_INF:
        print(f"no pair of paths fits budget {b}: nothing to call")
        return 0
    t0 = time.perf_counter()
    levels, best = ctx.dp_genotype_margins(paths, b, cls)
    wall = time.perf_counter() - t0
    stats = ctx.dp_genotype_stats()
    print(f"one dp_genotype_margins call took {wall:.3f} s wall: {stats['n_segments']} segments (joint_state_bytes {ctx.dp_get_option('joint_state_bytes')}), "
          f"{stats['levels_twice']} levels swept forward twice, peak {stats['peak_bytes'] / 1e9:.3f} GB reserved, {stats['launches']} launches")
    inner = levels[0, 1:-1]
    has = inner["alt_vertex1"] >= 0
    joint = np.where(has, inner["value"].astype(np.int64) - inner["alt_value"], BIG)
    positive = joint[has & (joint > 0)]
    print(f"value {best}; inner levels {inner.size}, with another genotype {int(has.sum())}, margin 0 on {int((joint == 0).sum())}, "
          f"smallest positive margin {int(positive.min()) if positive.size else '-'}")
    failed = False
    if best != plane or (levels["value"] != plane).any():
        print(f"FAILED: the run's plane holds {plane}, best_value is {best}, {int((levels['value'] != plane).sum())} levels have another value")
        failed = True
    if (joint < 0).any():
        print(f"FAILED: {int((joint < 0).sum())} levels have a negative margin")
        failed = True
    try:
        cond, _ = ctx.dp_call_margins(b, cls)
    except capi.DgError as e:
        print(f"no conditional margins to compare with: {e}")
        cond = None
    ctx.close()
    if cond is not None:
        c = cond[:, 1:-1]
        cm = np.where(c["alt_vertex"] >= 0, c["value"].astype(np.int64) - c["alt_value"], BIG)
        print(f"levels where the joint margin is smaller than both conditional margins: {int((joint < cm.min(axis=0)).sum())}; equal to the smaller: {int((joint == cm.min(axis=0)).sum())}")
        if (joint[None, :] > cm).any():
            print(f"FAILED: the joint margin exceeds a conditional one on {int((joint[None, :] > cm).any(axis=0).sum())} levels")
            failed = True
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())

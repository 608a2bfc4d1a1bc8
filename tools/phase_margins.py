#!/usr/bin/env python3
"""Phase margins of the run's own answer on a dumped graph, with dp_answer_paths and dp_phase_margins.

usage: phase_margins.py GRAPH.dpg [--budget b] [--classes FILE.cls] [--state-bytes N] [--check N] [--seed S]
       phase_margins.py GRAPH.dpg --budgets all|a,b,c [--singles] [--classes FILE.cls] [--state-bytes N]

Runs the sweep (dp_run_budgets of the one budget; default: the graph's R), takes the answer as a pair of paths and asks
dp_phase_margins for it: per pair of neighbouring het levels the best pair of paths that keeps the answer's phase between them (cis)
against the best that switches it (trans) (FILE.cls: raw int32 per vertex, as bin/DipGenie --phase-margins -D writes it; without it
every vertex is its own class).  --state-bytes N sets option joint_state_bytes, the bound of the forward states of one segment.
Prints the wall time of the call and its statistics (het levels, records, backward launches on the seeded state, read-out launches,
segments, peak bytes reserved) beside the wall time of dp_genotype_margins on the same arguments (each call once, the phase call
first: what a first call costs is in its time), the records with a reachable trans,
those with margin 0 and the smallest positive margin.  --check N recomputes N sampled records with two dp_run_pinned each (require-
ordered pins on every cell of the class pair at both levels; a level with more than 4096 such cells is skipped).  Exit status 1 if a
cis_value differs from the run's plane, a margin is negative or a recomputed value disagrees.

--budgets: one sweep answers every listed budget (dp_run_budgets), and ONE dp_phase_margins_budgets call describes the phase of all
the answers that exist, each at its own budget.  Prints the call's wall time and statistics (queries, records, seed keys, slot-levels,
launches on the slots, read-outs, live slots, segments, peak bytes) and one line per budget: het levels, records, records with margin
0, smallest positive margin.  --singles also runs one dp_phase_margins per budget, compares every record and prints both walls.  Exit
status 1 if a cis_value differs from the plane at its budget or a record differs from the one-budget call's."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dipgenie_amd import capi

NEG_INF = -(2 ** 31) // 4
MAX_CELLS = 4096


def class_cells(g, ids, level, x0, x1):
    vs = np.arange(g.level_off[level], g.level_off[level + 1])
    return [(int(i), int(j)) for i in vs[ids[vs] == x0] for j in vs[ids[vs] == x1]]


def budgets_mode(a, g, cls):
    listed = list(range(g.R + 1)) if a.budgets == "all" else [int(x) for x in a.budgets.split(",")]
    ctx = capi.Context(0)
    ctx.dp_set_option("joint_state_bytes", a.state_bytes)
    ctx.dp_load_graph(g)
    ctx.dp_run_budgets(sorted(set(listed)))
    planes = ctx.dp_budget_values()
    fit = [b for b in listed if planes[b] != NEG_INF]
    if not fit:
        print("no pair of paths fits a listed budget: nothing to call")
        ctx.close()
        return 0
    called = np.stack([ctx.dp_answer_paths(b) for b in fit])
    t0 = time.perf_counter()
    records, best = ctx.dp_phase_margins_budgets(called, fit, cls)
    wall = time.perf_counter() - t0
    st = ctx.dp_phase_budget_stats()
    print(f"one dp_phase_margins_budgets call for budgets {fit} took {wall:.3f} s wall: {st['queries']} queries, {st['records']} records, {st['seed_keys']} seed keys, "
          f"{st['slot_levels']} slot-levels ({st['slot_levels'] / g.n_levels:.3f} per level), {st['backward_launches']} backward launches on the slots, {st['readout_launches']} read-out "
          f"launches, at most {st['max_live_slots']} live slots ({st['slots_allocated']} allocated), {st['segments']} segments (joint_state_bytes "
          f"{ctx.dp_get_option('joint_state_bytes')}), peak {st['peak_bytes'] / 1e9:.3f} GB reserved")
    failed = False
    for q, b in enumerate(fit):
        r = records[q]
        has = r["trans_vertex1"] >= 0
        margin = r["cis_value"].astype(np.int64) - r["trans_value"]
        positive = margin[has & (margin > 0)]
        het = int((ids_of(g, cls)[called[q, 0]] != ids_of(g, cls)[called[q, 1]]).sum())
        print(f"budget {b}: value {int(best[q])}, het levels {het}, records {len(r)}, margin 0 on {int((margin[has] == 0).sum())}, smallest positive margin "
              f"{int(positive.min()) if positive.size else '-'}")
        if best[q] != planes[b] or (r["cis_value"] != planes[b]).any():
            print(f"FAILED: budget {b}: the run's plane holds {int(planes[b])}, best_value is {int(best[q])}, {int((r['cis_value'] != planes[b]).sum())} records have another cis_value")
            failed = True
    if a.singles:
        t0 = time.perf_counter()
        ones = [ctx.dp_phase_margins(called[q], b, cls) for q, b in enumerate(fit)]
        wall_1 = time.perf_counter() - t0
        for q, b in enumerate(fit):
            if ones[q][1] != best[q] or not np.array_equal(ones[q][0], records[q]):
                print(f"FAILED: budget {b}: the one-budget call answers otherwise")
                failed = True
        print(f"{len(fit)} dp_phase_margins calls took {wall_1:.3f} s wall together: the one call takes {wall / wall_1:.3f} of that")
    ctx.close()
    return 1 if failed else 0


def ids_of(g, cls):
    return np.arange(g.n_vertices) if cls is None else cls


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("graph")
    ap.add_argument("--budget", type=int, default=None)
    ap.add_argument("--classes", default=None)
    ap.add_argument("--state-bytes", type=int, default=0, help="option joint_state_bytes (<= 0: the default)")
    ap.add_argument("--check", type=int, default=0, help="records recomputed with dp_run_pinned")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--budgets", default=None, help="all or a,b,c: one dp_phase_margins_budgets call for the answers at these budgets")
    ap.add_argument("--singles", action="store_true", help="with --budgets: also one dp_phase_margins call per budget, compared and timed")
    a = ap.parse_args()
    g = capi.DpGraphArrays.load(a.graph)
    if a.budgets is not None:
        return budgets_mode(a, g, np.fromfile(a.classes, np.int32) if a.classes else None)
    b = g.R if a.budget is None else a.budget
    cls = np.fromfile(a.classes, np.int32) if a.classes else None
    ids = np.arange(g.n_vertices) if cls is None else cls
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
    records, best = ctx.dp_phase_margins(paths, b, cls)
    wall = time.perf_counter() - t0
    st = ctx.dp_phase_stats()
    t0 = time.perf_counter()
    ctx.dp_genotype_margins(paths, b, cls)
    wall_gm = time.perf_counter() - t0
    gs = ctx.dp_genotype_stats()
    print(f"one dp_phase_margins call took {wall:.3f} s wall: {st['het_levels']} het levels, {st['records']} records, {st['seeded_launches']} backward launches on the seeded state, "
          f"{st['readout_launches']} read-outs, {st['segments']} segments (joint_state_bytes {ctx.dp_get_option('joint_state_bytes')}), peak {st['peak_bytes'] / 1e9:.3f} GB reserved")
    print(f"one dp_genotype_margins call on the same arguments took {wall_gm:.3f} s wall ({gs['n_segments']} segments, {gs['launches']} launches, peak {gs['peak_bytes'] / 1e9:.3f} GB): "
          f"ratio {wall / wall_gm:.3f}")
    has = records["trans_vertex1"] >= 0
    margin = records["cis_value"].astype(np.int64) - records["trans_value"]
    positive = margin[has & (margin > 0)]
    far = int((records["level_b"] - records["level_a"] > 1).sum())
    print(f"value {best}; records {len(records)} ({far} between levels that are not adjacent), with a reachable trans {int(has.sum())}, margin 0 on {int((margin[has] == 0).sum())}, "
          f"smallest positive margin {int(positive.min()) if positive.size else '-'}")
    failed = False
    if best != plane or (records["cis_value"] != plane).any():
        print(f"FAILED: the run's plane holds {plane}, best_value is {best}, {int((records['cis_value'] != plane).sum())} records have another cis_value")
        failed = True
    if (margin[has] < 0).any():
        print(f"FAILED: {int((margin[has] < 0).sum())} records have a negative margin")
        failed = True
    if a.check and len(records):
        rng = np.random.default_rng(a.seed)
        checked = skipped = 0
        for q in rng.choice(len(records), min(a.check, len(records)), replace=False).tolist():
            r = records[q]
            la, le = int(r["level_a"]), int(r["level_b"])
            xa, xe = (ids[paths[0, la]], ids[paths[1, la]]), (ids[paths[0, le]], ids[paths[1, le]])
            at_e = class_cells(g, ids, le, *xe)
            for which, x in (("cis", xa), ("trans", xa[::-1])):
                at_a = class_cells(g, ids, la, *x)
                if max(len(at_a), len(at_e)) > MAX_CELLS:
                    skipped += 1
                    continue
                pins = [(la, i, j, capi.PIN_REQUIRE) for i, j in at_a] + [(le, i, j, capi.PIN_REQUIRE) for i, j in at_e]
                value = ctx.dp_run_pinned(pins, [b])[0].value
                checked += 1
                if value != r[which + "_value"]:
                    print(f"FAILED: levels {la}, {le}: {which}_value is {int(r[which + '_value'])}, dp_run_pinned gives {value}")
                    failed = True
        print(f"{checked} values recomputed with dp_run_pinned, {skipped} skipped for more than {MAX_CELLS} cells of a class pair")
    ctx.close()
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())

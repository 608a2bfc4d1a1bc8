#!/usr/bin/env python3
"""The genotype table of a dumped graph, with dp_answer_paths and dp_genotype_table.

usage: genotype_table.py GRAPH.dpg [--budget b] [--classes FILE.cls] [--state-bytes N] [--table-bytes N]

Runs the sweep (dp_run_budgets of the one budget; default: the graph's R), takes the answer as a pair of paths and makes ONE
dp_genotype_table call with it as the called cells: per level every genotype that a pair of paths within the budget passes through,
with its best cell and value, and the margin records of dp_genotype_margins from the same pass (FILE.cls: raw int32 per vertex, as
bin/DipGenie --genotype-table -D writes it; without it every vertex is its own class).  --state-bytes N sets option
joint_state_bytes, --table-bytes N option genotype_table_bytes (the device staging of finished entries).  Prints the entries, the
levels with at least 2 genotypes, the levels with at least 2 genotypes at the run's value, the largest level, the call's statistics
and its wall time.  Exit status 1 if the largest entry of a level is not the run's plane, or a margin record is not what the table
implies: its value the entry of the called genotype where the called cell is that genotype's best, its alternative the largest entry
among the other genotypes, ties to the smallest vertex1, then the smallest vertex2."""
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
    ap.add_argument("--state-bytes", type=int, default=0, help="option joint_state_bytes (<= 0: the default)")
    ap.add_argument("--table-bytes", type=int, default=0, help="option genotype_table_bytes (<= 0: the default)")
    a = ap.parse_args()
    g = capi.DpGraphArrays.load(a.graph)
    b = g.R if a.budget is None else a.budget
    cls = np.fromfile(a.classes, np.int32) if a.classes else None
    L = g.n_levels
    widths = np.diff(g.level_off).astype(np.int64)
    print(f"{a.graph}: {L} levels, {g.n_vertices} vertices, widest level {int(widths.max())}, R = {g.R}, budget {b}")
    ctx = capi.Context(0)
    ctx.dp_set_option("joint_state_bytes", a.state_bytes)
    ctx.dp_set_option("genotype_table_bytes", a.table_bytes)
    ctx.dp_load_graph(g)
    ctx.dp_run_budgets([b])
    plane = int(ctx.dp_budget_values()[b])
    paths = ctx.dp_answer_paths(b)
    if plane == NEG_INF:
        print(f"no pair of paths fits budget {b}: the table is empty")
        return 0
    t0 = time.perf_counter()
    off, entries, best, levels = ctx.dp_genotype_table(b, cls, paths)
    wall = time.perf_counter() - t0
    stats = ctx.dp_genotype_stats()
    t1 = time.perf_counter()
    entries.copy()
    print(f"(inside that wall time the binding copies the {entries.nbytes / 1e6:.0f} MB of entries out of the library's buffer once: a copy of that size takes {time.perf_counter() - t1:.3f} s here)")
    table_bytes = ctx.dp_get_option("genotype_table_bytes")
    ctx.close()
    per_level = np.diff(off)
    value = entries["value"].astype(np.int64)
    level = np.repeat(np.arange(L), per_level)
    at_best = np.bincount(level[value == best], minlength=L)
    print(f"one dp_genotype_table call took {wall:.3f} s wall: {stats['n_segments']} segments, {stats['levels_twice']} levels swept forward twice, "
          f"peak {stats['peak_bytes'] / 1e9:.3f} GB reserved, {stats['launches']} launches, {stats['staging_copies']} staging copies (genotype_table_bytes {table_bytes})")
    print(f"value {best}; entries {len(entries)}, levels with at least 2 genotypes {int((per_level >= 2).sum())}, with at least 2 genotypes at the value "
          f"{int((at_best >= 2).sum())}, largest level {int(per_level.max())} genotypes (level {int(per_level.argmax())})")
    failed = False
    if best != plane or (per_level < 1).any() or (np.maximum.reduceat(value, off[:-1]) != plane).any():
        print(f"FAILED: the run's plane holds {plane}, best_value is {best}; levels without an entry or with another maximum exist")
        return 1
    # the margin records against the table
    rec = levels[0]
    ids = np.arange(g.n_vertices, dtype=np.int64) if cls is None else cls.astype(np.int64)
    c1, c2 = ids[paths[0]], ids[paths[1]]
    g1, g2 = np.minimum(c1, c2), np.maximum(c1, c2)
    own = (entries["class1"] == g1[level]) & (entries["class2"] == g2[level])
    v1, v2 = np.minimum(paths[0], paths[1]), np.maximum(paths[0], paths[1])
    rep = own & (entries["vertex1"] == v1[level]) & (entries["vertex2"] == v2[level])     # the called cell is its genotype's best
    if (value[rep] != rec["value"][level[rep]]).any():
        print(f"FAILED: {int((value[rep] != rec['value'][level[rep]]).sum())} records have another value than the entry of their genotype")
        failed = True
    other = np.flatnonzero(~own)
    order = other[np.lexsort((entries["vertex2"][other], entries["vertex1"][other], -value[other], level[other]))]
    first = np.ones(len(order), bool)
    first[1:] = level[order][1:] != level[order][:-1]
    alt = np.full((L, 3), (-1, -1, NEG_INF), np.int64)
    top = order[first]
    alt[level[top]] = np.stack([entries["vertex1"][top], entries["vertex2"][top], value[top]], axis=1)
    got = np.stack([rec["alt_vertex1"], rec["alt_vertex2"], rec["alt_value"]], axis=1)
    if (alt != got).any():
        print(f"FAILED: {int((alt != got).any(axis=1).sum())} records have another alternative than the table implies")
        failed = True
    print(f"margin records: {int(rep.sum())} of {L} called cells are the best of their genotype, {int((alt[:, 0] >= 0).sum())} levels have another genotype; "
          f"{'all agree with the table' if not failed else 'DISAGREEMENT'}")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())

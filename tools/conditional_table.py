#!/usr/bin/env python3
"""The genotype table of a dumped graph under pins, against the unpinned one, with dp_genotype_table and dp_genotype_table_pinned.

usage: conditional_table.py GRAPH.dpg --pins FILE [--budget b] [--classes FILE.cls] [--state-bytes N] [--check N] [--seed S]

FILE holds the rows of bin/DipGenie --pins: level <tab> vertex1 <tab> vertex2 [<tab> require|forbid|require-ordered|forbid-ordered],
'.' = any vertex, '#' starts a comment; an unordered row is its cell in both orders.  Makes one dp_genotype_table call and one
dp_genotype_table_pinned call at the budget (default: the graph's R; FILE.cls: raw int32 per vertex, as bin/DipGenie -D writes it
beside a table option; without it every vertex is its own class) and prints the levels whose best genotype under the pins differs from
the unpinned table's -- the level, both genotypes with their best cells and values, and what the pins cost there -- then the value of
both DPs, the pinned call's wall time, segments and mask launches.  The best genotype of a level is its entry with the largest value,
among equals the first in the table's order.  --state-bytes N sets option joint_state_bytes.

--check N: N sampled entries of the pinned table are recomputed by one dp_run_pinned each -- the pins of FILE and the entry's cell
required in every order the pins allow (the level's own require-pins go: a second require-pin widens a level) -- and the exit status is
1 if a run's value at the budget is not the entry's."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dipgenie_amd import capi

NEG_INF = -(2 ** 31) // 4
KINDS = {"require": (capi.PIN_REQUIRE, False), "forbid": (capi.PIN_FORBID, False), "require-ordered": (capi.PIN_REQUIRE, True), "forbid-ordered": (capi.PIN_FORBID, True)}


def read_pins(path):
    """the rows of FILE as pins (level, vertex1, vertex2, kind), -1 = any"""
    pins = []
    for n, line in enumerate(open(path), 1):
        line = line.split("#")[0].rstrip("\n").rstrip()
        if not line:
            continue
        f = line.split("\t")
        if len(f) not in (3, 4) or (len(f) == 4 and f[3] not in KINDS):
            raise SystemExit(f"{path}: line {n}: level <tab> vertex1 <tab> vertex2 [<tab> {'|'.join(KINDS)}]")
        level, v1, v2 = int(f[0]), *(-1 if x == "." else int(x) for x in f[1:3])
        kind, ordered = KINDS[f[3]] if len(f) == 4 else KINDS["require"]
        pins.append((level, v1, v2, kind))
        if not ordered and v1 != v2:
            pins.append((level, v2, v1, kind))
    return pins


def allowed(pins, level, i, j):
    """is the ordered cell (i, j) of the level allowed under the pins"""
    mine = [p for p in pins if p[0] == level]
    hit = lambda p: p[1] in (-1, i) and p[2] in (-1, j)
    req = [p for p in mine if p[3] == capi.PIN_REQUIRE]
    return (not req or any(hit(p) for p in req)) and not any(hit(p) for p in mine if p[3] == capi.PIN_FORBID)


def top_entries(off, entries, L):
    """per level the index of its entry with the largest value (the first among equals), -1 for a level without entries"""
    out = np.full(L, -1, np.int64)
    for l in range(L):
        if off[l + 1] > off[l]:
            out[l] = off[l] + int(np.argmax(entries["value"][off[l]:off[l + 1]]))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("graph")
    ap.add_argument("--pins", required=True)
    ap.add_argument("--budget", type=int, default=None)
    ap.add_argument("--classes", default=None)
    ap.add_argument("--state-bytes", type=int, default=0, help="option joint_state_bytes (<= 0: the default)")
    ap.add_argument("--check", type=int, default=0, help="entries of the pinned table to recompute with dp_run_pinned")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    g = capi.DpGraphArrays.load(a.graph)
    b = g.R if a.budget is None else a.budget
    cls = np.fromfile(a.classes, np.int32) if a.classes else None
    pins = read_pins(a.pins)
    L = g.n_levels
    print(f"{a.graph}: {L} levels, {g.n_vertices} vertices, widest level {int(np.diff(g.level_off).max())}, R = {g.R}, budget {b}; {len(pins)} pins on "
          f"{len({p[0] for p in pins})} levels")
    ctx = capi.Context(0)
    ctx.dp_set_option("joint_state_bytes", a.state_bytes)
    ctx.dp_load_graph(g)
    t0 = time.perf_counter()
    off_u, ent_u, best_u = ctx.dp_genotype_table(b, cls)
    t1 = time.perf_counter()
    off_p, ent_p, best_p = ctx.dp_genotype_table_pinned(pins, b, cls)
    t2 = time.perf_counter()
    stats, pin_stats = ctx.dp_genotype_stats(), ctx.dp_genotype_pin_stats()
    print(f"unpinned: value {best_u}, {len(ent_u)} entries, {t1 - t0:.3f} s wall; pinned: value {best_p}, {len(ent_p)} entries, {t2 - t1:.3f} s wall, {stats['n_segments']} segments, "
          f"{stats['launches']} launches of which {pin_stats['mask_launches']} masks")
    if best_p == NEG_INF:
        print(f"no pair of paths satisfies the pins within budget {b}: the pinned table is empty")
        ctx.close()
        return 0
    top_u, top_p = top_entries(off_u, ent_u, L), top_entries(off_p, ent_p, L)
    changed = 0
    for l in range(L):
        u, p = ent_u[top_u[l]], ent_p[top_p[l]]
        if (u["class1"], u["class2"]) != (p["class1"], p["class2"]):
            changed += 1
            print(f"level {l}: ({u['class1']}, {u['class2']}) at cell ({u['vertex1']}, {u['vertex2']}) worth {u['value']} -> ({p['class1']}, {p['class2']}) at cell "
                  f"({p['vertex1']}, {p['vertex2']}) worth {p['value']}: {int(u['value']) - int(p['value'])} less")
    print(f"{changed} of {L} levels change their best genotype under the pins; the optimum drops by {best_u - best_p}")
    failed = 0
    if a.check > 0 and len(ent_p):
        if b > g.R:
            raise SystemExit(f"--check: dp_run_pinned answers budgets up to R = {g.R}")
        rng = np.random.default_rng(a.seed)
        level = np.repeat(np.arange(L), np.diff(off_p))
        inner = np.flatnonzero((level >= 1) & (level <= L - 2))
        for x in rng.choice(inner, size=min(a.check, len(inner)), replace=False):
            l, v1, v2, want = int(level[x]), int(ent_p["vertex1"][x]), int(ent_p["vertex2"][x]), int(ent_p["value"][x])
            cell = [(l, i, j, capi.PIN_REQUIRE) for i, j in {(v1, v2), (v2, v1)} if allowed(pins, l, i, j)]
            got = ctx.dp_run_pinned([p for p in pins if not (p[0] == l and p[3] == capi.PIN_REQUIRE)] + cell, [b])[0].value
            if got != want:
                failed += 1
                print(f"FAILED: level {l} cell ({v1}, {v2}): the table says {want}, dp_run_pinned {got}")
        print(f"--check: {min(a.check, len(inner))} entries recomputed by dp_run_pinned, {failed} disagree")
    ctx.close()
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())

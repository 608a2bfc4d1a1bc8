#!/usr/bin/env python3
"""Pinned runs against the genotype table of a dumped graph: dp_run_pinned must realise what dp_genotype_table promises.

usage: pin_audit.py GRAPH.dpg [--budget b] [--entries N] [--seed S] [--classes FILE.cls] [--time n1,n2,...]

Takes the genotype table of the graph (every vertex its own class: one entry per reachable cell vertex1 <= vertex2 of a level, with
the best value of any pair of paths through it within the budget; default budget: the graph's R), samples N entries of the inner
levels and pins each entry's genotype in both orders (capi.genotype_pins).  FAILS (exit status 1) if a pinned value differs from the
entry's value, if the answer paths of the pinned run do not pass through the genotype, or if dp_score_paths of those paths disagrees
with the pinned value or spends more than the budget.  At every sampled level it also forbids the cell the unpinned answer passes,
in both orders: the value must then be the alt_value of dp_genotype_margins for that answer.

--classes FILE.cls (raw int32 per vertex, as bin/DipGenie -D writes it beside a margin or table option): the table of allele classes
instead -- one entry per genotype with its best cell, which is what gets pinned -- where the table of all cells would not fit (a
workload-sized graph); the forbidden calls are then checked against a dp_genotype_margins call of its own, without classes.

--time n1,n2,...: afterwards, the forward and total ms (dp_timing) of dp_run_pinned with n1, n2, ... pins -- forbid-pins of sampled
entries that are not the answer's cell, in both orders, so the answer stays -- beside the unpinned dp_run_budgets, each the median of
three warm passes, with the mask launches, the level pairs run as two launches and the batches issued plainly of the pinned run."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dipgenie_amd import capi

NEG_INF = -(2 ** 31) // 4


def timed(ctx, run, reps=3):
    run()                                                # warm: captures this run's batches
    rows = []
    for _ in range(reps):
        t0 = time.perf_counter()
        run()
        wall = 1e3 * (time.perf_counter() - t0)
        tm = ctx.dp_timing()
        rows.append((tm.forward_ms, tm.total_ms, wall))
    return np.median(np.array(rows), axis=0)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("graph")
    ap.add_argument("--budget", type=int, default=None)
    ap.add_argument("--entries", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--classes", default=None)
    ap.add_argument("--time", default="", help="pin counts to time, separated by commas")
    a = ap.parse_args()
    g = capi.DpGraphArrays.load(a.graph)
    b = g.R if a.budget is None else a.budget
    L = g.n_levels
    print(f"{a.graph}: {L} levels, {g.n_vertices} vertices, widest level {int(np.diff(g.level_off).max())}, R = {g.R}, budget {b}")
    ctx = capi.Context(0)
    ctx.dp_load_graph(g)
    free = ctx.dp_run_budgets([b])[0]
    if free.value == NEG_INF:
        print(f"no pair of paths fits budget {b}: nothing to pin")
        return 0
    answer = ctx.dp_answer_paths(b)
    cls = np.fromfile(a.classes, np.int32) if a.classes else None
    t0 = time.perf_counter()
    off, entries, best, margins = ctx.dp_genotype_table(b, cls, answer)
    alt_value = margins[0]["alt_value"] if cls is None else ctx.dp_genotype_margins(answer, b)[0][0]["alt_value"]
    print(f"genotype table{' and margins' if cls is not None else ''}: {time.perf_counter() - t0:.2f} s")
    assert best == free.value
    inner = np.arange(off[1], off[L - 1])
    rng = np.random.default_rng(a.seed)
    sample = np.sort(rng.choice(inner, size=min(a.entries, inner.size), replace=False))
    level_of = np.searchsorted(off, sample, side="right") - 1
    print(f"value {best}; {len(entries)} entries, {inner.size} on the inner levels, {sample.size} sampled")
    failed = 0
    for e, l in zip(sample, level_of):
        v1, v2, want = int(entries["vertex1"][e]), int(entries["vertex2"][e]), int(entries["value"][e])
        out = ctx.dp_run_pinned(capi.genotype_pins(l, v1, v2), [b])[0]
        paths = ctx.dp_answer_paths(b)
        s = ctx.dp_score_paths(paths[None])[0]
        ok = out.value == want and {int(paths[0][l]), int(paths[1][l])} == {v1, v2} and int(s["value"]) == out.value and int(s["r1"]) + int(s["r2"]) <= b
        if not ok:
            failed += 1
            print(f"FAILED: level {l} genotype ({v1}, {v2}): entry {want}, pinned run {out.value}, its paths pass ({int(paths[0][l])}, {int(paths[1][l])}) and score "
                  f"{int(s['value'])} with {int(s['r1'])} + {int(s['r2'])} recombinations")
    lowered = 0
    for l in sorted(set(level_of.tolist())):
        c1, c2 = int(answer[0][l]), int(answer[1][l])
        out = ctx.dp_run_pinned(capi.genotype_pins(l, c1, c2, capi.PIN_FORBID), [b])[0]
        want = int(alt_value[l])
        lowered += out.value < best
        if out.value != want:
            failed += 1
            print(f"FAILED: level {l}: the answer's cell ({c1}, {c2}) forbidden gives {out.value}, alt_value of dp_genotype_margins is {want}")
    print(f"{sample.size} pinned genotypes and {len(set(level_of.tolist()))} forbidden calls ({lowered} of them cost value): {'all agree' if not failed else str(failed) + ' DISAGREE'}")
    if a.time:
        pool = rng.permutation(inner)
        pins = []
        for e in pool:
            l = int(np.searchsorted(off, e, side="right") - 1)
            v1, v2 = int(entries["vertex1"][e]), int(entries["vertex2"][e])
            if {v1, v2} != {int(answer[0][l]), int(answer[1][l])}:
                pins += capi.genotype_pins(l, v1, v2, capi.PIN_FORBID)
            if len(pins) >= max(int(x) for x in a.time.split(",")):
                break
        fwd, tot, wall = timed(ctx, lambda: ctx.dp_run_budgets([b]))
        print(f"unpinned dp_run_budgets: forward {fwd:.3f} ms, total {tot:.3f} ms, wall {wall:.3f} ms")
        for n in (int(x) for x in a.time.split(",")):
            p = np.array(pins[:n], np.int32)
            fwd, tot, wall = timed(ctx, lambda: ctx.dp_run_pinned(p, [b]))
            st = ctx.dp_pin_stats()
            same = ctx.dp_run_pinned(p, [b])[0].value == best
            print(f"dp_run_pinned, {len(p)} pins on {st['levels']} levels: forward {fwd:.3f} ms, total {tot:.3f} ms, wall {wall:.3f} ms; {st['mask_launches']} mask launches, "
                  f"{st['pairs_as_singles']} pairs as singles, {st['batches_plain']} batches issued plainly; value {'unchanged' if same else 'CHANGED'}")
    ctx.close()
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Reference-independent audit of the sweep on a dumped graph: no sampled pair of source -> sink paths may score more than the
plane of the sink that its recombinations fit (plane r = the best pair with r1 + r2 <= r).

usage: optimality_audit.py GRAPH.dpg [--pairs N] [--seed S] [--p-w0 P]

Runs dp_run_budgets(all budgets 0..R), samples N random pairs -- half of them by a uniformly random out-edge per step, half taking a
weight-0 out-edge with probability P wherever one exists, so that the low planes get samples too -- scores them in ONE
dp_score_paths call and prints, per plane, the optimum, the best sampled score and the number of samples.  Exit status 1 if a sample
beats its plane."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dipgenie_amd import capi

NEG_INF = -(2 ** 31) // 4


def sample_paths(g, rng, n, p_w0):
    """[n, n_levels] vertex ids; p_w0 None: a uniformly random out-edge per step"""
    out_off, out_dst, out_w = g.out_off, g.out_dst.astype(np.int64), g.out_w
    w0_edge = np.flatnonzero(out_w == 0)
    src = np.repeat(np.arange(g.n_vertices), np.diff(out_off))
    w0_off = np.zeros(g.n_vertices + 1, np.int64)
    np.cumsum(np.bincount(src[w0_edge], minlength=g.n_vertices), out=w0_off[1:])
    paths = np.zeros((n, g.n_levels), np.int32)
    cur = np.zeros(n, np.int64)
    for l in range(1, g.n_levels):
        deg = out_off[cur + 1] - out_off[cur]
        if (deg <= 0).any():
            raise SystemExit(f"vertex {int(cur[np.argmin(deg)])} of level {l - 1} has no out-edge: cannot sample through it")
        e = out_off[cur] + np.minimum((rng.random(n) * deg).astype(np.int64), deg - 1)
        if p_w0 is not None and w0_edge.size:
            d0 = w0_off[cur + 1] - w0_off[cur]
            take = (d0 > 0) & (rng.random(n) < p_w0)
            pick = w0_off[cur] + np.minimum((rng.random(n) * d0).astype(np.int64), np.maximum(d0 - 1, 0))
            e = np.where(take, w0_edge[np.minimum(pick, w0_edge.size - 1)], e)
        cur = out_dst[e]
        paths[:, l] = cur
    return paths


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("graph")
    ap.add_argument("--pairs", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--p-w0", type=float, default=0.98)
    a = ap.parse_args()
    g = capi.DpGraphArrays.load(a.graph)
    rng = np.random.default_rng(a.seed)
    n_uni = a.pairs - a.pairs // 2
    halves = [(n_uni, None), (a.pairs // 2, a.p_w0)]
    paths = np.concatenate([np.stack([sample_paths(g, rng, n, p), sample_paths(g, rng, n, p)], axis=1) for n, p in halves if n > 0])
    ctx = capi.Context(0)
    ctx.dp_load_graph(g)
    ctx.dp_run_budgets(range(g.R + 1))
    values = ctx.dp_budget_values()
    t0 = time.perf_counter()
    sc = ctx.dp_score_paths(paths)
    dt = time.perf_counter() - t0
    ctx.close()
    r = sc["r1"].astype(np.int64) + sc["r2"]
    print(f"{a.graph}: {g.n_levels} levels, {g.n_vertices} vertices, R = {g.R}; {len(paths)} pairs scored in {dt * 1e3:.1f} ms "
          f"({len(paths) / max(dt, 1e-9):.0f} pairs/s, upload included)")
    print("plane\toptimum\tbest_sample\tsamples")
    n_bad = 0
    for b in range(g.R + 1):
        here = r == b
        best = int(sc["value"][here].max()) if here.any() else None
        opt = "unreachable" if values[b] == NEG_INF else int(values[b])
        flag = ""
        if best is not None and best > values[b]:        # (a sample on an unreachable plane beats NEG_INF)
            n_bad += int((sc["value"][here] > values[b]).sum())
            flag = "\t<-- a sample beats the optimum"
        print(f"{b}\t{opt}\t{'-' if best is None else best}\t{int(here.sum())}{flag}")
    print(f"beyond R: {int((r > g.R).sum())} samples (not comparable)")
    if n_bad:
        print(f"FAILED: {n_bad} sampled pairs score more than the plane they fit")
        return 1
    print("ok: no sample beats its plane")
    return 0


if __name__ == "__main__":
    sys.exit(main())

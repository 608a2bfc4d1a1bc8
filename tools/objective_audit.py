#!/usr/bin/env python3
"""The surrogate the sweep maximises beside the objective it stands for, on a dumped graph.  The sweep's value adds inter + symd per
transition, so a colour on many vertices of a path counts many times; the objective (dg_dp_objective_paths) counts every colour once:
hom colours both paths cover plus het colours exactly one covers.

usage: objective_audit.py GRAPH.dpg [--pairs N] [--seed S] [--budget b] [--p-w0 P]

Runs dp_run_budgets(all budgets 0..R) and prints surrogate and objective of the answer per budget (dp_answer_objectives); samples N
random pairs as optimality_audit.py does, scores each with dp_score_paths and dp_objective_paths, and prints the Spearman rank
correlation of the two measures and the best sampled objective among the pairs whose recombinations fit budget b (default R) beside
the answer's.  A sampled pair with a larger objective than the answer is a finding, not a failure: the DP does not maximise the
objective.  Exit status 1 only if dp_answer_objectives disagrees with dp_objective_paths(dp_answer_paths(b)) at some budget."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dipgenie_amd import capi
from optimality_audit import NEG_INF, sample_paths

FIELDS = ("hom_shared", "hom_single", "het_single", "het_both")


def ranks(x):
    """average ranks (ties share the mean of their positions)"""
    order = np.argsort(x, kind="stable")
    xs = x[order]
    first = np.flatnonzero(np.r_[True, xs[1:] != xs[:-1]])
    last = np.r_[first[1:], xs.size] - 1
    mean = (first + last) / 2.0
    out = np.empty(x.size, float)
    out[order] = np.repeat(mean, last - first + 1)
    return out


def spearman(a, b):
    ra, rb = ranks(np.asarray(a)), ranks(np.asarray(b))
    if ra.std() == 0 or rb.std() == 0:
        return float("nan")
    return float(np.corrcoef(ra, rb)[0, 1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("graph")
    ap.add_argument("--pairs", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--budget", type=int, default=None)
    ap.add_argument("--p-w0", type=float, default=0.98)
    a = ap.parse_args()
    t_start = time.perf_counter()
    g = capi.DpGraphArrays.load(a.graph)
    budget = g.R if a.budget is None else a.budget
    if not 0 <= budget <= g.R:
        raise SystemExit(f"--budget {budget} is outside 0..R = {g.R}")
    rng = np.random.default_rng(a.seed)
    halves = [(a.pairs - a.pairs // 2, None), (a.pairs // 2, a.p_w0)]
    paths = np.concatenate([np.stack([sample_paths(g, rng, n, p), sample_paths(g, rng, n, p)], axis=1) for n, p in halves if n > 0])
    ctx = capi.Context(0)
    ctx.dp_load_graph(g)
    budgets = list(range(g.R + 1))
    ctx.dp_run_budgets(budgets)
    values = ctx.dp_budget_values()
    t0 = time.perf_counter()
    answers = ctx.dp_answer_objectives(budgets)
    t_first = time.perf_counter() - t0                   # builds the colour dictionary
    n_bad = 0
    print(f"{a.graph}: {g.n_levels} levels, {g.n_vertices} vertices, R = {g.R}")
    print("r\tdp_value\tobjective\thom_shared\thom_single\thet_single\thet_both")
    for b in budgets:
        rec = answers[b]
        if values[b] == NEG_INF:
            print(f"{b}\t.\t.\t.\t.\t.\t.")
            ok = all(rec[f] == -1 for f in FIELDS)
        else:
            print(f"{b}\t{int(values[b])}\t{int(rec['hom_shared']) + int(rec['het_single'])}\t" + "\t".join(str(int(rec[f])) for f in FIELDS))
            ok = ctx.dp_objective_paths(ctx.dp_answer_paths(b)[None])[0] == rec
        if not ok:
            n_bad += 1
            print(f"FAILED: budget {b}: dp_answer_objectives gives {rec}, dp_objective_paths of dp_answer_paths does not")
    t0 = time.perf_counter()
    sc = ctx.dp_score_paths(paths)
    t_score = time.perf_counter() - t0
    t0 = time.perf_counter()
    ob = ctx.dp_objective_paths(paths)
    t_obj = time.perf_counter() - t0
    ctx.close()
    objective = ob["hom_shared"].astype(np.int64) + ob["het_single"]
    r = sc["r1"].astype(np.int64) + sc["r2"]
    print(f"{len(paths)} sampled pairs: dp_score_paths {t_score * 1e3:.1f} ms, dp_objective_paths {t_obj * 1e3:.1f} ms (uploads included); "
          f"dp_answer_objectives of {len(budgets)} budgets, dictionary included, {t_first * 1e3:.1f} ms")
    print(f"rank correlation (Spearman) of surrogate and objective over the samples: {spearman(sc['value'], objective):.4f}")
    fit = r <= budget
    if values[budget] == NEG_INF:
        print(f"budget {budget} is unreachable: nothing to compare")
    elif fit.any():
        best = int(np.argmax(np.where(fit, objective, -1)))
        mine = int(answers[budget]["hom_shared"]) + int(answers[budget]["het_single"])
        print(f"budget {budget}: the answer's objective {mine} (surrogate {int(values[budget])}); best sampled objective among the {int(fit.sum())} pairs "
              f"that fit {int(objective[best])} (surrogate {int(sc['value'][best])}, r1 + r2 = {int(r[best])})")
        if objective[best] > mine:
            print(f"finding: a sampled pair beats the answer's objective by {int(objective[best]) - mine} colours (the DP maximises the surrogate, not the objective)")
    else:
        print(f"budget {budget}: no sampled pair fits (raise --p-w0 or --pairs)")
    print(f"wall time {time.perf_counter() - t_start:.2f} s")
    if n_bad:
        return 1
    print("ok: dp_answer_objectives agrees with dp_objective_paths of the answer paths at every budget")
    return 0


if __name__ == "__main__":
    sys.exit(main())

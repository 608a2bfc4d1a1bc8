"""The graphs of tests/test_gpu_sweep_variant_parity.py -- test infrastructure.  Two families of six- to eight-level graphs, the
smallest on which every instantiated sweep kernel variant (dg_dp_sweep.hip: SWEEP_RCS) can go wrong, each at five budgets:
R + 1 = 8, 19, 33 are the three all-planes chunks, so every partial chunk below them is a candidate; R + 1 = 10 and 21 are smaller
than the all-planes chunk that sweeps them (19 and 33).  tests/test_sweep_variant_graphs.py checks on the CPU, from the arrays and
the oracle alone, that the committed seeds give what the GPU test relies on.

lean:    inner levels of 20..24 vertices with 10..17 rows of more than 8 in-edges (more heavy rows than ride in the kernel
         arguments), in-degrees 9, 10, 11 among them (uneven cooperative quarters, step tails at every unroll depth); the first
         level has rows of at most two in-edges and dead columns; the sink has in-degree > 200: a giant column, the general
         variant at k2 = 1.
general: 1, 100, 12, 100, 12, 1 vertices.  Every row of the 12-wide levels has 64..107 in-edges (two 64-edge trips, giant columns
         over several slot blocks; seed 13001 has one vertex of exactly 64, the largest column that is not giant); the 100-wide
         levels have in-degrees 0..6: the lean variant with rows of at most two in-edges, rows of more, and dead columns.
         With these widths no vertex can have 9, 10 or 11 in-edges (about 83 into a 12-wide level, about 1.2 into a 100-wide
         one), which the family must have as well, so it has a sixth graph with a 12-wide level behind the first 12-wide one
         (1, 100, 12, 12, 100, 12, 1): in-degrees 5..13 there, every one of 9, 10, 11 among them.
The arrays do not depend on R, so the oracle's answer at budget r serves every graph of the same seed with R >= r."""
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import graphgen
import oracle_py as orc

LEAN = dict(min_width=20, max_width=24, n_levels=8, extra_edges=8.0, p_w1=0.5, p_colour=0.6)
GENERAL = dict(widths=[1, 100, 12, 100, 12, 1], extra_edges=9.0, p_w1=0.5, p_colour=0.5, dup_edges=False)
GENERAL_MID = dict(GENERAL, widths=[1, 100, 12, 12, 100, 12, 1])
# case id -> (family, generator arguments, seed, R): one seed for the three all-planes budgets, another for the two budgets below an all-planes chunk
GRAPHS = {
    "lean-R7": ("lean", LEAN, 12000, 7), "lean-R18": ("lean", LEAN, 12000, 18), "lean-R32": ("lean", LEAN, 12000, 32),
    "lean-R9": ("lean", LEAN, 12001, 9), "lean-R20": ("lean", LEAN, 12001, 20),
    "general-R7": ("general", GENERAL, 13002, 7), "general-R18": ("general", GENERAL, 13002, 18), "general-R32": ("general", GENERAL, 13002, 32),
    "general-R9": ("general", GENERAL, 13001, 9), "general-R20": ("general", GENERAL, 13001, 20),
    "general-mid12-R7": ("general", GENERAL_MID, 13004, 7),
}
FAMILIES = ("lean", "general")
_ORACLE = {}                                                # (seed, r) -> the oracle's answer with digests, and its wall time


def family(case):
    return GRAPHS[case][0]


def graph(case, R=None):
    _, kw, seed, R_case = GRAPHS[case]
    return graphgen.random_levelized(seed, R=R_case if R is None else R, **kw)


def _solve(case, r):
    g = graph(case, r)
    t0 = time.perf_counter()
    ref = orc.dp_solve(g, want_digest=True)
    ref["seconds"] = time.perf_counter() - t0
    return ref


def oracle_per_budget(case):
    """the oracle on the case's arrays with g.R = r for r = 0..R (as tests/test_gpu_budgets.py does): a list of orc.dp_solve's
    dictionaries with digests, plus "seconds".  Each (seed, r) is solved once per process, four at a time (the oracle is a pure
    function; ctypes releases the interpreter lock); treat the answers as read-only."""
    seed, R = GRAPHS[case][2:]
    todo = [r for r in range(R + 1) if (seed, r) not in _ORACLE]
    with ThreadPoolExecutor(4) as pool:
        for r, ref in zip(todo, pool.map(lambda r: _solve(case, r), todo)):
            _ORACLE[(seed, r)] = ref
    return [_ORACLE[(seed, r)] for r in range(R + 1)]


def oracle(case):
    """orc.dp_solve(graph(case), want_digest=True), from the same store"""
    return oracle_per_budget(case)[-1]


def in_degrees(g):
    """per destination level 1..n_levels-1: the in-degree of each of its vertices (parallel edges count, as in the sweep's tables)"""
    deg = np.bincount(g.out_dst, minlength=g.n_vertices)
    return [deg[g.level_off[l]:g.level_off[l + 1]] for l in range(1, g.n_levels)]


def recombinations(ref):
    """weight-1 edges on the oracle's two paths: its edge lists hold those and, last, the edge into the sink"""
    return len(ref["p1"]) - 1 + len(ref["p2"]) - 1

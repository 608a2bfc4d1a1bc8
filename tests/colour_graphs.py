"""The graphs of tests/test_gpu_colour_lists.py -- test infrastructure.  Topologies that the GPU suite already runs, with colour
lists that the random generator's defaults never produce (graphgen.recolour): hundreds to thousands of ids per list, ids over
the whole int32 range, score deltas beyond 8 and beyond 15 bits.  tests/test_colour_graphs.py checks on the CPU, from the arrays
and the oracle alone, that every case reaches what its name claims.

Sizes are set by the oracle, which merges the four lists of every pair of edges anew (about 20 us per pair at these lengths):
  * the general topology is narrower than sweep_variant_graphs.GENERAL (30 and 4 vertices instead of 100 and 12; the rows of the
    narrow levels keep their 65..255 in-edges, so those levels still take the general kernel variants): 1.8e5 edge pairs, not 2e6;
  * lean and general run at R = 3: the all-planes chunk is 8 as at R = 7, so the same kernel variants are candidates, and the
    sink's value per budget costs four oracle runs;
  * disjoint_big, whose merges run over ~40,000 ids, takes a shorter graph of each kind (TOPOLOGIES_BIG).
The oracle answers of one topology are computed together, eight at a time, the first time one of them is asked for."""
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import graphgen
import oracle_py as orc
import sweep_variant_graphs as sv

GENERAL_NARROW = dict(sv.GENERAL, widths=[1, 30, 4, 30, 4, 1])
# name -> (seed, generator arguments)
TOPOLOGIES = {
    "w30": (9701, dict(max_width=30, n_levels=40, R=6)),
    "w65": (9718, dict(min_width=63, max_width=66, n_levels=12, R=9, p_w1=0.4)),
    "lean": (12000, dict(sv.LEAN, R=3)),
    "general": (13002, dict(GENERAL_NARROW, R=3)),
    "small": (7115, dict(n_levels=10, max_width=4, R=3, extra_edges=0.5, p_w1=0.25)),      # enumerable: test_gpu_score_paths.ENUMERABLE[0]
}
TOPOLOGIES_BIG = {
    "w30": (9701, dict(max_width=30, n_levels=12, R=6)),
    "w65": (9718, dict(min_width=63, max_width=66, n_levels=4, R=9, p_w1=0.4, extra_edges=0.3)),
    "lean": (12000, dict(sv.LEAN, R=3, n_levels=5, extra_edges=4.0)),
    "general": (13002, dict(sv.GENERAL, R=3, widths=[1, 36, 2, 36, 1], extra_edges=3.0)),
    "small": TOPOLOGIES["small"],
}
SWEEP_TOPOLOGIES = ("w30", "w65", "lean", "general")     # every colour case runs on these; "small" serves the path scoring calls
VARIANT_TOPOLOGIES = ("lean", "general")
POOL = 3000
# name -> recolour arguments; BANDS: where the case's largest score delta over all edge pairs must lie
CASES = {
    "long": dict(p_empty=0.15, p_short=0.15, long_range=(60, 350), pool=POOL),
    "mixed": dict(p_empty=0.7, p_short=0.2, long_range=(200, 2000), pool=4000),
    "hom_only": dict(p_empty=0.4, p_short=0.2, long_range=(100, 400), pool=500, hom_only=True),
    "het_only": dict(p_empty=0.4, p_short=0.2, long_range=(60, 350), pool=POOL, het_only=True),
    "extreme_ids": dict(p_empty=0.3, p_short=0.3, long_range=(60, 150), pool=200, id_map=graphgen.spread_ids(200)),
    "identical": dict(p_empty=0.0, p_short=0.0, long_range=(300, 300), pool=POOL, shared=True),
    "disjoint_big": None,                                # graphgen.recolour_disjoint_big on TOPOLOGIES_BIG
}
BANDS = {"long": (256, 32767), "mixed": (256, 32767), "hom_only": (256, 32767), "het_only": (256, 32767), "extreme_ids": (256, 32767),
         "identical": (300, 300), "disjoint_big": (32768, 65535)}
ALL_SETTINGS = ("long", "mixed")                         # the cases that run under every option setting
PATH_CASES = ("long", "disjoint_big")                    # the cases of the variant loop and of the path scoring calls
_GRAPH, _ORACLE = {}, {}


def topology(topo, big=False):
    seed, kw = (TOPOLOGIES_BIG if big else TOPOLOGIES)[topo]
    return graphgen.random_levelized(seed, **kw)


def graph(topo, case):
    """the recoloured graph, made once per process; treat it as read-only"""
    if (topo, case) not in _GRAPH:
        seed = 5000 + 100 * list(TOPOLOGIES).index(topo) + list(CASES).index(case)
        if case == "disjoint_big":
            g = graphgen.recolour_disjoint_big(topology(topo, big=True), seed)
        else:
            g = graphgen.recolour(topology(topo), seed, hom_high=(case == "extreme_ids" and topo in ("w65", "general")), **CASES[case])
        _GRAPH[topo, case] = g
    return _GRAPH[topo, case]


def lists(g):
    """(hom, het): per vertex its id array"""
    return tuple([col[off[v]:off[v + 1]] for v in range(g.n_vertices)] for off, col in ((g.hom_off, g.hom_col), (g.het_off, g.het_col)))


def with_budget(g, R):
    """g's arrays with another R"""
    return graphgen._with_colours(g, *lists(g), R=R)


def _solve(key):
    topo, case, R = key
    g = graph(topo, case)
    t0 = time.perf_counter()
    ref = orc.dp_solve(g if R == g.R else with_budget(g, R), want_digest=True)
    ref["seconds"] = time.perf_counter() - t0
    return ref


def _wanted(topo):
    """the oracle runs that the tests ask for on one topology: every case at the graph's R, the path cases at every smaller budget too where
    the sink's value per plane is compared"""
    cases = PATH_CASES if topo == "small" else list(CASES)
    keys = [(topo, case, graph(topo, case).R) for case in cases]
    if topo in VARIANT_TOPOLOGIES or topo == "small":
        keys += [(topo, case, r) for case in PATH_CASES for r in range(graph(topo, case).R)]
    return keys


def oracle(topo, case, R=None):
    """orc.dp_solve with digests (plus "seconds", the run's wall time) of graph(topo, case), at the graph's R or another; solved once
    per process (the oracle is a pure function; ctypes releases the interpreter lock); treat the answers as read-only"""
    key = (topo, case, graph(topo, case).R if R is None else R)
    if key not in _ORACLE:
        todo = [k for k in dict.fromkeys(_wanted(topo) + [key]) if k not in _ORACLE]
        with ThreadPoolExecutor(8) as pool:
            for k, ref in zip(todo, pool.map(_solve, todo)):
                _ORACLE[k] = ref
    return _ORACLE[key]


def planes(topo, case):
    """the oracle's sink value per budget 0..R"""
    return [oracle(topo, case, r)["value"] for r in range(graph(topo, case).R + 1)]


def largest_delta(g):
    """(the largest score delta over all edge pairs of all transitions, its (level, e, f), edge pairs per class [no edge coloured, one, both])"""
    top, where, classes = -1, None, np.zeros(3, np.int64)
    for l in range(1, g.n_levels):
        delta, _, coloured = graphgen.transition_deltas(g, l)
        if int(delta.max()) > top:
            e, f = np.unravel_index(int(np.argmax(delta)), delta.shape)
            top, where = int(delta.max()), (l, int(e), int(f))
        n = int(coloured.sum())
        classes += ((coloured.size - n) ** 2, 2 * n * (coloured.size - n), n * n)
    return top, where, classes

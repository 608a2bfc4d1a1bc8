"""CPU: tests/paths_model.py (the score of a pair of paths, written from its definition) against what already exists.  On graphs
small enough to enumerate, for every budget b = 0..R the maximum of the model's value over ALL ordered pairs of source -> sink
paths with r1 + r2 <= b must be the oracle's value for R = b -- and there is no such pair exactly where the oracle answers
NEG_INF.  This is the claim every reported result rests on, and it validates the yardstick of tests/test_gpu_score_paths.py."""
import copy
import os

import numpy as np
import pytest

import graphgen
import oracle_py as orc
from dipgenie_amd import capi
from paths_model import NEG_INF, PathModel, strip_colours

HERE = os.path.dirname(os.path.abspath(__file__))
# ordered pairs enumerated per graph, so that the whole file runs in seconds.  toy1 has 391 paths = 152,881 ordered pairs, the
# largest here; it is enumerated in full, not sampled (the model evaluates one of (p, q) and (q, p): they score alike).
MAX_PAIRS = 160_000

# 6-10 levels, width <= 4, R = 3; few extra edges keep the path count enumerable, and they still give fan-in
SMALL = {
    name: (seed, dict(n_levels=n_levels, max_width=4, R=3, extra_edges=extra, p_w1=p_w1, p_colour=p_colour))
    for name, seed, n_levels, extra, p_w1, p_colour in [
        ("a", 7100, 6, 1.0, 0.3, 0.4), ("b", 7101, 9, 0.6, 0.4, 0.2), ("c", 7111, 10, 0.5, 0.25, 0.3), ("d", 7115, 10, 0.5, 0.25, 0.3),
        ("e", 7129, 10, 0.5, 0.25, 0.3), ("f", 7102, 8, 0.7, 0.2, 0.3), ("g", 7129, 6, 1.0, 0.3, 0.4), ("h", 7126, 9, 0.6, 0.4, 0.2),
    ]
}


COLOURLESS = {"c": [3, 4], "e": [5], "h": [2, 3, 7]}      # levels whose colour lists are emptied


def small_graph(name):
    seed, kw = SMALL[name]
    g = graphgen.random_levelized(seed, **kw)
    return strip_colours(g, COLOURLESS[name]) if name in COLOURLESS else g


def oracle_values(g, R):
    out = []
    for b in range(R + 1):
        gb = copy.copy(g)
        gb.R = b
        out.append(orc.dp_solve(gb)["value"])
    return out


def check_graph(g, R):
    m = PathModel(g)
    n_paths = m.count_paths()
    assert n_paths ** 2 <= MAX_PAIRS, f"{n_paths} paths: too many pairs to enumerate"
    paths = m.all_paths()
    assert len(paths) == n_paths and len(set(paths)) == n_paths and all(m.check_path(p) is None for p in paths)
    best, n_pairs = m.best_per_budget(R, paths)
    want = oracle_values(g, R)
    assert len(best) == len(want) == R + 1
    for b in range(R + 1):                              # every plane, the unreachable ones included
        assert (best[b] is None) == (want[b] == NEG_INF), (b, best, want)
        assert best[b] is None or best[b] == want[b], (b, best, want)
    return m, best, n_pairs


@pytest.mark.parametrize("name", list(SMALL))
def test_enumerated_maximum_is_the_oracle_value_on_every_plane(name):
    g = small_graph(name)
    m, best, n_pairs = check_graph(g, g.R)
    print(f"graph {name}: {g.n_levels} levels, {g.n_vertices} vertices, {n_pairs} pairs, best per budget {best}")


def test_the_generated_graphs_cover_what_they_should():
    """against a vacuous file: colourless levels, fan-in, unreachable planes and planes that differ all occur"""
    colourless = fan_in = unreachable = rising = 0
    for name in SMALL:
        g = small_graph(name)
        m = PathModel(g)
        has_col = [any(m.hom[v] or m.het[v] for v in range(g.level_off[l], g.level_off[l + 1])) for l in range(g.n_levels)]
        colourless += sum(1 for l in range(g.n_levels) if not has_col[l])
        indeg = np.zeros(g.n_vertices, int)
        for v in range(g.n_vertices):
            for t in m.succ[v]:
                indeg[t] += 1
        fan_in += int((indeg > 1).sum())
        want = oracle_values(g, g.R)
        unreachable += sum(1 for w in want if w == NEG_INF)
        rising += len({w for w in want if w != NEG_INF}) >= 2
    print(f"colourless levels {colourless}, fan-in vertices {fan_in}, unreachable planes {unreachable}, graphs whose planes differ {rising}")
    assert colourless >= 3 and fan_in >= 20 and unreachable >= 2 and rising >= 3


@pytest.mark.parametrize("name", ["toy1_k5w3_R2.dpg", "toy2_R2.dpg"])
def test_committed_toys(name):
    g = capi.DpGraphArrays.load(os.path.join(HERE, "golden", name))
    m, best, n_pairs = check_graph(g, g.R)
    print(f"{name}: {g.n_levels} levels, {g.n_vertices} vertices, {n_pairs} pairs, best per budget {best}")
    assert best[g.R] == {"toy2_R2.dpg": 8, "toy1_k5w3_R2.dpg": 14}[name]


def test_model_rejects_what_is_not_a_path():
    g = small_graph("d")
    m = PathModel(g)
    p = list(m.all_paths()[0])
    assert m.check_path(p) is None
    bad = list(p)
    bad[3] = int(g.level_off[5])                        # a vertex of another level
    assert m.check_path(bad) == (3, "level")
    # a hop without an edge: some vertex of level l that p[l-1] has no edge to
    for l in range(1, g.n_levels):
        others = [v for v in range(g.level_off[l], g.level_off[l + 1]) if v not in m.succ[p[l - 1]]]
        if others:
            bad = list(p)
            bad[l] = others[0]
            assert m.check_path(bad)[0] in (l, l + 1) and m.check_path(bad)[1] == "edge"
            break
    else:
        pytest.fail("no missing edge to test with")


def test_samplers_return_paths_with_their_recombinations():
    g = graphgen.random_levelized(7201, n_levels=30, max_width=8, R=6, p_w1=0.3)
    m = PathModel(g)
    rng = np.random.default_rng(5)
    for p_w0 in (None, 0.95):
        paths, rec = m.sample_paths(rng, 200, p_w0)
        for p, r in zip(paths, rec):
            assert m.check_path(p) is None and m.recombinations(p) == r
    uni = m.sample_paths(np.random.default_rng(6), 2000)[1].mean()
    low = m.sample_paths(np.random.default_rng(6), 2000, 0.95)[1].mean()
    assert low < uni / 2, (low, uni)                    # the biased mode reaches the low planes

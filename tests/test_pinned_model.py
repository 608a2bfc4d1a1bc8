"""CPU: tests/pinned_model.py (the diploid DP with per-level cell constraints, written from its definition) against brute force.  On
the enumerable graphs of tests/test_gpu_score_paths.py, for a list of pin sets per graph: the model's value on every plane 0..b is
the maximum of PathModel.score over ALL ordered pairs of source -> sink paths that satisfy the pins with r1 + r2 <= plane, NEG_INF
exactly where no such pair exists; the numpy form of the model gives the same planes.  This validates the yardstick of
tests/test_gpu_pinned_run.py.  The pin sets: random require and forbid sets, wildcards, several pins per level, several levels,
unsatisfiable sets, pins that only one order of a pair satisfies; test_the_cases_are_not_vacuous asserts that they are what they are
meant to be."""
import numpy as np
import pytest

from paths_model import NEG_INF, PathModel
from pinned_model import FORBID, REQUIRE, brute_force_planes, pinned_planes, pinned_planes_np
from test_gpu_score_paths import ENUMERABLE
from test_partner_model import enumerable_graph

B = 3                                                   # = R of these graphs: planes 0..3
_CASES = {}


def case(q):
    """graph, model, all paths, their recombinations, the score of every ordered pair -- computed once"""
    if q not in _CASES:
        g = enumerable_graph(q)
        m = PathModel(g)
        paths = m.all_paths()
        rec = [m.recombinations(p) for p in paths]
        full = np.array([[m.score(p, x)[0] for x in paths] for p in paths], np.int64)
        _CASES[q] = (g, m, paths, rec, full)
    return _CASES[q]


def random_pins(m, rng, n_levels, per_level, p_wild=0.25, p_forbid=0.4):
    """per_level pins on each of n_levels distinct inner levels: vertices drawn inside the level, -1 with p_wild"""
    pins = []
    for l in rng.choice(np.arange(1, m.L - 1), size=min(n_levels, m.L - 2), replace=False):
        a0, a1 = int(m.level_off[l]), int(m.level_off[l + 1])
        for _ in range(per_level):
            v = [-1 if rng.random() < p_wild else int(rng.integers(a0, a1)) for _ in range(2)]
            pins.append((int(l), v[0], v[1], FORBID if rng.random() < p_forbid else REQUIRE))
    return pins


def pin_sets(q):
    """[(tag, pins)] for graph q"""
    g, m, paths, rec, full = case(q)
    rng = np.random.default_rng(700 + q)
    out = [("none", [])]
    for n_levels, per_level in ((1, 1), (1, 3), (2, 2), (3, 1), (m.L - 2, 2)):
        out.append((f"random {n_levels}x{per_level}", random_pins(m, rng, n_levels, per_level)))
    out.append(("forbid only", random_pins(m, rng, 2, 2, p_forbid=1.0)))
    out.append(("require only", random_pins(m, rng, 2, 2, p_forbid=0.0)))
    out.append(("wildcards", random_pins(m, rng, 2, 1, p_wild=0.7)))
    # one order only: the cell that two different paths pass on a level where they differ, and its mirror
    a, c = next((a, c) for a in range(len(paths)) for c in range(len(paths)) if any(x != y for x, y in zip(paths[a], paths[c])))
    l = next(l for l in range(m.L) if paths[a][l] != paths[c][l])
    out.append(("ordered", [(l, paths[a][l], paths[c][l], REQUIRE)]))
    out.append(("mirror", [(l, paths[c][l], paths[a][l], REQUIRE)]))
    # the best pair's cell on every inner level, required (the optimum stays) and forbidden in both orders, level by level
    best = np.unravel_index(np.argmax(np.where(np.add.outer(rec, rec) <= B, full, NEG_INF)), full.shape)
    pa, pc = paths[best[0]], paths[best[1]]
    out.append(("identity", [(l, pa[l], pc[l], REQUIRE) for l in range(1, m.L - 1)]))
    for l in range(1, m.L - 1):
        out.append((f"forbid best {l}", [(l, pa[l], pc[l], FORBID), (l, pc[l], pa[l], FORBID)]))
    # every single require-pin of one inner level (the through-values of its cells)
    l = 1 + q % (m.L - 2)
    for i in range(int(m.level_off[l]), int(m.level_off[l + 1])):
        for j in range(int(m.level_off[l]), int(m.level_off[l + 1])):
            out.append((f"cell {l} {i} {j}", [(l, i, j, REQUIRE)]))
    # unsatisfiable: two require-pins of a level that a forbid excludes, and a require on one level against a forbid-all on another
    a0 = int(m.level_off[1])
    out.append(("excluded", [(1, a0, -1, REQUIRE), (1, -1, a0, REQUIRE), (1, -1, -1, FORBID)]))
    out.append(("forbid all", [(m.L - 2, -1, -1, FORBID), (1, a0, a0, REQUIRE)]))
    return out


@pytest.mark.parametrize("q", range(len(ENUMERABLE)))
def test_model_is_the_brute_force_maximum(q):
    g, m, paths, rec, full = case(q)
    assert g.R == B
    for tag, pins in pin_sets(q):
        want, _ = brute_force_planes(m, paths, rec, full, B, pins)
        assert pinned_planes(m, B, pins) == want, (q, tag, pins)
        assert pinned_planes_np(m, B, pins).tolist() == want, (q, tag, pins)
        for b in range(B):                               # a smaller budget is the same planes, cut
            assert pinned_planes(m, b, pins) == want[:b + 1], (q, tag, b)


def test_no_pins_is_the_unpinned_optimum():
    for q in range(len(ENUMERABLE)):
        g, m, paths, rec, full = case(q)
        best, _ = m.best_per_budget(B, paths)
        assert pinned_planes(m, B, []) == [NEG_INF if v is None else v for v in best]


def test_the_cases_are_not_vacuous():
    mirror_differs = lowered = kept = late = unsat = several = wild = 0
    for q in range(len(ENUMERABLE)):
        g, m, paths, rec, full = case(q)
        free, _ = brute_force_planes(m, paths, rec, full, B, [])
        sets = dict(pin_sets(q))
        _, s1 = brute_force_planes(m, paths, rec, full, B, sets["ordered"])
        _, s2 = brute_force_planes(m, paths, rec, full, B, sets["mirror"])
        assert s1.any() and s2.any() and np.array_equal(s1, s2.T)
        mirror_differs += not np.array_equal(s1, s2)
        assert brute_force_planes(m, paths, rec, full, B, sets["identity"])[0][B] == free[B]
        for tag, pins in sets.items():
            planes, sat = brute_force_planes(m, paths, rec, full, B, pins)
            if tag.startswith("forbid best"):
                assert planes[B] <= free[B]
                lowered += planes[B] < free[B]
                kept += planes[B] == free[B]
            late += planes[0] == NEG_INF and planes[2] != NEG_INF
            unsat += not sat.any()
            levels = [p[0] for p in pins]
            several += len(set(levels)) >= 2 and len(levels) > len(set(levels))
            wild += any(p[1] == -1 or p[2] == -1 for p in pins)
        assert not brute_force_planes(m, paths, rec, full, B, sets["excluded"])[1].any()
    assert mirror_differs >= 1                           # an ordered pin and its mirror pick different sets of pairs
    assert lowered >= 1 and kept >= 1                    # a forbid that costs value, and one that a tie elsewhere absorbs
    assert late >= 1                                     # unsatisfiable at budget 0, satisfiable at budget 2
    assert unsat >= 2 * len(ENUMERABLE) and several >= 1 and wild >= 1

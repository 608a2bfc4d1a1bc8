"""CPU: tests/partner_model.py (the best partner of a given path, written from its definition) against what already exists.  On
the enumerable graphs of tests/test_gpu_score_paths.py, for every path p and every budget b: the model's value is the brute-force
maximum of PathModel.score(p, q) over all q with r(q) <= b, NEG_INF exactly where no such q exists, and the returned partner scores
that value; and for every b the maximum over p of model(p, b - r(p)) is the enumerated optimum of plane b and the oracle's value.
This validates the yardstick of tests/test_gpu_partner.py.  Cases 5..10 are the same graphs with dead-end
vertices (tests/loader_graphs.py): the yardstick of tests/test_gpu_dead_ends.py."""
import numpy as np
import pytest

import graphgen
from loader_graphs import N_ENUMERABLE_DEAD, dead_ends_enumerable
from partner_model import best_partner, best_partners
from paths_model import NEG_INF, PathModel
from test_gpu_score_paths import ENUMERABLE
from test_paths_model import oracle_values

BUDGETS = range(4)                                      # 0..3 = 0..R of these graphs
_CASES = {}
DEAD_ENDS = range(len(ENUMERABLE), len(ENUMERABLE) + N_ENUMERABLE_DEAD)   # cases 5..: the same graphs with dead-end vertices (tests/loader_graphs.py)


def enumerable_graph(q):
    if q >= len(ENUMERABLE):
        return dead_ends_enumerable(q - len(ENUMERABLE))
    seed, n_levels, extra, p_w1, p_colour = ENUMERABLE[q]
    return graphgen.random_levelized(seed, n_levels=n_levels, max_width=4, R=3, extra_edges=extra, p_w1=p_w1, p_colour=p_colour)


def case(q):
    """graph, model, all paths, their recombinations, the model's answer for every (path, budget) -- computed once"""
    if q not in _CASES:
        g = enumerable_graph(q)
        m = PathModel(g)
        paths = m.all_paths()
        rec = [m.recombinations(p) for p in paths]
        answers = {(a, b): best_partner(m, p, b) for a, p in enumerate(paths) for b in BUDGETS}
        _CASES[q] = (g, m, paths, rec, answers)
    return _CASES[q]


@pytest.mark.parametrize("q", [*range(len(ENUMERABLE)), *DEAD_ENDS])
def test_model_is_the_brute_force_maximum(q):
    g, m, paths, rec, answers = case(q)
    assert g.R == 3
    full = np.array([[m.score(p, x)[0] for x in paths] for p in paths])
    for a, p in enumerate(paths):
        for b in BUDGETS:
            value, partner, planes, _ = answers[(a, b)]
            fits = [x for x in range(len(paths)) if rec[x] <= b]
            if not fits:
                assert value == NEG_INF and partner is None, (q, a, b)
                continue
            assert value == max(full[a, x] for x in fits), (q, a, b)
            assert m.check_path(partner) is None and m.recombinations(partner) <= b
            assert m.score(p, partner)[0] == value, (q, a, b)
            assert planes[b] == value and planes == [answers[(a, r)][0] for r in range(b + 1)]       # "at most": plane r is budget r's answer


@pytest.mark.parametrize("q", [*range(len(ENUMERABLE)), *DEAD_ENDS])
def test_maximum_over_given_paths_is_the_plane_of_the_sweep(q):
    g, m, paths, rec, answers = case(q)
    best, _ = m.best_per_budget(g.R, paths)
    want = oracle_values(g, g.R)
    for b in BUDGETS:
        got = [answers[(a, b - rec[a])][0] for a in range(len(paths)) if rec[a] <= b]
        top = max(got) if got else NEG_INF
        assert top == (NEG_INF if best[b] is None else best[b]) == want[b], (q, b, top, best, want)


def test_the_cases_are_not_vacuous():
    unreachable = other = ties = 0
    for q in range(len(ENUMERABLE)):
        g, m, paths, rec, answers = case(q)
        for (a, b), (value, partner, _, n_ties) in answers.items():
            unreachable += value == NEG_INF
            other += partner is not None and partner != paths[a]
            ties += n_ties > 0
    print(f"unreachable (path, budget) {unreachable}, partners other than the given path {other}, answers with a tie decided by the tie-break {ties}")
    assert unreachable >= 1 and other >= 1 and ties >= 1


def test_a_decided_tie_goes_to_the_smallest_source():
    """where the walked chain met a tie, another path within the budget scores the same value: the tie-break chose between real alternatives"""
    seen = 0
    for q in range(len(ENUMERABLE)):
        g, m, paths, rec, answers = case(q)
        for (a, b), (value, partner, _, n_ties) in answers.items():
            if not n_ties:
                continue
            equal = [x for x in paths if m.recombinations(x) <= b and x != partner and m.score(paths[a], x)[0] == value]
            assert equal, (q, a, b)
            seen += 1
    assert seen >= 1


@pytest.mark.parametrize("q", [*range(len(ENUMERABLE)), *DEAD_ENDS])
def test_the_batched_model_is_the_model(q):
    g, m, paths, rec, answers = case(q)
    given = np.array([p for p in paths for b in BUDGETS], np.int32)
    budgets = np.array([b for p in paths for b in BUDGETS], np.int32)
    values, partners = best_partners(m, given, budgets)
    for i, (a, b) in enumerate((a, b) for a in range(len(paths)) for b in BUDGETS):
        value, partner, _, _ = answers[(a, b)]
        assert values[i] == value
        assert tuple(partners[i]) == (partner if partner is not None else (-1,) * m.L), (q, a, b)

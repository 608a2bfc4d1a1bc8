"""CPU: tests/marginals_model.py (partner marginals, written from their definition) against brute force.  On the enumerable graphs
of tests/test_gpu_score_paths.py, for every sixth path as the given one and every budget 0..R + 1: M[v] is the maximum of
PathModel.score(given, q) over all paths q through v with r(q) <= b, NEG_INF exactly where there is none; source and sink, and the
best vertex of every level, are worth what partner_model.best_partner answers; the level records follow the tie rule; and the
batched form is the plain one.  This validates the yardstick of tests/test_gpu_marginals.py.  Cases 5..10 are the same graphs with
dead-end vertices (tests/loader_graphs.py; every second path given): the yardstick of tests/test_gpu_dead_ends.py."""
import numpy as np
import pytest

from marginals_model import level_records, partner_marginals, partner_marginals_batch
from partner_model import best_partner
from paths_model import NEG_INF, PathModel
from test_gpu_score_paths import ENUMERABLE
from test_partner_model import DEAD_ENDS, enumerable_graph

BUDGETS = range(5)                                      # 0..4 = 0..R + 1 of these graphs
_CASES = {}


def case(q):
    """graph, model, all paths, their recombinations, the indices of the given paths, the model's answer per (given, budget)"""
    if q not in _CASES:
        g = enumerable_graph(q)
        m = PathModel(g)
        paths = m.all_paths()
        rec = [m.recombinations(p) for p in paths]
        some = list(range(0, len(paths), 2 if q in DEAD_ENDS else 6))      # (the graphs with dead ends have as few as five paths)
        answers = {(a, b): partner_marginals(m, paths[a], b) for a in some for b in BUDGETS}
        _CASES[q] = (g, m, paths, rec, some, answers)
    return _CASES[q]


@pytest.mark.parametrize("q", [*range(len(ENUMERABLE)), *DEAD_ENDS])
def test_marginal_is_the_brute_force_maximum_through_the_vertex(q):
    g, m, paths, rec, some, answers = case(q)
    assert g.R == 3 and len(some) >= 2
    for a in some:
        scores = [m.score(paths[a], x)[0] for x in paths]
        for b in BUDGETS:
            M, _ = answers[(a, b)]
            want = [NEG_INF] * m.nV
            for x, p in enumerate(paths):
                if rec[x] <= b:
                    for v in p:
                        want[v] = max(want[v], scores[x])
            assert M == want, (q, a, b)


@pytest.mark.parametrize("q", [*range(len(ENUMERABLE)), *DEAD_ENDS])
def test_source_sink_and_every_level_are_worth_the_best_partner(q):
    g, m, paths, rec, some, answers = case(q)
    for a in some:
        for b in BUDGETS:
            M, records = answers[(a, b)]
            value = best_partner(m, paths[a], b)[0]
            assert M[0] == M[m.nV - 1] == value, (q, a, b)
            assert len(records) == m.L
            for l, (v1, x1, v2, x2) in enumerate(records):
                assert x1 == value == max(M[int(m.level_off[l]):int(m.level_off[l + 1])]), (q, a, b, l)
                assert x2 <= x1
                if value == NEG_INF:
                    assert (v1, x1, v2, x2) == (-1, NEG_INF, -1, NEG_INF)
            assert max(M) == value and (value != NEG_INF or set(M) == {NEG_INF})


@pytest.mark.parametrize("q", [*range(len(ENUMERABLE)), *DEAD_ENDS])
def test_level_records_follow_the_tie_rule(q):
    """stated once more without a sort: best = the first vertex in id order that reaches the level's maximum, second = the first
    other vertex that reaches the maximum of the rest"""
    g, m, paths, rec, some, answers = case(q)
    for (a, b), (M, records) in answers.items():
        for l, (v1, x1, v2, x2) in enumerate(records):
            ids = [v for v in range(int(m.level_off[l]), int(m.level_off[l + 1])) if M[v] != NEG_INF]
            if not ids:
                assert (v1, x1, v2, x2) == (-1, NEG_INF, -1, NEG_INF)
                continue
            top = max(M[v] for v in ids)
            assert (v1, x1) == (next(v for v in ids if M[v] == top), top)
            others = [v for v in ids if v != v1]
            if not others:
                assert (v2, x2) == (-1, NEG_INF)
                continue
            nxt = max(M[v] for v in others)
            assert (v2, x2) == (next(v for v in others if M[v] == nxt), nxt)
            assert v2 != v1 and (x2 < x1 or v2 > v1)
    # and on a hand-made level: ties to the smallest id, an unreachable vertex never listed
    assert level_records([NEG_INF, 5, 7, 7, NEG_INF, 3], [0, 1, 4, 5, 6]) == [(-1, NEG_INF, -1, NEG_INF), (2, 7, 3, 7), (-1, NEG_INF, -1, NEG_INF), (5, 3, -1, NEG_INF)]
    assert level_records([4, 4, 9], [0, 3]) == [(2, 9, 0, 4)]


def test_the_cases_are_not_vacuous():
    unreachable = ties = margins = 0
    for q in range(len(ENUMERABLE)):
        g, m, paths, rec, some, answers = case(q)
        for (a, b), (M, records) in answers.items():
            unreachable += M[m.nV - 1] == NEG_INF
            for v1, x1, v2, x2 in records:
                ties += v2 >= 0 and x2 == x1
                margins += v2 >= 0 and x1 > x2
    print(f"unreachable (given, budget) {unreachable}, levels with second_value == best_value {ties}, levels with a positive margin {margins}")
    assert unreachable >= 1 and ties >= 1 and margins >= 1


@pytest.mark.parametrize("q", [*range(len(ENUMERABLE)), *DEAD_ENDS])
def test_the_batched_model_is_the_model(q):
    g, m, paths, rec, some, answers = case(q)
    keys = [(a, b) for a in some for b in BUDGETS]
    given = np.array([paths[a] for a, b in keys], np.int32)
    budgets = np.array([b for a, b in keys], np.int32)
    records, M = partner_marginals_batch(m, given, budgets)
    assert records.shape == (len(keys), m.L, 4) and M.shape == (len(keys), m.nV)
    for i, key in enumerate(keys):
        want_M, want_rec = answers[key]
        assert M[i].tolist() == want_M, (q, key)
        assert [tuple(x) for x in records[i].tolist()] == want_rec, (q, key)

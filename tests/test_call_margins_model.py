"""CPU: tests/call_margins_model.py (call margins, written from their definition) against brute force.  On the enumerable graphs of
tests/test_gpu_score_paths.py, for every budget 0..R and for the first and the last of the best pairs within it (what a run's answer
is: a pair worth the enumerated optimum of the plane): value is the plane's optimum on every level of both rows; the alternative of
a level is the maximum of PathModel.score(given, q) over all enumerated partner paths q within the partner budget that pass through
a vertex of another class than the called one, at the smallest such vertex id, and (-1, NEG_INF) exactly where there is none -- for
no classes, one class for all, and 2..4 classes drawn per level.  This validates the yardstick of tests/test_gpu_call_margins.py."""
import numpy as np
import pytest

from call_margins_model import call_margins, call_margins_batch, class_arrays
from paths_model import NEG_INF, PathModel
from test_gpu_score_paths import ENUMERABLE
from test_partner_model import enumerable_graph

BUDGETS = range(4)                                      # 0..3 = 0..R of these graphs
_CASES = {}


def case(q):
    """graph, model, all paths, their recombinations, the score of every ordered pair, the class arrays, and per reachable budget
    (optimum, [the first and the last pair that reach it])"""
    if q not in _CASES:
        g = enumerable_graph(q)
        m = PathModel(g)
        paths = m.all_paths()
        rec = [m.recombinations(p) for p in paths]
        full = np.array([[m.score(p, x)[0] for x in paths] for p in paths])
        answers = {}
        for b in BUDGETS:
            fits = [(a, c) for a in range(len(paths)) for c in range(len(paths)) if rec[a] + rec[c] <= b]
            if not fits:
                continue
            top = max(full[a, c] for a, c in fits)
            best = [(a, c) for a, c in fits if full[a, c] == top]
            answers[b] = (int(top), [best[0], best[-1]])
        _CASES[q] = (g, m, paths, rec, full, class_arrays(g, 100 + q), answers)
    return _CASES[q]


def brute_force(m, paths, rec, full, called, given, budget, cls):
    """per level (alt_vertex, alt_value): over the partners x of paths[given] with rec[x] <= budget"""
    out = []
    for l in range(m.L):
        c = paths[called][l]
        best = {}
        for x, p in enumerate(paths):
            v = p[l]
            if rec[x] <= budget and (v != c if cls is None else cls[v] != cls[c]):
                best[v] = max(best.get(v, NEG_INF), int(full[given, x]))
        out.append(min(((-s, v) for v, s in best.items()), default=None))
    return [(-1, NEG_INF) if t is None else (t[1], -t[0]) for t in out]


@pytest.mark.parametrize("q", range(len(ENUMERABLE)))
def test_model_is_the_brute_force_maximum_over_other_classes(q):
    g, m, paths, rec, full, classes, answers = case(q)
    assert g.R == 3 and len(answers) >= 2
    for b, (top, pairs) in answers.items():
        for a, c in pairs:
            for cls in classes:
                rows = call_margins(m, paths[a], paths[c], b, cls)
                for h, (called, given) in enumerate(((a, c), (c, a))):
                    want = brute_force(m, paths, rec, full, called, given, b - rec[given], cls)
                    assert [r[0] for r in rows[h]] == list(paths[called])
                    assert [r[1] for r in rows[h]] == [top] * m.L, (q, b, a, c, h)      # value == V_b on every level
                    assert [r[2:] for r in rows[h]] == want, (q, b, a, c, h)
                    assert all(r[3] <= r[1] for r in rows[h])


@pytest.mark.parametrize("q", range(len(ENUMERABLE)))
def test_one_class_for_all_has_no_alternative_and_no_classes_means_another_vertex(q):
    g, m, paths, rec, full, classes, answers = case(q)
    for b, (top, pairs) in answers.items():
        a, c = pairs[0]
        none, ones, drawn = (call_margins(m, paths[a], paths[c], b, cls) for cls in classes)
        own = call_margins(m, paths[a], paths[c], b, np.arange(g.n_vertices))
        assert own == none
        for h in range(2):
            assert all(r[2:] == (-1, NEG_INF) for r in ones[h])
            assert none[h][0][2:] == (-1, NEG_INF) and none[h][-1][2:] == (-1, NEG_INF)      # source and sink stand alone
            # fewer candidates never raise the alternative
            assert all(d[3] <= n[3] for d, n in zip(drawn[h], none[h]))


@pytest.mark.parametrize("q", range(len(ENUMERABLE)))
def test_the_batched_model_is_the_model(q):
    g, m, paths, rec, full, classes, answers = case(q)
    for b, (top, pairs) in answers.items():
        for a, c in pairs:
            M, records = call_margins_batch(m, paths[a], paths[c], b, classes)
            assert M.shape == (2, m.nV) and len(records) == 3
            for cls, got in zip(classes, records):
                assert got.shape == (2, m.L, 4)
                assert [[tuple(r) for r in row] for row in got.tolist()] == call_margins(m, paths[a], paths[c], b, cls)


def test_the_cases_are_not_vacuous():
    with_alt = margin0 = positive = no_alt_drawn = 0
    for q in range(len(ENUMERABLE)):
        g, m, paths, rec, full, classes, answers = case(q)
        for b, (top, pairs) in answers.items():
            for a, c in pairs:
                for cls in (classes[0], classes[2]):
                    for row in call_margins(m, paths[a], paths[c], b, cls):
                        for vertex, value, alt_vertex, alt_value in row[1:-1]:
                            with_alt += alt_vertex >= 0
                            margin0 += alt_vertex >= 0 and alt_value == value
                            positive += alt_vertex >= 0 and alt_value < value
                            no_alt_drawn += cls is not None and alt_vertex < 0
    print(f"levels with an alternative {with_alt}, with margin 0 {margin0}, with a positive margin {positive}, drawn classes without one {no_alt_drawn}")
    assert with_alt >= 1 and margin0 >= 1 and positive >= 1 and no_alt_drawn >= 1

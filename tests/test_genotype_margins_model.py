"""CPU: tests/genotype_margins_model.py (genotype margins, written from their definition) against brute force.  On the enumerable
graphs of tests/test_gpu_score_paths.py, for every budget 0..3: T equals the maximum over all enumerated ordered pairs of paths
through the cell, for every cell, unreachable ones included; T is symmetric; its maximum on every level is V_b, which is the
oracle's value at that budget; the joint marginal J is at least the conditional M of tests/marginals_model.py for either half of an
optimal pair, and strictly greater somewhere; the alternative of a record is the brute-force one for three kinds of classes; and the
numpy form is the plain one.  This validates the yardstick of tests/test_gpu_genotype_margins.py.  Cases 5..10 are the same graphs with dead-end vertices
(tests/loader_graphs.py): the yardstick of tests/test_gpu_dead_ends.py."""
import numpy as np
import pytest

from call_margins_model import class_arrays
from genotype_margins_model import genotype_margins_np, joint_marginals, level_records, through_values, through_values_np
from marginals_model import partner_marginals
from paths_model import NEG_INF, PathModel
from test_gpu_score_paths import ENUMERABLE
from test_partner_model import DEAD_ENDS, enumerable_graph
from test_paths_model import oracle_values

BUDGETS = range(4)
_CASES = {}


def case(q):
    """graph, model, all paths [n, L], their recombinations [n], the score of every ordered pair [n, n], per budget the model's (T, V)
    and the brute-force through-values"""
    if q not in _CASES:
        g = enumerable_graph(q)
        m = PathModel(g)
        P = np.array(m.all_paths(), np.int64)
        rec = np.array([m.recombinations(p) for p in P.tolist()], np.int64)
        n = len(P)
        S = np.zeros((n, n), np.int64)
        for l in range(1, m.L):                          # the score of every ordered pair, transition by transition
            a0, b0 = int(m.level_off[l - 1]), int(m.level_off[l])
            ka, kb = int(m.level_off[l] - a0), int(m.level_off[l + 1] - b0)
            D = np.array([[[[sum(m.delta(a0 + u, a0 + v, b0 + i, b0 + j)) for j in range(kb)] for i in range(kb)] for v in range(ka)] for u in range(ka)], np.int64)
            S += D[(P[:, l - 1] - a0)[:, None], (P[:, l - 1] - a0)[None, :], (P[:, l] - b0)[:, None], (P[:, l] - b0)[None, :]]
        rng = np.random.default_rng(q)
        for a, c in rng.integers(0, n, (40, 2)).tolist():                  # ... is what PathModel.score says
            assert S[a, c] == m.score(P[a], P[c])[0]
        brute = {}
        for b in BUDGETS:
            ok = (rec[:, None] + rec[None, :]) <= b
            vals = np.where(ok, S, NEG_INF)
            per_level = []
            for l in range(m.L):
                a0, k = int(m.level_off[l]), int(m.level_off[l + 1] - m.level_off[l])
                Tl = np.full((k, k), NEG_INF, np.int64)
                ii, jj = np.broadcast_arrays((P[:, l] - a0)[:, None], (P[:, l] - a0)[None, :])
                np.maximum.at(Tl, (ii, jj), vals)
                per_level.append(Tl)
            brute[b] = per_level
        model = {b: through_values(m, b) for b in BUDGETS}
        _CASES[q] = (g, m, P, rec, S, model, brute)
    return _CASES[q]


@pytest.mark.parametrize("q", [*range(len(ENUMERABLE)), *DEAD_ENDS])
def test_through_value_is_the_brute_force_maximum_in_every_cell(q):
    g, m, P, rec, S, model, brute = case(q)
    assert g.R == 3
    cells = 0
    for b in BUDGETS:
        T, V = model[b]
        assert len(T) == m.L
        for l in range(m.L):
            k = int(m.level_off[l + 1] - m.level_off[l])
            got = np.array(T[l], np.int64)
            assert got.shape == (k, k) == brute[b][l].shape                  # no cell is skipped, the unreachable ones included
            assert np.array_equal(got, brute[b][l]), (q, b, l)
            assert np.array_equal(got, got.T), (q, b, l)
            assert got.max() == V, (q, b, l)
            cells += k * k
    assert cells == len(BUDGETS) * int((np.diff(m.level_off).astype(np.int64) ** 2).sum())
    assert [model[b][1] for b in BUDGETS] == oracle_values(g, g.R)


def test_joint_marginal_is_at_least_the_conditional_one_and_sometimes_more():
    strict = compared = 0
    for q in range(len(ENUMERABLE)):
        g, m, P, rec, S, model, brute = case(q)
        for b in BUDGETS:
            T, V = model[b]
            if V == NEG_INF:
                continue
            J = joint_marginals(m, T)
            assert len(J) == m.nV and max(J) == V
            ok = (rec[:, None] + rec[None, :]) <= b
            a, c = np.argwhere(ok & (S == V))[0]
            for given in (int(a), int(c)):
                M, _ = partner_marginals(m, P[given].tolist(), b - int(rec[given]))
                for v in range(m.nV):
                    assert J[v] >= M[v], (q, b, given, v)
                    strict += J[v] > M[v]
                    compared += 1
    print(f"(vertex, budget, half) cases {compared}, with J > M {strict}")
    assert strict > 0


def _called_kinds(m, P, rec, S, V, b, seed):
    """an optimal pair (if there is one), a sampled pair of paths, and a list of cells that is no pair of paths"""
    rng = np.random.default_rng(seed)
    out = []
    if V != NEG_INF:
        a, c = np.argwhere(((rec[:, None] + rec[None, :]) <= b) & (S == V))[0]
        out.append(np.stack([P[a], P[c]]))
    a, c = rng.integers(0, len(P), 2)
    out.append(np.stack([P[a], P[c]]))
    out.append(np.array([[rng.integers(m.level_off[l], m.level_off[l + 1]) for l in range(m.L)] for _ in range(2)], np.int64))
    return out


@pytest.mark.parametrize("q", [*range(len(ENUMERABLE)), *DEAD_ENDS])
def test_the_alternative_is_the_brute_force_one(q):
    g, m, P, rec, S, model, brute = case(q)
    n_alt = n_none = 0
    for b in BUDGETS:
        T, V = model[b]
        for kind, cls in enumerate(class_arrays(g, 11 + q)):
            for called in _called_kinds(m, P, rec, S, V, b, 100 * q + b):
                records = level_records(m, T, called, cls)
                assert len(records) == m.L
                for l, (c1, c2, value, a1, a2, alt) in enumerate(records):
                    a0, k = int(m.level_off[l]), int(m.level_off[l + 1] - m.level_off[l])
                    assert (c1, c2) == (called[0][l], called[1][l]) and value == brute[b][l][c1 - a0, c2 - a0]
                    geno = frozenset((c1, c2)) if cls is None else frozenset((int(cls[c1]), int(cls[c2])))
                    # every ordered cell whose genotype differs, as (-value, min, max): the smallest is the alternative
                    cands = [(-int(brute[b][l][i, j]), a0 + min(i, j), a0 + max(i, j)) for i in range(k) for j in range(k)
                             if brute[b][l][i, j] != NEG_INF and
                             (frozenset((a0 + i, a0 + j)) if cls is None else frozenset((int(cls[a0 + i]), int(cls[a0 + j])))) != geno]
                    want = min(cands) if cands else None
                    assert (a1, a2, alt) == ((-1, -1, NEG_INF) if want is None else (want[1], want[2], -want[0])), (q, b, kind, l)
                    assert a1 <= a2
                    n_alt += want is not None
                    n_none += want is None
                if kind == 1:                             # one class for all: no other genotype exists
                    assert all(r[3:] == (-1, -1, NEG_INF) for r in records)
    assert n_alt > 0 and n_none > 0


@pytest.mark.parametrize("q", [*range(len(ENUMERABLE)), *DEAD_ENDS])
def test_the_numpy_form_is_the_plain_form(q):
    g, m, P, rec, S, model, brute = case(q)
    for b in BUDGETS:
        T, V = model[b]
        Tn, Vn = through_values_np(m, b)
        assert Vn == V and len(Tn) == m.L
        for l in range(m.L):
            assert np.array_equal(Tn[l], np.array(T[l], np.int64)), (q, b, l)
        for cls in class_arrays(g, 11 + q):
            called = np.stack(_called_kinds(m, P, rec, S, V, b, 100 * q + b))
            records, V2, J = genotype_margins_np(m, called, b, cls, Tn, Vn)
            assert V2 == V and J.tolist() == joint_marginals(m, T)
            for i in range(len(called)):
                assert [tuple(r) for r in records[i].tolist()] == level_records(m, T, called[i], cls), (q, b, i)


def test_margin_zero_levels_exist():
    """interior levels where the best other genotype is worth as much as the optimal one: the joint margin of an optimal pair is 0"""
    zero = interior = 0
    for q in range(len(ENUMERABLE)):
        g, m, P, rec, S, model, brute = case(q)
        for b in BUDGETS:
            T, V = model[b]
            if V == NEG_INF:
                continue
            called = _called_kinds(m, P, rec, S, V, b, 0)[0]
            for c1, c2, value, a1, a2, alt in level_records(m, T, called)[1:-1]:
                assert value == V and alt <= value
                interior += 1
                zero += alt == value
    print(f"interior levels {interior}, with joint margin 0 {zero}")
    assert 0 < zero < interior

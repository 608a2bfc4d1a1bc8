"""CPU: the claim dg_dp_genotype_margins_budgets rests on, held against models that already exist.  tests/genotype_budgets_model.py
computes the forward and backward states ONCE at bmax and cuts T^b out of them; on the five enumerable graphs, for bmax = 3 and for
bmax one beyond what any pair of paths of the graph spends, every slice b = 0..bmax must be genotype_margins_model.through_values_np(m, b)
-- under pins pinned_joint_model.pinned_through_values_np(m, b, pins) -- cell by cell, V_b included, and the records of a call with
mixed budgets must be those of genotype_margins_np / pinned_genotype_margins_np query by query."""
import numpy as np
import pytest

from call_margins_model import class_arrays
from genotype_budgets_model import genotype_margins_budgets_np, joint_states_np, sliced_through_values
from genotype_margins_model import genotype_margins_np, through_values_np
from paths_model import NEG_INF
from pinned_joint_model import pinned_genotype_margins_np, pinned_through_values_np
from test_gpu_score_paths import ENUMERABLE
from test_pinned_model import case, pin_sets


def _bmaxes(rec):
    return (3, 2 * max(rec) + 1)                         # a pair spends at most twice what its costlier path does


def _pin_choice(q):
    """the composed sets of test_pinned_model.pin_sets (random, one-order, identity, forbid best, unsatisfiable): not the single cells"""
    return [(tag, pins) for tag, pins in pin_sets(q) if pins and not tag.startswith("cell ")]


@pytest.mark.parametrize("q", range(len(ENUMERABLE)))
def test_every_slice_is_the_through_value_at_its_budget(q):
    g, m, paths, rec, full = case(q)
    differ = 0
    for bmax in _bmaxes(rec):
        F, B = joint_states_np(m, bmax)
        last = None
        for b in range(bmax + 1):
            T, V = sliced_through_values(m, F, B, b)
            want, want_V = through_values_np(m, b)
            assert V == want_V, (q, bmax, b)
            for l in range(m.L):
                assert np.array_equal(T[l], want[l]), (q, bmax, b, l)
            differ += last is not None and any(not np.array_equal(x, y) for x, y in zip(T, last))
            last = T
    assert differ >= 1                                   # the budgets do not all answer alike


@pytest.mark.parametrize("q", range(len(ENUMERABLE)))
def test_every_slice_is_the_pinned_through_value_at_its_budget(q):
    g, m, paths, rec, full = case(q)
    asymmetric = unsat = 0
    for n, (tag, pins) in enumerate(_pin_choice(q)):
        bmax = _bmaxes(rec)[n % 2]
        F, B = joint_states_np(m, bmax, pins)
        for b in range(bmax + 1):
            T, V = sliced_through_values(m, F, B, b)
            want, want_V = pinned_through_values_np(m, b, pins)
            assert V == want_V, (q, tag, bmax, b)
            for l in range(m.L):
                assert np.array_equal(T[l], want[l]), (q, tag, bmax, b, l)
            asymmetric += any(not np.array_equal(t, t.T) for t in T)
        unsat += V == NEG_INF
    assert asymmetric >= 1 and unsat >= 1


@pytest.mark.parametrize("q", range(len(ENUMERABLE)))
def test_records_are_those_of_the_one_budget_models(q):
    g, m, paths, rec, full = case(q)
    rng = np.random.default_rng(80 + q)
    budgets = [3, 0, 2, 1, 2, 2 * max(rec) + 1]
    called = np.array([[[rng.integers(m.level_off[l], m.level_off[l + 1]) for l in range(m.L)] for _ in range(2)] for _ in budgets], np.int32)
    called[0] = np.asarray(m.sample_paths(rng, 2)[0], np.int32)
    sets = [None, []] + [pins for _, pins in _pin_choice(q)[:4]]
    for cls in class_arrays(g, 21 + q):
        for pins in sets:
            got, V = genotype_margins_budgets_np(m, called, budgets, cls, pins)
            for x, b in enumerate(budgets):
                if pins is None:
                    want, want_V, _ = genotype_margins_np(m, called[x:x + 1], b, cls)
                else:
                    T, TV = pinned_through_values_np(m, b, pins)
                    want, want_V, _ = pinned_genotype_margins_np(m, called[x:x + 1], T, TV, cls)
                assert V[x] == want_V and np.array_equal(got[x], want[0]), (q, x, b, pins)

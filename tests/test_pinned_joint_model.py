"""CPU: tests/pinned_joint_model.py (the joint pass of the diploid DP under per-level cell constraints, written from its definition)
against brute force.  On the enumerable graphs of tests/test_gpu_score_paths.py, at budgets 0..3 and for the pin sets of
tests/test_pinned_model.py: T of every cell of every level is the maximum of PathModel.score over ALL ordered pairs of source -> sink
paths that satisfy the pins, pass the cell in that order and spend at most the budget, NEG_INF exactly where there is none; the
numpy form gives the same; the maximum of every level is the pinned run's plane.  This validates the yardstick of
tests/test_gpu_pinned_joint.py.  test_the_cases_are_not_vacuous asserts that the pin sets do what they are meant to do to T."""
import numpy as np
import pytest

from call_margins_model import class_arrays
from genotype_margins_model import level_records, through_values_np
from paths_model import NEG_INF
from pinned_joint_model import (brute_force_through_values, folded, pinned_genotype_margins_np, pinned_genotype_table, pinned_genotype_table_np,
                                pinned_level_records, pinned_through_values, pinned_through_values_np)
from pinned_model import pinned_planes
from test_gpu_score_paths import ENUMERABLE
from test_pinned_model import B, case, pin_sets


@pytest.mark.parametrize("q", range(len(ENUMERABLE)))
def test_model_is_the_brute_force_maximum(q):
    g, m, paths, rec, full = case(q)
    assert g.R == B
    for tag, pins in pin_sets(q):
        planes = pinned_planes(m, B, pins)
        for b in range(B + 1):
            want = brute_force_through_values(m, paths, rec, full, b, pins)
            T, V = pinned_through_values(m, b, pins)
            Tn, Vn = pinned_through_values_np(m, b, pins)
            assert V == Vn == planes[b], (q, tag, b)
            for l in range(m.L):
                assert np.array_equal(np.asarray(T[l], np.int64), want[l]), (q, tag, b, l, pins)
                assert np.array_equal(Tn[l], want[l]), (q, tag, b, l, pins)
                assert want[l].max() == planes[b], (q, tag, b, l)      # the closing check: every level's maximum is the optimum


@pytest.mark.parametrize("q", range(len(ENUMERABLE)))
def test_records_and_tables_of_the_two_forms_agree(q):
    g, m, paths, rec, full = case(q)
    rng = np.random.default_rng(40 + q)
    for n, (tag, pins) in enumerate(pin_sets(q)):
        b = n % (B + 1)
        T, V = pinned_through_values(m, b, pins)
        Tn, Vn = pinned_through_values_np(m, b, pins)
        called = np.array([[[rng.integers(m.level_off[l], m.level_off[l + 1]) for l in range(m.L)] for _ in range(2)] for _ in range(3)], np.int64)
        for cls in class_arrays(g, 50 + q):
            recs, _, J = pinned_genotype_margins_np(m, called, Tn, Vn, cls)
            for x in range(len(called)):
                assert recs[x].tolist() == [list(r) for r in pinned_level_records(m, T, called[x], cls)], (q, tag, b, x)
            off, rows = pinned_genotype_table_np(m, Tn, cls)
            plain = pinned_genotype_table(m, T, cls)
            assert [len(r) for r in plain] == np.diff(off).tolist()
            assert [list(r) for level in plain for r in level] == rows.tolist(), (q, tag, b)
            assert J.tolist() == [max(row) for l in range(m.L) for row in T[l]]
        if not pins:                                     # no pins: the unpinned model, records included
            Tu, Vu = through_values_np(m, b)
            assert Vu == V and all(np.array_equal(x, y) for x, y in zip(Tu, Tn))
            assert pinned_level_records(m, T, called[0]) == level_records(m, Tu, called[0])


def test_the_cases_are_not_vacuous():
    asymmetric = lowered = late = unchanged = 0
    for q in range(len(ENUMERABLE)):
        g, m, paths, rec, full = case(q)
        free, _ = through_values_np(m, B)
        for tag, pins in pin_sets(q):
            T, V = pinned_through_values_np(m, B, pins)
            for l in range(m.L):
                assert (T[l] <= free[l]).all(), (q, tag, l)              # T(. | P) <= T(.)
            asymmetric += any(not np.array_equal(t, t.T) for t in T)
            lowered += any((t < f).any() and t.max() != NEG_INF for t, f in zip(T, free))
            unchanged += bool(pins) and all(np.array_equal(t, f) for t, f in zip(T, free))
            late += pinned_through_values_np(m, 0, pins)[1] == NEG_INF and pinned_through_values_np(m, 2, pins)[1] != NEG_INF
            if tag in ("excluded", "forbid all"):                      # unsatisfiable: NEG_INF everywhere, the empty table
                assert V == NEG_INF and all((t == NEG_INF).all() for t in T) and len(pinned_genotype_table_np(m, T)[1]) == 0
            if not np.array_equal(T[1], T[1].T):                        # the folded values are symmetric, the ordered ones are not
                assert np.array_equal(folded(T)[1], folded(T)[1].T)
    assert asymmetric >= 1                               # a set that makes T asymmetric
    assert lowered >= 1                                  # a set that lowers T somewhere and leaves the level reachable
    assert late >= 1                                     # unsatisfiable at budget 0, satisfiable at 2
    assert unchanged >= 1                                # a set (not the empty one) that leaves T as it was

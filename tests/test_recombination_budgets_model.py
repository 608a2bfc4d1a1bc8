"""CPU: tests/recombination_budgets_model.py (recombination margins for every listed budget from ONE pair of joint states at the largest)
against tests/recombination_margins_model.py at each budget, which tests/test_recombination_margins_model.py pins to brute force.  On the
enumerable graphs of tests/test_gpu_score_paths.py and the graphs of tests/test_gpu_phase_margins.py, at bmax 3 and 5: the planes 0..b
of the states at bmax give exactly the records, called_out and V of the one-budget model at b.  Then the floor that keeps
tests/test_gpu_recombination_budgets.py from being vacuous (the records depend on the budget at most transitions, so a kernel that pairs
the wrong planes cannot pass), a budget nobody fits beside one that somebody does, and the padded-graph claim of tests/padded_graphs.py
for a call of mixed budgets."""
import numpy as np
import pytest

import graphgen
import padded_graphs as pg
from paths_model import NEG_INF, PathModel
from phase_margins_model import joint_states_fb
from recombination_budgets_model import recombination_margins_budgets_np, sliced_states
from recombination_margins_model import recombination_margins_np, remap_rows
from test_gpu_phase_margins import SEEDS, case as gpu_case
from test_gpu_score_paths import ENUMERABLE
from test_partner_model import enumerable_graph

MIXED = [3, 0, 2, 1, 2]                                 # unsorted, with a repeat


def _called(m, n, seed):
    """n called pairs: sampled pairs of paths, and cells that are no pair of paths in every third query"""
    rng = np.random.default_rng(seed)
    out = []
    for q in range(n):
        if q % 3 == 2:
            out.append(np.array([[rng.integers(m.level_off[l], m.level_off[l + 1]) for l in range(m.L)] for _ in range(2)], np.int64))
        else:
            out.append(np.asarray(m.sample_paths(rng, 2, p_w0=0.9)[0], np.int64))
    return np.stack(out)


def graphs():
    for q in range(len(ENUMERABLE)):
        yield f"enumerable{q}", PathModel(enumerable_graph(q))
    for seed in SEEDS:
        yield f"seed{seed}", gpu_case(seed)[1]


@pytest.mark.parametrize("bmax", [3, 5])
def test_every_slice_is_the_one_budget_model(bmax):
    n = 0
    for name, m in graphs():
        states = joint_states_fb(m, bmax)
        called = _called(m, 3, bmax)
        for b in range(bmax + 1):
            want, want_out, V = recombination_margins_np(m, b, called)
            got, out, Vb = recombination_margins_np(m, b, called, sliced_states(states, b))
            assert Vb == V, (name, bmax, b)
            assert np.array_equal(got, want) and np.array_equal(out, want_out), (name, bmax, b)
            n += 1
    assert n == (len(ENUMERABLE) + len(SEEDS)) * (bmax + 1)


def test_a_mixed_call_is_the_one_budget_model_query_by_query():
    for name, m in graphs():
        called = _called(m, len(MIXED), 11)
        rec, out, V = recombination_margins_budgets_np(m, MIXED, called)
        assert rec.shape == (len(MIXED), m.L - 1, 16) and out.shape == (len(MIXED), m.L - 1, 2) and V.shape == (len(MIXED),)
        plain, none, V2 = recombination_margins_budgets_np(m, MIXED)
        assert none is None and np.array_equal(plain, rec) and np.array_equal(V2, V)          # the records do not depend on called
        for q, b in enumerate(MIXED):
            want, want_out, Vb = recombination_margins_np(m, b, called[q:q + 1])
            assert V[q] == Vb and np.array_equal(rec[q], want) and np.array_equal(out[q], want_out[0]), (name, q, b)
        assert np.array_equal(rec[2], rec[4])                                                  # queries of one budget share their records


def test_the_records_depend_on_the_budget():
    """on the graphs of tests/test_gpu_phase_margins.py: the transitions whose record at some budget in 0..3 differs from that at 5"""
    differ = total = 0
    for seed in SEEDS:
        m = gpu_case(seed)[1]
        rec, _, _ = recombination_margins_budgets_np(m, [0, 1, 2, 3, 5])
        differ += int((rec[:4] != rec[4][None]).any(axis=2).any(axis=0).sum())
        total += m.L - 1
    print(f"transitions {total}: the record of some budget in 0..3 differs from that at 5 on {differ}")
    assert total == 150 and differ >= 100


def unfit_graph():
    """every edge weighs 1: a pair of paths spends 2 (L - 1) = 10 (the graph of test_gpu_recombination_margins.test_a_budget_nobody_fits)"""
    return graphgen.random_levelized(9611, widths=[1, 3, 4, 3, 4, 1], R=3, p_w1=1.0, dup_edges=True, extra_edges=1.2, p_colour=0.5)


def test_a_budget_nobody_fits_beside_one_that_somebody_does():
    m = PathModel(unfit_graph())
    called = np.stack([m.sample_paths(np.random.default_rng(1), 2)[0]] * 3)
    rec, out, V = recombination_margins_budgets_np(m, [9, 10, 0], called)
    assert V[0] == V[2] == NEG_INF != V[1]
    for q in (0, 2):
        assert (rec[q, :, 1:4] == NEG_INF).all() and (rec[q, :, 4:] == -1).all() and (out[q, :, 1] == NEG_INF).all()
    assert (rec[1, :, 3] == V[1]).all() and (rec[1, :, 1:3] == NEG_INF).all() and (out[1, :, 1] != NEG_INF).any()
    assert (out[:, :, 0] == 2).all()


@pytest.mark.parametrize("shape", sorted(pg.SHAPES))
def test_the_padded_graph_claim_carries_over(shape):
    g, gp, new_id = pg.SHAPES[shape](small=True)
    budgets = [pg.DEEP_BUDGET if shape == "deep" else 3, 0, 2, 1, 2]
    m = PathModel(g)
    called = _called(m, len(budgets), 5)
    want, want_out, V = recombination_margins_budgets_np(m, budgets, called)
    got, out, Vp = recombination_margins_budgets_np(PathModel(gp), budgets, pg.remap_called(called, new_id))
    assert np.array_equal(Vp, V) and V[0] != NEG_INF
    for q in range(len(budgets)):
        assert np.array_equal(got[q], remap_rows(want[q], new_id)), (shape, q)
    assert np.array_equal(out, want_out)
    ids = got[:, :, 4:]
    assert not pg.pad_mask(gp, new_id)[ids[ids >= 0]].any()                 # no pad is in a record

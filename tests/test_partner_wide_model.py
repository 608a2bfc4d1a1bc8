"""CPU: the shapes of tests/partner_wide_shapes.py stay what the tests of the device-memory route (option partner_wide) need them to
be -- buildable, beyond the 16,384 cells of the LDS route and within the 2^24 of the other, with reachable and, where a test counts
on them, unreachable queries.  A later change to tests/graphgen.py that moved a shape to the other side of the limit, or emptied its
answers, would leave those GPU tests passing on nothing."""
import numpy as np
import pytest

import graphgen
from partner_wide_shapes import MAX_CELLS, SHAPES, WIDE_MAX_CELLS, marginals_ref, partner_ref, shape
from paths_model import NEG_INF

# shape -> (which model answers it here, the shape must hold an unreachable query, budgets on either side of the LDS limit)
EXPECT = {"over_one_row": ("partner", False, True), "wide1100": ("partner", False, True), "long_rows": ("partner", True, False),
          "long_rows_short": ("marginals", True, False)}


@pytest.mark.parametrize("name", list(SHAPES))
def test_shape_is_on_its_side_of_the_limit(name):
    g, m, given, budgets = shape(name)
    _, _, widest, cells = SHAPES[name]
    widths = np.diff(g.level_off)
    assert int(widths.max()) == widest and widest * (int(budgets.max()) + 1) == cells
    assert MAX_CELLS < cells <= WIDE_MAX_CELLS and widest <= 32767
    assert all(m.check_path(p) is None for p in given) and len(given) == len(budgets)
    if name == "over_one_row":
        assert cells - MAX_CELLS == 128 and (widths[1:-1] == 129).all()        # exactly one row of 128 planes past the limit
    if name == "wide1100":
        assert (widths[1:-1] == 1100).all() and widest > 1024                  # wider than the in-edge stage
    if name.startswith("long_rows"):
        assert int(budgets.max()) + 1 > 1024 and widths[1:-1].min() >= 12      # rows longer than any workgroup
    which, unreachable, mixed = EXPECT[name]
    within = widest * (budgets.astype(np.int64) + 1) <= MAX_CELLS
    assert (~within).any() and (within.any() or not mixed)
    values = partner_ref(name)[4] if which == "partner" else marginals_ref(name)[5][:, -1]     # (the sink's marginal is the partner's value)
    reach = values != NEG_INF
    assert reach.any() and len(set(values[reach].tolist())) >= 3
    assert (~reach).any() or not unreachable


def test_long_rows_budget_binds():
    """the partners of the two largest budgets use every recombination they may; 600 and 0 reach nothing"""
    g, m, given, budgets, values, partners = partner_ref("long_rows")
    assert budgets.tolist() == [1100, 1100, 1050, 600, 0]
    assert [m.recombinations(p) for p in partners[:3]] == [1100, 1100, 1050]
    assert (values[:3] != NEG_INF).all() and (values[3:] == NEG_INF).all() and (partners[3:] == -1).all()


def test_long_rows_short_answers_on_either_side():
    g, m, given, budgets, records, M = marginals_ref("long_rows_short")
    assert budgets.tolist() == [1100, 1100, 20, 5, 0, 1030]
    assert (M[:, -1] != NEG_INF).tolist() == [True, True, True, False, False, True]
    assert (M[3:5] == NEG_INF).all() and (records[3:5, :, 0] == -1).all()


def test_call_margins_graph_is_beyond_the_limit_at_any_answer():
    """7 levels: a path has at most 6 recombinations, so each partner budget of the answer at R = 79 is at least 73"""
    g = graphgen.random_levelized(8826, n_levels=7, max_width=260, min_width=260, R=79, extra_edges=0.2)
    assert g.n_levels == 7 and int(np.diff(g.level_off).max()) == 260 and g.R == 79
    assert 260 * (79 - 6 + 1) == 19240 > MAX_CELLS

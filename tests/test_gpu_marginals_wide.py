"""-m gpu: dg_dp_partner_marginals on the device-memory route (option partner_wide): the forward kernel reads the previous level back
from the values it stores, the backward kernel keeps its two level states in device memory and scatters with global atomics.

Integers only: every comparison is exact.  Forced (partner_wide = 2) on the cases of tests/test_gpu_marginals.py the route must give
what tests/marginals_model.py gives and what the LDS route gives in the same process; beyond the 16,384 cells (partner_wide = 1,
the shapes of tests/partner_wide_shapes.py) there is the model, and dg_dp_best_partners on the same route."""
import numpy as np
import pytest

import test_gpu_marginals as tm
from dipgenie_amd import capi
from partner_wide_shapes import SHAPES, marginals_ref
from paths_model import NEG_INF

pytestmark = pytest.mark.gpu


def _footprint(g, widest, bmax):
    """bytes of one query in a slab on the device-memory route, as include/dipgenie_hip.h states them: the LDS route's plus the state"""
    return tm._footprint(g, bmax) + 8 * widest * (bmax + 1)


def _check(levels, values, records, M, tag):
    bad = np.argwhere(values != M)
    assert bad.size == 0, (tag, bad[:5], values[tuple(bad[:5].T)], M[tuple(bad[:5].T)])
    bad = np.argwhere((tm._rows(levels) != records).any(axis=-1))
    assert bad.size == 0, (tag, bad[:5], tm._rows(levels)[tuple(bad[:5].T)], records[tuple(bad[:5].T)])


@pytest.mark.parametrize("name", list(tm.CASES))
def test_forced_route_equals_model_and_lds_route(gpu_ctx, name):
    g, m, given, budgets, records, M = tm._case(name)
    widest = int(np.diff(g.level_off).max())
    assert (M[:, -1] != NEG_INF).any() and len(given) % 7 != 0
    gpu_ctx.dp_load_graph(g)
    lds_levels, lds_values = gpu_ctx.dp_partner_marginals(given, budgets, want_vertices=True)
    assert gpu_ctx.dp_partner_route() == (1, widest * (int(budgets.max()) + 1))
    for per_slab in (None, 7, 1):
        sub = slice(None) if per_slab != 1 else slice(0, 9)
        bmax = int(budgets[sub].max())
        opts = {"partner_slab_bytes": per_slab * _footprint(g, widest, bmax)} if per_slab else {}
        with gpu_ctx.dp_options(partner_wide=2, **opts):
            levels, values = gpu_ctx.dp_partner_marginals(given[sub], budgets[sub], want_vertices=True)
            assert gpu_ctx.dp_partner_route() == (2, widest * (bmax + 1))
            levels2, none = gpu_ctx.dp_partner_marginals(given[sub], budgets[sub])                # vertex_values = NULL
        _check(levels, values, records[sub], M[sub], (name, per_slab))
        assert np.array_equal(levels, lds_levels[sub]) and np.array_equal(values, lds_values[sub])
        assert none is None and np.array_equal(levels2, levels)


@pytest.mark.parametrize("name", ["over_one_row", "wide1100", "long_rows_short"])
def test_beyond_the_lds_limit(gpu_ctx, name):
    g, m, given, budgets, records, M = marginals_ref(name)
    _, _, widest, cells = SHAPES[name]
    gpu_ctx.dp_load_graph(g)
    with pytest.raises(capi.DgError, match=rf"rc=-5.*\b{widest}\b.*\b{int(budgets.max()) + 1}\b.*16384"):       # partner_wide = 0
        gpu_ctx.dp_partner_marginals(given, budgets)
    with gpu_ctx.dp_options(partner_wide=1):
        levels, values = gpu_ctx.dp_partner_marginals(given, budgets, want_vertices=True)
        assert gpu_ctx.dp_partner_route() == (2, cells)
        # no model: dg_dp_best_partners on the same route, whose value is the best marginal of every level
        rec, _ = gpu_ctx.dp_best_partners(given, budgets, want_paths=False)
        assert gpu_ctx.dp_partner_route() == (2, cells)
    _check(levels, values, records, M, name)
    assert np.array_equal(levels["best_value"], np.repeat(rec["value"][:, None], g.n_levels, axis=1))
    dead = rec["value"] == NEG_INF
    assert (~dead).any() and (values[dead] == NEG_INF).all() and (levels["best_vertex"][dead] == -1).all()
    if name == "long_rows_short":
        assert dead.tolist() == [False, False, False, True, True, False]


def test_forced_route_sampled_paths_bound_the_marginals_from_below(gpu_ctx):
    """no model: tests/test_gpu_marginals.py's check against sampled partner paths, on the device-memory route"""
    with gpu_ctx.dp_options(partner_wide=2):
        tm.test_sampled_paths_bound_the_marginals_from_below(gpu_ctx)
        assert gpu_ctx.dp_partner_route()[0] == 2

"""-m gpu: dg_dp_best_partners on the device-memory route (option partner_wide): the two level states of a query in device memory
instead of LDS, so that widest level x (budget + 1) may exceed 16,384 cells.

Integers only: every comparison is exact.  Forced (partner_wide = 2) on every case of tests/test_gpu_partner.py, the route must give
what tests/partner_model.py gives and what the LDS route gives in the same process; beyond the limit (partner_wide = 1, the shapes
of tests/partner_wide_shapes.py, which tests/test_partner_wide_model.py keeps beyond it) there is only the model."""
import numpy as np
import pytest

import test_gpu_partner as tp
from dipgenie_amd import capi
from partner_wide_shapes import MAX_CELLS, SHAPES, partner_records, partner_ref
from paths_model import NEG_INF

pytestmark = pytest.mark.gpu


def _footprint(g, widest, bmax):
    """bytes of one query in a slab on the device-memory route, as include/dipgenie_hip.h states them: the LDS route's plus the state"""
    return tp._footprint(g, bmax) + 8 * widest * (bmax + 1)


def _check(got, want, partners, tag):
    rec, rows = got
    bad = np.flatnonzero((tp._rows(rec) != want).any(axis=1))
    assert bad.size == 0, (tag, bad[:5], tp._rows(rec)[bad[:5]], want[bad[:5]])
    bad = np.flatnonzero((rows != partners).any(axis=1))
    assert bad.size == 0, (tag, bad[:5])


@pytest.mark.parametrize("name", list(tp.CASES))
def test_forced_route_equals_model_and_lds_route(gpu_ctx, name):
    g, m, given, budgets, values, partners = tp._case(name)
    n = len(given)
    widest = int(np.diff(g.level_off).max())
    want = partner_records(m, given, budgets, values, partners)
    assert (values != NEG_INF).any() and n % 7 != 0
    gpu_ctx.dp_load_graph(g)
    lds = gpu_ctx.dp_best_partners(given, budgets)
    assert gpu_ctx.dp_partner_route() == (1, widest * (int(budgets.max()) + 1))
    for per_slab in (None, 7, 1):                        # all queries in one slab, 7 per slab (the last one short), 1 per slab
        sub = slice(None) if per_slab != 1 else slice(0, 9)
        bmax = int(budgets[sub].max())
        opts = {"partner_slab_bytes": per_slab * _footprint(g, widest, bmax)} if per_slab else {}
        with gpu_ctx.dp_options(partner_wide=2, **opts):
            got = gpu_ctx.dp_best_partners(given[sub], budgets[sub])
            assert gpu_ctx.dp_partner_route() == (2, widest * (bmax + 1))
            rec2, none = gpu_ctx.dp_best_partners(given[sub], budgets[sub], want_paths=False)
        _check(got, want[sub], partners[sub], (name, per_slab))
        assert np.array_equal(got[0], lds[0][sub]) and np.array_equal(got[1], lds[1][sub])
        assert none is None and np.array_equal(rec2, got[0])
    again = gpu_ctx.dp_best_partners(given[:9], budgets[:9])                    # the default is the LDS route again
    assert gpu_ctx.dp_partner_route() == (1, widest * (int(budgets[:9].max()) + 1))
    assert np.array_equal(again[0], lds[0][:9]) and np.array_equal(again[1], lds[1][:9])


def test_forced_route_maximum_over_given_paths_is_the_plane_of_the_sweep(gpu_ctx):
    """no model: tests/test_gpu_partner.py's check against the sweep, every partner call on the device-memory route"""
    with gpu_ctx.dp_options(partner_wide=2):
        tp.test_maximum_over_given_paths_is_the_plane_of_the_sweep(gpu_ctx)
        assert gpu_ctx.dp_partner_route()[0] == 2


@pytest.mark.parametrize("name", ["over_one_row", "wide1100", "long_rows"])
def test_beyond_the_lds_limit(gpu_ctx, name):
    g, m, given, budgets, values, partners = partner_ref(name)
    _, _, widest, cells = SHAPES[name]
    want = partner_records(m, given, budgets, values, partners)
    gpu_ctx.dp_load_graph(g)
    before = gpu_ctx.dp_partner_route()
    with pytest.raises(capi.DgError, match=rf"rc=-5.*\b{widest}\b.*\b{int(budgets.max()) + 1}\b.*16384"):       # partner_wide = 0
        gpu_ctx.dp_best_partners(given, budgets)
    assert gpu_ctx.dp_partner_route() == before          # a call that fails before choosing a route leaves it
    with gpu_ctx.dp_options(partner_wide=1):
        got = gpu_ctx.dp_best_partners(given, budgets)
        assert gpu_ctx.dp_partner_route() == (2, cells)
        within = np.flatnonzero(widest * (budgets.astype(np.int64) + 1) <= MAX_CELLS)
        if name != "long_rows":
            # budgets on either side of the limit went up together above: one route per call.  Those within it alone take the LDS route
            assert 0 < within.size < len(budgets)
            few = gpu_ctx.dp_best_partners(given[within], budgets[within])
            assert gpu_ctx.dp_partner_route() == (1, widest * (int(budgets[within].max()) + 1))
            _check(few, want[within], partners[within], (name, "within"))
    _check(got, want, partners, name)
    if name == "long_rows":                              # the budget binds, and rows of 1,101 planes are longer than the workgroup
        assert got[0]["r2"][:3].tolist() == [1100, 1100, 1050] and (got[0]["value"][3:] == NEG_INF).all() and (got[1][3:] == -1).all()


def test_the_wide_cap(gpu_ctx):
    """widest level 129 x (200,000 + 1) is beyond 2^24 cells: refused before anything is allocated or written, both numbers named"""
    g, m, given, budgets, _, _ = partner_ref("over_one_row")
    gpu_ctx.dp_load_graph(g)
    bd = np.array([3, 200000, 200000], np.int32)
    gv = np.ascontiguousarray(given[:3])
    out = np.full(12, -7, np.int32).view(capi.PARTNER)
    part = np.full((3, g.n_levels), -7, np.int32)
    for mode in (1, 2):
        with gpu_ctx.dp_options(partner_wide=mode):
            before = gpu_ctx.dp_partner_route()
            with pytest.raises(capi.DgError, match=r"rc=-5.*dg_dp_best_partners.*query 1\b.*\b129\b.*\b200001\b"):
                gpu_ctx.dp_best_partners(gv, bd)
            assert capi.lib.dg_dp_best_partners(gpu_ctx.h, gv.ctypes.data, 3, bd.ctypes.data, part.ctypes.data, out.ctypes.data) == -5
            assert (out.view(np.int32) == -7).all() and (part == -7).all() and gpu_ctx.dp_partner_route() == before
            with pytest.raises(capi.DgError, match=r"rc=-5.*dg_dp_partner_marginals.*query 1\b.*\b129\b.*\b200001\b"):
                gpu_ctx.dp_partner_marginals(gv, bd)
            assert gpu_ctx.dp_partner_route() == before
    # the option is clamped to 0..2
    with gpu_ctx.dp_options(partner_wide=7):
        assert gpu_ctx.dp_get_option("partner_wide") == 2
    with gpu_ctx.dp_options(partner_wide=-3):
        assert gpu_ctx.dp_get_option("partner_wide") == 0
    assert gpu_ctx.dp_get_option("partner_wide") == 0

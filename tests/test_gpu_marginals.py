"""-m gpu: dg_dp_partner_marginals / Context.dp_partner_marginals -- what the best partner through every vertex is worth, and per
level the best vertex, the best of the others and the margin between them.

Integers only: every comparison is exact.  The yardstick is tests/marginals_model.py, itself pinned to brute force by
tests/test_marginals_model.py; the tests against dg_dp_best_partners and against sampled paths need no model at all."""
import numpy as np
import pytest

import graphgen
from dipgenie_amd import capi
from marginals_model import partner_marginals_batch
from paths_model import NEG_INF, PathModel
from test_gpu_partner import CASES, MAX_CELLS, _given

pytestmark = pytest.mark.gpu

_REF = {}
FIELDS = ("best_vertex", "best_value", "second_vertex", "second_value")


def _footprint(g, bmax):
    """bytes of one query in a slab, as include/dipgenie_hip.h states them"""
    return 4 * g.n_vertices * (bmax + 1) + 2 * len(g.out_dst) + 4 * g.n_vertices + 20 * g.n_levels


def _case(name):
    """graph, model, given paths, budgets (those of tests/test_gpu_partner.py), the model's level records and marginals -- computed once"""
    if name not in _REF:
        make, b_max, n = CASES[name]
        g = make()
        m = PathModel(g)
        given, _ = _given(m, 41, n)
        budgets = np.random.default_rng(42).integers(0, (g.R if b_max is None else b_max) + 1, n).astype(np.int32)
        if name == "full_lds":
            budgets[:4] = 127
        records, M = partner_marginals_batch(m, given, budgets)
        _REF[name] = (g, m, given, budgets, records, M)
    return _REF[name]


def _rows(levels):
    return np.stack([levels[f] for f in FIELDS], axis=-1)


@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_model(gpu_ctx, name):
    g, m, given, budgets, records, M = _case(name)
    n = len(given)
    widths = np.diff(g.level_off)
    if name == "two_levels":
        assert g.n_levels == 2
    if name == "wide":
        assert widths.max() * (budgets.max() + 1) > 256
    if name == "fat1100":
        assert np.bincount(g.out_dst, minlength=g.n_vertices).max() > 1024
    if name == "full_lds":
        assert widths.max() * (budgets.max() + 1) == MAX_CELLS
    reach = M[:, -1] != NEG_INF
    assert reach.any() and (name in ("two_levels", "full_lds") or len(set(budgets.tolist())) >= 3)
    if name == "parallel66":
        assert reach.any() and (~reach).any()            # budgets either side of reachability
    gpu_ctx.dp_load_graph(g)                             # no run before the call
    for per_slab in (None, 7, 1):
        sub = slice(None) if per_slab != 1 else slice(0, 9)
        opts = {"partner_slab_bytes": per_slab * _footprint(g, int(budgets[sub].max()))} if per_slab else {}   # 7: the last slab is short; a query is sized for the call's largest budget
        with gpu_ctx.dp_options(**opts):
            levels, values = gpu_ctx.dp_partner_marginals(given[sub], budgets[sub], want_vertices=True)
            levels2, none = gpu_ctx.dp_partner_marginals(given[sub], budgets[sub])                 # vertex_values = NULL
        assert n % 7 != 0
        assert levels.shape == (len(given[sub]), g.n_levels) and values.shape == (len(given[sub]), g.n_vertices)
        bad = np.argwhere(values != M[sub])
        assert bad.size == 0, (name, per_slab, bad[:5], values[tuple(bad[:5].T)], M[sub][tuple(bad[:5].T)])
        bad = np.argwhere((_rows(levels) != records[sub]).any(axis=-1))
        assert bad.size == 0, (name, per_slab, bad[:5], _rows(levels)[tuple(bad[:5].T)], records[sub][tuple(bad[:5].T)])
        assert none is None and np.array_equal(levels2, levels)


@pytest.mark.parametrize("name", ["levels65", "wide"])
def test_against_best_partners(gpu_ctx, name):
    """no model: the level records and the marginals against dg_dp_best_partners on the same queries"""
    g, m, given, budgets, _, _ = _case(name)
    n, nV = len(given), g.n_vertices
    gpu_ctx.dp_load_graph(g)
    rec, partner = gpu_ctx.dp_best_partners(given, budgets)
    levels, values = gpu_ctx.dp_partner_marginals(given, budgets, want_vertices=True)
    value = rec["value"]
    dead = value == NEG_INF
    assert (dead.any() or name != "levels65") and (~dead).any()          # (every budget of `wide` is reachable)
    assert np.array_equal(levels["best_value"], np.repeat(value[:, None], g.n_levels, axis=1))
    assert (values <= value[:, None]).all()
    live = np.flatnonzero(~dead)
    assert (values[live[:, None], partner[live]] == value[live, None]).all()
    assert (values[dead] == NEG_INF).all()
    for f in FIELDS:
        assert (levels[f][dead] == (-1 if f.endswith("vertex") else NEG_INF)).all(), f
    # a reachable query: the best vertex is in its level and holds best_value, the second another vertex of the level worth no more
    lv = levels[live]
    lo, hi = g.level_off[:-1][None, :], g.level_off[1:][None, :]
    assert ((lv["best_vertex"] >= lo) & (lv["best_vertex"] < hi)).all()
    assert (values[live[:, None], lv["best_vertex"]] == lv["best_value"]).all()
    has2 = lv["second_vertex"] >= 0
    assert has2.any() and ((lv["second_vertex"] != lv["best_vertex"]) & (lv["second_value"] <= lv["best_value"]))[has2].all()
    assert (lv["second_value"][~has2] == NEG_INF).all()
    # every M is non-decreasing in the budget
    some = given[:40]
    nb = int(budgets.max()) + 2
    assert widths_ok(g, nb)
    _, vb = gpu_ctx.dp_partner_marginals(np.repeat(some, nb, axis=0), np.tile(np.arange(nb, dtype=np.int32), len(some)), want_vertices=True)
    vb = vb.reshape(len(some), nb, nV)
    assert (np.diff(vb, axis=1) >= 0).all() and (np.diff(vb, axis=1) > 0).any()


def widths_ok(g, n_planes):
    return int(np.diff(g.level_off).max()) * n_planes <= MAX_CELLS


def test_sampled_paths_bound_the_marginals_from_below(gpu_ctx):
    """no model: a partner path q with r(q) recombinations is one candidate of every vertex it passes through at budget r(q)"""
    g, m, given, _, _, _ = _case("levels65")
    q, rq = m.sample_paths(np.random.default_rng(77), 200, 0.8)
    assert len(set(rq.tolist())) >= 3 and widths_ok(g, int(rq.max()) + 1)
    gpu_ctx.dp_load_graph(g)
    scored = gpu_ctx.dp_score_paths(np.ascontiguousarray(np.stack([given, q], axis=1)))
    assert np.array_equal(scored["r2"], rq)
    _, values = gpu_ctx.dp_partner_marginals(given, rq.astype(np.int32), want_vertices=True)
    through = values[np.arange(200)[:, None], q]
    assert (through >= scored["value"][:, None]).all(), np.argwhere(through < scored["value"][:, None])[:5]
    assert (through > scored["value"][:, None]).any()    # and the sample is not the optimum everywhere


def test_errors(gpu_ctx):
    g, m, given, budgets, records, M = _case("levels65")
    L, n, nV = g.n_levels, len(given), g.n_vertices
    fresh = capi.Context(0)
    try:
        with pytest.raises(capi.DgError, match=r"rc=-6.*no graph loaded"):
            fresh.dp_partner_marginals(given, budgets)
    finally:
        fresh.close()
    gpu_ctx.dp_load_graph(g)
    call = capi.lib.dg_dp_partner_marginals
    levels, values = gpu_ctx.dp_partner_marginals(np.zeros((0, L), np.int32), np.zeros(0, np.int32), want_vertices=True)       # n = 0
    assert levels.shape == (0, L) and values.shape == (0, nV)
    assert call(gpu_ctx.h, None, 0, None, None, None) == 0
    out = np.full((n, L, 4), -7, np.int32)
    vals = np.full((n, nV), -7, np.int32)
    gp, bp = given.ctypes.data, budgets.ctypes.data
    assert call(gpu_ctx.h, None, 4, bp, out.ctypes.data, vals.ctypes.data) == -1
    assert call(gpu_ctx.h, gp, 4, None, out.ctypes.data, vals.ctypes.data) == -1
    assert call(gpu_ctx.h, gp, 4, bp, None, vals.ctypes.data) == -1
    assert call(gpu_ctx.h, gp, -1, bp, out.ctypes.data, vals.ctypes.data) == -1

    def untouched():
        return (out == -7).all() and (vals == -7).all()

    def fails(gv, bd, rc, pattern):
        gv, bd = np.ascontiguousarray(gv, np.int32), np.ascontiguousarray(bd, np.int32)
        with pytest.raises(capi.DgError, match=pattern):
            gpu_ctx.dp_partner_marginals(gv, bd, want_vertices=True)
        assert call(gpu_ctx.h, gv.ctypes.data, len(gv), bd.ctypes.data, out.ctypes.data, vals.ctypes.data) == rc
        assert untouched()

    assert untouched()
    with gpu_ctx.dp_options(partner_slab_bytes=7 * _footprint(g, int(budgets.max()))):           # 29 slabs
        neg = budgets.copy()
        neg[123] = -1
        neg[150] = -3
        fails(given, neg, -1, r"rc=-1.*dg_dp_partner_marginals.*query 123\b.*budget -1")
        # three bad queries in three slabs: the first (query, level) is the one named, whatever its kind
        bad = given.copy()
        bad[180, 5] = g.level_off[9]                     # a vertex of another level
        bad[100, 40] = 2 ** 31 - 1
        hop_l = next(l for l in range(L - 1, 0, -1) if g.level_off[l + 1] - g.level_off[l] > len(m.succ[int(given[30, l - 1])]))
        hop_v = next(v for v in range(g.level_off[hop_l], g.level_off[hop_l + 1]) if v not in m.succ[int(given[30, hop_l - 1])])
        bad[30, hop_l] = hop_v
        assert m.check_path(bad[30]) == (hop_l, "edge")
        fails(bad, budgets, -1, rf"rc=-1.*query 30 level {hop_l}\b.*no edge {int(bad[30, hop_l - 1])} -> {hop_v}")
        bad[30] = given[30]
        fails(bad, budgets, -1, r"rc=-1.*query 100 level 40\b.*not in that level")
        bad[100] = given[100]
        bad[180, 3] = -5
        fails(bad, budgets, -1, r"rc=-1.*query 180 level 3\b.*not in that level")
        # and the same call with valid paths succeeds, into the caller's arrays
        assert call(gpu_ctx.h, gp, n, bp, out.ctypes.data, vals.ctypes.data) == 0
        assert np.array_equal(out, records) and np.array_equal(vals, M)
    with pytest.raises(ValueError):
        gpu_ctx.dp_partner_marginals(given[:, :-1], budgets)
    with pytest.raises(ValueError):
        gpu_ctx.dp_partner_marginals(given, budgets[:-1])
    # an unreachable budget is an answer, not an error
    dead = M[:, -1] == NEG_INF
    assert dead.any()
    levels, values = gpu_ctx.dp_partner_marginals(given, budgets, want_vertices=True)
    assert (values[dead] == NEG_INF).all() and (levels["best_vertex"][dead] == -1).all() and (levels["best_vertex"][~dead] >= 0).all()
    # the cell limit: widest level 200, budget 100
    wide = graphgen.random_levelized(8813, n_levels=4, max_width=200, min_width=200, R=2, extra_edges=0.2)
    mw = PathModel(wide)
    gw, _ = mw.sample_paths(np.random.default_rng(1), 3)
    gpu_ctx.dp_load_graph(wide)
    out = np.full((3, 4, 4), -7, np.int32)
    vals = np.full((3, wide.n_vertices), -7, np.int32)
    fails(gw, [1, 100, 100], -5, r"rc=-5.*query 1\b.*200.*101")
    levels, _ = gpu_ctx.dp_partner_marginals(gw, [1, 80, 0])                                     # 200 x 81 cells fit
    assert (levels["best_value"] >= 0).any()


def test_a_marginals_call_leaves_the_last_run_alone(gpu_ctx):
    g, m, given, budgets, records, M = _case("levels65")
    with gpu_ctx.dp_options(digest=1):
        gpu_ctx.dp_load_graph(g)
        outs = [o.key() for o in gpu_ctx.dp_run_budgets(range(g.R + 1))]
        planes = gpu_ctx.dp_budget_values().copy()
        digest = gpu_ctx.dp_level_digest(g.n_levels).copy()
        assert digest[1:].any()
        got = gpu_ctx.dp_partner_marginals(given, budgets, want_vertices=True)
        assert np.array_equal(got[1], M)
        assert np.array_equal(gpu_ctx.dp_budget_values(), planes)
        assert np.array_equal(gpu_ctx.dp_level_digest(g.n_levels), digest)
        bad = given.copy()
        bad[3, 10] = 0
        with pytest.raises(capi.DgError):
            gpu_ctx.dp_partner_marginals(bad, budgets)
        assert np.array_equal(gpu_ctx.dp_budget_values(), planes)
        assert np.array_equal(gpu_ctx.dp_level_digest(g.n_levels), digest)
        assert [o.key() for o in gpu_ctx.dp_run_budgets(range(g.R + 1))] == outs                  # and the next run answers as before
        assert np.array_equal(gpu_ctx.dp_level_digest(g.n_levels), digest)
        again = gpu_ctx.dp_partner_marginals(given, budgets, want_vertices=True)
        assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1])
        # and dg_dp_best_partners, whose kernels the call shares, still answers the same query
        rec, _ = gpu_ctx.dp_best_partners(given, budgets, want_paths=False)
        assert np.array_equal(rec["value"], M[:, -1])


def test_capi_layout(gpu_ctx):
    assert capi.LEVEL_MARGIN.itemsize == 16 and capi.LEVEL_MARGIN.names == FIELDS
    g, m, given, budgets, records, M = _case("two_levels")
    gpu_ctx.dp_load_graph(g)
    raw = np.full(3 * g.n_levels * 4, -7, np.int32)
    assert capi.lib.dg_dp_partner_marginals(gpu_ctx.h, given.ctypes.data, 3, budgets.ctypes.data, raw.ctypes.data, None) == 0
    assert np.array_equal(raw.reshape(3, g.n_levels, 4), records[:3])       # sizeof(dg_dp_level_margin) == 16: four words per (query, level)

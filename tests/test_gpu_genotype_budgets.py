"""-m gpu: dg_dp_genotype_margins_budgets / Context.dp_genotype_margins_budgets -- genotype margins with one budget per query, from
one joint pass at the largest budget.

Integers only: every comparison is exact.  The yardsticks are tests/genotype_budgets_model.py (pinned to the one-budget models by
tests/test_genotype_budgets_model.py) and the one-budget device calls dp_genotype_margins / dp_genotype_margins_pinned, query by query."""
import numpy as np
import pytest

import graphgen
from call_margins_model import class_arrays
from dipgenie_amd import capi
from genotype_budgets_model import genotype_margins_budgets_np
from paths_model import NEG_INF, PathModel
from pinned_model import FORBID, REQUIRE
from test_gpu_genotype_margins import BUDGETS, FIELDS, MAX_PLANES, MAX_QUERIES, WIDTHS, _rows, _state_bytes
from test_gpu_score_paths import ENUMERABLE
from test_partner_model import enumerable_graph

pytestmark = pytest.mark.gpu

MIXED = [3, 0, 2, 1, 2]                                 # unsorted, with a repeat


def _cells(m, rng, n):
    """[n, 2, L]: per query a different random cell per level; query 0 is a sampled pair of paths"""
    called = np.array([[[rng.integers(m.level_off[l], m.level_off[l + 1]) for l in range(m.L)] for _ in range(2)] for _ in range(n)], np.int32)
    called[0] = np.asarray(m.sample_paths(rng, 2)[0], np.int32)
    return called


def _equals_single_calls(ctx, called, budgets, cls, levels, best, pins=None, tag=None):
    for q, b in enumerate(budgets):
        one, V = ctx.dp_genotype_margins(called[q], b, cls) if pins is None else ctx.dp_genotype_margins_pinned(pins, called[q], b, cls)
        assert best[q] == V and np.array_equal(levels[q], one[0]), (tag, q, b, _rows(levels[q:q + 1]), _rows(one))


def _equals_model(m, called, budgets, cls, levels, best, pins=None, tag=None):
    want, V = genotype_margins_budgets_np(m, called, budgets, cls, pins)
    assert levels.shape == want.shape[:2] and best.dtype == np.int32 and np.array_equal(best, V), (tag, best, V)
    bad = np.argwhere((_rows(levels) != want).any(axis=-1))
    assert bad.size == 0, (tag, bad[:5], _rows(levels)[tuple(bad[:5].T)], want[tuple(bad[:5].T)])


@pytest.mark.parametrize("q", range(len(ENUMERABLE)))
def test_device_equals_model_and_single_calls_on_the_enumerable_graphs(gpu_ctx, q):
    g = enumerable_graph(q)
    m = PathModel(g)
    gpu_ctx.dp_load_graph(g)
    called = _cells(m, np.random.default_rng(140 + q), len(MIXED))
    for kind, cls in enumerate(class_arrays(g, 21 + q)):
        levels, best = gpu_ctx.dp_genotype_margins_budgets(called, MIXED, cls)
        _equals_model(m, called, MIXED, cls, levels, best, tag=(q, kind))
        _equals_single_calls(gpu_ctx, called, MIXED, cls, levels, best, tag=(q, kind))


@pytest.mark.parametrize("w", range(len(WIDTHS)))
def test_device_equals_model_on_prescribed_widths(gpu_ctx, w):
    """budgets 0, 1, 2, 7, 18 in one call: 19 planes, no power of two, more than the graphs' R; parallel edges and unreached vertices"""
    unreached = 0
    for k, p_w1 in enumerate((0.0, 0.3, 1.0)):
        g = graphgen.random_levelized(9100 + 10 * w + k, widths=WIDTHS[w], R=3, p_w1=p_w1, dup_edges=True, extra_edges=1.2, p_colour=0.5)
        m = PathModel(g)
        indeg = np.bincount(g.out_dst, minlength=g.n_vertices)
        unreached += int((indeg[1:] == 0).sum())
        gpu_ctx.dp_load_graph(g)
        called = _cells(m, np.random.default_rng(150 + w), len(BUDGETS))
        for kind, cls in enumerate(class_arrays(g, 31 + w)):
            levels, best = gpu_ctx.dp_genotype_margins_budgets(called, BUDGETS, cls)
            _equals_model(m, called, BUDGETS, cls, levels, best, tag=(w, p_w1, kind))
        # every edge weighs 1: a path has L - 1 recombinations and a pair 2 (L - 1), between 4 and 10 here.  So the budget-0 query has no
        # answer and the budget-18 query has one on every graph, in the same call; which of 1, 2 and 7 have one depends on L (the model says)
        if p_w1 == 1.0:
            assert best[0] == NEG_INF and best[4] != NEG_INF
            want = np.concatenate([called[0].T, np.broadcast_to(np.array([NEG_INF, -1, -1, NEG_INF]), (g.n_levels, 4))], axis=-1)
            assert np.array_equal(_rows(levels)[0], want)
    if max(WIDTHS[w]) >= 63:
        assert unreached >= 1


def test_wider_than_any_tile_equals_the_single_calls(gpu_ctx):
    g = graphgen.random_levelized(9200, widths=[1, 130, 300, 129, 1], R=18, p_w1=0.3, extra_edges=1.5, p_colour=0.5)
    m = PathModel(g)
    gpu_ctx.dp_load_graph(g)
    budgets = [0, 2, 7]
    called = _cells(m, np.random.default_rng(9), len(budgets))
    cls = class_arrays(g, 41)[2]
    levels, best = gpu_ctx.dp_genotype_margins_budgets(called, budgets, cls)
    _equals_single_calls(gpu_ctx, called, budgets, cls, levels, best)
    assert (best != NEG_INF).any() and (levels["alt_vertex1"][:, 1:-1] >= 0).any()


def test_the_most_queries_equal_their_single_calls(gpu_ctx):
    g = graphgen.random_levelized(9501, widths=[1, 4, 6, 3, 1], R=3, p_colour=0.5)
    m = PathModel(g)
    gpu_ctx.dp_load_graph(g)
    rng = np.random.default_rng(16)
    called = _cells(m, rng, MAX_QUERIES + 1)
    budgets = np.arange(MAX_QUERIES + 1, dtype=np.int32) % 5
    levels, best = gpu_ctx.dp_genotype_margins_budgets(called[:MAX_QUERIES], budgets[:MAX_QUERIES])
    _equals_single_calls(gpu_ctx, called[:MAX_QUERIES], budgets[:MAX_QUERIES], None, levels, best)
    with pytest.raises(capi.DgError, match=rf"rc=-5.*dg_dp_genotype_margins_budgets.*\b{MAX_QUERIES + 1}\b.*\b{MAX_QUERIES}\b"):
        gpu_ctx.dp_genotype_margins_budgets(called, budgets)
    # one query, a scalar budget: exactly dp_genotype_margins
    one, V1 = gpu_ctx.dp_genotype_margins_budgets(called[3], 2)
    want, V = gpu_ctx.dp_genotype_margins(called[3], 2)
    assert one.shape == (1, g.n_levels) and V1.tolist() == [V] and np.array_equal(one, want)


def _pin_cases():
    out = []
    for q in (1, 3):
        g = enumerable_graph(q)
        out.append((f"enumerable {q}", g))
    out.append(("prescribed", graphgen.random_levelized(9130, widths=[1, 3, 64, 65, 2, 1], R=3, p_w1=0.3, dup_edges=True, extra_edges=1.2, p_colour=0.5)))
    return out


@pytest.mark.parametrize("which", range(3))
def test_pins(gpu_ctx, which):
    tag, g = _pin_cases()[which]
    m = PathModel(g)
    gpu_ctx.dp_load_graph(g)
    rng = np.random.default_rng(170 + which)
    budgets = MIXED if which < 2 else [7, 0, 2, 1, 2]
    called = _cells(m, rng, len(budgets))
    wide = 1 + int(np.argmax(np.diff(g.level_off)[1:-1]))
    a0, a1 = int(g.level_off[wide]), int(g.level_off[wide + 1])
    l2 = 1 if wide != 1 else g.n_levels - 2
    c0 = int(g.level_off[l2])
    sets = {
        "require": [(wide, a0, -1, REQUIRE), (wide, a1 - 1, a0, REQUIRE)],
        "forbid": [(wide, -1, a0, FORBID), (l2, c0, -1, FORBID)],
        "both": [(wide, a0, -1, REQUIRE), (wide, -1, a1 - 1, REQUIRE), (l2, c0, c0, FORBID)],
        "unsatisfiable": [(wide, a0, -1, REQUIRE), (wide, a0, -1, FORBID)],
    }
    cls = class_arrays(g, 61 + which)[2]
    for name, pins in sets.items():
        for c in (None, cls):
            levels, best = gpu_ctx.dp_genotype_margins_budgets(called, budgets, c, pins=pins)
            assert gpu_ctx.dp_genotype_pin_stats() == dict(pins=len(pins), mask_launches=2 * len({p[0] for p in pins})), (tag, name)
            _equals_model(m, called, budgets, c, levels, best, pins=pins, tag=(tag, name))
        _equals_single_calls(gpu_ctx, called, budgets, cls, levels, best, pins=pins, tag=(tag, name))
        if name == "unsatisfiable":
            assert (best == NEG_INF).all() and (levels["value"] == NEG_INF).all() and (levels["alt_vertex1"] == -1).all()
    # no pins, given as an empty list: the unpinned call, output for output and statistic for statistic
    want = gpu_ctx.dp_genotype_margins_budgets(called, budgets, cls)
    stats = gpu_ctx.dp_genotype_stats()
    assert gpu_ctx.dp_genotype_pin_stats() == dict(pins=0, mask_launches=0)
    for none in ([], np.zeros((0, 4), np.int32)):
        gpu_ctx.dp_genotype_margins_budgets(called, budgets, cls, pins=sets["forbid"])        # so that the zeros below are this call's
        got = gpu_ctx.dp_genotype_margins_budgets(called, budgets, cls, pins=none)
        assert all(np.array_equal(x, y) for x, y in zip(want, got))
        assert gpu_ctx.dp_genotype_stats() == stats and gpu_ctx.dp_genotype_pin_stats() == dict(pins=0, mask_launches=0)


def test_segments_change_nothing(gpu_ctx):
    g = graphgen.random_levelized(9130, widths=WIDTHS[2], R=3, p_w1=0.3, dup_edges=True, extra_edges=1.2, p_colour=0.5)
    m = PathModel(g)
    gpu_ctx.dp_load_graph(g)
    L = g.n_levels
    budgets = [7, 0, 2, 1, 2]
    called = _cells(m, np.random.default_rng(13), len(budgets))
    cls = class_arrays(g, 51)[2]
    found = gpu_ctx.dp_get_option("joint_state_bytes")
    ragged = int(2.5 * _state_bytes(g, max(budgets)).mean())
    got = {}
    for name, nbytes in (("every level", 1), ("ragged", ragged), ("default", 0)):
        with gpu_ctx.dp_options(joint_state_bytes=nbytes):
            got[name] = gpu_ctx.dp_genotype_margins_budgets(called, budgets, cls)
        got[name + " stats"] = gpu_ctx.dp_genotype_stats()
    for name in ("ragged", "default"):
        for x, y in zip(got["every level"], got[name]):
            assert np.array_equal(x, y), name
    assert got["every level stats"]["n_segments"] == L and got["every level stats"]["levels_twice"] == 0
    assert 1 < got["ragged stats"]["n_segments"] < L and got["ragged stats"]["levels_twice"] >= 1
    assert got["default stats"]["n_segments"] == 1 and got["default stats"]["levels_twice"] == 0
    assert gpu_ctx.dp_get_option("joint_state_bytes") == found
    _equals_model(m, called, budgets, cls, *got["ragged"])


def test_one_pass_by_the_calls_own_stats(gpu_ctx):
    """five distinct budgets: the segments, the levels swept twice and -- but for nothing -- the launches of ONE call at the largest"""
    g = graphgen.random_levelized(9130, widths=WIDTHS[2], R=3, p_w1=0.3, dup_edges=True, extra_edges=1.2, p_colour=0.5)
    m = PathModel(g)
    gpu_ctx.dp_load_graph(g)
    called = _cells(m, np.random.default_rng(14), len(BUDGETS))
    ragged = int(2.5 * _state_bytes(g, max(BUDGETS)).mean())
    for nbytes in (0, ragged):
        with gpu_ctx.dp_options(joint_state_bytes=nbytes):
            gpu_ctx.dp_genotype_margins(called[0], max(BUDGETS))
            single = gpu_ctx.dp_genotype_stats()
            gpu_ctx.dp_genotype_margins_budgets(called, BUDGETS)
            multi = gpu_ctx.dp_genotype_stats()
        assert multi["n_segments"] == single["n_segments"] and multi["levels_twice"] == single["levels_twice"]
        assert 3 * g.n_levels <= multi["launches"] < 2 * single["launches"], (multi, single)
        assert multi["entries"] == 0 and multi["staging_copies"] == 0 and multi["peak_bytes"] >= int(_state_bytes(g, max(BUDGETS)).max())
    assert single["levels_twice"] >= 1


def test_the_call_leaves_the_run_alone(gpu_ctx):
    g = graphgen.random_levelized(9401, n_levels=30, max_width=9, R=4, p_colour=0.5)
    m = PathModel(g)
    gpu_ctx.dp_load_graph(g)
    rng = np.random.default_rng(15)
    budgets = list(range(g.R + 1))
    called = _cells(m, rng, 3)
    pins = [(3, int(g.level_off[3]), -1, FORBID)]

    def snapshot():
        return ([(o.value, o.s_het, tuple(o.p1), tuple(o.p2)) for o in outs], gpu_ctx.dp_budget_values().tolist(), [gpu_ctx.dp_answer_paths(b).tolist() for b in budgets],
                gpu_ctx.dp_pin_stats(), [getattr(gpu_ctx.dp_timing(), f) for f, _ in capi.DpTiming._fields_])

    for run in (lambda: gpu_ctx.dp_run_budgets(budgets), lambda: gpu_ctx.dp_run_pinned([(5, -1, int(g.level_off[5]), FORBID)], budgets)):
        outs = run()
        before = snapshot()
        first = gpu_ctx.dp_genotype_margins_budgets(called, [0, g.R, g.R + 3]), gpu_ctx.dp_genotype_margins_budgets(called, [g.R, 1, 1], pins=pins)
        assert snapshot() == before
        again = gpu_ctx.dp_genotype_margins_budgets(called, [0, g.R, g.R + 3]), gpu_ctx.dp_genotype_margins_budgets(called, [g.R, 1, 1], pins=pins)
        assert all(np.array_equal(x, y) for one, two in zip(first, again) for x, y in zip(one, two))
        assert snapshot() == before
    outs = gpu_ctx.dp_run_budgets(budgets)              # the unpinned run's answers, called at their own budgets, are worth the planes
    planes = gpu_ctx.dp_budget_values()
    fit = [b for b in budgets if planes[b] != NEG_INF]
    levels, best = gpu_ctx.dp_genotype_margins_budgets(np.stack([gpu_ctx.dp_answer_paths(b) for b in fit]), fit)
    assert np.array_equal(best, planes[fit]) and (levels["value"] == best[:, None]).all() and (levels["value"] >= levels["alt_value"]).all()


def test_errors_and_layout(gpu_ctx):
    g = graphgen.random_levelized(9501, widths=[1, 4, 6, 3, 1], R=3, p_colour=0.5)
    m = PathModel(g)
    L = g.n_levels
    NAME = "dg_dp_genotype_margins_budgets"
    call = capi.lib.dg_dp_genotype_margins_budgets
    fresh = capi.Context(0)
    try:
        with pytest.raises(capi.DgError, match=rf"rc=-6.*{NAME}: no graph loaded"):
            fresh.dp_genotype_margins_budgets(np.zeros((2, L), np.int32), 0)
    finally:
        fresh.close()
    gpu_ctx.dp_load_graph(g)
    called = _cells(m, np.random.default_rng(6), 3)
    n = len(called)
    budgets = np.array([2, 0, 3], np.int32)
    out = np.full((n, L, 8), -7, np.int32)
    best = np.full(n, -7, np.int32)
    gpu_ctx.dp_genotype_margins_budgets(called, budgets)
    stats = gpu_ctx.dp_genotype_stats()

    def raw(p=called, b=budgets, count=n, lv=out, bv=best, pins=None, n_pins=0):
        ptr = lambda a: a.ctypes.data if a is not None else None
        return call(gpu_ctx.h, ptr(pins), n_pins, ptr(p), ptr(b), count, None, ptr(lv), ptr(bv))

    def refused(rc, start, **kw):
        got = raw(**kw)
        msg = capi.lib.dg_last_error().decode()
        return got == rc and msg.startswith(f"{NAME}: {start}") and (out == -7).all() and (best == -7).all() or pytest.fail(f"{kw.keys()}: rc {got}, {msg}")

    bad = called.copy()
    bad[1, 1, 2] = g.level_off[3]                        # query 1, row 1, level 2: the first vertex of level 3
    bad[2, 0, 3] = 0                                     # (a later one too: the first is named)
    assert refused(-1, "query 1 row 1 level 2:", p=bad)
    with pytest.raises(capi.DgError, match=rf"rc=-1.*{NAME}: query 1 row 1 level 2\b"):
        gpu_ctx.dp_genotype_margins_budgets(bad, budgets)
    assert refused(-1, "query 2: budget -4 is negative", b=np.array([2, 0, -4], np.int32))
    assert refused(-1, "n_called = 0", count=0) and refused(-1, "n_called = -2", count=-2)
    for null in ("p", "b", "lv", "bv"):
        assert refused(-1, "called, budgets, levels and best_values are required", **{null: None})
    assert refused(-5, "", b=np.array([2, MAX_PLANES, 3], np.int32)) and f"{MAX_PLANES + 1}" in capi.lib.dg_last_error().decode()
    good = np.array([[1, int(g.level_off[1]), -1, REQUIRE]], np.int32)
    assert refused(-1, "pin 1: ", pins=np.array([good[0], [0, 0, 0, REQUIRE]], np.int32), n_pins=2) and "level 0" in capi.lib.dg_last_error().decode()
    assert refused(-1, "pin 0: ", pins=np.array([[1, int(g.level_off[2]), -1, REQUIRE]], np.int32), n_pins=1)
    assert refused(-1, "pin 0: ", pins=np.array([[1, -1, -1, 2]], np.int32), n_pins=1) and "kind 2" in capi.lib.dg_last_error().decode()
    assert refused(-1, "n_pins = -1", pins=good, n_pins=-1) and refused(-1, "null pins", pins=None, n_pins=2)
    assert gpu_ctx.dp_genotype_stats() == stats          # a refused call leaves the statistics too
    with pytest.raises(ValueError):
        gpu_ctx.dp_genotype_margins_budgets(called[:, :, :-1], budgets)
    with pytest.raises(ValueError):
        gpu_ctx.dp_genotype_margins_budgets(called, budgets[:2])
    with pytest.raises(ValueError):
        gpu_ctx.dp_genotype_margins_budgets(called, 2)
    with pytest.raises(ValueError):
        gpu_ctx.dp_genotype_margins_budgets(called, budgets, np.zeros(g.n_vertices - 1, np.int32))
    # the raw call writes eight words per (query, level): the six fields and two zeros
    want, V = gpu_ctx.dp_genotype_margins_budgets(called, budgets)
    assert want.dtype == capi.GENOTYPE_MARGIN and want.dtype.names == FIELDS + ("reserved",)
    assert raw() == 0 and np.array_equal(best, V)
    assert np.array_equal(out[:, :, :6], _rows(want)) and (out[:, :, 6:] == 0).all()
    assert raw(pins=good, n_pins=1) == 0 and np.array_equal(out[:, :, :6], _rows(gpu_ctx.dp_genotype_margins_budgets(called, budgets, pins=good)[0]))

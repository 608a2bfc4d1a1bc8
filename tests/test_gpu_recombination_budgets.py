"""-m gpu: dg_dp_recombination_margins_budgets / Context.dp_recombination_margins_budgets -- the recombination margins of every listed
budget from one joint pass at the largest.

Integers only: every comparison is exact.  The yardsticks are tests/recombination_budgets_model.py (pinned to the one-budget model by
tests/test_recombination_budgets_model.py, which also holds the floor under this file's graphs: the records depend on the budget on
every transition of them) and the one-budget call dg_dp_recombination_margins itself, query by query."""
import numpy as np
import pytest

import graphgen
import padded_graphs as pg
from dipgenie_amd import capi
from pair_graphs import with_R
from paths_model import NEG_INF, PathModel
from phase_margins_model import joint_states_fb
from recombination_budgets_model import recombination_margins_budgets_np
from recombination_margins_model import FIELDS, remap_rows, rows
from test_gpu_genotype_margins import BUDGETS as WIDTH_BUDGETS, MAX_PLANES, MAX_QUERIES, WIDTHS, wide_case
from test_gpu_phase_margins import SEEDS, case
from test_gpu_score_paths import ENUMERABLE
from test_partner_model import enumerable_graph
from test_recombination_budgets_model import MIXED, _called, unfit_graph

pytestmark = pytest.mark.gpu

SEED_BUDGETS = [5, 0, 2, 5, 1]


def rows3(records):
    """a RECOMBINATION_MARGIN record array [n, T] as int64 [n, T, 16] in the order of FIELDS"""
    return np.stack([rows(r) for r in records]) if len(records) else np.zeros((0, 0, 16), np.int64)


def same(got, want, tag):
    got, want = np.asarray(got, np.int64), np.asarray(want, np.int64)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (tag, bad[:5], got[tuple(bad[:5].T)], want[tuple(bad[:5].T)])


def against_singles(ctx, budgets, called, got, tag):
    """query q of the one call against dp_recombination_margins(budgets[q], called[q])"""
    rec, out, best = got
    for q, b in enumerate(budgets):
        r1, o1, v1 = ctx.dp_recombination_margins(int(b), None if called is None else called[q:q + 1])
        assert best[q] == v1, (tag, q, b)
        same(rows(rec[q]), rows(r1), (tag, q, b, "single"))
        if called is not None:
            same(out[q], o1[0], (tag, q, b, "single called_out"))


def against_model(ctx, m, budgets, tag, seed, states=None):
    """the called variants: none; sampled pairs and cells that are no paths (every third query)"""
    mixed = _called(m, len(budgets), seed)
    cells = mixed[[2] * len(budgets)]
    for kind, called in (("none", None), ("mixed", mixed), ("cells", cells)):
        want, want_out, V = recombination_margins_budgets_np(m, budgets, called, states)
        got = ctx.dp_recombination_margins_budgets(budgets, called)
        assert got[0].shape == (len(budgets), m.L - 1) and got[2].dtype == np.int32
        same(got[2], V, (tag, kind, "best_values"))
        same(rows3(got[0]), want, (tag, kind))
        if called is None:
            assert got[1] is None
        else:
            same(got[1], want_out, (tag, kind, "called_out"))
        against_singles(ctx, budgets, None if called is None else called.astype(np.int32), got, (tag, kind))
    assert (want_out[:, :, 0] == -1).any()               # cells that are no paths
    return want


@pytest.mark.parametrize("q", range(len(ENUMERABLE)))
def test_device_equals_model_on_the_enumerable_graphs(gpu_ctx, q):
    g = enumerable_graph(q)
    gpu_ctx.dp_load_graph(g)
    against_model(gpu_ctx, PathModel(g), MIXED, q, 70 + q)


@pytest.mark.parametrize("seed", SEEDS)
def test_device_equals_model(gpu_ctx, seed):
    g, m, _, _ = case(seed)
    gpu_ctx.dp_load_graph(g)
    want = against_model(gpu_ctx, m, SEED_BUDGETS, seed, seed, joint_states_fb(m, 5))
    assert (want[0] != want[1]).any() and (want[2] != want[4]).any() and np.array_equal(want[0], want[3])
    st = gpu_ctx.dp_recombination_budget_stats()
    assert (st["queries"], st["distinct_budgets"], st["transitions"]) == (5, 4, g.n_levels - 1)


@pytest.mark.parametrize("w", range(len(WIDTHS)))
def test_device_equals_model_on_prescribed_widths(gpu_ctx, w):
    for k, p_w1 in enumerate((0.0, 0.3, 1.0)):
        g = graphgen.random_levelized(9100 + 10 * w + k, widths=WIDTHS[w], R=3, p_w1=p_w1, dup_edges=True, extra_edges=1.2, p_colour=0.5)
        m = PathModel(g)
        gpu_ctx.dp_load_graph(g)
        called = _called(m, len(WIDTH_BUDGETS), 50 + w)
        want, want_out, V = recombination_margins_budgets_np(m, WIDTH_BUDGETS, called)
        rec, out, best = gpu_ctx.dp_recombination_margins_budgets(WIDTH_BUDGETS, called)
        same(best, V, (w, p_w1, "best_values"))
        same(rows3(rec), want, (w, p_w1))
        same(out, want_out, (w, p_w1, "called_out"))


def test_wider_than_any_tile_against_the_one_budget_call(gpu_ctx):
    g, m, planes = wide_case(gpu_ctx)
    budgets = [18, 3, 0]
    called = np.ascontiguousarray(_called(m, 3, 3), np.int32)
    got = gpu_ctx.dp_recombination_margins_budgets(budgets, called)
    assert got[2][0] == planes[18] != NEG_INF
    against_singles(gpu_ctx, budgets, called, got, "wide")
    assert (got[0]["value"][0] != got[0]["value"][1]).any() and (got[0]["value"][1] != got[0]["value"][2]).any()


def test_a_budget_nobody_fits_beside_one_that_somebody_does(gpu_ctx):
    g = unfit_graph()
    m = PathModel(g)
    gpu_ctx.dp_load_graph(g)
    budgets = [9, 10, 0]
    called = np.stack([m.sample_paths(np.random.default_rng(1), 2)[0]] * 3)
    want, want_out, V = recombination_margins_budgets_np(m, budgets, called)
    rec, out, best = gpu_ctx.dp_recombination_margins_budgets(budgets, called)
    same(best, V, "best_values")
    same(rows3(rec), want, "unfit")
    same(out, want_out, "unfit called_out")
    assert best[0] == best[2] == NEG_INF != best[1]
    for q in (0, 2):
        assert (rec["value"][q] == NEG_INF).all() and (rec["from1"][q] == -1).all() and (rec["to2"][q] == -1).all() and (out[q, :, 1] == NEG_INF).all()
    assert (rec["value"][1][:, 2] == best[1]).all() and (out[:, :, 0] == 2).all()


def test_256_queries_and_no_more(gpu_ctx):
    g, m, _, _ = case(9300)
    gpu_ctx.dp_load_graph(g)
    budgets = np.arange(MAX_QUERIES + 1, dtype=np.int32) % 5
    called = np.ascontiguousarray(m.sample_pairs(np.random.default_rng(7), MAX_QUERIES + 1, p_w0=0.9)[0], np.int32)
    want, want_out, V = recombination_margins_budgets_np(m, budgets[:MAX_QUERIES], called[:MAX_QUERIES])
    rec, out, best = gpu_ctx.dp_recombination_margins_budgets(budgets[:MAX_QUERIES], called[:MAX_QUERIES])
    same(best, V, "256 best_values")
    same(rows3(rec), want, "256")
    same(out, want_out, "256 called_out")
    st = gpu_ctx.dp_recombination_budget_stats()
    assert (st["queries"], st["distinct_budgets"]) == (MAX_QUERIES, 5)
    with pytest.raises(capi.DgError, match=rf"rc=-5.*dg_dp_recombination_margins_budgets.*\b{MAX_QUERIES + 1}\b.*\b{MAX_QUERIES}\b"):
        gpu_ctx.dp_recombination_margins_budgets(budgets, called)
    assert gpu_ctx.dp_recombination_budget_stats() == st


@pytest.mark.parametrize("which", ["levels26", "wide"])
def test_segments_change_nothing(gpu_ctx, which):
    if which == "wide":
        g, m, _ = wide_case(gpu_ctx)
        budgets = [18, 3, 0]
    else:
        g, m, _, _ = case(9302)
        gpu_ctx.dp_load_graph(g)
        budgets = SEED_BUDGETS
    called = _called(m, len(budgets), 5)
    got = {}
    for name, nbytes in (("every level", 1), ("default", 0)):
        with gpu_ctx.dp_options(joint_state_bytes=nbytes):
            got[name] = gpu_ctx.dp_recombination_margins_budgets(budgets, called)
        got[name + " stats"] = gpu_ctx.dp_recombination_budget_stats()
    for x, y in zip(got["every level"], got["default"]):
        assert np.array_equal(x, y)
    one, each = got["default stats"], got["every level stats"]
    assert each["segments"] == g.n_levels and one["segments"] == 1 and each["levels_twice"] == one["levels_twice"] == 0
    for f in ("queries", "distinct_budgets", "transitions", "edge_launches", "finish_launches", "launches"):
        assert each[f] == one[f], f
    widest = int(np.diff(g.level_off).max())
    assert one["peak_bytes"] >= 3 * 4 * widest * widest * (max(budgets) + 1)   # F of the widest level and the two rolling states of B, at bmax


@pytest.mark.parametrize("nbytes", [0, 1, 3000])
def test_as_many_launches_as_the_one_budget_call_at_the_largest(gpu_ctx, nbytes):
    """two gathers per transition whatever the number of budgets: the schedule is that of dp_recombination_margins(bmax)"""
    g, m, _, _ = case(9304)
    gpu_ctx.dp_load_graph(g)
    with gpu_ctx.dp_options(joint_state_bytes=nbytes):
        gpu_ctx.dp_recombination_margins_budgets(SEED_BUDGETS)
        many = gpu_ctx.dp_recombination_budget_stats()
        gpu_ctx.dp_recombination_margins(max(SEED_BUDGETS))
        one = gpu_ctx.dp_recombination_stats()
    for f in ("transitions", "edge_launches", "finish_launches", "segments", "levels_twice", "launches"):
        assert many[f] == one[f], (f, many, one)
    assert many["distinct_budgets"] == 4 and many["queries"] == 5 and many["edge_launches"] == g.n_levels - 1
    if nbytes == 3000:
        assert 1 < many["segments"] < g.n_levels and many["levels_twice"] > 0


def test_the_runs_own_answers_and_nothing_else_touched(gpu_ctx):
    """after dp_run_budgets: the answer at b is an optimal pair at b, so every transition of it is worth the plane at b and its called
    crossovers are those dp_score_paths counts; the run's planes, answers, timing and every other statistics block stay as they were"""
    g, m, two, _ = case(9303)
    gpu_ctx.dp_load_graph(g)
    gpu_ctx.dp_run_budgets(range(g.R + 1))
    planes = gpu_ctx.dp_budget_values().copy()
    fit = [b for b in range(g.R + 1) if planes[b] != NEG_INF]
    assert len(fit) >= 2
    paths = {b: gpu_ctx.dp_answer_paths(b).copy() for b in fit}
    gpu_ctx.dp_genotype_margins(paths[g.R], g.R, two)
    gpu_ctx.dp_phase_margins(paths[g.R], g.R, two)
    gpu_ctx.dp_recombination_margins(g.R, paths[g.R][None])

    def others():
        return (gpu_ctx.dp_genotype_stats(), gpu_ctx.dp_phase_stats(), gpu_ctx.dp_phase_budget_stats(), gpu_ctx.dp_pin_stats(), gpu_ctx.dp_recombination_stats(),
                bytes(gpu_ctx.dp_timing()))

    before = others()
    order = fit[::-1]
    called = np.stack([paths[b] for b in order])
    rec, out, best = gpu_ctx.dp_recombination_margins_budgets(order, called)
    scores = gpu_ctx.dp_score_paths(called)
    for q, b in enumerate(order):
        assert best[q] == planes[b] and (out[q, :, 1] == planes[b]).all() and (rec["value"][q].max(axis=1) == planes[b]).all()
        assert out[q, :, 0].sum() == scores[q]["r1"] + scores[q]["r2"] <= b
    assert others() == before
    assert np.array_equal(gpu_ctx.dp_budget_values(), planes)
    for b in fit:
        assert np.array_equal(gpu_ctx.dp_answer_paths(b), paths[b])


def test_errors_and_layout(gpu_ctx):
    assert capi.RECOMBINATION_MARGIN.itemsize == 64 and capi.RECOMBINATION_MARGIN.names == FIELDS
    g, m, _, per_budget = case(9300)
    L = g.n_levels
    call = capi.lib.dg_dp_recombination_margins_budgets
    fresh = capi.Context(0)
    try:
        with pytest.raises(capi.DgError, match=r"rc=-6.*dg_dp_recombination_margins_budgets: no graph loaded"):
            fresh.dp_recombination_margins_budgets([0])
    finally:
        fresh.close()
    gpu_ctx.dp_load_graph(g)
    called = np.ascontiguousarray(np.stack([per_budget[2], per_budget[5]]), np.int32)
    budgets = np.array([2, 5], np.int32)
    want, want_out, V = gpu_ctx.dp_recombination_margins_budgets(budgets, called)
    gpu_ctx.dp_recombination_margins(2, called)
    stats = (gpu_ctx.dp_recombination_budget_stats(), gpu_ctx.dp_recombination_stats())
    rec = np.full((2, L - 1, 16), -7, np.int32)
    out = np.full((2, L - 1, 2), -7, np.int32)
    best = np.full(2, -7, np.int32)

    def ptr(a):
        return a.ctypes.data if a is not None else None

    def raw(b=budgets, n=2, p=called, records=rec, cout=out, bests=best):
        return call(gpu_ctx.h, ptr(b), n, ptr(p), ptr(records), ptr(cout), ptr(bests))

    def untouched():
        return (rec == -7).all() and (out == -7).all() and (best == -7).all()

    bad = called.copy()
    bad[1, 1, 2] = g.level_off[3]                        # query 1, row 1, level 2: the first vertex of level 3
    bad[1, 1, 3] = 0                                     # (a later one too: the first is named)
    with pytest.raises(capi.DgError, match=r"rc=-1.*dg_dp_recombination_margins_budgets.*query 1 row 1 level 2\b"):
        gpu_ctx.dp_recombination_margins_budgets(budgets, bad)
    assert raw(p=bad) == -1 and untouched()
    with pytest.raises(capi.DgError, match=r"rc=-1.*dg_dp_recombination_margins_budgets.*query 1.*budget -3"):
        gpu_ctx.dp_recombination_margins_budgets([0, -3, -1])
    assert raw(b=np.array([2, -1], np.int32)) == -1 and untouched()
    assert raw(b=None) == -1 and raw(records=None) == -1 and raw(bests=None) == -1 and raw(cout=None) == -1 and raw(n=0) == -1 and raw(n=-1) == -1 and untouched()
    with pytest.raises(capi.DgError, match=r"rc=-1.*dg_dp_recombination_margins_budgets"):
        gpu_ctx.dp_recombination_margins_budgets([])
    with pytest.raises(capi.DgError, match=rf"rc=-5.*dg_dp_recombination_margins_budgets.*\b{MAX_PLANES + 1}\b.*\b{MAX_PLANES}\b"):
        gpu_ctx.dp_recombination_margins_budgets([1, MAX_PLANES])
    assert raw(b=np.array([MAX_PLANES, 0], np.int32)) == -5 and untouched()
    assert raw(n=MAX_QUERIES + 1) == -5 and untouched()
    assert (gpu_ctx.dp_recombination_budget_stats(), gpu_ctx.dp_recombination_stats()) == stats      # a refused call leaves the statistics too
    with pytest.raises(ValueError):
        gpu_ctx.dp_recombination_margins_budgets(budgets, called[:, :, :-1])
    with pytest.raises(ValueError):
        gpu_ctx.dp_recombination_margins_budgets(budgets, called[0])
    with pytest.raises(ValueError):
        gpu_ctx.dp_recombination_margins_budgets([2], called)
    # the raw call writes sixteen words per record, and without called needs no called_out
    assert raw() == 0 and np.array_equal(best, V)
    assert np.array_equal(rec, rows3(want)) and np.array_equal(out, want_out)
    rec[:] = -7
    out[:] = -7
    assert raw(p=None, cout=None) == 0 and np.array_equal(rec, rows3(want)) and (out == -7).all()
    with pytest.raises(capi.DgError, match=r"rc=-1.*dg_dp_get_recombination_budget_stats"):
        capi._check(capi.lib.dg_dp_get_recombination_budget_stats(gpu_ctx.h, None, 9), "dg_dp_get_recombination_budget_stats")
    assert capi.lib.dg_dp_get_recombination_budget_stats(gpu_ctx.h, np.zeros(9, np.int64).ctypes.data, 8) == -1


def test_lanes_beyond_the_grid_cap(gpu_ctx):
    """rb_edges_budgets_kernel has JT_X_BLOCKS workgroups per row and budget and its lanes stride beyond.  The lanes shape of
    tests/padded_graphs.py with the budgets (4,095, 2, 0) in one call against the model of the base graph: level 2 has 300 * 4,096 lanes
    per row at the first budget, more than 2^20, beside rows of 900 and 300 lanes in the same launch; 4,095 is worth what the saturating
    budget 2 (L - 1) is"""
    g, gp, new_id = pg.lanes()
    m = PathModel(g)
    saturated = 2 * (g.n_levels - 1)
    assert pg.LANES_BUDGET == MAX_PLANES - 1 and pg.widest_level(gp) * (pg.LANES_BUDGET + 1) > pg.LANES_PER_ROW
    gpu_ctx.dp_load_graph(with_R(gp, saturated))
    called = _called(m, 3, 96)
    want, want_out, V = recombination_margins_budgets_np(m, [saturated, 2, 0], called)
    rec, out, best = gpu_ctx.dp_recombination_margins_budgets([pg.LANES_BUDGET, 2, 0], pg.remap_called(called, new_id))
    same(best, V, "lanes best_values")
    assert V[0] != NEG_INF
    same(rows3(rec), np.stack([remap_rows(w, new_id) for w in want]), "lanes")
    same(out, want_out, "lanes called_out")
    ids = rows3(rec)[:, :, 4:]
    assert not pg.pad_mask(gp, new_id)[ids[ids >= 0]].any()
    assert (want[0][:, 2] != NEG_INF).any() and (want[0][:, 3] != NEG_INF).any() and (want[0] != want[1]).any()
    assert gpu_ctx.dp_recombination_budget_stats()["peak_bytes"] >= 4 * 300 * 300 * (pg.LANES_BUDGET + 1)      # the call ran at the padded width

"""-m gpu: dg_dp_recombination_margins / Context.dp_recombination_margins -- per transition the best pair of paths that spends 0, 1 or 2
crossovers there, with the hop pair that attains it, from the joint pass with one more gather per level.

Integers only: every comparison is exact.  The yardstick is tests/recombination_margins_model.py, itself pinned to brute force by
tests/test_recombination_margins_model.py (which also holds the floors under this file's graphs); the tests without a model hold every
entry against dp_run_pinned (plane b of the run that requires the ordered cell (from1, from2) at l and (to1, to2) at l + 1 is value[s])
and dp_score_paths."""
import numpy as np
import pytest

import graphgen
import loader_graphs as lg
import padded_graphs as pg
from dipgenie_amd import capi
from pair_graphs import with_R
from paths_model import NEG_INF, PathModel
from phase_margins_model import joint_states_fb
from recombination_margins_model import FIELDS, recombination_margins_np, remap_rows, rows
from test_gpu_genotype_margins import MAX_PLANES, MAX_QUERIES, _called, wide_case
from test_gpu_phase_margins import BUDGETS, SEEDS, case

pytestmark = pytest.mark.gpu


def same(got, want, tag):
    got, want = np.asarray(got, np.int64), np.asarray(want, np.int64)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    bad = np.argwhere((got != want).reshape(len(got), -1).any(axis=-1))
    assert bad.size == 0, (tag, bad[:5].ravel(), got[bad[:5].ravel()], want[bad[:5].ravel()])


def expected_stats(g, n_segments=1):
    """what one segment launches: the out-index (3), the source fill and the sink fill, a forward launch per level but the first, an
    edge and a finish launch per transition, a backward launch per level but the first and the last; and a score launch with each of
    the recurrences and gathers on a coloured transition (counted by the caller: `launches` is only bounded here)"""
    T = g.n_levels - 1
    return dict(transitions=T, edge_launches=T, finish_launches=T, segments=n_segments), 3 + 2 + T + 2 * T + (T - 1)


@pytest.mark.parametrize("seed", SEEDS)
def test_device_equals_model(gpu_ctx, seed):
    g, m, two, sampled = case(seed)
    gpu_ctx.dp_load_graph(g)
    rng = np.random.default_rng(seed)
    for b in BUDGETS:
        states = joint_states_fb(m, b)
        three = np.concatenate([sampled[b][None], _called(m, rng)])         # the sampled pair, another, cells that are no paths
        for tag, called in (("none", None), ("one", three[:1]), ("cells", three[2:]), ("three", three)):
            want, want_out, V = recombination_margins_np(m, b, called, states)
            got, out, best = gpu_ctx.dp_recombination_margins(b, called)
            assert best == V, (seed, b, tag, best, V)
            same(rows(got), want, (seed, b, tag))
            if called is None:
                assert out is None
            else:
                same(out, want_out, (seed, b, tag, "called_out"))
            stats = gpu_ctx.dp_recombination_stats()
            fixed, floor = expected_stats(g)
            assert {k: stats[k] for k in fixed} == fixed and stats["levels_twice"] == 0, stats
            assert floor <= stats["launches"] <= floor + 2 * (g.n_levels - 1), stats      # at most one score launch per forward and per transition
        assert (want_out[2, :, 0] == -1).any() and (want_out[0, :, 0] >= 0).all()


def _pinned(ctx, n_levels, l, cell_from, cell_to, b):
    """plane b of the run that requires both cells (the first and the last level hold one cell and take no pin)"""
    pins = [(lvl, int(c[0]), int(c[1]), capi.PIN_REQUIRE) for lvl, c in ((l, cell_from), (l + 1, cell_to)) if 0 < lvl < n_levels - 1]
    return ctx.dp_run_pinned(pins, [b])[0].value


def _against_pinned_runs(ctx, m, records, b, tag):
    """every reachable (transition, s): plane b of the pinned run is value[s], and its answer takes s weight-1 hops there"""
    n = 0
    for r in records:
        l = int(r["level"])
        for s in range(3):
            if r["value"][s] == NEG_INF:
                assert (r["from1"][s], r["from2"][s], r["to1"][s], r["to2"][s]) == (-1, -1, -1, -1), (tag, l, s)
                continue
            frm, to = (r["from1"][s], r["from2"][s]), (r["to1"][s], r["to2"][s])
            assert _pinned(ctx, m.L, l, frm, to, b) == r["value"][s], (tag, l, s)
            paths = ctx.dp_answer_paths(b)
            assert (paths[0, l], paths[1, l]) == frm and (paths[0, l + 1], paths[1, l + 1]) == to, (tag, l, s)
            assert m.succ[int(paths[0, l])][int(paths[0, l + 1])] + m.succ[int(paths[1, l])][int(paths[1, l + 1])] == s, (tag, l, s)
            score = ctx.dp_score_paths(paths[None])[0]
            assert score["value"] == r["value"][s] and score["r1"] + score["r2"] <= b, (tag, l, s)
            assert frm[0] <= frm[1]
            n += 1
    return n


@pytest.mark.parametrize("seed", SEEDS)
def test_every_entry_is_a_pinned_run(gpu_ctx, seed):
    g, m, _, _ = case(seed)
    gpu_ctx.dp_load_graph(g)
    records, _, best = gpu_ctx.dp_recombination_margins(2)
    assert (records["value"].max(axis=1) == best).all() and best != NEG_INF
    assert _against_pinned_runs(gpu_ctx, m, records, 2, seed) >= g.n_levels - 1


def test_wider_than_any_tile_against_pinned_runs(gpu_ctx):
    g, m, planes = wide_case(gpu_ctx)
    b = 18
    answer = gpu_ctx.dp_answer_paths(b).copy()
    records, out, best = gpu_ctx.dp_recombination_margins(b, answer[None])
    assert best == planes[b] and len(records) == 4 and records["level"].tolist() == [0, 1, 2, 3]
    assert (records["value"].max(axis=1) == best).all()
    score = gpu_ctx.dp_score_paths(answer[None])[0]
    assert (out[0, :, 1] == best).all() and out[0, :, 0].sum() == score["r1"] + score["r2"]     # the run's own answer
    assert (records["value"][1:3] != NEG_INF).all()                          # both inner transitions offer 0, 1 and 2 crossovers
    assert _against_pinned_runs(gpu_ctx, m, records, b, "wide") >= 8
    print(f"wide: V {best}, records {rows(records).tolist()}")


@pytest.mark.parametrize("which", ["levels26", "wide"])
def test_segments_change_nothing(gpu_ctx, which):
    if which == "wide":
        g, m, _ = wide_case(gpu_ctx)
        b = 18
    else:
        g, m, _, _ = case(9302)
        gpu_ctx.dp_load_graph(g)
        b = 5
    called = _called(m, np.random.default_rng(5))
    got = {}
    for name, nbytes in (("every level", 1), ("default", 0)):
        with gpu_ctx.dp_options(joint_state_bytes=nbytes):
            got[name] = gpu_ctx.dp_recombination_margins(b, called)
        got[name + " stats"] = gpu_ctx.dp_recombination_stats()
    for x, y in zip(got["every level"], got["default"]):
        assert np.array_equal(x, y)
    one, each = got["default stats"], got["every level stats"]
    assert each["segments"] == g.n_levels and one["segments"] == 1 and each["levels_twice"] == one["levels_twice"] == 0
    for f in ("transitions", "edge_launches", "finish_launches", "launches"):      # a level per segment: its state is the checkpoint, nothing is swept twice
        assert each[f] == one[f], f
    widest = int(np.diff(g.level_off).max())
    assert one["peak_bytes"] >= 3 * 4 * widest * widest * (b + 1)              # F of the widest level and the two rolling states of B


def test_the_runs_own_answers(gpu_ctx):
    """after dp_run_budgets: the run's answer at b is an optimal pair at b, so every transition of it is worth the plane, and its
    called crossovers are those dp_score_paths counts; the run's planes, answers and the other statistics stay as they were"""
    g, m, two, _ = case(9303)
    gpu_ctx.dp_load_graph(g)
    gpu_ctx.dp_run_budgets(range(g.R + 1))
    planes = gpu_ctx.dp_budget_values().copy()
    paths = [gpu_ctx.dp_answer_paths(b).copy() for b in range(g.R + 1)]
    gpu_ctx.dp_genotype_margins(paths[g.R], g.R, two)
    gpu_ctx.dp_phase_margins(paths[g.R], g.R, two)
    before = (gpu_ctx.dp_genotype_stats(), gpu_ctx.dp_phase_stats(), gpu_ctx.dp_phase_budget_stats(), gpu_ctx.dp_pin_stats())
    n = 0
    for b in range(g.R + 1):
        if planes[b] == NEG_INF:
            continue
        records, out, best = gpu_ctx.dp_recombination_margins(b, paths[b][None])
        score = gpu_ctx.dp_score_paths(paths[b][None])[0]
        assert best == planes[b] and (out[0, :, 1] == planes[b]).all()
        assert out[0, :, 0].sum() == score["r1"] + score["r2"] <= b
        n += 1
    assert n >= 2
    assert np.array_equal(gpu_ctx.dp_budget_values(), planes)
    for b in range(g.R + 1):
        assert np.array_equal(gpu_ctx.dp_answer_paths(b), paths[b])
    assert (gpu_ctx.dp_genotype_stats(), gpu_ctx.dp_phase_stats(), gpu_ctx.dp_phase_budget_stats(), gpu_ctx.dp_pin_stats()) == before


def test_a_budget_nobody_fits(gpu_ctx):
    """every edge weighs 1: a pair of paths spends 2 (L - 1) = 10.  At b = 9 nobody fits: DG_OK, NEG_INF / -1 in every record; at 10
    everybody does, and every transition is two crossovers"""
    g = graphgen.random_levelized(9611, widths=[1, 3, 4, 3, 4, 1], R=3, p_w1=1.0, dup_edges=True, extra_edges=1.2, p_colour=0.5)
    m = PathModel(g)
    gpu_ctx.dp_load_graph(g)
    called = m.sample_paths(np.random.default_rng(1), 2)[0][None]
    for b in (0, 9, 10):
        want, want_out, V = recombination_margins_np(m, b, called)
        got, out, best = gpu_ctx.dp_recombination_margins(b, called)
        assert best == V and (V == NEG_INF) == (b < 10)
        same(rows(got), want, b)
        same(out, want_out, b)
        assert (out[0, :, 0] == 2).all()
        if b < 10:
            assert (got["value"] == NEG_INF).all() and (got["from1"] == -1).all() and (got["to2"] == -1).all() and (out[0, :, 1] == NEG_INF).all()
        else:
            assert (got["value"][:, 2] == V).all() and (got["value"][:, :2] == NEG_INF).all()


@pytest.mark.parametrize("name", sorted(lg.dead_ends()))
def test_dead_ends(gpu_ctx, name):
    g = lg.dead_ends()[name]
    m = PathModel(g)
    dead = lg.dead_end_vertices(g)
    gpu_ctx.dp_load_graph(g)
    called = PathModel(lg.prune(g)).sample_pairs(np.random.default_rng(62), 2, p_w0=0.9)[0]
    for b in (0, g.R):
        want, want_out, V = recombination_margins_np(m, b, called)
        got, out, best = gpu_ctx.dp_recombination_margins(b, called)
        assert best == V
        same(rows(got), want, (name, b))
        same(out, want_out, (name, b))
        assert not np.isin(rows(got)[:, 4:], dead).any()


def test_256_queries_and_no_more(gpu_ctx):
    g, m, _, _ = case(9300)
    gpu_ctx.dp_load_graph(g)
    called = m.sample_pairs(np.random.default_rng(7), MAX_QUERIES + 1, p_w0=0.9)[0]
    want, want_out, V = recombination_margins_np(m, 2, called[:MAX_QUERIES])
    got, out, best = gpu_ctx.dp_recombination_margins(2, called[:MAX_QUERIES])
    assert best == V
    same(rows(got), want, "256")
    same(out, want_out, "256 called_out")
    with pytest.raises(capi.DgError, match=rf"rc=-5.*dg_dp_recombination_margins.*\b{MAX_QUERIES + 1}\b.*\b{MAX_QUERIES}\b"):
        gpu_ctx.dp_recombination_margins(2, called)


def test_errors_and_layout(gpu_ctx):
    assert capi.RECOMBINATION_MARGIN.itemsize == 64 and capi.RECOMBINATION_MARGIN.names == FIELDS
    g, m, _, per_budget = case(9300)
    L = g.n_levels
    call = capi.lib.dg_dp_recombination_margins
    fresh = capi.Context(0)
    try:
        with pytest.raises(capi.DgError, match=r"rc=-6.*dg_dp_recombination_margins: no graph loaded"):
            fresh.dp_recombination_margins(0)
    finally:
        fresh.close()
    gpu_ctx.dp_load_graph(g)
    called = np.ascontiguousarray(np.stack([per_budget[2], per_budget[5]]), np.int32)
    want, want_out, V = gpu_ctx.dp_recombination_margins(2, called)
    stats = gpu_ctx.dp_recombination_stats()
    rec = np.full((L - 1, 16), -7, np.int32)
    out = np.full((2, L - 1, 2), -7, np.int32)
    best = capi.C.c_int32(-7)

    def raw(b, p=called, n=2, records=rec, cout=out, best_ref=capi.C.byref(best)):
        return call(gpu_ctx.h, b, p.ctypes.data if p is not None else None, n, records.ctypes.data if records is not None else None,
                    cout.ctypes.data if cout is not None else None, best_ref)

    def untouched():
        return (rec == -7).all() and (out == -7).all() and best.value == -7

    bad = called.copy()
    bad[1, 1, 2] = g.level_off[3]                        # query 1, row 1, level 2: the first vertex of level 3
    bad[1, 1, 3] = 0                                     # (a later one too: the first is named)
    with pytest.raises(capi.DgError, match=r"rc=-1.*dg_dp_recombination_margins.*query 1 row 1 level 2\b"):
        gpu_ctx.dp_recombination_margins(2, bad)
    assert raw(2, bad) == -1 and untouched()
    bad = called.copy()
    bad[0, 0, 0] = -1
    with pytest.raises(capi.DgError, match=r"rc=-1.*query 0 row 0 level 0\b"):
        gpu_ctx.dp_recombination_margins(2, bad)
    with pytest.raises(capi.DgError, match=r"rc=-1.*dg_dp_recombination_margins.*budget -1"):
        gpu_ctx.dp_recombination_margins(-1)
    assert raw(-1) == -1 and untouched()
    assert raw(2, records=None) == -1 and raw(2, best_ref=None) == -1 and raw(2, p=None) == -1 and raw(2, cout=None) == -1 and raw(2, n=-1) == -1 and untouched()
    with pytest.raises(capi.DgError, match=rf"rc=-5.*dg_dp_recombination_margins.*\b{MAX_PLANES + 1}\b.*\b{MAX_PLANES}\b"):
        gpu_ctx.dp_recombination_margins(MAX_PLANES)
    assert raw(MAX_PLANES) == -5 and untouched()
    assert raw(2, n=MAX_QUERIES + 1) == -5 and untouched()
    assert gpu_ctx.dp_recombination_stats() == stats     # a refused call leaves the statistics too
    with pytest.raises(ValueError):
        gpu_ctx.dp_recombination_margins(2, called[:, :, :-1])
    with pytest.raises(ValueError):
        gpu_ctx.dp_recombination_margins(2, called[0])
    # the raw call writes sixteen words per record, and with n_called = 0 needs neither called nor called_out
    assert raw(2) == 0 and best.value == V
    assert np.array_equal(rec, rows(want)) and np.array_equal(out, want_out)
    rec[:] = -7
    assert raw(2, p=None, n=0, cout=None) == 0 and np.array_equal(rec, rows(want))
    with pytest.raises(capi.DgError, match=r"rc=-1.*dg_dp_get_recombination_stats"):
        capi._check(capi.lib.dg_dp_get_recombination_stats(gpu_ctx.h, None, 7), "dg_dp_get_recombination_stats")
    assert capi.lib.dg_dp_get_recombination_stats(gpu_ctx.h, np.zeros(7, np.int64).ctypes.data, 6) == -1


def test_lanes_beyond_the_grid_cap(gpu_ctx):
    """the one grid cap of the new kernels: rb_edges_kernel has JT_X_BLOCKS workgroups per row and its lanes stride beyond, as the
    recurrences do.  The lanes shape of tests/padded_graphs.py at budget 4,095 against the model of the base graph at the saturating
    budget 2 (L - 1): level 2 has 300 * 4,096 lanes per row, more than 2^20"""
    g, gp, new_id = pg.lanes()
    m = PathModel(g)
    saturated = 2 * (g.n_levels - 1)
    assert pg.LANES_BUDGET == MAX_PLANES - 1 and pg.widest_level(gp) * (pg.LANES_BUDGET + 1) > pg.LANES_PER_ROW
    gpu_ctx.dp_load_graph(with_R(gp, saturated))
    called = _called(m, np.random.default_rng(96))
    want, want_out, V = recombination_margins_np(m, saturated, called)
    got, out, best = gpu_ctx.dp_recombination_margins(pg.LANES_BUDGET, pg.remap_called(called, new_id))
    assert best == V != NEG_INF
    same(rows(got), remap_rows(want, new_id), "lanes")
    same(out, want_out, "lanes called_out")
    ids = rows(got)[:, 4:]
    assert not pg.pad_mask(gp, new_id)[ids[ids >= 0]].any()
    assert (want[:, 2] != NEG_INF).any() and (want[:, 3] != NEG_INF).any()
    assert gpu_ctx.dp_recombination_stats()["peak_bytes"] >= 4 * 300 * 300 * (pg.LANES_BUDGET + 1)      # the call ran at the padded width

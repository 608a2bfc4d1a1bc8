"""-m gpu: dg_dp_get_answer_paths / Context.dp_answer_paths -- the answer of the last run as the pair of paths it walked.

Integers only: every comparison is exact, and no model is needed.  After dp_run_budgets(range(R + 1)) on the graphs of
tests/test_gpu_partner.py, for every budget: both rows are paths of the graph, dp_score_paths of the pair returns the plane's value
and the result's s_het, and the weight-1 hops of each row plus the closing entry that the finish kernel adds are the result's edge
lists."""
import copy

import numpy as np
import pytest

from dipgenie_amd import capi
from paths_model import NEG_INF, PathModel, edge_list
from test_gpu_partner import CASES

pytestmark = pytest.mark.gpu

SWEPT = ["two_levels", "levels65", "parallel66", "levels257", "levels600", "fat_column", "colourless", "wide", "full_lds"]
_GRAPHS = {}


def graph_of(name, R=None):
    """graph (with another R if given) and its model -- built once"""
    if (name, R) not in _GRAPHS:
        g = CASES[name][0]()
        if R is not None:
            g = copy.copy(g)
            g.R = R
        _GRAPHS[(name, R)] = (g, PathModel(g))
    return _GRAPHS[(name, R)]


def check_answers(ctx, g, m, outs, budgets):
    """the checks of this file on the run whose outcomes are `outs`; returns {budget: paths}"""
    values = ctx.dp_budget_values()
    got = {b: ctx.dp_answer_paths(b) for b in budgets}
    live = [b for b in budgets if values[b] != NEG_INF]
    for b, out in zip(budgets, outs):
        assert got[b].shape == (2, g.n_levels) and got[b].dtype == np.int32
        assert out.value == values[b]
        if values[b] == NEG_INF:
            assert (got[b] == -1).all(), b
            continue
        for h in range(2):
            assert m.check_path(got[b][h]) is None, (b, h, m.check_path(got[b][h]))       # every vertex in its level, every hop an edge
        assert edge_list(m, got[b][0]) == sorted(out.p1) and edge_list(m, got[b][1]) == sorted(out.p2), b
    if live:
        scored = ctx.dp_score_paths(np.stack([got[b] for b in live]))
        for b, s in zip(live, scored):
            out = outs[budgets.index(b)]
            assert (s["value"], s["s_het"]) == (values[b], out.s_het), (b, s, out.key())
            assert (s["r1"], s["r2"]) == (len(out.p1) - 1, len(out.p2) - 1) and s["r1"] + s["r2"] <= b
    return got


@pytest.mark.parametrize("name", SWEPT)
def test_answer_paths_of_every_budget(gpu_ctx, name):
    g, m = graph_of(name)
    if name == "two_levels":
        assert g.n_levels == 2
    if name in ("levels65", "levels257"):
        assert g.n_levels in (65, 257)                   # one lane per level in blocks of 256: 64 + 1 and 256 + 1
    budgets = list(range(g.R + 1))
    gpu_ctx.dp_load_graph(g)
    outs = gpu_ctx.dp_run_budgets(budgets)
    got = check_answers(gpu_ctx, g, m, outs, budgets)
    values = gpu_ctx.dp_budget_values()
    if name == "parallel66":
        assert g.R == 4 and (values == NEG_INF).all() and all((p == -1).all() for p in got.values())    # no pair fits: an answer, DG_OK
    else:
        assert (values != NEG_INF).any()
    # a plain run afterwards: the one chain of budget R
    out = gpu_ctx.dp_run()
    again = check_answers(gpu_ctx, g, m, [out], [g.R])
    assert np.array_equal(again[g.R], got[g.R])
    assert g.R > 0
    with pytest.raises(capi.DgError, match=r"rc=-6.*dg_dp_get_answer_paths.*budget 0\b"):
        gpu_ctx.dp_answer_paths(0)
    # a subset in another order: chains are found by budget
    if g.R >= 2:
        subset = [g.R, 0, g.R // 2]
        outs = gpu_ctx.dp_run_budgets(subset)
        sub = check_answers(gpu_ctx, g, m, outs, subset)
        for b in subset:
            assert np.array_equal(sub[b], got[b]), b


def test_parallel66_with_a_budget_that_fits(gpu_ctx):
    """no path of parallel66 has fewer than 6 recombinations: with R = 14 the budgets either side of 12 answer differently"""
    g, m = graph_of("parallel66", 14)
    budgets = [11, 12, 13, 14]
    gpu_ctx.dp_load_graph(g)
    outs = gpu_ctx.dp_run_budgets(budgets)
    got = check_answers(gpu_ctx, g, m, outs, budgets)
    values = gpu_ctx.dp_budget_values()
    assert values[11] == NEG_INF and values[12] != NEG_INF and (got[11] == -1).all() and (got[12] >= 0).all()


def test_every_lattice_mode_every_walker_gives_the_same_paths(gpu_ctx):
    g, m = graph_of("levels600", 8)                      # (no pair of its paths has fewer than 4 recombinations: R = 8 gives five answers)
    budgets = list(range(g.R + 1))
    gpu_ctx.dp_load_graph(g)
    outs = gpu_ctx.dp_run_budgets(budgets)
    want = check_answers(gpu_ctx, g, m, outs, budgets)
    assert sum(1 for b in budgets if (want[b] >= 0).all()) == 5
    assert gpu_ctx.dp_timing().n_segments == 1 and gpu_ctx.dp_timing().n_chunks == 1
    cells = int(outs[0].cells)
    for opts in ({"segment_cells": max(1, cells // 4)}, {"segment_cells": max(1, cells // 4), "plane_limit": 0},
                 {"lattice_chunk_cells": max(2, cells // 5)}, {"lean_chain": 0}, {"lean_chain": 1},
                 {"lean_chain": 0, "segment_cells": max(1, cells // 4)}, {"lean_chain": 0, "lattice_chunk_cells": max(2, cells // 5)}):
        with gpu_ctx.dp_options(**opts):
            gpu_ctx.dp_load_graph(g)
            outs2 = gpu_ctx.dp_run_budgets(budgets)
            t = gpu_ctx.dp_timing()
            if "segment_cells" in opts:
                assert t.n_segments >= 3, (opts, t.n_segments)
            if "lattice_chunk_cells" in opts:
                assert t.n_chunks > 1, (opts, t.n_chunks)
            assert [o.key() for o in outs2] == [o.key() for o in outs], opts
            for b in budgets:
                assert np.array_equal(gpu_ctx.dp_answer_paths(b), want[b]), (opts, b)
    gpu_ctx.dp_load_graph(g)                             # the tables of the default options again


def test_the_call_leaves_the_run_alone(gpu_ctx):
    g, m = graph_of("levels65")
    with gpu_ctx.dp_options(digest=1):
        gpu_ctx.dp_load_graph(g)
        outs = gpu_ctx.dp_run_budgets(range(g.R + 1))
        planes = gpu_ctx.dp_budget_values().copy()
        digest = gpu_ctx.dp_level_digest(g.n_levels).copy()
        t = gpu_ctx.dp_timing()
        timing = [getattr(t, f) for f, _ in capi.DpTiming._fields_]
        first = [gpu_ctx.dp_answer_paths(b) for b in range(g.R + 1)]
        again = [gpu_ctx.dp_answer_paths(b) for b in range(g.R + 1)]
        assert all(np.array_equal(a, b) for a, b in zip(first, again))
        assert np.array_equal(gpu_ctx.dp_budget_values(), planes) and np.array_equal(gpu_ctx.dp_level_digest(g.n_levels), digest)
        t = gpu_ctx.dp_timing()
        assert [getattr(t, f) for f, _ in capi.DpTiming._fields_] == timing
        assert [o.key() for o in gpu_ctx.dp_run_budgets(range(g.R + 1))] == [o.key() for o in outs]


def test_errors(gpu_ctx):
    g, m = graph_of("levels65")
    L = g.n_levels
    call = capi.lib.dg_dp_get_answer_paths
    fresh = capi.Context(0)
    try:
        with pytest.raises(capi.DgError, match=r"rc=-6.*dg_dp_get_answer_paths: no graph loaded"):
            fresh.dp_answer_paths(0)
    finally:
        fresh.close()
    out = np.full((2, L), -7, np.int32)
    gpu_ctx.dp_load_graph(g)
    with pytest.raises(capi.DgError, match=r"rc=-6.*dg_dp_get_answer_paths: no completed dg_dp_run"):     # before any run
        gpu_ctx.dp_answer_paths(g.R)
    assert call(gpu_ctx.h, g.R, out.ctypes.data) == -6 and (out == -7).all()
    gpu_ctx.dp_run_budgets([0, 2, g.R])
    want = gpu_ctx.dp_answer_paths(2)
    for b in (1, g.R + 1, -1):                           # budgets the run did not list
        with pytest.raises(capi.DgError, match=rf"rc=-6.*budget {b}\b"):
            gpu_ctx.dp_answer_paths(b)
        assert call(gpu_ctx.h, b, out.ctypes.data) == -6 and (out == -7).all()
    assert call(gpu_ctx.h, 2, None) == -1                # null paths
    assert b"paths" in capi.lib.dg_last_error()
    assert (out == -7).all()
    assert call(gpu_ctx.h, 2, out.ctypes.data) == 0 and np.array_equal(out, want)
    # a failed run takes the answer with it, and so does a load
    with pytest.raises(capi.DgError):
        gpu_ctx.dp_run_budgets([g.R + 1])
    assert np.array_equal(gpu_ctx.dp_answer_paths(2), want)              # (rejected before anything ran: the earlier run still stands)
    gpu_ctx.dp_load_graph(g)
    with pytest.raises(capi.DgError, match=r"rc=-6.*no completed dg_dp_run"):                               # after a reload without a run
        gpu_ctx.dp_answer_paths(2)
    out[:] = -7
    assert call(gpu_ctx.h, 2, out.ctypes.data) == -6 and (out == -7).all()
    gpu_ctx.dp_run()
    assert np.array_equal(gpu_ctx.dp_answer_paths(g.R), gpu_ctx.dp_answer_paths(g.R))
    with pytest.raises(capi.DgError, match=r"rc=-6.*budget 2\b"):
        gpu_ctx.dp_answer_paths(2)

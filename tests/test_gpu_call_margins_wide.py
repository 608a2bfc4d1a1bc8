"""-m gpu: dg_dp_call_margins on the device-memory route (option partner_wide): a run whose answer's own partner budgets are beyond
the 16,384 cells of LDS state -- widest level 260, R = 79, 7 levels, so each haplotype leaves the other at least 79 - 6.

Integers only: every comparison is exact.  The yardstick is tests/call_margins_model.py applied to the pair of paths the call
returns, and the closing check value == the run's value."""
import numpy as np
import pytest

import graphgen
from call_margins_model import call_margins_batch
from dipgenie_amd import capi
from paths_model import NEG_INF, PathModel
from test_gpu_call_margins import _rows

pytestmark = pytest.mark.gpu

MAX_CELLS = 16384


def _three_classes(g, seed):
    """3 classes drawn per level"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 3, g.n_vertices).astype(np.int32)


def _check_model(m, g, got, paths, b, classes, V, tag):
    _, want = call_margins_batch(m, paths[0], paths[1], b, classes)
    for kind, (levels, rec) in enumerate(zip(got, want)):
        bad = np.argwhere((_rows(levels) != rec).any(axis=-1))
        assert bad.size == 0, (tag, kind, bad[:5], _rows(levels)[tuple(bad[:5].T)], rec[tuple(bad[:5].T)])
        assert (levels["value"] == V).all()              # on every level of both rows


def test_answer_beyond_the_lds_limit(gpu_ctx):
    g = graphgen.random_levelized(8826, n_levels=7, max_width=260, min_width=260, R=79, extra_edges=0.2)
    m = PathModel(g)
    classes = [None, _three_classes(g, 11)]
    assert len(set(classes[1][g.level_off[3]:g.level_off[4]].tolist())) == 3
    gpu_ctx.dp_load_graph(g)
    V = gpu_ctx.dp_run().value
    assert V != NEG_INF and V == gpu_ctx.dp_budget_values()[79]
    before = gpu_ctx.dp_partner_route()
    with pytest.raises(capi.DgError, match=r"rc=-5.*dg_dp_call_margins.*\b260\b.*\b80\b.*16384"):              # partner_wide = 0, as ever
        gpu_ctx.dp_call_margins(79)
    assert gpu_ctx.dp_partner_route() == before
    with gpu_ctx.dp_options(partner_wide=1):
        got, paths = [], None
        for cls in classes:
            levels, paths = gpu_ctx.dp_call_margins(79, cls, want_paths=True)
            got.append(levels)
            route = gpu_ctx.dp_partner_route()
            # the queries themselves are beyond LDS: what each haplotype leaves the other
            r = [m.recombinations(p) for p in paths]
            bmax = 79 - min(r)
            assert m.check_path(paths[0]) is None and m.check_path(paths[1]) is None and max(r) <= 6 and 79 - max(r) >= 73
            assert 260 * (79 - max(r) + 1) >= 19240 > MAX_CELLS
            assert route == (2, 260 * (bmax + 1))
    assert np.array_equal(paths, gpu_ctx.dp_answer_paths(79))
    _check_model(m, g, got, paths, 79, classes, V, "beyond")
    inner = got[0][:, 1:-1]
    assert (inner["alt_vertex"] >= 0).any()              # not vacuous: some level has an alternative


def test_budget_beyond_but_queries_that_may_fit(gpu_ctx):
    """the graph of tests/test_gpu_call_margins.py's cell limit: 260 x 64 is refused on the budget itself by default; with partner_wide
    = 1 it answers, on whichever route its two queries need"""
    g = graphgen.random_levelized(8814, n_levels=4, max_width=260, min_width=260, R=63, extra_edges=0.2)
    m = PathModel(g)
    classes = [None, _three_classes(g, 12)]
    gpu_ctx.dp_load_graph(g)
    V = gpu_ctx.dp_run().value
    with pytest.raises(capi.DgError, match=r"rc=-5.*dg_dp_call_margins.*260.*64"):
        gpu_ctx.dp_call_margins(63)
    with gpu_ctx.dp_options(partner_wide=1):
        got = [gpu_ctx.dp_call_margins(63, cls, want_paths=True) for cls in classes]
        assert gpu_ctx.dp_partner_route()[0] in (1, 2)
    paths = got[0][1]
    _check_model(m, g, [lv for lv, _ in got], paths, 63, classes, V, "may fit")


def test_the_wide_cap_on_the_budget(gpu_ctx):
    """widest level 260 x (R + 1) beyond 2^24: refused on the budget itself, naming it and both numbers, nothing written"""
    g = graphgen.random_levelized(8814, n_levels=4, max_width=260, min_width=260, R=63, extra_edges=0.2)
    gpu_ctx.dp_load_graph(g)
    gpu_ctx.dp_run()
    out = np.full((2, 4, 4), -7, np.int32)
    rows = np.full((2, 4), -7, np.int32)
    with gpu_ctx.dp_options(partner_wide=1):
        before = gpu_ctx.dp_partner_route()
        b = (1 << 24) // 260                             # 260 x (b + 1) = 16,777,280
        assert capi.lib.dg_dp_call_margins(gpu_ctx.h, b, None, out.ctypes.data, rows.ctypes.data) == -5
        msg = capi.lib.dg_last_error().decode()
        assert "dg_dp_call_margins" in msg and f"budget {b}" in msg and "260" in msg and str(b + 1) in msg, msg
        assert (out == -7).all() and (rows == -7).all() and gpu_ctx.dp_partner_route() == before

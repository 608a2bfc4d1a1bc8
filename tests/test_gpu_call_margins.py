"""-m gpu: dg_dp_call_margins / Context.dp_call_margins -- per haplotype of the run's own answer and per level, the called vertex,
what the best partner through it is worth with the other haplotype fixed, and the best vertex of another class.

Integers only: every comparison is exact.  The yardstick is tests/call_margins_model.py, itself pinned to brute force by
tests/test_call_margins_model.py, applied to the pair that dp_answer_paths returns (tests/test_gpu_answer_paths.py checks that pair);
the tests against dp_partner_marginals and dp_budget_values need no model at all."""
import numpy as np
import pytest

import graphgen
from call_margins_model import call_margins_batch, class_arrays
from dipgenie_amd import capi
from paths_model import NEG_INF, PathModel
from test_gpu_answer_paths import graph_of
from test_gpu_partner import MAX_CELLS

pytestmark = pytest.mark.gpu

FIELDS = ("vertex", "value", "alt_vertex", "alt_value")
# name -> (R of the load (None: the graph's), budgets asked, the smallest budget a pair of paths fits: twice the fewest recombinations
# of a path, tests/paths_model.py).  No path of parallel66 has fewer than 6: with R = 14 the budgets lie either side of the first pair
# that fits; the only path of two_levels has one
MODEL_CASES = {"two_levels": (None, [0, 1, 2], 2), "levels65": (None, [1, 2, 4, 6], 2), "parallel66": (14, [11, 12, 13, 14], 12),
               "colourless": (None, [1, 2, 3, 4], 2), "fat_column": (None, [0, 2, 3, 4], 0), "wide": (None, [0, 4, 8, 9], 0)}


def _rows(levels):
    return np.stack([levels[f] for f in FIELDS], axis=-1)


def _footprint(g, bmax):
    """bytes of one query in a slab, as include/dipgenie_hip.h states them for dg_dp_partner_marginals"""
    return 4 * g.n_vertices * (bmax + 1) + 2 * len(g.out_dst) + 4 * g.n_vertices + 20 * g.n_levels


def _run(ctx, g, budgets):
    ctx.dp_load_graph(g)
    ctx.dp_run_budgets(budgets)
    return ctx.dp_budget_values()


def _reduce(g, M, called, cls):
    """numpy: per level the best reachable vertex of another class than the called one, the smallest id among equals"""
    out = np.zeros((g.n_levels, 4), np.int32)
    for l in range(g.n_levels):
        a, e = int(g.level_off[l]), int(g.level_off[l + 1])
        ids = np.arange(a, e)
        c = int(called[l])
        keep = ((ids != c) if cls is None else (cls[a:e] != cls[c])) & (M[a:e] != NEG_INF)
        out[l] = (c, M[c], -1, NEG_INF)
        if keep.any():
            cand = ids[keep]
            best = cand[np.argmax(M[cand])]              # the first among equals = the smallest id
            out[l, 2:] = (best, M[best])
    return out


@pytest.mark.parametrize("name", list(MODEL_CASES))
def test_device_equals_model(gpu_ctx, name):
    R, budgets, first_fit = MODEL_CASES[name]
    g, m = graph_of(name, R)
    classes = class_arrays(g, 7)
    values = _run(gpu_ctx, g, budgets)
    assert len(budgets) >= 3 and max(budgets) == g.R
    n_alt = n_zero = n_pos = 0
    for b in budgets:
        got = [gpu_ctx.dp_call_margins(b, cls, want_paths=True) for cls in classes]
        paths = got[0][1]
        assert np.array_equal(paths, gpu_ctx.dp_answer_paths(b)) and all(np.array_equal(p, paths) for _, p in got)
        assert (values[b] == NEG_INF) == (b < first_fit), (b, values[b])
        if values[b] == NEG_INF:
            assert (paths == -1).all()
            for levels, _ in got:
                assert (_rows(levels) == (-1, NEG_INF, -1, NEG_INF)).all()
            continue
        _, want = call_margins_batch(m, paths[0], paths[1], b, classes)
        for kind, ((levels, _), rec) in enumerate(zip(got, want)):
            bad = np.argwhere((_rows(levels) != rec).any(axis=-1))
            assert bad.size == 0, (name, b, kind, bad[:5], _rows(levels)[tuple(bad[:5].T)], rec[tuple(bad[:5].T)])
            assert (levels["value"] == values[b]).all()
        assert (got[1][0]["alt_vertex"] == -1).all() and (got[1][0]["alt_value"] == NEG_INF).all()      # one class for all
        inner = got[0][0][:, 1:-1]
        n_alt += int((inner["alt_vertex"] >= 0).sum())
        n_zero += int(((inner["alt_vertex"] >= 0) & (inner["alt_value"] == inner["value"])).sum())
        n_pos += int(((inner["alt_vertex"] >= 0) & (inner["alt_value"] < inner["value"])).sum())
    assert (values[budgets] != NEG_INF).sum() >= (1 if name == "two_levels" else 3)
    print(f"{name}: inner levels with an alternative {n_alt}, with margin 0 {n_zero}, with a positive margin {n_pos}")
    if name != "two_levels":
        assert n_alt >= 1 and n_zero + n_pos == n_alt, (n_alt, n_zero, n_pos)


@pytest.mark.parametrize("name", ["levels257", "full_lds"])
def test_against_partner_marginals(gpu_ctx, name):
    """no model: the records are a numpy reduction of dp_partner_marginals(the other haplotype, b - r, want_vertices=True)"""
    g, m = graph_of(name)
    widths = np.diff(g.level_off)
    if name == "full_lds":
        assert widths.max() == 128 and g.R == 4         # a level wider than one wave, at a small budget
    classes = class_arrays(g, 8)
    budgets = list(range(g.R + 1))
    values = _run(gpu_ctx, g, budgets)
    assert (values != NEG_INF).all()
    for b in (0, g.R // 2, g.R):
        paths = gpu_ctx.dp_answer_paths(b)
        r = gpu_ctx.dp_score_paths(paths[None])[0]
        assert r["value"] == values[b] and r["r1"] + r["r2"] <= b
        _, M = gpu_ctx.dp_partner_marginals(paths[::-1], [b - r["r2"], b - r["r1"]], want_vertices=True)    # row h: given = the other haplotype
        for cls in classes:
            levels, _ = gpu_ctx.dp_call_margins(b, cls)
            for h in range(2):
                want = _reduce(g, M[h], paths[h], cls)
                bad = np.flatnonzero((_rows(levels[h]) != want).any(axis=-1))
                assert bad.size == 0, (name, b, h, bad[:5], _rows(levels[h])[bad[:5]], want[bad[:5]])
            assert (levels["value"] == values[b]).all()  # value == V_b on every level of both rows
    assert np.array_equal(gpu_ctx.dp_budget_values(), values)


def test_levels_without_an_alternative(gpu_ctx):
    """a level of width 1, and a level whose vertices all share the called vertex's class: -1 and NEG_INF"""
    g, m = graph_of("levels65")
    widths = np.diff(g.level_off)
    values = _run(gpu_ctx, g, [g.R])
    cls = class_arrays(g, 9)[2].copy()
    one = np.flatnonzero(widths[1:-1] == 1) + 1
    shared = int(np.argmax(widths))                      # the widest level gets one class
    assert widths[shared] >= 4 and widths[0] == 1 and widths[-1] == 1
    cls[g.level_off[shared]:g.level_off[shared + 1]] = 5
    for c in (None, cls):
        levels, _ = gpu_ctx.dp_call_margins(g.R, c)
        for l in [0, g.n_levels - 1, *one.tolist()] + ([shared] if c is not None else []):
            assert (levels["alt_vertex"][:, l] == -1).all() and (levels["alt_value"][:, l] == NEG_INF).all(), l
            assert (levels["value"][:, l] == values[g.R]).all()
    free, _ = gpu_ctx.dp_call_margins(g.R, None)
    assert (free["alt_vertex"][:, shared] >= 0).any()    # without classes that level has an alternative


def test_one_slab_or_two(gpu_ctx):
    g, m = graph_of("wide")
    values = _run(gpu_ctx, g, range(g.R + 1))
    cls = class_arrays(g, 10)[2]
    for b in (g.R, g.R // 2):
        paths = gpu_ctx.dp_answer_paths(b)
        r = gpu_ctx.dp_score_paths(paths[None])[0]
        bmax = b - min(int(r["r1"]), int(r["r2"]))
        one, p1 = gpu_ctx.dp_call_margins(b, cls, want_paths=True)                       # the default holds both queries
        for nbytes in (_footprint(g, bmax), 2 * _footprint(g, bmax) - 1, 1):             # one query per slab
            with gpu_ctx.dp_options(partner_slab_bytes=nbytes):
                two, p2 = gpu_ctx.dp_call_margins(b, cls, want_paths=True)
            assert np.array_equal(one, two) and np.array_equal(p1, p2), (b, nbytes)
        with gpu_ctx.dp_options(partner_slab_bytes=2 * _footprint(g, bmax)):             # exactly both
            two, _ = gpu_ctx.dp_call_margins(b, cls)
        assert np.array_equal(one, two)


def test_the_call_leaves_the_run_alone(gpu_ctx):
    g, m = graph_of("levels65")
    with gpu_ctx.dp_options(digest=1):
        gpu_ctx.dp_load_graph(g)
        outs = gpu_ctx.dp_run_budgets(range(g.R + 1))
        planes = gpu_ctx.dp_budget_values().copy()
        digest = gpu_ctx.dp_level_digest(g.n_levels).copy()
        assert digest[1:].any()
        t = gpu_ctx.dp_timing()
        timing = [getattr(t, f) for f, _ in capi.DpTiming._fields_]
        first = [gpu_ctx.dp_call_margins(b, want_paths=True) for b in range(g.R + 1)]
        assert np.array_equal(gpu_ctx.dp_budget_values(), planes) and np.array_equal(gpu_ctx.dp_level_digest(g.n_levels), digest)
        t = gpu_ctx.dp_timing()
        assert [getattr(t, f) for f, _ in capi.DpTiming._fields_] == timing
        again = [gpu_ctx.dp_call_margins(b, want_paths=True) for b in range(g.R + 1)]
        for (l1, p1), (l2, p2) in zip(first, again):
            assert np.array_equal(l1, l2) and np.array_equal(p1, p2)
        assert [o.key() for o in gpu_ctx.dp_run_budgets(range(g.R + 1))] == [o.key() for o in outs]      # and the next run answers as before
        assert np.array_equal(gpu_ctx.dp_level_digest(g.n_levels), digest)


def test_errors_and_layout(gpu_ctx):
    assert capi.CALL_MARGIN.itemsize == 16 and capi.CALL_MARGIN.names == FIELDS
    g, m = graph_of("levels65")
    L = g.n_levels
    call = capi.lib.dg_dp_call_margins
    fresh = capi.Context(0)
    try:
        with pytest.raises(capi.DgError, match=r"rc=-6.*dg_dp_call_margins: no graph loaded"):
            fresh.dp_call_margins(0)
    finally:
        fresh.close()
    out = np.full((2, L, 4), -7, np.int32)
    rows = np.full((2, L), -7, np.int32)

    def untouched():
        return (out == -7).all() and (rows == -7).all()

    gpu_ctx.dp_load_graph(g)
    with pytest.raises(capi.DgError, match=r"rc=-6.*dg_dp_call_margins: no completed dg_dp_run"):
        gpu_ctx.dp_call_margins(g.R)
    assert call(gpu_ctx.h, g.R, None, out.ctypes.data, rows.ctypes.data) == -6 and untouched()
    gpu_ctx.dp_run_budgets([0, 2, g.R])
    for b in (1, g.R + 1, -1):
        with pytest.raises(capi.DgError, match=rf"rc=-6.*dg_dp_call_margins.*budget {b}\b"):
            gpu_ctx.dp_call_margins(b)
        assert call(gpu_ctx.h, b, None, out.ctypes.data, rows.ctypes.data) == -6 and untouched()
    assert call(gpu_ctx.h, 2, None, None, rows.ctypes.data) == -1 and untouched()
    with pytest.raises(ValueError):
        gpu_ctx.dp_call_margins(2, np.zeros(g.n_vertices - 1, np.int32))
    want, paths = gpu_ctx.dp_call_margins(2, want_paths=True)
    assert call(gpu_ctx.h, 2, None, out.ctypes.data, rows.ctypes.data) == 0              # four words per (row, level)
    assert np.array_equal(out, _rows(want)) and np.array_equal(rows, paths)
    gpu_ctx.dp_load_graph(g)                             # after a reload without a run
    with pytest.raises(capi.DgError, match=r"rc=-6.*no completed dg_dp_run"):
        gpu_ctx.dp_call_margins(2)
    # the cell limit, on the budget itself: widest level 260, R = 63
    wide = graphgen.random_levelized(8814, n_levels=4, max_width=260, min_width=260, R=63, extra_edges=0.2)
    assert np.diff(wide.level_off).max() == 260 and 260 * 64 > MAX_CELLS
    gpu_ctx.dp_load_graph(wide)
    gpu_ctx.dp_run()
    out[:] = -7
    rows[:] = -7
    with pytest.raises(capi.DgError, match=r"rc=-5.*dg_dp_call_margins.*260.*64"):
        gpu_ctx.dp_call_margins(63)
    assert call(gpu_ctx.h, 63, None, out.ctypes.data, rows.ctypes.data) == -5 and untouched()
    assert gpu_ctx.dp_answer_paths(63).shape == (2, 4)  # the paths themselves have no such limit

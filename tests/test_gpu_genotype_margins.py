"""-m gpu: dg_dp_genotype_margins / Context.dp_genotype_margins -- the best pair of paths through every cell of a level with both
haplotypes free, per level the called cell against the best cell of another genotype, the joint marginal of every vertex.

Integers only: every comparison is exact.  The yardstick is tests/genotype_margins_model.py, itself pinned to brute force by
tests/test_genotype_margins_model.py; the tests on the widest graph need no model: they hold the call against dp_solve,
dp_score_paths, dp_partner_marginals and dp_call_margins."""
import numpy as np
import pytest

import graphgen
from call_margins_model import class_arrays
from dipgenie_amd import capi
from genotype_margins_model import genotype_margins_np, through_values_np
from paths_model import NEG_INF, PathModel
from test_gpu_score_paths import ENUMERABLE
from test_partner_model import enumerable_graph

pytestmark = pytest.mark.gpu

FIELDS = ("vertex1", "vertex2", "value", "alt_vertex1", "alt_vertex2", "alt_value")
MAX_PLANES, MAX_QUERIES = 4096, 256                     # the limits include/dipgenie_hip.h states


def _rows(levels):
    assert (levels["reserved"] == 0).all()
    return np.stack([levels[f] for f in FIELDS], axis=-1)


def _called(m, rng, best=None):
    """[n, 2, L]: the given optimal pair (if any), a sampled pair of paths, and a list of cells that is no pair of paths"""
    paths, _ = m.sample_paths(rng, 2)
    cells = np.array([[rng.integers(m.level_off[l], m.level_off[l + 1]) for l in range(m.L)] for _ in range(2)], np.int32)
    return np.stack(([np.asarray(best, np.int32)] if best is not None else []) + [paths, cells]).astype(np.int32)


def _compare(ctx, g, m, b, called, classes, tag):
    """every field of every record, best_value and vertex_values against the numpy model, for each class array"""
    T, V = through_values_np(m, b)
    for kind, cls in enumerate(classes):
        want, _, J = genotype_margins_np(m, called, b, cls, T, V)
        levels, best, vv = ctx.dp_genotype_margins(called, b, cls, want_vertices=True)
        assert levels.shape == (len(called), g.n_levels) and best == V, (tag, b, kind, best, V)
        bad = np.argwhere((_rows(levels) != want).any(axis=-1))
        assert bad.size == 0, (tag, b, kind, bad[:5], _rows(levels)[tuple(bad[:5].T)], want[tuple(bad[:5].T)])
        assert np.array_equal(vv, J), (tag, b, kind, np.flatnonzero(vv != J)[:5])
    return T, V


@pytest.mark.parametrize("q", range(len(ENUMERABLE)))
def test_device_equals_model_on_the_enumerable_graphs(gpu_ctx, q):
    g = enumerable_graph(q)
    m = PathModel(g)
    gpu_ctx.dp_load_graph(g)
    gpu_ctx.dp_run_budgets(range(g.R + 1))
    planes = gpu_ctx.dp_budget_values()
    rng = np.random.default_rng(40 + q)
    for b in range(4):
        best = gpu_ctx.dp_answer_paths(b) if planes[b] != NEG_INF else None
        called = _called(m, rng, best)
        T, V = _compare(gpu_ctx, g, m, b, called, class_arrays(g, 21 + q), q)
        assert V == planes[b]
        if best is not None:                             # the run's answer is an optimal pair: its cell is worth V on every level
            levels, _ = gpu_ctx.dp_genotype_margins(best, b)
            assert (levels["value"] == V).all() and (levels["alt_value"] <= V).all()


WIDTHS = [[1, 1, 1], [1, 2, 1], [1, 3, 64, 65, 2, 1], [1, 63, 64, 1], [1, 70, 5, 70, 1]]
BUDGETS = [0, 1, 2, 7, 18]                              # 19 planes: no power of two, and more than the graphs' R


@pytest.mark.parametrize("w", range(len(WIDTHS)))
def test_device_equals_model_on_prescribed_widths(gpu_ctx, w):
    unreached = unreachable_planes = 0
    for k, p_w1 in enumerate((0.0, 0.3, 1.0)):
        g = graphgen.random_levelized(9100 + 10 * w + k, widths=WIDTHS[w], R=3, p_w1=p_w1, dup_edges=True, extra_edges=1.2, p_colour=0.5)
        m = PathModel(g)
        indeg = np.bincount(g.out_dst, minlength=g.n_vertices)
        unreached += int((indeg[1:] == 0).sum())
        gpu_ctx.dp_load_graph(g)
        rng = np.random.default_rng(50 + w)
        classes = class_arrays(g, 31 + w)
        for b in BUDGETS:
            T, V = _compare(gpu_ctx, g, m, b, _called(m, rng), classes if b in (2, 18) else classes[2:], (w, p_w1))
            unreachable_planes += V == NEG_INF
    if max(WIDTHS[w]) >= 63:
        assert unreached >= 1                            # vertices that nothing reaches: the generator leaves some
    if len(WIDTHS[w]) >= 4:
        assert unreachable_planes >= 1                   # p_w1 = 1.0: every path has L - 1 recombinations


_WIDE = {}


def wide_case(ctx):
    """widths [1, 130, 300, 129, 1], R = 18: graph, model, the run's planes -- loaded and run here, so call it first"""
    if not _WIDE:
        g = graphgen.random_levelized(9200, widths=[1, 130, 300, 129, 1], R=18, p_w1=0.3, extra_edges=1.5, p_colour=0.5)
        _WIDE["g"], _WIDE["m"] = g, PathModel(g)
    g, m = _WIDE["g"], _WIDE["m"]
    ctx.dp_load_graph(g)
    ctx.dp_run_budgets([2, 18])
    return g, m, ctx.dp_budget_values().copy()


@pytest.mark.parametrize("b", [2, 18])
def test_wider_than_any_tile_without_a_model(gpu_ctx, b):
    g, m, planes = wide_case(gpu_ctx)
    assert b <= g.R and planes[b] != NEG_INF
    paths = gpu_ctx.dp_answer_paths(b)
    cls = class_arrays(g, 41)[2]
    levels, best, J = gpu_ctx.dp_genotype_margins(paths, b, cls, want_vertices=True)
    assert best == planes[b]
    assert (levels["value"] == best).all()
    assert (levels["value"] - levels["alt_value"] >= 0).all()
    assert (levels["alt_vertex1"] <= levels["alt_vertex2"]).all()
    assert (levels["alt_vertex1"][0, 1:-1] >= 0).all()      # hundreds of reachable cells and 2..4 classes per level: another genotype exists
    r = gpu_ctx.dp_score_paths(paths[None])[0]
    assert 300 * (b + 1) <= 16384                        # dp_partner_marginals holds the level state in LDS: partner_wide stays 0
    _, M = gpu_ctx.dp_partner_marginals(paths[::-1], [b - int(r["r2"]), b - int(r["r1"])], want_vertices=True)
    assert (J[None, :] >= M).all()
    pairs, rec = m.sample_pairs(np.random.default_rng(b), 200, p_w0=0.9)
    scores = gpu_ctx.dp_score_paths(pairs)
    fits = (scores["r1"] + scores["r2"]) <= b
    assert fits.sum() >= 20
    for h in range(2):                                   # T at each of the pair's cells is at most J of both of its vertices
        assert (scores["value"][fits, None] <= J[pairs[fits, h, :]]).all()
    assert J.max() == best


def _state_bytes(g, b):
    return 4 * (np.diff(g.level_off).astype(np.int64) ** 2) * (b + 1)


@pytest.mark.parametrize("which", ["prescribed", "wide"])
def test_segments_change_nothing(gpu_ctx, which):
    if which == "wide":
        g, m, _ = wide_case(gpu_ctx)
        b = 18
    else:
        g = graphgen.random_levelized(9130, widths=WIDTHS[2], R=3, p_w1=0.3, dup_edges=True, extra_edges=1.2, p_colour=0.5)
        m = PathModel(g)
        gpu_ctx.dp_load_graph(g)
        b = 7
    called = _called(m, np.random.default_rng(3))
    cls = class_arrays(g, 51)[2]
    L = g.n_levels
    ragged = int(2.5 * _state_bytes(g, b).mean())
    got = {}
    for name, nbytes in (("every level", 1), ("ragged", ragged), ("default", 0)):
        with gpu_ctx.dp_options(joint_state_bytes=nbytes):
            got[name] = gpu_ctx.dp_genotype_margins(called, b, cls, want_vertices=True)
        got[name + " stats"] = gpu_ctx.dp_genotype_stats()
    for name in ("ragged", "default"):
        for x, y in zip(got["every level"], got[name]):
            assert np.array_equal(x, y), name
    assert got["every level stats"]["n_segments"] == L and got["every level stats"]["levels_twice"] == 0
    assert 1 < got["ragged stats"]["n_segments"] < L and got["ragged stats"]["levels_twice"] >= 1
    assert got["default stats"]["n_segments"] == 1 and got["default stats"]["levels_twice"] == 0
    for name in ("every level", "ragged", "default"):
        assert got[name + " stats"]["peak_bytes"] >= int(_state_bytes(g, b).max()) and got[name + " stats"]["launches"] >= 3 * L
    assert gpu_ctx.dp_get_option("joint_state_bytes") == 8 << 30


@pytest.mark.parametrize("seed", [9301, 9302])
def test_joint_margin_is_at_most_each_conditional_margin(gpu_ctx, seed):
    g = graphgen.random_levelized(seed, n_levels=14, max_width=9, min_width=2, R=4, p_w1=0.3, extra_edges=1.5, p_colour=0.5)
    gpu_ctx.dp_load_graph(g)
    gpu_ctx.dp_run()
    V = gpu_ctx.dp_budget_values()[g.R]
    assert V != NEG_INF
    compared = smaller = 0
    for cls in class_arrays(g, seed):
        cond, paths = gpu_ctx.dp_call_margins(g.R, cls, want_paths=True)
        joint, best = gpu_ctx.dp_genotype_margins(paths, g.R, cls)
        assert best == V and (joint["value"] == V).all() and (cond["value"] == V).all()
        for h in range(2):
            has = cond["alt_vertex"][h] >= 0
            assert (joint["alt_vertex1"][0][has] >= 0).all()                # a conditional alternative is a joint alternative
            assert (joint["alt_value"][0][has] >= cond["alt_value"][h][has]).all()
            compared += int(has.sum())
            smaller += int((joint["alt_value"][0][has] > cond["alt_value"][h][has]).sum())
    print(f"seed {seed}: (haplotype, level) with a conditional alternative {compared}, joint margin strictly smaller {smaller}")
    assert compared >= 1


def test_the_call_leaves_the_run_alone(gpu_ctx):
    g = graphgen.random_levelized(9401, n_levels=30, max_width=9, R=4, p_colour=0.5)
    m = PathModel(g)
    with gpu_ctx.dp_options(digest=1):
        gpu_ctx.dp_load_graph(g)
        outs = gpu_ctx.dp_run_budgets(range(g.R + 1))
        planes = gpu_ctx.dp_budget_values().copy()
        digest = gpu_ctx.dp_level_digest(g.n_levels).copy()
        assert digest[1:].any()
        paths = [gpu_ctx.dp_answer_paths(b).copy() for b in range(g.R + 1)]
        t = gpu_ctx.dp_timing()
        timing = [getattr(t, f) for f, _ in capi.DpTiming._fields_]
        called = _called(m, np.random.default_rng(5), paths[g.R])
        first = [gpu_ctx.dp_genotype_margins(called, b, want_vertices=True) for b in (0, g.R, g.R + 3)]
        assert np.array_equal(gpu_ctx.dp_budget_values(), planes) and np.array_equal(gpu_ctx.dp_level_digest(g.n_levels), digest)
        for b in range(g.R + 1):
            assert np.array_equal(gpu_ctx.dp_answer_paths(b), paths[b])
        t = gpu_ctx.dp_timing()
        assert [getattr(t, f) for f, _ in capi.DpTiming._fields_] == timing
        again = [gpu_ctx.dp_genotype_margins(called, b, want_vertices=True) for b in (0, g.R, g.R + 3)]
        for one, two in zip(first, again):
            assert all(np.array_equal(x, y) for x, y in zip(one, two))
        assert [o.key() for o in gpu_ctx.dp_run_budgets(range(g.R + 1))] == [o.key() for o in outs]      # and the next run answers as before
        assert np.array_equal(gpu_ctx.dp_level_digest(g.n_levels), digest)


def test_errors_and_layout(gpu_ctx):
    assert capi.GENOTYPE_MARGIN.itemsize == 32 and capi.GENOTYPE_MARGIN.names == FIELDS + ("reserved",)
    g = graphgen.random_levelized(9501, widths=[1, 4, 6, 3, 1], R=3, p_colour=0.5)
    m = PathModel(g)
    L = g.n_levels
    call = capi.lib.dg_dp_genotype_margins
    fresh = capi.Context(0)
    try:
        with pytest.raises(capi.DgError, match=r"rc=-6.*dg_dp_genotype_margins: no graph loaded"):
            fresh.dp_genotype_margins(np.zeros((2, L), np.int32), 0)
    finally:
        fresh.close()
    gpu_ctx.dp_load_graph(g)
    called = _called(m, np.random.default_rng(6))
    n = len(called)
    out = np.full((n, L, 8), -7, np.int32)
    vv = np.full(g.n_vertices, -7, np.int32)
    best = capi.C.c_int32(-7)

    def raw(p, count, b):
        return call(gpu_ctx.h, p.ctypes.data if p is not None else None, count, b, None, out.ctypes.data, vv.ctypes.data, capi.C.byref(best))

    def untouched():
        return (out == -7).all() and (vv == -7).all() and best.value == -7

    bad = called.copy()
    bad[1, 1, 2] = g.level_off[3]                        # query 1, row 1, level 2: the first vertex of level 3
    bad[1, 1, 3] = 0                                     # (a later one too: the first is named)
    with pytest.raises(capi.DgError, match=r"rc=-1.*dg_dp_genotype_margins.*query 1 row 1 level 2\b"):
        gpu_ctx.dp_genotype_margins(bad, 2)
    assert raw(bad, n, 2) == -1 and untouched()
    bad = called.copy()
    bad[0, 0, 0] = -1
    with pytest.raises(capi.DgError, match=r"rc=-1.*query 0 row 0 level 0\b"):
        gpu_ctx.dp_genotype_margins(bad, 2)
    with pytest.raises(capi.DgError, match=r"rc=-1.*dg_dp_genotype_margins.*budget -1"):
        gpu_ctx.dp_genotype_margins(called, -1)
    assert raw(called, n, -1) == -1 and untouched()
    with pytest.raises(capi.DgError, match=r"rc=-1.*dg_dp_genotype_margins.*n_called = 0"):
        gpu_ctx.dp_genotype_margins(called[:0], 2)
    assert raw(called, 0, 2) == -1 and raw(None, n, 2) == -1 and untouched()
    assert call(gpu_ctx.h, called.ctypes.data, n, 2, None, None, None, capi.C.byref(best)) == -1
    assert call(gpu_ctx.h, called.ctypes.data, n, 2, None, out.ctypes.data, None, None) == -1 and untouched()
    with pytest.raises(capi.DgError, match=rf"rc=-5.*dg_dp_genotype_margins.*\b{MAX_PLANES + 1}\b.*\b{MAX_PLANES}\b"):
        gpu_ctx.dp_genotype_margins(called, MAX_PLANES)
    assert raw(called, n, MAX_PLANES) == -5 and untouched()
    many = np.repeat(called[:1], MAX_QUERIES + 1, axis=0)
    with pytest.raises(capi.DgError, match=rf"rc=-5.*dg_dp_genotype_margins.*\b{MAX_QUERIES + 1}\b.*\b{MAX_QUERIES}\b"):
        gpu_ctx.dp_genotype_margins(many, 2)
    with pytest.raises(ValueError):
        gpu_ctx.dp_genotype_margins(called[:, :, :-1], 2)
    with pytest.raises(ValueError):
        gpu_ctx.dp_genotype_margins(called, 2, np.zeros(g.n_vertices - 1, np.int32))
    # the raw call writes eight words per (query, level): the six fields and two zeros
    want, V, J = gpu_ctx.dp_genotype_margins(called, 2, want_vertices=True)
    assert raw(called, n, 2) == 0 and best.value == V and np.array_equal(vv, J)
    assert np.array_equal(out[:, :, :6], _rows(want)) and (out[:, :, 6:] == 0).all()
    # a [2, L] array is one query
    one, V1 = gpu_ctx.dp_genotype_margins(called[1], 2)
    assert one.shape == (1, L) and V1 == V and np.array_equal(one[0], want[1])
    # the most queries a call takes
    full, Vf = gpu_ctx.dp_genotype_margins(np.tile(called, (MAX_QUERIES // n + 1, 1, 1))[:MAX_QUERIES], 2)
    assert Vf == V and np.array_equal(full[:n], want) and np.array_equal(full[-1], want[(MAX_QUERIES - 1) % n])


def test_a_budget_nobody_fits(gpu_ctx):
    """a chain of width 1 with one level whose only edge has weight 1: at b = 0 no pair fits (both paths pay it, so b = 1 does not
    either); DG_OK, NEG_INF / -1 everywhere"""
    g = graphgen.random_levelized(9601, widths=[1, 1, 1, 1, 1], R=2, p_w1=0.0, dup_edges=False, extra_edges=0.0)
    w = g.out_w.copy()
    w[2] = 1
    g = capi.DpGraphArrays(g.R, **{**{name: getattr(g, name) for name in capi.DpGraphArrays.NAMES}, "out_w": w})
    assert len(g.out_dst) == 4 and g.out_w.tolist() == [0, 0, 1, 0]
    gpu_ctx.dp_load_graph(g)
    called = np.arange(5, dtype=np.int32)[None, :].repeat(2, axis=0)
    for b in (0, 1):
        levels, best, J = gpu_ctx.dp_genotype_margins(called, b, want_vertices=True)
        assert best == NEG_INF and (J == NEG_INF).all()
        assert (_rows(levels)[0] == np.array([[v, v, NEG_INF, -1, -1, NEG_INF] for v in range(5)])).all()
    levels, best = gpu_ctx.dp_genotype_margins(called, 2)
    assert best != NEG_INF and (levels["value"] == best).all() and (levels["alt_vertex1"] == -1).all()

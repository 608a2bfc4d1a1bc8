"""-m gpu: dg_dp_score_paths / Context.dp_score_paths -- caller-supplied pairs of paths scored on the loaded graph.

Integers only: every comparison is exact.  The yardstick is tests/paths_model.py, itself pinned to the oracle by
tests/test_paths_model.py; the optimality test needs neither reference nor oracle to be right about any single path: no sampled
pair may beat the plane of the sweep that its recombinations fit."""
import copy

import numpy as np
import pytest

import graphgen
import oracle_py as orc
from dipgenie_amd import capi
from paths_model import NEG_INF, PathModel, repeat_edge, strip_colours

pytestmark = pytest.mark.gpu

N_PAIRS = 500


def _fat_column():
    """a column of in-degree > 64: one in-edge of a mid-level vertex listed 70 more times (parallel, equal weight)"""
    g = graphgen.random_levelized(8804, n_levels=20, max_width=12, R=4, p_colour=0.5)
    return repeat_edge(g, int(g.out_off[g.level_off[9]]), 70)


# width <= 12; depths up to 40, plus 2 (source -> sink only), 65 / 66 (one full wave / one transition more), 257 (one full
# workgroup) and 600 (three level blocks per pair, the last one partly filled)
DEVICE_MODEL = {
    "wide40": lambda: graphgen.random_levelized(8800, n_levels=40, max_width=12, R=6, p_colour=0.5),
    "two_levels": lambda: graphgen.random_levelized(8801, n_levels=2, R=2),
    "levels65": lambda: graphgen.random_levelized(8802, n_levels=65, max_width=8, R=6),
    "levels257": lambda: graphgen.random_levelized(8803, n_levels=257, max_width=6, R=6, p_w1=0.1),
    "fat_column": _fat_column,
    "colourless": lambda: strip_colours(graphgen.random_levelized(8805, n_levels=30, max_width=10, R=4), [0, 4, 5, 6, 11, 20, 21, 29]),
    "parallel66": lambda: graphgen.random_levelized(8806, n_levels=66, max_width=5, R=4, extra_edges=3.0),
    "levels600": lambda: graphgen.random_levelized(8808, n_levels=600, max_width=4, R=4, p_w1=0.05, max_list=6),
}


def _pairs(m, seed, n):
    """half uniform, half biased towards weight-0 edges"""
    rng = np.random.default_rng(seed)
    a, ra = m.sample_pairs(rng, n - n // 2)
    b, rb = m.sample_pairs(rng, n // 2, 0.9)
    return np.concatenate([a, b]), np.concatenate([ra, rb])


def _as_rows(res):
    return np.stack([res["value"], res["s_het"], res["r1"], res["r2"]], axis=1)


def _values_per_budget(g):
    out = []
    for b in range(g.R + 1):
        gb = copy.copy(g)
        gb.R = b
        out.append(orc.dp_solve(gb)["value"])
    return out


@pytest.mark.parametrize("name", list(DEVICE_MODEL))
def test_device_equals_model(gpu_ctx, name):
    g = DEVICE_MODEL[name]()
    m = PathModel(g)
    if name == "fat_column":
        indeg = np.bincount(g.out_dst, minlength=g.n_vertices)
        assert indeg.max() > 64
    if name == "colourless":
        assert sum(1 for l in range(1, g.n_levels) if not any(m.hom[v] or m.het[v] for v in range(g.level_off[l - 1], g.level_off[l + 1]))) >= 2
    if name in ("parallel66", "fat_column"):
        pairs_of_ends = list(zip(np.repeat(np.arange(g.n_vertices), np.diff(g.out_off)), g.out_dst))
        assert len(set(pairs_of_ends)) < len(pairs_of_ends)
    paths, rec = _pairs(m, 31, N_PAIRS)
    want = m.score_many(paths)
    assert np.array_equal(want[:, 2:], rec)
    gpu_ctx.dp_load_graph(g)                             # no run before the scoring call
    with gpu_ctx.dp_options(**({"score_slab_bytes": 64 * 2 * g.n_levels * 4} if name in ("wide40", "fat_column", "levels600") else {})):   # 64 pairs per slab: 8 slabs, the last one short
        got = _as_rows(gpu_ctx.dp_score_paths(paths))
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (name, bad[:5], got[bad[:5]], want[bad[:5]])
    assert want[:, 0].max() > 0 or name == "two_levels"
    # one pair, and the same pairs one per slab
    one = _as_rows(gpu_ctx.dp_score_paths(paths[7:8]))
    assert np.array_equal(one, want[7:8])
    with gpu_ctx.dp_options(score_slab_bytes=1):
        assert np.array_equal(_as_rows(gpu_ctx.dp_score_paths(paths[:5])), want[:5])


ENUMERABLE = [(7115, 10, 0.5, 0.25, 0.3), (7101, 9, 0.6, 0.4, 0.2), (7129, 6, 1.0, 0.3, 0.4), (7126, 9, 0.6, 0.4, 0.2), (7100, 6, 1.0, 0.3, 0.4)]


def _consistent(m, path, edges):
    """is `path` a path whose weight-1 edges, followed by its last edge, are the result's edge list (approximator.cpp:673-692)"""
    mine = [(int(path[l - 1]), int(path[l])) for l in range(1, m.L) if m.succ[int(path[l - 1])][int(path[l])] == 1]
    mine.append((int(path[m.L - 2]), int(path[m.L - 1])))
    return mine == list(edges)


def walked_pairs_score_their_plane(ctx, g, m, what):
    """the check of test_walked_paths_score_their_plane on one enumerable graph (m = PathModel(g)); returns, per reachable budget,
    (budget, the candidate pairs [n, 2, L], the device's records of them, the index of one that is worth the plane)"""
    all_paths = m.all_paths()
    ctx.dp_load_graph(g)
    outs = ctx.dp_run_budgets(range(g.R + 1))
    values = ctx.dp_budget_values()
    checked = []
    for b, out in enumerate(outs):
        assert out.value == values[b]
        if out.value == NEG_INF:
            continue
        c1 = [p for p in all_paths if _consistent(m, p, out.p1)]
        c2 = [p for p in all_paths if _consistent(m, p, out.p2)]
        assert c1 and c2, (what, b)
        cand = np.array([[p, q] for p in c1 for q in c2], np.int32)
        got = ctx.dp_score_paths(cand)
        assert (got["r1"] == len(out.p1) - 1).all() and (got["r2"] == len(out.p2) - 1).all()
        assert (got["r1"] + got["r2"] <= b).all() and (got["value"] <= out.value).all(), (what, b)
        hit = (got["value"] == out.value) & (got["s_het"] == out.s_het)
        assert hit.any(), (what, b, out.key(), got)
        checked.append((b, cand, got, int(np.argmax(hit))))
    return checked


def test_walked_paths_score_their_plane(gpu_ctx):
    """every reachable budget's two paths, rebuilt from the returned edge lists plus the graph (all paths that spend exactly those
    weight-1 edges; stretches of weight-0 edges may leave a choice), scored by the device: r1 / r2 are the lists' lengths, none
    beats the plane's value and one is worth exactly the plane's value with the result's s_het"""
    n_checked = 0
    for seed, n_levels, extra, p_w1, p_colour in ENUMERABLE:
        g = graphgen.random_levelized(seed, n_levels=n_levels, max_width=4, R=3, extra_edges=extra, p_w1=p_w1, p_colour=p_colour)
        n_checked += len(walked_pairs_score_their_plane(gpu_ctx, g, PathModel(g), seed))
    assert n_checked >= 12, n_checked


OPTIMALITY = [(8901, 0.08), (8902, 0.12), (8903, 0.04), (8904, 0.12)]      # (seed, share of weight-1 edges): every plane 0..R gets samples
_OPT = {}


def _optimality_case(q):
    """graph, 20,000 sampled pairs with their (r1, r2), the oracle's value per budget -- computed once"""
    if q not in _OPT:
        seed, p_w1 = OPTIMALITY[q]
        g = graphgen.random_levelized(seed, n_levels=60, max_width=8, min_width=6, R=6, p_w1=p_w1, p_colour=0.5)
        m = PathModel(g)
        rng = np.random.default_rng(seed)
        parts = [m.sample_pairs(rng, 5000), m.sample_pairs(rng, 5000, 0.8), m.sample_pairs(rng, 5000, 0.95), m.sample_pairs(rng, 5000, 0.995)]
        paths = np.concatenate([p for p, _ in parts])
        rec = np.concatenate([r for _, r in parts])
        _OPT[q] = (g, m, paths, rec, _values_per_budget(g))
    return _OPT[q]


@pytest.mark.parametrize("q", range(len(OPTIMALITY)))
def test_no_sampled_pair_beats_its_plane(gpu_ctx, q):
    g, m, paths, rec, oracle_values = _optimality_case(q)
    assert paths.shape == (20000, 2, 60)
    # CPU first: the seeds give samples on at least three planes, and the model agrees with the oracle about a few of them
    r = rec.sum(axis=1)
    planes = sorted(set(int(x) for x in r[r <= g.R]))
    print(f"graph {q}: samples per plane {[int((r == b).sum()) for b in range(g.R + 1)]}, beyond R {int((r > g.R).sum())}, oracle {oracle_values}")
    assert len(planes) >= 3, planes
    some = np.flatnonzero(r <= g.R)[:: max(1, int((r <= g.R).sum()) // 200)]
    for idx in some:
        assert m.score(paths[idx, 0], paths[idx, 1])[0] <= oracle_values[int(r[idx])]
    # the device: one call
    gpu_ctx.dp_load_graph(g)
    gpu_ctx.dp_run_budgets(range(g.R + 1))
    values = gpu_ctx.dp_budget_values()
    assert list(values) == oracle_values
    got = gpu_ctx.dp_score_paths(paths)
    assert np.array_equal(got["r1"], rec[:, 0]) and np.array_equal(got["r2"], rec[:, 1])
    rr = got["r1"] + got["r2"]
    within = rr <= g.R
    assert within.any()                                  # not vacuous
    best = [int(got["value"][rr == b].max()) if (rr == b).any() else None for b in range(g.R + 1)]
    print(f"graph {q}: optimum per plane {list(values)}, best sample per plane {best}")
    over = np.flatnonzero(within & (got["value"] > values[np.minimum(rr, g.R)]))
    assert over.size == 0, (q, over[:5], got[over[:5]])
    assert all(values[b] != NEG_INF for b in planes)     # a sample on a plane means the plane is reachable
    for idx in some:
        assert tuple(got[idx]) == m.score(paths[idx, 0], paths[idx, 1])


def test_errors(gpu_ctx):
    g = DEVICE_MODEL["wide40"]()
    m = PathModel(g)
    L = g.n_levels
    paths, _ = _pairs(m, 77, 300)
    want = m.score_many(paths)
    fresh = capi.Context(0)
    try:
        with pytest.raises(capi.DgError, match=r"rc=-6.*no graph loaded"):
            fresh.dp_score_paths(paths)
    finally:
        fresh.close()
    gpu_ctx.dp_load_graph(g)
    assert gpu_ctx.dp_score_paths(np.zeros((0, 2, L), np.int32)).size == 0            # n_pairs = 0
    assert capi.lib.dg_dp_score_paths(gpu_ctx.h, None, 0, None) == 0
    out = np.zeros(4, capi.PAIR_SCORE)
    assert capi.lib.dg_dp_score_paths(gpu_ctx.h, None, 4, out.ctypes.data) == -1 and capi.lib.dg_dp_score_paths(gpu_ctx.h, paths.ctypes.data, 4, None) == -1
    assert capi.lib.dg_dp_score_paths(gpu_ctx.h, paths.ctypes.data, -1, out.ctypes.data) == -1
    with gpu_ctx.dp_options(score_slab_bytes=64 * 2 * L * 4):                         # 5 slabs
        # the sink of path 1 of the last pair replaced by a vertex of another level: the last level of the last pair of the last slab
        bad = paths.copy()
        bad[299, 1, L - 1] = g.level_off[L - 2]
        with pytest.raises(capi.DgError, match=rf"rc=-1.*pair 299 path 1 level {L - 1}\b.*not in that level"):
            gpu_ctx.dp_score_paths(bad)
        # ids far outside the graph are argument errors like any other
        wild = paths.copy()
        wild[150, 0, 17] = 2 ** 31 - 1
        wild[150, 1, 3] = -5
        with pytest.raises(capi.DgError, match=r"rc=-1.*pair 150 path 0 level 17\b.*not in that level"):
            gpu_ctx.dp_score_paths(wild)
        # a hop without an edge: the vertex before the sink replaced by one of its level that has no edge to the sink -- if
        # every vertex of that level has one, the hop into it from a vertex that has no edge to it
        hop = paths.copy()
        sink_level = L - 1
        lvl = None
        for l in range(sink_level, 0, -1):
            for v in range(g.level_off[l], g.level_off[l + 1]):
                if v not in m.succ[int(hop[299, 1, l - 1])]:
                    lvl, vtx = l, v
                    break
            if lvl is not None:
                break
        assert lvl is not None and lvl >= L - 3
        hop[299, 1, lvl] = vtx
        with pytest.raises(capi.DgError, match=rf"rc=-1.*pair 299 path 1 level {lvl}\b.*no edge {int(hop[299, 1, lvl - 1])} -> {vtx}"):
            gpu_ctx.dp_score_paths(hop)
        assert m.check_path(hop[299, 1]) == (lvl, "edge")
        # the first bad hop is the one named
        hop[120, 0, 9] = g.level_off[3]
        with pytest.raises(capi.DgError, match=r"pair 120 path 0 level 9\b"):
            gpu_ctx.dp_score_paths(hop)
        # a failed call writes nothing
        out = np.full(300, -7, np.int32).repeat(4).view(capi.PAIR_SCORE)
        assert capi.lib.dg_dp_score_paths(gpu_ctx.h, hop.ctypes.data, 300, out.ctypes.data) == -1
        assert (out.view(np.int32) == -7).all()
        # and the same call with valid paths succeeds
        assert np.array_equal(_as_rows(gpu_ctx.dp_score_paths(paths)), want)
    with pytest.raises(ValueError):
        gpu_ctx.dp_score_paths(paths[:, :, :-1])


def test_a_scoring_call_leaves_the_last_run_alone(gpu_ctx):
    g = DEVICE_MODEL["levels65"]()
    m = PathModel(g)
    paths, _ = _pairs(m, 5, 200)
    with gpu_ctx.dp_options(digest=1):
        gpu_ctx.dp_load_graph(g)
        outs = [o.key() for o in gpu_ctx.dp_run_budgets(range(g.R + 1))]
        values = gpu_ctx.dp_budget_values().copy()
        digest = gpu_ctx.dp_level_digest(g.n_levels).copy()
        assert digest[1:].any()
        got = gpu_ctx.dp_score_paths(paths)
        assert np.array_equal(gpu_ctx.dp_budget_values(), values)
        assert np.array_equal(gpu_ctx.dp_level_digest(g.n_levels), digest)
        bad = paths.copy()
        bad[3, 0, 10] = 0
        with pytest.raises(capi.DgError):
            gpu_ctx.dp_score_paths(bad)
        assert np.array_equal(gpu_ctx.dp_budget_values(), values)
        assert np.array_equal(gpu_ctx.dp_level_digest(g.n_levels), digest)
        assert [o.key() for o in gpu_ctx.dp_run_budgets(range(g.R + 1))] == outs           # and the next run answers as before
        assert np.array_equal(gpu_ctx.dp_level_digest(g.n_levels), digest)
        assert np.array_equal(gpu_ctx.dp_score_paths(paths), got)

"""-m gpu: dg_dp_objective_paths / dg_dp_answer_objectives -- pairs of paths by the distinct-colour objective, on the device.

Integers only: every comparison is exact.  The yardstick is tests/objective_model.py (two independent forms of the definition,
checked against each other and against hand-written counts by tests/test_objective_model.py).  Shapes are chosen for where the
kernels can go wrong: fewer levels than lanes, 65 / 66 levels, lanes that loop over the levels; dictionaries of 0, 1 and either
side of one and two bitmap words; ids over the whole int32 range, a negative one, one present in both kinds; both routes on the
same pairs (objective_lds_bytes of a few bytes forces the bitmaps into device memory), one graph that takes the global route by
itself; one pair per slab on either route."""
import copy

import numpy as np
import pytest

import graphgen
from dipgenie_amd import capi
from objective_model import ObjectiveRanks, as_rows, objective_sets_many
from paths_model import NEG_INF, PathModel
from test_gpu_partner import CASES

pytestmark = pytest.mark.gpu

N_PAIRS = 64
GLOBAL = dict(objective_lds_bytes=4)                     # smaller than any non-empty pair of bitmaps
# (more levels, more colours: a path through 1,100 levels covers a small pool whole, and every pair would answer the same)
LEVELS = {3: dict(max_width=9, n_colours=40), 65: dict(max_width=9, n_colours=40), 66: dict(max_width=9, n_colours=40),
          300: dict(max_width=6, p_w1=0.1, n_colours=600), 1100: dict(max_width=4, p_w1=0.05, max_list=6, n_colours=3000)}
_CACHE = {}


def _pairs(m, seed, n=N_PAIRS):
    """half uniform, half biased towards weight-0 edges"""
    rng = np.random.default_rng(seed)
    a, _ = m.sample_pairs(rng, n - n // 2)
    b, _ = m.sample_pairs(rng, n // 2, 0.9)
    return np.concatenate([a, b])


def levels_case(n_levels):
    """graph, model, 64 pairs and the model's answer -- computed once"""
    if n_levels not in _CACHE:
        g = graphgen.random_levelized(9900 + n_levels, n_levels=n_levels, R=4, p_colour=0.5, **LEVELS[n_levels])
        m = PathModel(g)
        paths = _pairs(m, n_levels)
        want = objective_sets_many(m, paths)
        assert np.array_equal(ObjectiveRanks(g).many(paths), want)
        _CACHE[n_levels] = (g, m, paths, want)
    return _CACHE[n_levels]


def both_routes(ctx, paths):
    """the LDS route's and the global route's answers as [n, 4] rows"""
    lds = as_rows(ctx.dp_objective_paths(paths))
    with ctx.dp_options(**GLOBAL):
        glob = as_rows(ctx.dp_objective_paths(paths))
    return lds, glob


@pytest.mark.parametrize("n_levels", list(LEVELS))
def test_device_equals_model_over_the_level_counts(gpu_ctx, n_levels):
    g, m, paths, want = levels_case(n_levels)
    assert g.n_levels == n_levels and np.diff(g.level_off).max() <= 9 and paths.shape == (N_PAIRS, 2, n_levels)
    assert want.sum(axis=0).all() or n_levels == 3       # every one of the four counts occurs
    gpu_ctx.dp_load_graph(g)                             # no run before the call
    assert gpu_ctx.dp_get_option("objective_lds_bytes") == 131072
    lds, glob = both_routes(gpu_ctx, paths)
    for got in (lds, glob):
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, (n_levels, bad[:5], got[bad[:5]], want[bad[:5]])
    # one pair, and the same pairs one per slab: on the global route a pair's bitmaps count, so 8 * L bytes still hold one pair only
    assert np.array_equal(as_rows(gpu_ctx.dp_objective_paths(paths[7:8])), want[7:8])
    with gpu_ctx.dp_options(score_slab_bytes=1):
        assert np.array_equal(as_rows(gpu_ctx.dp_objective_paths(paths[:9])), want[:9])
    with gpu_ctx.dp_options(score_slab_bytes=8 * n_levels + 8, **GLOBAL):
        assert np.array_equal(as_rows(gpu_ctx.dp_objective_paths(paths[:9])), want[:9])
    with gpu_ctx.dp_options(score_slab_bytes=5 * 8 * n_levels):          # 5 pairs per slab: 13 slabs, the last one short
        assert np.array_equal(as_rows(gpu_ctx.dp_objective_paths(paths)), want)


SIZES = [0, 1, 31, 32, 33, 64, 65]


def exact_dictionary(topo, seed, ch, ct):
    """a copy of topo with exactly ch distinct hom and ct distinct het colours.  Ids: spread over the whole non-negative int32
    range, 0 and 2^31 - 1 included; the smallest het id is negative; with two or more ids of either kind, 2^31 - 1 is in both."""
    rng = np.random.default_rng(seed)

    def ids(n):
        return np.unique(np.round(np.linspace(0, 2 ** 31 - 1, n)).astype(np.int64)) if n > 1 else np.zeros(n, np.int64)
    hom_ids, het_ids = ids(ch), ids(ct)
    if ct:
        het_ids[0] = -5
    assert hom_ids.size == ch and het_ids.size == ct
    out = []
    for pool in (hom_ids, het_ids):
        lists = [set() for _ in range(topo.n_vertices)]
        for c in pool:                                   # every id sits somewhere, some of them on several vertices
            for v in rng.choice(topo.n_vertices, int(rng.integers(1, 4)), replace=False):
                lists[int(v)].add(int(c))
        out.append([np.array(sorted(x), np.int64) for x in lists])
    return graphgen._with_colours(topo, *out)


@pytest.mark.parametrize("ch", SIZES)
def test_dictionary_sizes(gpu_ctx, ch):
    topo = graphgen.random_levelized(9950, n_levels=12, max_width=5, R=3)
    for ct in SIZES:
        g = exact_dictionary(topo, 100 * ch + ct, ch, ct)
        ranks = ObjectiveRanks(g)
        assert (ranks.n_hom, ranks.n_het) == (ch, ct)
        if ct:
            assert g.het_col.min() == -5
        if ch > 1 and ct > 1:
            assert g.hom_col.max() == 2 ** 31 - 1 and g.het_col.max() == 2 ** 31 - 1 and g.hom_col.min() == 0
        m = PathModel(g)
        paths = _pairs(m, ch + ct)
        want = objective_sets_many(m, paths)
        assert np.array_equal(ranks.many(paths), want)
        gpu_ctx.dp_load_graph(g)
        lds, glob = both_routes(gpu_ctx, paths)
        assert np.array_equal(lds, want), (ch, ct)
        assert np.array_equal(glob, want), (ch, ct)
        if ch == 0 and ct == 0:
            assert (lds == 0).all()                      # a colourless graph answers zeros
        elif ch + ct > 30:
            assert want.any()


def test_spread_ids_and_shared_lists(gpu_ctx):
    """the colourings of the model's own test, on a longer graph: lists of hundreds of ids over the whole id range"""
    topo = graphgen.random_levelized(9960, n_levels=40, max_width=9, R=4)
    for variant in (dict(id_map=graphgen.spread_ids(600)), dict(shared=True), dict(hom_only=True), dict(het_only=True)):
        g = graphgen.recolour(topo, 9961, p_empty=0.4, p_short=0.3, long_range=(100, 500), pool=600, **variant)
        m = PathModel(g)
        paths = _pairs(m, 5)
        want = ObjectiveRanks(g).many(paths)
        assert np.array_equal(objective_sets_many(m, paths[:8]), want[:8])
        gpu_ctx.dp_load_graph(g)
        lds, glob = both_routes(gpu_ctx, paths)
        assert np.array_equal(lds, want) and np.array_equal(glob, want), variant


def test_bitmaps_beyond_the_lds_bound_take_the_global_route(gpu_ctx):
    """no option forced: more distinct het colours than 131,072 bytes of bitmaps hold"""
    topo = graphgen.random_levelized(9970, widths=[1] + [2] * 58 + [1], R=3, p_colour=0.0)
    g = graphgen.recolour_disjoint_big(topo, 9971, per_level=2, lengths=(9000, 10000))
    ranks = ObjectiveRanks(g)
    assert gpu_ctx.dp_get_option("objective_lds_bytes") == 131072 and ranks.bitmap_bytes() > 131072, ranks.bitmap_bytes()
    m = PathModel(g)
    paths = _pairs(m, 3, 8)
    want = ranks.many(paths)
    assert want[:, 2].min() > 0 and (want[:, :2] == 0).all()
    gpu_ctx.dp_load_graph(g)
    assert np.array_equal(as_rows(gpu_ctx.dp_objective_paths(paths)), want)
    with gpu_ctx.dp_options(score_slab_bytes=1):         # one pair, one set of bitmaps, per slab
        assert np.array_equal(as_rows(gpu_ctx.dp_objective_paths(paths[:3])), want[:3])


def test_option_objective_lds_bytes(gpu_ctx):
    old = gpu_ctx.dp_get_option("objective_lds_bytes")
    assert old == 131072
    with gpu_ctx.dp_options(objective_lds_bytes=4):
        assert gpu_ctx.dp_get_option("objective_lds_bytes") == 4
        gpu_ctx.dp_set_option("objective_lds_bytes", 0)                  # <= 0: the default
        assert gpu_ctx.dp_get_option("objective_lds_bytes") == 131072
        gpu_ctx.dp_set_option("objective_lds_bytes", 1 << 40)            # clamped to what a workgroup can have
        assert 65536 - 64 <= gpu_ctx.dp_get_option("objective_lds_bytes") <= 160 * 1024
    assert gpu_ctx.dp_get_option("objective_lds_bytes") == old


def test_errors(gpu_ctx):
    g, m, _, _ = levels_case(66)
    L = g.n_levels
    paths = _pairs(m, 77, 300)
    want = objective_sets_many(m, paths)
    call = capi.lib.dg_dp_objective_paths
    sentinel = lambda n: np.full(4 * n, -7, np.int32).view(capi.PAIR_OBJECTIVE)
    fresh = capi.Context(0)
    try:
        out = sentinel(300)
        with pytest.raises(capi.DgError, match=r"rc=-6.*dg_dp_objective_paths: no graph loaded"):
            fresh.dp_objective_paths(paths)
        assert call(fresh.h, paths.ctypes.data, 300, out.ctypes.data) == -6 and (out.view(np.int32) == -7).all()
    finally:
        fresh.close()
    gpu_ctx.dp_load_graph(g)
    assert gpu_ctx.dp_objective_paths(np.zeros((0, 2, L), np.int32)).size == 0            # n_pairs = 0
    assert call(gpu_ctx.h, None, 0, None) == 0
    out = sentinel(4)
    assert call(gpu_ctx.h, None, 4, out.ctypes.data) == -1 and call(gpu_ctx.h, paths.ctypes.data, 4, None) == -1
    assert call(gpu_ctx.h, paths.ctypes.data, -1, out.ctypes.data) == -1
    assert (out.view(np.int32) == -7).all()
    for route in ({}, GLOBAL):
        with gpu_ctx.dp_options(score_slab_bytes=64 * 2 * L * 4, **route):             # 5 slabs on the LDS route, more on the global one
            # a vertex of the wrong level, path 0 of pair 0
            bad = paths.copy()
            bad[0, 0, 5] = g.level_off[7]
            assert m.check_path(bad[0, 0]) == (5, "level")
            with pytest.raises(capi.DgError, match=r"rc=-1.*dg_dp_objective_paths: pair 0 path 0 level 5\b.*not in that level"):
                gpu_ctx.dp_objective_paths(bad)
            # the sink of path 1 of the last pair replaced by a vertex of another level: the last level of the last pair of the last slab
            bad = paths.copy()
            bad[299, 1, L - 1] = g.level_off[L - 2]
            assert m.check_path(bad[299, 1]) == (L - 1, "level")
            with pytest.raises(capi.DgError, match=rf"rc=-1.*pair 299 path 1 level {L - 1}\b.*not in that level"):
                gpu_ctx.dp_objective_paths(bad)
            # ids far outside the graph are argument errors like any other; path 0 comes before path 1
            wild = paths.copy()
            wild[150, 0, 17] = 2 ** 31 - 1
            wild[150, 1, 3] = -5
            with pytest.raises(capi.DgError, match=r"rc=-1.*pair 150 path 0 level 17\b.*not in that level"):
                gpu_ctx.dp_objective_paths(wild)
            # a hop without an edge, in pair 0 and in a later slab, on either path
            for pair, path in ((0, 1), (299, 0)):
                hop = paths.copy()
                lvl = None
                for l in range(L - 1, 0, -1):
                    for v in range(g.level_off[l], g.level_off[l + 1]):
                        if v not in m.succ[int(hop[pair, path, l - 1])]:
                            lvl, vtx = l, v
                            break
                    if lvl is not None:
                        break
                assert lvl is not None
                hop[pair, path, lvl] = vtx
                assert m.check_path(hop[pair, path]) == (lvl, "edge")
                with pytest.raises(capi.DgError, match=rf"rc=-1.*pair {pair} path {path} level {lvl}\b.*no edge {int(hop[pair, path, lvl - 1])} -> {vtx}"):
                    gpu_ctx.dp_objective_paths(hop)
            # the first bad hop is the one named
            hop[120, 0, 9] = g.level_off[3]
            with pytest.raises(capi.DgError, match=r"pair 120 path 0 level 9\b"):
                gpu_ctx.dp_objective_paths(hop)
            hop[120, 1, 8] = g.level_off[3]
            with pytest.raises(capi.DgError, match=r"pair 120 path 0 level 9\b"):
                gpu_ctx.dp_objective_paths(hop)
            # a failed call writes nothing
            out = sentinel(300)
            assert call(gpu_ctx.h, hop.ctypes.data, 300, out.ctypes.data) == -1
            assert (out.view(np.int32) == -7).all()
            # and the same call with valid paths succeeds
            assert np.array_equal(as_rows(gpu_ctx.dp_objective_paths(paths)), want)
    with pytest.raises(ValueError):
        gpu_ctx.dp_objective_paths(paths[:, :, :-1])


def _timing(ctx):
    t = ctx.dp_timing()
    return [getattr(t, f) for f, _ in capi.DpTiming._fields_]


def test_a_call_leaves_the_last_run_alone(gpu_ctx):
    g, m, paths, want = levels_case(65)
    budgets = list(range(g.R + 1))
    with gpu_ctx.dp_options(digest=1):
        gpu_ctx.dp_load_graph(g)
        assert np.array_equal(as_rows(gpu_ctx.dp_objective_paths(paths)), want)       # before any run
        outs = [o.key() for o in gpu_ctx.dp_run_budgets(budgets)]
        values = gpu_ctx.dp_budget_values().copy()
        digest = gpu_ctx.dp_level_digest(g.n_levels).copy()
        answers = [gpu_ctx.dp_answer_paths(b) for b in budgets]
        timing = _timing(gpu_ctx)
        assert digest[1:].any()
        for route in ({}, GLOBAL):
            with gpu_ctx.dp_options(**route):
                assert np.array_equal(as_rows(gpu_ctx.dp_objective_paths(paths)), want)
                first = gpu_ctx.dp_answer_objectives(budgets)
                bad = paths.copy()
                bad[3, 0, 10] = 0
                with pytest.raises(capi.DgError):
                    gpu_ctx.dp_objective_paths(bad)
            assert np.array_equal(gpu_ctx.dp_budget_values(), values)
            assert np.array_equal(gpu_ctx.dp_level_digest(g.n_levels), digest)
            assert _timing(gpu_ctx) == timing
            assert all(np.array_equal(gpu_ctx.dp_answer_paths(b), a) for b, a in zip(budgets, answers))
            assert np.array_equal(gpu_ctx.dp_answer_objectives(budgets), first)
        assert [o.key() for o in gpu_ctx.dp_run_budgets(budgets)] == outs             # and the next run answers as before
        assert np.array_equal(gpu_ctx.dp_level_digest(g.n_levels), digest)
        assert np.array_equal(as_rows(gpu_ctx.dp_objective_paths(paths)), want)


def test_a_load_rebuilds_the_dictionary(gpu_ctx):
    topo = graphgen.random_levelized(9980, n_levels=30, max_width=7, R=3)
    g1 = graphgen.recolour(topo, 1, p_empty=0.3, p_short=0.3, long_range=(20, 80), pool=300)
    g2 = graphgen.recolour(topo, 2, p_empty=0.3, p_short=0.3, long_range=(20, 80), pool=90, id_map=graphgen.spread_ids(90))
    m1, m2 = PathModel(g1), PathModel(g2)
    paths = _pairs(m1, 11)
    w1, w2 = objective_sets_many(m1, paths), objective_sets_many(m2, paths)
    assert not np.array_equal(w1, w2) and ObjectiveRanks(g1).n_hom != ObjectiveRanks(g2).n_hom
    for g, want in ((g1, w1), (g2, w2), (g1, w1)):
        gpu_ctx.dp_load_graph(g)
        lds, glob = both_routes(gpu_ctx, paths)
        assert np.array_equal(lds, want) and np.array_equal(glob, want)


def answers_agree(ctx, g, m, budgets):
    """dp_answer_objectives of the run at hand against dp_objective_paths of its answer paths and against the model; returns the rows"""
    values = ctx.dp_budget_values()
    got = as_rows(ctx.dp_answer_objectives(budgets))
    assert got.shape == (len(budgets), 4)
    for row, b in zip(got, budgets):
        paths = ctx.dp_answer_paths(b)
        if values[b] == NEG_INF:
            assert (paths == -1).all() and (row == -1).all(), (b, row)
            continue
        assert np.array_equal(as_rows(ctx.dp_objective_paths(paths[None]))[0], row), b
        assert np.array_equal(objective_sets_many(m, paths[None])[0], row), b
    return got


@pytest.mark.parametrize("name", ["levels65", "levels257", "fat_column", "colourless", "two_levels"])
def test_answer_objectives_of_every_budget(gpu_ctx, name):
    g = CASES[name][0]()
    m = PathModel(g)
    budgets = list(range(g.R + 1))
    gpu_ctx.dp_load_graph(g)
    gpu_ctx.dp_run_budgets(budgets)
    lds = answers_agree(gpu_ctx, g, m, budgets)
    with gpu_ctx.dp_options(**GLOBAL):
        assert np.array_equal(answers_agree(gpu_ctx, g, m, budgets), lds)
    assert (lds >= 0).any()
    # any order, a budget twice
    pick = [g.R, 0, g.R]
    assert np.array_equal(as_rows(gpu_ctx.dp_answer_objectives(pick)), lds[pick])
    # a plain run: the one chain of budget R
    gpu_ctx.dp_run()
    assert np.array_equal(as_rows(gpu_ctx.dp_answer_objectives([g.R]))[0], lds[g.R])


def test_unreachable_budgets_answer_minus_one(gpu_ctx):
    """no path of parallel66 has fewer than 6 recombinations: budget 0 (and every budget up to 11) fits no pair"""
    g = copy.copy(CASES["parallel66"][0]())
    g.R = 14
    m = PathModel(g)
    budgets = [0, 11, 12, 14]
    gpu_ctx.dp_load_graph(g)
    gpu_ctx.dp_run_budgets(budgets)
    values = gpu_ctx.dp_budget_values()
    assert values[0] == NEG_INF and values[11] == NEG_INF and values[12] != NEG_INF
    for route in ({}, GLOBAL):
        with gpu_ctx.dp_options(**route):
            got = answers_agree(gpu_ctx, g, m, budgets)
            assert (got[:2] == -1).all() and (got[2:] >= 0).all()
    # the caller's own paths get no such allowance: a negative id is an argument error
    with pytest.raises(capi.DgError, match=r"rc=-1.*pair 0 path 0 level 0\b"):
        gpu_ctx.dp_objective_paths(np.full((1, 2, g.n_levels), -1, np.int32))


def test_answer_objectives_errors(gpu_ctx):
    g = CASES["levels65"][0]()
    call = capi.lib.dg_dp_answer_objectives
    want_b = np.array([2], np.int32)
    out = np.full(4, -7, np.int32)
    fresh = capi.Context(0)
    try:
        with pytest.raises(capi.DgError, match=r"rc=-6.*dg_dp_answer_objectives: no graph loaded"):
            fresh.dp_answer_objectives([0])
    finally:
        fresh.close()
    gpu_ctx.dp_load_graph(g)
    with pytest.raises(capi.DgError, match=r"rc=-6.*dg_dp_answer_objectives: budget 2\b.*no completed dg_dp_run"):     # before any run
        gpu_ctx.dp_answer_objectives([2])
    assert call(gpu_ctx.h, want_b.ctypes.data, 1, out.ctypes.data) == -6 and (out == -7).all()
    gpu_ctx.dp_run_budgets([0, 2, g.R])
    want = gpu_ctx.dp_answer_objectives([2])
    for b in (1, g.R + 1, -1):                           # budgets the run did not list
        with pytest.raises(capi.DgError, match=rf"rc=-6.*dg_dp_answer_objectives.*budget {b}\b"):
            gpu_ctx.dp_answer_objectives([2, b])
        two = np.array([2, b], np.int32)
        out8 = np.full(8, -7, np.int32)
        assert call(gpu_ctx.h, two.ctypes.data, 2, out8.ctypes.data) == -6 and (out8 == -7).all()
    assert call(gpu_ctx.h, None, 1, out.ctypes.data) == -1 and call(gpu_ctx.h, want_b.ctypes.data, 1, None) == -1
    assert call(gpu_ctx.h, want_b.ctypes.data, 0, out.ctypes.data) == -1 and call(gpu_ctx.h, want_b.ctypes.data, -3, out.ctypes.data) == -1
    assert (out == -7).all()
    assert call(gpu_ctx.h, want_b.ctypes.data, 1, out.ctypes.data) == 0 and np.array_equal(out, as_rows(want)[0])
    gpu_ctx.dp_load_graph(g)                             # a load takes the answers with it
    with pytest.raises(capi.DgError, match=r"rc=-6.*budget 2\b.*no completed dg_dp_run"):
        gpu_ctx.dp_answer_objectives([2])


def test_answer_objectives_in_every_lattice_mode(gpu_ctx):
    g = copy.copy(CASES["levels600"][0]())               # (no pair of its paths has fewer than 4 recombinations: R = 8 gives five answers)
    g.R = 8
    m = PathModel(g)
    budgets = list(range(g.R + 1))
    gpu_ctx.dp_load_graph(g)
    outs = gpu_ctx.dp_run_budgets(budgets)
    want = answers_agree(gpu_ctx, g, m, budgets)
    assert (want[:, 0] >= 0).sum() == 5 and gpu_ctx.dp_timing().n_segments == 1 and gpu_ctx.dp_timing().n_chunks == 1
    cells = int(outs[0].cells)
    for opts in ({"segment_cells": max(1, cells // 4)}, {"lattice_chunk_cells": max(2, cells // 5)}):
        with gpu_ctx.dp_options(**opts):
            gpu_ctx.dp_load_graph(g)
            gpu_ctx.dp_run_budgets(budgets)
            t = gpu_ctx.dp_timing()
            assert t.n_segments >= 3 if "segment_cells" in opts else t.n_chunks > 1, (opts, t.n_segments, t.n_chunks)
            assert np.array_equal(as_rows(gpu_ctx.dp_answer_objectives(budgets)), want), opts
    gpu_ctx.dp_load_graph(g)                             # the tables of the default options again

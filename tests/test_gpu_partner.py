"""-m gpu: dg_dp_best_partners / Context.dp_best_partners -- the best partner of a given path, the DP with one haplotype fixed.

Integers only: every comparison is exact.  The yardstick is tests/partner_model.py, itself pinned to brute force, to the enumerated
optimum and to the oracle by tests/test_partner_model.py; the tests against the sweep need no model at all: plane b of the sink is
the maximum over all given paths p of partner_value(p, b - r(p))."""
import numpy as np
import pytest

import graphgen
from dipgenie_amd import capi
from partner_model import best_partners
from paths_model import NEG_INF, PathModel, repeat_edge
from test_gpu_score_paths import DEVICE_MODEL, ENUMERABLE, OPTIMALITY, _optimality_case

pytestmark = pytest.mark.gpu

N_GIVEN = 200
MAX_CELLS = 16384


def _wide():
    """more cells per level than a 256-lane workgroup: widths 30..40, budgets up to 9"""
    return graphgen.random_levelized(8810, n_levels=12, max_width=40, min_width=30, R=9, p_colour=0.5)


def _fat1100():
    """a level with more in-edges than the kernel stages in LDS: one in-edge listed 1,100 more times"""
    g = graphgen.random_levelized(8811, n_levels=10, max_width=12, R=4, p_colour=0.5)
    return repeat_edge(g, int(g.out_off[g.level_off[5]]), 1100)


def _full_lds():
    """widest level 128 (exactly): with budget 127 the state is the 16,384 cells that are the limit"""
    return graphgen.random_levelized(8812, n_levels=5, max_width=128, min_width=128, R=4, p_colour=0.5, extra_edges=0.5)


# name -> (graph, largest budget drawn (None: the graph's R), queries).  parallel66 has no path of fewer than 6 recombinations
# (R = 4): its budgets go up to 10, so that answers exist on either side
CASES = {name: (DEVICE_MODEL[name], 10 if name == "parallel66" else None, N_GIVEN) for name in ("two_levels", "levels65", "parallel66", "levels257", "levels600", "fat_column", "colourless")}
CASES["wide"] = (_wide, 9, N_GIVEN)
CASES["fat1100"] = (_fat1100, 5, 40)
CASES["full_lds"] = (_full_lds, 127, 12)
_REF = {}


def _footprint(g, bmax):
    """bytes of one query in a slab, as include/dipgenie_hip.h states them"""
    return 2 * g.n_vertices * (bmax + 1) + 2 * len(g.out_dst) + 8 * g.n_levels


def _given(m, seed, n):
    """half uniform, half biased towards weight-0 edges"""
    rng = np.random.default_rng(seed)
    a, ra = m.sample_paths(rng, n - n // 2)
    b, rb = m.sample_paths(rng, n // 2, 0.9)
    return np.concatenate([a, b]), np.concatenate([ra, rb])


def _case(name):
    """graph, model, given paths, budgets (mixed, 0..b_max), the model's values and partners -- computed once"""
    if name not in _REF:
        make, b_max, n = CASES[name]
        g = make()
        m = PathModel(g)
        given, _ = _given(m, 41, n)
        budgets = np.random.default_rng(42).integers(0, (g.R if b_max is None else b_max) + 1, n).astype(np.int32)
        if name == "full_lds":
            budgets[:4] = 127
        values, partners = best_partners(m, given, budgets)
        _REF[name] = (g, m, given, budgets, values, partners)
    return _REF[name]


def _rows(rec):
    return np.stack([rec["value"], rec["s_het"], rec["r1"], rec["r2"]], axis=1)


@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_model(gpu_ctx, name):
    g, m, given, budgets, values, partners = _case(name)
    n = len(given)
    widths = np.diff(g.level_off)
    if name == "wide":
        assert widths.max() * (budgets.max() + 1) > 256
    if name == "fat1100":
        assert np.bincount(g.out_dst, minlength=g.n_vertices).max() > 1024
    if name == "full_lds":
        assert widths.max() * (budgets.max() + 1) == MAX_CELLS
    reach = values != NEG_INF
    assert reach.any() and (name in ("two_levels", "full_lds") or len(set(budgets.tolist())) >= 3)
    # what the records must hold: the pair (given, partner) as the model scores it
    want = np.zeros((n, 4), np.int64)
    for i in range(n):
        want[i] = m.score(given[i], partners[i]) if reach[i] else (NEG_INF, 0, m.recombinations(given[i]), 0)
    assert np.array_equal(want[:, 0], values) and (want[reach, 3] <= budgets[reach]).all()
    gpu_ctx.dp_load_graph(g)                             # no run before the call
    for per_slab in (None, 7, 1):
        sub = slice(None) if per_slab != 1 else slice(0, 9)
        opts = {"partner_slab_bytes": per_slab * _footprint(g, int(budgets[sub].max()))} if per_slab else {}   # 7: the last slab is short; a query is sized for the call's largest budget
        with gpu_ctx.dp_options(**opts):
            rec, rows = gpu_ctx.dp_best_partners(given[sub], budgets[sub])
            rec2, none = gpu_ctx.dp_best_partners(given[sub], budgets[sub], want_paths=False)     # partners = NULL
        assert n % 7 != 0
        bad = np.flatnonzero((_rows(rec) != want[sub]).any(axis=1))
        assert bad.size == 0, (name, per_slab, bad[:5], _rows(rec)[bad[:5]], want[sub][bad[:5]])
        bad = np.flatnonzero((rows != partners[sub]).any(axis=1))
        assert bad.size == 0, (name, per_slab, bad[:5])
        assert none is None and np.array_equal(rec2, rec)


def test_maximum_over_given_paths_is_the_plane_of_the_sweep(gpu_ctx):
    """enumerable graphs: for every b, max over all paths p with r(p) <= b of partner_value(p, b - r(p)) = plane b of the sweep"""
    n_planes = n_unreachable = 0
    for seed, n_levels, extra, p_w1, p_colour in ENUMERABLE:
        g = graphgen.random_levelized(seed, n_levels=n_levels, max_width=4, R=3, extra_edges=extra, p_w1=p_w1, p_colour=p_colour)
        m = PathModel(g)
        paths = np.array(m.all_paths(), np.int32)
        rec = np.array([m.recombinations(p) for p in paths])
        gpu_ctx.dp_load_graph(g)
        gpu_ctx.dp_run_budgets(range(g.R + 1))
        planes = gpu_ctx.dp_budget_values()
        for b in range(g.R + 1):
            fit = rec <= b
            top = NEG_INF
            if fit.any():
                got, _ = gpu_ctx.dp_best_partners(paths[fit], b - rec[fit], want_paths=False)
                top = int(got["value"].max())
            assert top == planes[b], (seed, b, top, list(planes))
            n_planes += 1
            n_unreachable += top == NEG_INF
    assert n_planes == 20 and n_unreachable >= 1


@pytest.mark.parametrize("q", range(len(OPTIMALITY)))
def test_sampled_pairs_and_planes_bound_the_partner_value(gpu_ctx, q):
    g, m, paths, rec, oracle_values = _optimality_case(q)
    some = np.arange(0, len(paths), 100)
    assert len(some) == 200
    gpu_ctx.dp_load_graph(g)
    gpu_ctx.dp_run_budgets(range(g.R + 1))
    planes = gpu_ctx.dp_budget_values()
    assert list(planes) == oracle_values
    # no sampled pair (p, q) beats partner_value(p, r(q))
    scored = gpu_ctx.dp_score_paths(paths[some])
    assert np.array_equal(scored["r2"], rec[some, 1])
    got, _ = gpu_ctx.dp_best_partners(paths[some, 0], rec[some, 1], want_paths=False)
    assert (got["value"] >= scored["value"]).all(), np.flatnonzero(got["value"] < scored["value"])[:5]
    assert np.array_equal(got["r1"], rec[some, 0])
    # no partner_value(p, b) with r(p) + b <= R exceeds plane r(p) + b
    given, budgets = [], []
    for i in some:
        for b in range(g.R - int(rec[i, 0]) + 1):
            given.append(paths[i, 0])
            budgets.append(b)
    assert len(given) >= 50, len(given)                  # not vacuous
    given, budgets = np.array(given, np.int32), np.array(budgets, np.int32)
    got, _ = gpu_ctx.dp_best_partners(given, budgets, want_paths=False)
    over = np.flatnonzero(got["value"] > planes[got["r1"] + budgets])
    assert over.size == 0, (q, over[:5], got[over[:5]])
    print(f"graph {q}: {len(given)} (path, budget) queries, planes {list(planes)}, best partner value per plane "
          f"{[int(got['value'][got['r1'] + budgets == b].max()) if (got['r1'] + budgets == b).any() else None for b in range(g.R + 1)]}")


def test_properties(gpu_ctx):
    g, m, given, _, _, _ = _case("levels65")
    given = given[:60]
    n, R = len(given), g.R
    gpu_ctx.dp_load_graph(g)
    # the value does not fall when the budget grows
    nb = R + 3
    rec, rows = gpu_ctx.dp_best_partners(np.repeat(given, nb, axis=0), np.tile(np.arange(nb, dtype=np.int32), n))
    v = rec["value"].reshape(n, nb)
    assert (np.diff(v, axis=1) >= 0).all() and (np.diff(v, axis=1) > 0).any()
    # every partner is a path that dp_score_paths accepts, and its record is `out` field by field
    ok = rec["value"] != NEG_INF
    assert ok.any()
    pairs = np.ascontiguousarray(np.stack([np.repeat(given, nb, axis=0)[ok], rows[ok]], axis=1))
    assert np.array_equal(_rows(gpu_ctx.dp_score_paths(pairs)), _rows(rec[ok]))
    assert (rows[~ok] == -1).all() and (rec["s_het"][~ok] == 0).all() and (rec["r2"][~ok] == 0).all()
    # one ascent step with a total of T recombinations: the partner as the given path, with the budget T - r it leaves, is worth no less
    r1 = np.array([m.recombinations(p) for p in given])
    T = int(r1.max()) + 2
    assert np.diff(g.level_off).max() * (T + 1) <= MAX_CELLS
    a, qa = gpu_ctx.dp_best_partners(given, (T - r1).astype(np.int32))
    live = a["value"] != NEG_INF
    assert live.sum() >= 10
    b, _ = gpu_ctx.dp_best_partners(qa[live], (T - a["r2"][live]).astype(np.int32))
    assert (b["value"] >= a["value"][live]).all() and (b["value"] > a["value"][live]).any()
    assert np.array_equal(b["r1"], a["r2"][live])


def test_errors(gpu_ctx):
    g, m, given, budgets, values, partners = _case("levels65")
    L, n = g.n_levels, len(given)
    fresh = capi.Context(0)
    try:
        with pytest.raises(capi.DgError, match=r"rc=-6.*no graph loaded"):
            fresh.dp_best_partners(given, budgets)
    finally:
        fresh.close()
    gpu_ctx.dp_load_graph(g)
    call = capi.lib.dg_dp_best_partners
    rec, rows = gpu_ctx.dp_best_partners(np.zeros((0, L), np.int32), np.zeros(0, np.int32))       # n = 0
    assert rec.size == 0 and rows.shape == (0, L)
    assert call(gpu_ctx.h, None, 0, None, None, None) == 0
    out = np.full(4 * n, -7, np.int32).view(capi.PARTNER)
    part = np.full((n, L), -7, np.int32)
    gp, bp = given.ctypes.data, budgets.ctypes.data
    assert call(gpu_ctx.h, None, 4, bp, part.ctypes.data, out.ctypes.data) == -1
    assert call(gpu_ctx.h, gp, 4, None, part.ctypes.data, out.ctypes.data) == -1
    assert call(gpu_ctx.h, gp, 4, bp, part.ctypes.data, None) == -1
    assert call(gpu_ctx.h, gp, -1, bp, part.ctypes.data, out.ctypes.data) == -1

    def untouched():
        return (out.view(np.int32) == -7).all() and (part == -7).all()

    def fails(gv, bd, rc, pattern):
        gv, bd = np.ascontiguousarray(gv, np.int32), np.ascontiguousarray(bd, np.int32)
        with pytest.raises(capi.DgError, match=pattern):
            gpu_ctx.dp_best_partners(gv, bd)
        assert call(gpu_ctx.h, gv.ctypes.data, len(gv), bd.ctypes.data, part.ctypes.data, out.ctypes.data) == rc
        assert untouched()

    assert untouched()
    with gpu_ctx.dp_options(partner_slab_bytes=7 * _footprint(g, int(budgets.max()))):           # 29 slabs
        neg = budgets.copy()
        neg[123] = -1
        neg[150] = -3
        fails(given, neg, -1, r"rc=-1.*query 123\b.*budget -1")
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
        # and the same call with valid paths succeeds
        rec, rows = gpu_ctx.dp_best_partners(given, budgets)
        assert np.array_equal(rec["value"], values) and np.array_equal(rows, partners)
    with pytest.raises(ValueError):
        gpu_ctx.dp_best_partners(given[:, :-1], budgets)
    with pytest.raises(ValueError):
        gpu_ctx.dp_best_partners(given, budgets[:-1])
    # an unreachable budget is an answer, not an error
    r = np.array([m.recombinations(p) for p in given])
    assert (values == NEG_INF).any()
    rec, rows = gpu_ctx.dp_best_partners(given, budgets)
    dead = rec["value"] == NEG_INF
    assert np.array_equal(dead, values == NEG_INF) and (rows[dead] == -1).all() and (rows[~dead] >= 0).all()
    assert np.array_equal(rec["r1"], r) and (rec["s_het"][dead] == 0).all() and (rec["r2"][dead] == 0).all()
    # the cell limit: widest level 200, budget 100
    wide = graphgen.random_levelized(8813, n_levels=4, max_width=200, min_width=200, R=2, extra_edges=0.2)
    mw = PathModel(wide)
    gw, _ = mw.sample_paths(np.random.default_rng(1), 3)
    gpu_ctx.dp_load_graph(wide)
    part = np.full((3, 4), -7, np.int32)
    out = np.full(12, -7, np.int32).view(capi.PARTNER)
    fails(gw, [1, 100, 100], -5, r"rc=-5.*query 1\b.*200.*101")
    rec, _ = gpu_ctx.dp_best_partners(gw, [1, 80, 0])                                            # 200 x 81 cells fit
    assert (rec["value"] >= 0).sum() >= 1


def test_a_partner_call_leaves_the_last_run_alone(gpu_ctx):
    g, m, given, budgets, values, partners = _case("levels65")
    with gpu_ctx.dp_options(digest=1):
        gpu_ctx.dp_load_graph(g)
        outs = [o.key() for o in gpu_ctx.dp_run_budgets(range(g.R + 1))]
        planes = gpu_ctx.dp_budget_values().copy()
        digest = gpu_ctx.dp_level_digest(g.n_levels).copy()
        assert digest[1:].any()
        got = gpu_ctx.dp_best_partners(given, budgets)
        assert np.array_equal(got[0]["value"], values)
        assert np.array_equal(gpu_ctx.dp_budget_values(), planes)
        assert np.array_equal(gpu_ctx.dp_level_digest(g.n_levels), digest)
        bad = given.copy()
        bad[3, 10] = 0
        with pytest.raises(capi.DgError):
            gpu_ctx.dp_best_partners(bad, budgets)
        assert np.array_equal(gpu_ctx.dp_budget_values(), planes)
        assert np.array_equal(gpu_ctx.dp_level_digest(g.n_levels), digest)
        assert [o.key() for o in gpu_ctx.dp_run_budgets(range(g.R + 1))] == outs                  # and the next run answers as before
        assert np.array_equal(gpu_ctx.dp_level_digest(g.n_levels), digest)
        again = gpu_ctx.dp_best_partners(given, budgets)
        assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1])


def test_capi_layout(gpu_ctx):
    assert capi.PARTNER.itemsize == 16 and capi.PARTNER.names == ("value", "s_het", "r1", "r2")
    g, m, given, budgets, values, partners = _case("two_levels")
    gpu_ctx.dp_load_graph(g)
    raw = np.full(4 * 3, -7, np.int32)
    assert capi.lib.dg_dp_best_partners(gpu_ctx.h, given.ctypes.data, 3, budgets.ctypes.data, None, raw.ctypes.data) == 0
    assert np.array_equal(raw.reshape(3, 4)[:, 0], values[:3])       # sizeof(dg_dp_partner) == 16: value at stride 4 words

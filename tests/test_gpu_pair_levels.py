"""-m gpu: level pairs -- two adjacent low-fan-in levels swept by one composed launch (dipgenie_amd/csrc/dg_dp_pairs.hip,
dp_sweep_pair_kernel).  Every case sets pair_min = 1 (by default only graphs with thousands of pairs take the form) and compares, by
integer equality with the oracle: value, s_het, both edge lists, and the sink's value on every plane with the oracle solved per
budget; the pair profile must show the pairs that tests/pair_graphs.py expects from the arrays (tests/test_pair_graphs.py holds the
graphs' properties on the CPU).  The library re-scores the walked path against the DP value in every run (DG_ERR_STATE otherwise)."""
import numpy as np
import pytest

import oracle_py as orc
import pair_graphs as pg
from dipgenie_amd import capi

pytestmark = pytest.mark.gpu
_BUDGET_VALUES = {}


def _budget_values(key, g):
    if key not in _BUDGET_VALUES:
        _BUDGET_VALUES[key] = np.array([orc.dp_solve(pg.with_R(g, r))["value"] for r in range(g.R + 1)], np.int32)
    return _BUDGET_VALUES[key]


def _run(ctx, g, passes=1, **opts):
    """load + run under pair_min = 1 and opts: [(outcome, launch profile, pair profile, n_forward_launches, n_segments)] per pass"""
    got = []
    with ctx.dp_options(pair_min=1, **opts):
        ctx.dp_load_graph(g)
        for _ in range(passes):
            out = ctx.dp_run()
            tm = ctx.dp_timing()
            got.append((out, ctx.dp_launch_profile(), ctx.dp_pair_profile(), int(tm.n_forward_launches), int(tm.n_segments), ctx.dp_budget_values().copy()))
    return got


def _check(ctx, key, g, n_pairs=None, **opts):
    """one run against the oracle; n_pairs: pair launches expected (default: every pair of pg.expected_pairs)"""
    ref = orc.dp_solve(g)
    out, singles, pairs, n_launch, _, planes = _run(ctx, g, **opts)[0]
    assert (out.value, out.s_het, out.p1, out.p2) == (ref["value"], ref["s_het"], ref["p1"], ref["p2"]), key
    assert np.array_equal(planes, _budget_values(key, g)), key
    want = len(pg.expected_pairs(g)) if n_pairs is None else n_pairs
    assert sum(pairs.values()) == want and sum(singles.values()) == g.n_levels - 1 - 2 * want and n_launch == g.n_levels - 1 - want, (key, singles, pairs)
    assert want >= 1 or n_pairs == 0, key
    return pairs


@pytest.mark.parametrize("k", [2, 3, 5])
def test_ties_follow_the_level_by_level_order(gpu_ctx, k):
    """colourless, in-degree 2 on both levels: every candidate ties, and on these seeds the order of ranks within the composed lists
    would walk other edges than the reference's order (tests/test_pair_graphs.py)"""
    _check(gpu_ctx, ("tie", k), pg.tie_graph(k, pg.TIE_ORDER_SEEDS[k]))


@pytest.mark.parametrize("R", [1, 2, 3, 4, 18])
def test_plane_shift(gpu_ctx, R):
    """w = 4 and source planes below 0; R + 1 = 2, 3, 4, 5, 19 planes: a ragged last chunk for every chunk size above 1"""
    _check(gpu_ctx, ("plane", R), pg.plane_shift_graph(R))
    if R in (2, 4):                                                      # ... and on the larger chunks whatever the cost model takes
        with gpu_ctx.dp_options(rc_tw_ps=10 ** 7):                      # waves cost, planes per wave do not: the largest chunk size
            pairs = _check(gpu_ctx, ("plane", R), pg.plane_shift_graph(R))
        assert set(pairs) == {"dp_sweep_pair_kernel<4>"}


@pytest.mark.parametrize("mix", [(1, 8), (2, 4), (4, 2), (8, 1)])
def test_in_degree_limit(gpu_ctx, mix):
    """composed in-degree exactly 8 = mix[0] in-edges over sources of mix[1]: paired; exactly 9: levels 3 and 4 as two single launches"""
    total = mix[0] * mix[1]
    _check(gpu_ctx, ("limit", mix, 8), pg.indeg_limit_graph(mix, total), n_pairs=2)
    _check(gpu_ctx, ("limit", mix, 9), pg.indeg_limit_graph(mix, total + 1), n_pairs=1)


def test_shared_middle_cells(gpu_ctx):
    _check(gpu_ctx, "shared", pg.shared_middle_graph())
    for R in (0, 1):
        _check(gpu_ctx, ("shared", R), pg.shared_middle_graph(R))


@pytest.mark.parametrize("t,k", pg.SLOT_BLOCK_CASES)
def test_slot_blocks(gpu_ctx, t, k):
    _check(gpu_ctx, ("slots", t, k), pg.slot_block_graph(t, k, R=pg.SLOT_BLOCK_R.get((t, k), 18)))


@pytest.mark.parametrize("coloured", ["none", "first", "second", "both"])
@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_pairing_parity(gpu_ctx, n, coloured):
    _check(gpu_ctx, ("parity", n, coloured), pg.parity_graph(n, coloured))


@pytest.mark.parametrize("t,k", [(129, 65), (8, 1)])
def test_non_temporal_back_pointer_stores(gpu_ctx, t, k):
    """levels of 262,144 cells and more stream the back-pointers of their own cells non-temporally (bp_nt_min_cells): here every level"""
    _check(gpu_ctx, ("slots", t, k), pg.slot_block_graph(t, k, R=pg.SLOT_BLOCK_R.get((t, k), 18)), bp_nt_min_cells=1)
    _check(gpu_ctx, "shared", pg.shared_middle_graph(), bp_nt_min_cells=1)


def _long_graph():
    return pg.layered(4242, 5, [1] + [10] * 7 + [1], [1, 2, 2, 2, 2, 2, 2, 4], colour_levels=(2, 3, 5, 8))     # pairs (1,2) (3,4) (5,6) (7,8)


def test_refusals(gpu_ctx):
    g = _long_graph()
    assert pg.expected_pairs(g) == [2, 4, 6, 8]
    ref = orc.dp_solve(g, want_digest=True)
    paired = _check(gpu_ctx, "long", g)
    # digests: no pair launch, every level's digest the oracle's
    _check(gpu_ctx, "long", g, n_pairs=0, digest=1)
    with gpu_ctx.dp_options(pair_min=1, digest=1):
        gpu_ctx.dp_load_graph(g)
        gpu_ctx.dp_run()
        assert np.array_equal(gpu_ctx.dp_level_digest(g.n_levels)[1:], ref["digest"][1:])
    # a segmented lattice: more than one segment, no pair launch, the same answer
    seg = _run(gpu_ctx, g, segment_cells=2000)[0]
    assert seg[4] > 1 and not seg[2] and (seg[0].value, seg[0].s_het, seg[0].p1, seg[0].p2) == (ref["value"], ref["s_het"], ref["p1"], ref["p2"])
    assert np.array_equal(seg[5], _budget_values("long", g))
    # a forced chunk size, and the form switched off: every level its own launch, as without the tables
    _check(gpu_ctx, "long", g, n_pairs=0, test_force_rc=2)
    _check(gpu_ctx, "long", g, n_pairs=0, adaptive_rc=0)
    _check(gpu_ctx, "long", g, n_pairs=0, fast=0)
    off = _run(gpu_ctx, g, pair_levels=0)[0]
    gpu_ctx.dp_load_graph(g)                                             # default options: pair_min = 4096, nothing is paired
    gpu_ctx.dp_run()
    assert not off[2] and off[1] == gpu_ctx.dp_launch_profile() and not gpu_ctx.dp_pair_profile()
    assert sum(paired.values()) == 4


def test_batches_and_replays(gpu_ctx):
    """plain launches, the default batch, and batches of 3 levels (the pair (3, 4) straddles a batch edge and falls back to two single
    launches); three passes each: the second and third replay the captured batches"""
    g = _long_graph()
    ref = orc.dp_solve(g)
    profiles = {}
    for gb, n_pairs in ((0, 4), (-1, 4), (3, 3)):
        runs = _run(gpu_ctx, g, passes=3, graph_batch=gb)
        for out, singles, pairs, n_launch, _, planes in runs:
            assert (out.value, out.s_het, out.p1, out.p2) == (ref["value"], ref["s_het"], ref["p1"], ref["p2"]), gb
            assert np.array_equal(planes, _budget_values("long", g)), gb
            assert (singles, pairs, n_launch) == runs[0][1:4], gb
            assert sum(pairs.values()) == n_pairs and sum(singles.values()) == g.n_levels - 1 - 2 * n_pairs and n_launch == g.n_levels - 1 - n_pairs, gb
        profiles[gb] = runs[0][1:3]
    assert profiles[0] == profiles[-1]


def test_run_budgets_walks_through_pairs(gpu_ctx):
    """one chain per budget from the same lattice: each walks its own middle cells"""
    g = _long_graph()
    with gpu_ctx.dp_options(pair_min=1):
        gpu_ctx.dp_load_graph(g)
        outs = gpu_ctx.dp_run_budgets(range(g.R + 1))
        assert sum(gpu_ctx.dp_pair_profile().values()) == 4
    for r, out in enumerate(outs):
        ref = orc.dp_solve(pg.with_R(g, r))
        assert (out.value, out.s_het, out.p1, out.p2) == (ref["value"], ref["s_het"], ref["p1"], ref["p2"]), r


def test_every_instantiated_pair_variant_is_launched(gpu_ctx):
    """small levels take chunk size 1; 65 rows over three slot blocks take 2 at 19 planes and 4 at 41"""
    seen = set()
    seen |= set(_check(gpu_ctx, ("slots", 8, 1), pg.slot_block_graph(8, 1)))
    seen |= set(_check(gpu_ctx, ("slots", 129, 65, 18), pg.slot_block_graph(129, 65)))
    seen |= set(_check(gpu_ctx, ("slots", 129, 65), pg.slot_block_graph(129, 65, R=40)))
    inst = set(capi.Context.dp_pair_variants())
    assert len(inst) >= 1 and seen == inst, (sorted(seen), sorted(inst))

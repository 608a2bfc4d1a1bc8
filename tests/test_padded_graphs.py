"""tests/padded_graphs.py on the CPU: padding changes no real cell (the models on the padded graph equal the remapped models on the base
graph, NEG_INF on every pad), a saturated budget changes nothing, and each full-size shape of tests/test_gpu_joint_beyond_caps.py is
loader-legal and still crosses the cap it is named for -- so that an edit of a generator that moves a shape back under its cap fails
here instead of leaving the GPU tests testing nothing."""
import numpy as np
import pytest

import padded_graphs as pg
from call_margins_model import class_arrays
from genotype_margins_model import genotype_margins_np, through_values_np
from genotype_table_model import genotype_table_np
from paths_model import NEG_INF, PathModel
from phase_margins_model import het_levels, phase_margins_np
from pinned_joint_model import pinned_through_values_np
from pinned_model import FORBID, REQUIRE

SMALL_BUDGETS = dict(rows=(0, 2, 7), edges=(0, 2, 7), lanes=(0, 2, 8), deep=(0, 2, 4))
_SMALL, _FULL = {}, {}


def small(name):
    if name not in _SMALL:
        g, gp, new_id = pg.SHAPES[name](small=True)
        _SMALL[name] = (g, gp, new_id, PathModel(g), PathModel(gp))
    return _SMALL[name]


def full(name):
    if name not in _FULL:
        _FULL[name] = pg.SHAPES[name]()
    return _FULL[name]


@pytest.mark.parametrize("name", list(pg.SHAPES))
def test_padding_changes_no_real_cell(name):
    g, gp, new_id, m, mp = small(name)
    pads = pg.pad_mask(gp, new_id)
    assert name == "deep" or pads.sum() >= 15
    assert (np.diff(new_id) > 0).all()                    # monotone: the tie-breaks carry over
    rng = np.random.default_rng(7)
    cls = class_arrays(g, 71)[2]
    cls_p = pg.pad_classes(g, gp, new_id, cls, 72)
    assert np.array_equal(cls_p[new_id], cls) and (name == "deep" or (cls_p[pads] > cls.max()).any() and (cls_p[pads] <= cls.max()).any())
    called = np.stack([m.sample_paths(rng, 2)[0], np.array([[rng.integers(m.level_off[l], m.level_off[l + 1]) for l in range(m.L)] for _ in range(2)])])
    called_p = pg.remap_called(called, new_id)
    inner = [l for l in range(1, m.L - 1) if len(set(cls[m.level_off[l]:m.level_off[l + 1]].tolist())) > 1][:3]
    pair = pg.het_pair(m, cls, inner[:2], 73)
    for b in SMALL_BUDGETS[name]:
        T, V = through_values_np(m, b)
        Tp, Vp = through_values_np(mp, b)
        assert V == Vp
        for l, (want, got) in enumerate(zip(pg.embed_through_values(T, g, gp, new_id), Tp)):
            assert np.array_equal(want, got), (name, b, l)
            at = pads[gp.level_off[l]:gp.level_off[l + 1]]
            assert (got[at, :] == NEG_INF).all() and (got[:, at] == NEG_INF).all()
        for c, cp in ((None, None), (cls, cls_p)):
            rec, _, J = genotype_margins_np(m, called, b, c, T, V)
            rec_p, _, J_p = genotype_margins_np(mp, called_p, b, cp, Tp, Vp)
            assert np.array_equal(pg.remap_records(rec, new_id), rec_p) and np.array_equal(pg.remap_vertex_values(J, gp, new_id), J_p)
            assert (J_p[pads] == NEG_INF).all()
            off, rows = pg.remap_table(*genotype_table_np(m, T, c), new_id, own_classes=c is None)
            off_p, rows_p = genotype_table_np(mp, Tp, cp)
            assert np.array_equal(off, off_p) and np.array_equal(rows, rows_p), (name, b)
            assert not pads[rows_p[:, 2:4]].any()
            ph, Vh = phase_margins_np(m, pair, b, c)
            ph_p, Vh_p = phase_margins_np(mp, pg.remap_called(pair, new_id), b, cp)
            assert Vh == Vh_p == V and len(ph) >= 1 and np.array_equal(pg.remap_phase(ph, new_id), ph_p), (name, b)
            assert het_levels(m, pair, c) == het_levels(mp, pg.remap_called(pair, new_id), cp)
    # pins on real cells, and one that names a pad: forbidding a pad forbids nothing, requiring one alone leaves nothing
    l = int(np.argmax(np.diff(gp.level_off) - np.diff(g.level_off))) if pads.any() else inner[0]     # the level with the most pads
    a0, a1 = int(m.level_off[l]), int(m.level_off[l + 1])
    pins = [(l, a0, -1, FORBID), (l, -1, a1 - 1, FORBID), (inner[0], int(m.level_off[inner[0]]), -1, REQUIRE), (inner[0], -1, int(m.level_off[inner[0]]), REQUIRE)]
    b = SMALL_BUDGETS[name][1]
    T, V = pinned_through_values_np(m, b, pins)
    if pads.any():
        a_pad = int(np.flatnonzero(pads[gp.level_off[l]:gp.level_off[l + 1]])[0] + gp.level_off[l])
        Tp, Vp = pinned_through_values_np(mp, b, pg.remap_pins(pins, new_id) + [(l, a_pad, -1, FORBID)])
        assert V == Vp and all(np.array_equal(x, y) for x, y in zip(pg.embed_through_values(T, g, gp, new_id), Tp))
        Tp, Vp = pinned_through_values_np(mp, b, [(l, a_pad, -1, REQUIRE)])
        T0, V0 = pinned_through_values_np(m, b, [(l, -1, -1, FORBID)])
        assert Vp == V0 == NEG_INF and all((t == NEG_INF).all() for t in Tp + T0)


@pytest.mark.parametrize("name", ["rows", "lanes"])
def test_a_saturated_budget_changes_nothing(name):
    """states mean "at most r" and no pair of paths spends more than 2 (L - 1): every budget from there on gives the same values"""
    g, _, _, m, _ = small(name)                          # (edges has the base of rows; deep's GPU test uses no saturated budget)
    T, V = through_values_np(m, 2 * (m.L - 1))
    T40, V40 = through_values_np(m, 40)
    assert V == V40 != NEG_INF and all(np.array_equal(x, y) for x, y in zip(T, T40))


def loader_legal(g):
    """what dg_dp_load_graph asks of its arrays"""
    level_of = np.repeat(np.arange(g.n_levels), np.diff(g.level_off))
    src = np.repeat(np.arange(g.n_vertices), np.diff(g.out_off))
    assert g.level_off[0] == 0 and g.level_off[1] == 1 and g.level_off[-1] - g.level_off[-2] == 1 and (np.diff(g.level_off) >= 1).all()
    assert g.out_off[0] == 0 and (np.diff(g.out_off) >= 0).all() and g.out_off[-1] == len(g.out_dst) == len(g.out_w)
    assert (level_of[g.out_dst] == level_of[src] + 1).all()
    assert set(np.unique(g.out_w).tolist()) <= {0, 1}
    pair = src.astype(np.int64) * g.n_vertices + g.out_dst
    order = np.argsort(pair, kind="stable")
    same = pair[order][1:] == pair[order][:-1]
    assert (g.out_w[order][1:][same] == g.out_w[order][:-1][same]).all()      # parallel edges share a weight
    for off, col in ((g.hom_off, g.hom_col), (g.het_off, g.het_col)):
        assert off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] == len(col)
        inside = np.ones(len(col), bool)
        inside[off[:-1][np.diff(off) > 0]] = False        # the first id of every list
        assert (np.diff(col)[inside[1:]] > 0).all() and (col >= 0).all()      # sorted and unique
    assert not set(g.hom_col.tolist()) & set(g.het_col.tolist())


@pytest.mark.parametrize("name", list(pg.SHAPES))
def test_full_size_shapes_are_loader_legal(name):
    g, gp, new_id = full(name)
    loader_legal(gp)
    pads = pg.pad_mask(gp, new_id)
    src = np.repeat(np.arange(gp.n_vertices), np.diff(gp.out_off))
    assert not pads[gp.out_dst[~pads[src]]].any()         # no real vertex has an edge into a pad: nothing reaches one
    assert name == "deep" or (~pads[gp.out_dst[pads[src]]]).any()      # ... and some pads have an edge into a real vertex
    has = (np.diff(gp.hom_off) > 0) & (np.diff(gp.het_off) > 0)
    assert has[pads].all()                                # every pad carries both kinds of colour


def test_rows_crosses_the_row_cap():
    g, gp, new_id = full("rows")
    for l, (first_real, width) in ((2, (2020, 2154)), (3, (30, 2195))):
        pos = new_id[g.level_off[l]:g.level_off[l + 1]] - gp.level_off[l]
        assert pos[0] == first_real and gp.level_off[l + 1] - gp.level_off[l] == width > pg.ROW_BLOCKS
    pos = new_id[g.level_off[2]:g.level_off[3]] - gp.level_off[2]
    assert (pos < pg.ROW_BLOCKS).sum() >= 20 and (pos >= pg.ROW_BLOCKS).sum() >= 20      # real rows on both sides; the later ones come second in their workgroup
    pos = new_id[g.level_off[3]:g.level_off[4]] - gp.level_off[3]
    assert pos.max() < pg.ROW_BLOCKS and pos.max() + pg.ROW_BLOCKS < 2195                 # real rows first, a pad row second in the same workgroup
    assert pg.widest_level(gp) == 2195 and 2195 > 20 * (pg.ROW_BLOCKS // 19)             # 19 distinct budgets: 107 rows each, strided twenty times
    assert 4000 <= pg.in_edge_count(gp, 3) <= 6000


def test_edges_crosses_the_score_grid():
    g, gp, new_id = full("edges")
    T = pg.in_edge_count(gp, pg.EDGES_LEVEL)
    ranks = pg.real_in_edge_ranks(gp, new_id, pg.EDGES_LEVEL)
    print(f"edges: {T} in-edges, real ranks {ranks.min()}..{ranks.max()}, {int((ranks < pg.SCORE_Y_BLOCKS).sum())} below and {int((ranks >= pg.SCORE_Y_BLOCKS).sum())} at or above")
    assert pg.SCORE_Y_BLOCKS < T <= 17500 and T > pg.SCORE_X_BLOCKS * pg.THREADS
    assert (ranks < pg.SCORE_Y_BLOCKS).sum() >= 10 and (ranks >= pg.SCORE_Y_BLOCKS).sum() >= 10
    assert 2 * T * T < 700 << 20                         # the score matrix, uint16
    has = (np.diff(gp.hom_off) + np.diff(gp.het_off)) > 0
    assert has[gp.level_off[2]:gp.level_off[4]].any()     # the transition is coloured: jt_scores_kernel computes it


def test_lanes_crosses_the_lane_cap():
    g, gp, new_id = full("lanes")
    k = int(gp.level_off[3] - gp.level_off[2])
    assert k == 300 == pg.widest_level(gp) and k * (pg.LANES_BUDGET + 1) > pg.LANES_PER_ROW and k * (pg.LANES_BUDGET + 1) > pg.MASK_X_BLOCKS * pg.THREADS
    col = new_id[g.level_off[2]:g.level_off[3]] - gp.level_off[2]
    first = col * (pg.LANES_BUDGET + 1)                   # the lane of plane 0 of a real column
    assert (first < pg.LANES_PER_ROW).sum() >= 3 and (first >= pg.LANES_PER_ROW).sum() >= 3
    assert pg.LANES_BUDGET >= 2 * (g.n_levels - 1) and 4 * k * k * (pg.LANES_BUDGET + 1) < 2 << 30


def test_deep_crosses_the_scan_chunk_and_its_sink_is_reachable():
    g, _, _ = full("deep")
    assert g.n_levels == 1200 and pg.vertex_count(g) > 2 * pg.SCAN_CHUNK
    src = np.repeat(np.arange(g.n_vertices), np.diff(g.out_off))
    assert (np.bincount(src // pg.SCAN_CHUNK) > 0).all() and src.max() // pg.SCAN_CHUNK >= 2      # every chunk holds edges: the carry counts
    assert 2 * pg.min_recombinations(g) <= pg.DEEP_BUDGET

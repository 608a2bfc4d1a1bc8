"""CPU: the graphs of tests/test_gpu_pair_levels.py keep the properties that test relies on -- checked from the arrays, the oracle and
the plain model of tests/pair_graphs.py alone (no GPU, no library call)."""
import pytest

import oracle_py as orc
import pair_graphs as pg

NEG_INF = -(2 ** 31) // 4


def _model_equals_oracle(g, pairs, order="ref"):
    ref = orc.dp_solve(g)
    sink, p1, p2 = pg.solve_colourless(g, pairs, order)
    return sink[g.R] == (None if ref["value"] == NEG_INF else ref["value"]) and (p1, p2) == (ref["p1"], ref["p2"])


@pytest.mark.parametrize("k", [2, 3, 5])
def test_tie_graphs_tell_the_two_tie_orders_apart(k):
    g = pg.tie_graph(k, pg.TIE_ORDER_SEEDS[k])
    ins = pg.in_lists(g)
    assert g.hom_off[-1] == 0 and g.het_off[-1] == 0
    pairs = pg.expected_pairs(g)
    assert 4 in pairs
    for l in (3, 4):
        assert {len(ins[v]) for v in pg.level_vertices(g, l)} == {2}, l
    assert set(pg.composed_in_degrees(g, 4)) == {4}
    assert _model_equals_oracle(g, ())                                  # the model, level by level, is the oracle
    assert _model_equals_oracle(g, pairs, "ref")                        # composed under (ru2, rv2, ru1, rv1): the same paths
    assert pg.solve_colourless(g, pairs, "ranks")[0] == pg.solve_colourless(g, pairs, "ref")[0]      # the values do not depend on the order
    assert not _model_equals_oracle(g, pairs, "ranks")                  # under (ru2, ru1, rv2, rv1) the walk takes other edges


@pytest.mark.parametrize("R", [1, 2, 3, 4, 18])
def test_plane_shift_graph(R):
    g = pg.plane_shift_graph(R)
    ins = pg.in_lists(g)
    assert pg.expected_pairs(g) == [2, 4, 6]
    # a composed candidate of the pair (2, 3) with weight 1 on all four edges, and one that is lighter
    tot = [wu2 + wu1 + wv2 + wv1 for v in pg.level_vertices(g, 3) for (mi, wu2) in ins[v] for (_, wu1) in ins[g.level_off[2] + mi]
           for (mj, wv2) in ins[v] for (_, wv1) in ins[g.level_off[2] + mj]]
    assert max(tot) == 4 and min(tot) < 4
    assert _model_equals_oracle(g, ()) and _model_equals_oracle(g, [2, 4, 6])
    if R >= 2:
        assert orc.dp_solve(g)["value"] != NEG_INF


@pytest.mark.parametrize("mix", [(1, 8), (2, 4), (4, 2), (8, 1)])
def test_in_degree_limit_graphs(mix):
    a, b = mix
    g8, g9 = pg.indeg_limit_graph(mix, a * b), pg.indeg_limit_graph(mix, a * b + 1)
    assert set(pg.composed_in_degrees(g8, 4)) == {8} and pg.expected_pairs(g8) == [2, 4]
    assert {9} <= set(pg.composed_in_degrees(g9, 4)) <= {8, 9} and pg.expected_pairs(g9) == [2]      # one source more: 9 wherever that source leads
    assert {len(x) for x in (pg.in_lists(g8)[v] for v in pg.level_vertices(g8, 4))} == {a}


def test_shared_middle_graph():
    g = pg.shared_middle_graph()
    ins = pg.in_lists(g)
    assert pg.expected_pairs(g) == [2, 4]
    assert g.level_off[4] - g.level_off[3] == 2 and g.level_off[5] - g.level_off[4] == 40
    succ = {int(u) for u in range(g.n_vertices - 1) if g.out_off[u + 1] > g.out_off[u]}
    assert int(g.level_off[2]) + 4 not in succ                           # a dead end on level 2
    ref = orc.dp_solve(g)
    assert ref["value"] > 0
    sink_sources = {i for (i, _) in ins[g.n_vertices - 1]}
    through_0 = {j for j, v in enumerate(pg.level_vertices(g, 4)) if any(i == 0 for (i, _) in ins[v])}
    assert sink_sources <= through_0 and len(through_0) >= 30           # the answer passes the middle vertex that 30 vertices share


@pytest.mark.parametrize("t,k", pg.SLOT_BLOCK_CASES)
def test_slot_block_graphs(t, k):
    g = pg.slot_block_graph(t, k, R=pg.SLOT_BLOCK_R.get((t, k), 18))
    assert pg.expected_pairs(g) == [2, 4]
    assert pg.composed_in_edges(g, 4) == t and g.level_off[5] - g.level_off[4] == k
    assert orc.dp_solve(g)["value"] != NEG_INF


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_parity_graphs(n):
    want = {1: [4], 2: [2, 5], 3: [2, 6], 4: [2, 4]}[n]
    for coloured in ("none", "first", "second", "both"):
        g = pg.parity_graph(n, coloured)
        assert pg.expected_pairs(g) == want, coloured
        has = [any(g.hom_off[v + 1] > g.hom_off[v] or g.het_off[v + 1] > g.het_off[v] for v in pg.level_vertices(g, l)) for l in range(g.n_levels)]
        inner = range(1, g.n_levels - 1)
        assert [has[l] for l in inner] == [{"none": False, "first": bool(l & 1), "second": not l & 1, "both": True}[coloured] for l in inner]
    if n == 4:                                                          # the first transition (source width 1) and the sink inside a pair
        assert g.n_levels == 5 and want[0] == 2 and want[-1] == g.n_levels - 1


def test_every_graph_is_small():
    graphs = [pg.tie_graph(k, s) for k, s in pg.TIE_ORDER_SEEDS.items()] + [pg.plane_shift_graph(3), pg.shared_middle_graph()]
    graphs += [pg.indeg_limit_graph(m, m[0] * m[1] + e) for m in ((1, 8), (2, 4), (4, 2), (8, 1)) for e in (0, 1)]
    graphs += [pg.slot_block_graph(t, k) for t, k in pg.SLOT_BLOCK_CASES] + [pg.parity_graph(n, "both") for n in (1, 2, 3, 4)]
    for g in graphs:
        assert 4 <= g.n_levels <= 9 and max(int(g.level_off[l + 1] - g.level_off[l]) for l in range(g.n_levels)) <= 70

"""CPU: the graphs of tests/test_gpu_pair_levels.py and tests/test_gpu_pair_cells.py keep the properties those tests rely on -- checked
from the arrays, the oracle and the plain model of tests/pair_graphs.py alone (no GPU, no library call)."""
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


# ---------------------------------------------------------------------------------------------- the cases of tests/test_gpu_pair_cells.py
MAX_CELLS = 300_000             # per level: a GPU case stays within a few seconds
_SOLVED = {}


def _case(name):
    if name not in _SOLVED:
        g = pg.CELL_CASES[name][0]()
        _SOLVED[name] = (g, orc.dp_solve(g, want_digest=True))
    return _SOLVED[name]


def _widths(g):
    return [int(g.level_off[l + 1] - g.level_off[l]) for l in range(g.n_levels)]


@pytest.mark.parametrize("name", list(pg.CELL_CASES))
def test_cell_case_pairs_as_stated(name):
    """the pairs are exactly the stated list, at least one; every level is small; and every paired later level has a reachable cell
    (a non-zero digest in the oracle), except exactly where UNREACHABLE_PAIRED says that the planes cannot reach it"""
    g, ref = _case(name)
    stated = pg.CELL_CASES[name][1]
    assert pg.expected_pairs(g) == stated and len(stated) >= 1
    assert max(_widths(g)) ** 2 * (g.R + 1) <= MAX_CELLS
    assert [l for l in stated if ref["digest"][l] == 0] == pg.UNREACHABLE_PAIRED.get(name, [])
    assert set(pg.budgets_checked(g)) <= set(range(g.R + 1)) and {0, g.R} <= set(pg.budgets_checked(g))


def test_unreachable_paired_levels_are_the_light_planes_only():
    assert set(pg.UNREACHABLE_PAIRED) <= set(pg.CELL_CASES)
    for name in pg.UNREACHABLE_PAIRED:
        g = pg.CELL_CASES[name][0]()
        assert name.startswith("plane-") and g.R + 1 <= 7 and g.out_w.mean() >= 0.4, name


@pytest.mark.parametrize("name", list(pg.REFUSED_TWINS))
def test_refused_twin_has_no_pair_at_that_level(name):
    build, stated, refused = pg.REFUSED_TWINS[name]
    g = build()
    assert pg.expected_pairs(g) == stated and refused not in stated and refused - 1 not in stated
    assert max(_widths(g)) ** 2 * (g.R + 1) <= MAX_CELLS
    ref = orc.dp_solve(g, want_digest=True)
    assert ref["digest"][refused] != 0 and ref["digest"][refused - 1] != 0     # both levels show up in the digests when run singly


def test_field_limit_graphs_sit_on_their_limits():
    lists = {}

    def ins_of(g, l):
        if id(g) not in lists:
            lists[id(g)] = (g, pg.in_lists(g))
        return [lists[id(g)][1][v] for v in pg.level_vertices(g, l)]
    for role, l in (("source", 2), ("middle", 3), ("later", 4)):
        for width in (255, 256):
            g = pg.width_limit_graph(role, width)
            assert _widths(g)[l] == width and sorted(_widths(g)[2:5])[1] <= 40
            used = {i for x in ins_of(g, l + 1) for (i, _) in x} if l < 4 else {i for (i, _) in pg.in_lists(g)[g.n_vertices - 1]}
            assert width - 1 in used                                     # the last position is a source of the next level
    for T1 in (2047, 2048):
        g = pg.t_limit_graph(T1)
        deg3 = [len(x) for x in ins_of(g, 3)]
        assert sum(deg3) == T1 and max(deg3) <= pg.MAX_INDEG_LEAN and _widths(g)[3:5] == [255, 255]
        assert set(pg.composed_in_degrees(g, 4)) == {8} and ins_of(g, 4)[254] == [(254, 0)]      # ... whose in-edges are the last 8 delta rows
    g = pg.t2_max_graph()
    assert sum(len(x) for x in ins_of(g, 4)) == 2040 == 255 * pg.MAX_COMPOSED and set(pg.composed_in_degrees(g, 4)) == {8}
    assert 254 in {i for (i, _) in ins_of(g, 4)[254]}
    for n in (64, 65):
        g = pg.lean_limit_graph(n)
        assert max(len(x) for x in ins_of(g, 3)) == n and max(pg.composed_in_degrees(g, 4)) <= pg.MAX_COMPOSED
    assert min(len(x) for x in ins_of(pg.dead_column_graph(True), 3)) == 0 and min(len(x) for x in ins_of(pg.dead_column_graph(False), 3)) == 2
    g = pg.wide_budget_graph()
    assert g.R + 1 == 4097 and max(_widths(g)) <= 3 and len(pg.budgets_checked(g)) == 21


@pytest.mark.parametrize("mix", pg.RANK_MIXES)
def test_rank_graphs(mix):
    a, b = mix
    g = pg.rank_graph(mix)
    ins = pg.in_lists(g)
    assert {len(ins[v]) for v in pg.level_vertices(g, 4)} == {a} and {len(ins[v]) for v in pg.level_vertices(g, 3)} == {b}      # ranks 0..a-1, 0..b-1
    assert set(pg.composed_in_degrees(g, 4)) == {8}
    for l, n in ((4, a), (3, b)):                                       # parallel edges; bundles of either weight wherever there are two
        for v in pg.level_vertices(g, l):
            assert n == 1 or {w for (_, w) in ins[v]} == {0, 1}
            assert n < 8 or len({i for (i, _) in ins[v]}) < n
            assert all(len({w for (i, w) in ins[v] if i == p}) == 1 for p in {i for (i, _) in ins[v]})       # a bundle has one weight
    cw = [pg.composed_weights(g, 4, v, ins) for v in pg.level_vertices(g, 4)]
    if a >= 2:                                                          # w = 0..4 into the cell (v, v)
        assert {0, 1, 2} in cw
    else:                                                               # one in-edge fixes w2: three values per cell, 0..4 over the level
        assert {x + y for p in cw for q in cw for x in p for y in q} == {0, 1, 2, 3, 4}


def test_rank_graphs_reach_rank_7_on_both_levels():
    assert max(a for a, _ in pg.RANK_MIXES) == 8 == max(b for _, b in pg.RANK_MIXES) and all(a * b == 8 for a, b in pg.RANK_MIXES)


def test_plane_graphs():
    assert pg.PLANE_RPS == [1, 2, 3, 4, 5, 7, 19, 41]
    for rc in (2, 4):                                                   # a ragged last chunk for each chunk size above 1, and none
        assert any(RP % rc for RP in pg.PLANE_RPS) and any(RP > rc and RP % rc == 0 for RP in pg.PLANE_RPS + [20, 8])
    for RP in pg.PLANE_RPS:
        for w, want in (("w1", {1}), ("w0", {0}), ("mixed", {0, 1})):
            g = pg.plane_graph(RP, w)
            assert g.R + 1 == RP and set(g.out_w.tolist()) == want
            assert {len(x) for x in pg.in_lists(g)[1:]} <= {1, 2}
    # all four edges of weight 1: source rows r2 - 4 .. r2 - 1 < 0 for the first planes of every chunk size
    assert pg.composed_weights(pg.plane_graph(5, "w1"), 4, int(pg.plane_graph(5, "w1").level_off[4])) == {2}


def test_colour_modes_are_the_four_delta_routes():
    want = {"neither": (False, False), "first": (True, False), "second": (False, True), "both": (True, True)}
    for name, (build, _) in pg.CELL_CASES.items():
        if "/" in name:
            assert pg.delta_routes(build(), 4) == want[name.split("/")[1]], name
    import graphgen
    g = pg.delta_bound_pair_graph()
    assert [int(graphgen.transition_deltas(g, l)[0].max()) for l in (3, 4)] == [65532, 65532]      # both levels of the pair (3, 4)
    assert len(g.hom_col[g.hom_off[3]:g.hom_off[4]]) == 10922 and 6 * 10922 <= 65535 < 6 * 10923


def test_random_layered_graphs_cover_the_parameters():
    assert pg.N_RANDOM >= 40 and sorted(pg.RANDOM_PAIRS) == list(range(pg.N_RANDOM))
    graphs = [pg.random_layered(s) for s in range(pg.N_RANDOM)]
    assert {g.n_levels for g in graphs} == set(range(9, 16))
    assert all(1 <= w <= 40 for g in graphs for w in _widths(g)) and max(w for g in graphs for w in _widths(g)) >= 35
    assert {g.R for g in graphs} <= set(range(25)) and {0, 1, 2, 3, 24} <= {g.R for g in graphs}
    mean_w = [float(g.out_w.mean()) for g in graphs]
    assert [m == 0 for m in mean_w].count(True) >= 13 and [m == 1 for m in mean_w].count(True) >= 13 and [0.2 < m < 0.6 for m in mean_w].count(True) >= 13
    degs = set()
    for g in graphs:
        degs |= {len(x) for x in pg.in_lists(g)[1:]}
    assert {1, 2, 3, 4} <= degs
    later = [l for s in range(pg.N_RANDOM) for l in pg.RANDOM_PAIRS[s]]
    assert sum(l & 1 for l in later) >= 40 and sum(not l & 1 for l in later) >= 40                 # pairs at odd and at even offsets


# ---- the model's digests: solve_colourless(order="ref") is the oracle at every level that is not the earlier level of a pair
def _model_cost(g):
    return sum(w * w * (g.R + 1) * 64 for w in _widths(g))


MODEL_CASES = [n for n in pg.CELL_CASES if n.startswith(("rank-", "plane-", "tie-", "live-")) and (n.endswith("/neither") or "/" not in n)]
MODEL_CASES += [f"random-{s}" for s in (0, 27, 24, 15, 21, 3, 12)]


@pytest.mark.parametrize("name", MODEL_CASES)
def test_model_digests_are_the_oracles(name):
    g, ref = _case(name)
    assert g.hom_off[-1] == 0 and g.het_off[-1] == 0 and _model_cost(g) <= 5_000_000
    pairs = pg.CELL_CASES[name][1]
    single = pg.solve_colourless(g, (), want_digest=True)[3]
    assert single[1:] == [int(x) for x in ref["digest"][1:]]               # level by level: every level
    composed = pg.solve_colourless(g, pairs, "ref", want_digest=True)[3]
    for l in range(1, g.n_levels):
        assert composed[l] == (0 if l + 1 in pairs else int(ref["digest"][l])), l


def test_model_cases_cover_the_colourless_families():
    assert len(MODEL_CASES) >= 4 + 24 + 3 + 7 and sum(n.startswith("random-") for n in MODEL_CASES) >= 7


@pytest.mark.parametrize("k", [2, 3, 5])
def test_the_digest_tells_the_two_tie_orders_apart(k):
    """the order of ranks within the composed lists changes a middle cell some cell came through: the digest of a paired level differs,
    whether or not the walk from the sink passes that cell"""
    g = pg.tie_graph(k, pg.TIE_ORDER_SEEDS[k])
    pairs = pg.expected_pairs(g)
    ref = pg.solve_colourless(g, pairs, "ref", want_digest=True)[3]
    ranks = pg.solve_colourless(g, pairs, "ranks", want_digest=True)[3]
    assert any(ref[l] != ranks[l] for l in pairs)
    assert all(ref[l - 1] == ranks[l - 1] == 0 for l in pairs)


def test_every_graph_is_small():
    graphs = [pg.tie_graph(k, s) for k, s in pg.TIE_ORDER_SEEDS.items()] + [pg.plane_shift_graph(3), pg.shared_middle_graph()]
    graphs += [pg.indeg_limit_graph(m, m[0] * m[1] + e) for m in ((1, 8), (2, 4), (4, 2), (8, 1)) for e in (0, 1)]
    graphs += [pg.slot_block_graph(t, k) for t, k in pg.SLOT_BLOCK_CASES] + [pg.parity_graph(n, "both") for n in (1, 2, 3, 4)]
    for g in graphs:
        assert 4 <= g.n_levels <= 9 and max(int(g.level_off[l + 1] - g.level_off[l]) for l in range(g.n_levels)) <= 70

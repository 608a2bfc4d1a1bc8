"""CPU: the graphs of tests/pair_wide_graphs.py hold what tests/test_gpu_pair_wide.py relies on, and the model of the pairing rule
(choose_pairs) behaves as the rule is written: exactly the earlier rules' choice without the wide form and below pair_wide_min, the wider
choice from it on."""
import pytest

import pair_fanin_graphs as fg
import pair_graphs as pg
import pair_wide_graphs as wg

_G = {}


def _graph(name):
    if name not in _G:
        _G[name] = (wg.CASES.get(name) or wg.REFUSED[name])[0]()
    return _G[name]


def _widths(g):
    return [int(g.level_off[l + 1] - g.level_off[l]) for l in range(g.n_levels)]


def _earlier_rules(g, **rule):
    """the choice of tests/pair_fanin_graphs.py (no wide form), in this module's triples"""
    return [(l, b, False) for (l, b) in fg.choose_pairs(g, pair_fanin_max_big=fg.DEFAULT_MAX_BIG, **rule)]


@pytest.mark.parametrize("name", list(wg.CASES))
def test_the_model_chooses_what_the_case_says(name):
    g, want = _graph(name), wg.CASES[name][1]
    w = _widths(g)
    assert 6 <= g.n_levels <= 8 and 3 <= g.R + 1 <= 8 and max(w) <= 1024
    assert wg.choose_pairs(g) == want and 4 in [l for (l, _, _) in want]
    for (l, big, wide) in want:
        assert wide == (max(w[l - 2], w[l - 1], w[l]) > wg.NARROW_WIDTH and (w[l - 2] <= wg.WIDE_WIDTH or max(w[l - 1], w[l]) > wg.NARROW_WIDTH)), (l, w)
        comp = pg.composed_in_degrees(g, l)
        assert big == sum(c > fg.LIGHT_MAX for c in comp) <= fg.DEFAULT_MAX_BIG and 1 <= min(comp) and max(comp) <= fg.BIG_MAX
    # the gates: without the form, and below its threshold, exactly what the earlier rules choose
    n_wide = sum(1 for (_, _, wide) in want if wide)
    assert wg.choose_pairs(g, pair_wide=0) == wg.choose_pairs(g, pair_wide_min=n_wide + 1) == _earlier_rules(g)
    assert wg.choose_pairs(g, pair_wide_min=n_wide) == want and wg.choose_pairs(g, pair_min=len(want) + 1) == []
    # no big rows in a wide pair: those pairs go, the others stay or move
    assert all(not (wide and big) for (_, big, wide) in wg.choose_pairs(g, pair_wide_fanin=0))
    # a cap of 511 refuses what is wider
    for (l, _, wide) in wg.choose_pairs(g, pair_wide_max_width=511):
        assert not wide or max(w[l - 2], w[l - 1], w[l]) <= 511


@pytest.mark.parametrize("name", list(wg.REFUSED))
def test_refused_levels_lie_in_no_pair(name):
    g, (_, want) = _graph(name), wg.REFUSED[name]
    assert wg.choose_pairs(g) == want and all(l not in (3, 4) for (l, _, _) in want)
    assert name == "big-rows-5" or all(l != 5 for (l, _, _) in want)                            # levels 3 and 4 both materialised


def test_every_role_and_width_is_there():
    for role, l in (("source", 2), ("middle", 3), ("later", 4)):
        for width in (255, 256, 257, 1023):
            w = _widths(_graph(f"width-{role}-{width}"))
            assert w[l] == width and max(w[q] for q in (2, 3, 4) if q != l) <= 40, (role, width)       # this level only
    assert _widths(_graph("width-all-1023"))[2:5] == [1023, 1023, 1023]
    assert _widths(_graph("width-middle-1024"))[3] == 1024 and _widths(_graph("width-later-1024"))[4] == 1024 and _widths(_graph("width-source-1024"))[2] == 1024


def test_in_edge_counts_at_the_cap():
    def T(g, l):
        ins = pg.in_lists(g)
        return sum(len(ins[v]) for v in pg.level_vertices(g, l))
    assert [T(_graph("t-2047-2047"), l) for l in (3, 4)] == [2047, 2047]
    assert [T(_graph("t1-2048"), l) for l in (3, 4)] == [2048, 2047] and [T(_graph("t2-2048"), l) for l in (3, 4)] == [2047, 2048]


def _slot_blocks(comp):
    """64-slot blocks of whole destination columns, as dg_dp_pairs.hip packs them: [composed in-edges per block]"""
    blocks, used = [], 0
    for n in comp:
        if used + n > 64:
            blocks.append(used)
            used = 0
        used += n
    return blocks + [used]


def test_slot_blocks_and_columns():
    assert len(_slot_blocks(pg.composed_in_degrees(_graph("width-all-1023"), 4))) > 8          # composed columns over more than 8 slot blocks
    assert len(_slot_blocks(pg.composed_in_degrees(_graph("t-2047-2047"), 4))) > 8
    comp = pg.composed_in_degrees(_graph("full-blocks"), 4)
    assert set(comp) == {8} and set(_slot_blocks(comp)) == {64} and len(comp) == 320
    comp = pg.composed_in_degrees(_graph("two-columns-of-32"), 4)
    assert comp[256:] == [32, 32] and _slot_blocks(comp)[-1] == 64 and max(comp[:256]) <= 8
    comp = pg.composed_in_degrees(_graph("column-64"), 4)
    assert comp[259] == 64 and max(comp[:259]) <= 8 and len(comp) == 260


def test_the_answer_runs_through_high_middle_positions():
    """every path into the sink of width-all-1023 passes a middle position with bits 8 and 9 set, as row and as column"""
    g = _graph("width-all-1023")
    ins = pg.in_lists(g)
    b3, b4 = int(g.level_off[3]), int(g.level_off[4])
    sink = ins[g.n_vertices - 1]
    middles = {m for (j, _) in sink for (m, _) in ins[b4 + j]}
    assert len(sink) == 3 and middles and all(m & 0x300 == 0x300 for m in middles)
    assert any(j & 0x300 == 0x300 for (j, _) in sink) and all(len(ins[b3 + m]) == 2 for m in middles)
    # the widened graphs: the small graph's vertices sit behind the dead ends, from position 768 on where the level has 800 or more
    for name in ("tie-3/middle", "tie-big-0/all", "shared-middle/all", "indeg-2x4/all"):
        g = _graph(name)
        ins = pg.in_lists(g)
        w = _widths(g)
        assert w[3] >= 800
        for v in pg.level_vertices(g, 4):
            if int(g.out_off[v]) < int(g.out_off[v + 1]):                                       # a vertex with a successor: one of the small graph's
                assert all(m >= 768 for (m, _) in ins[v]), name


@pytest.mark.parametrize("k", list(pg.TIE_ORDER_SEEDS))
def test_widening_keeps_the_walk_of_the_small_graph(k):
    """dead ends in front of a level shift positions and change no rank: the widened tie graphs walk the small graph's edges (whose two
    tie orders differ: tests/test_pair_graphs.py), position by position"""
    small = pg.tie_graph(k, pg.TIE_ORDER_SEEDS[k])
    g = wg.widen(small, {2: 3, 3: 5, 4: 2})
    shift = {int(small.level_off[l]) + i: int(g.level_off[l]) + {2: 3, 3: 5, 4: 2}.get(l, 0) + i for l in range(small.n_levels) for i in range(int(small.level_off[l + 1] - small.level_off[l]))}
    a, b = pg.solve_colourless(small), pg.solve_colourless(g)
    assert a[0] == b[0] and [[(shift[u], shift[v]) for (u, v) in p] for p in a[1:]] == [list(p) for p in b[1:]]
    assert pg.solve_colourless(g, pairs=(4,), order="ref") == b and pg.solve_colourless(g, pairs=(4,), order="ranks")[1:] != b[1:]


def test_big_rows_at_the_gate_and_planes():
    assert [dict((l, b) for (l, b, _) in wg.CASES[n][1])[4] for n in ("big-rows-1/later", "shared-middle-big/all")] == [1, 4]
    g = _graph("big-rows-5")
    assert sum(c > fg.LIGHT_MAX for c in pg.composed_in_degrees(g, 4)) == 5 == fg.DEFAULT_MAX_BIG + 1
    assert (4, 5, True) in wg.choose_pairs(g, pair_fanin_max_big=5)
    assert wg.WIDE_BIG_INLINE == fg.DEFAULT_MAX_BIG                                            # every big row of a shipped wide pair rides inline; the list beyond is read at max_big 5
    planes = sorted({_graph(n).R + 1 for n in wg.CASES if n.startswith("planes-")})
    assert planes == list(wg.PLANES) and min(planes) == 3 and max(planes) == 8 and any(p % 4 and p % 2 for p in planes)
    for weights, want in (("w0", {0}), ("w1", {1})):
        g = _graph(next(n for n in wg.CASES if n.startswith(f"planes-5-{weights}")))
        core = [e for v in pg.level_vertices(g, 4) for e in range(int(g.out_off[v]), int(g.out_off[v + 1]))]
        assert {int(g.out_w[e]) for e in core} == want

"""CPU: the graphs of tests/pair_fanin_graphs.py hold what tests/test_gpu_pair_fanin.py relies on, and the model of the pairing rule
(choose_pairs) behaves as the rule is written: the narrow rule's choice below pair_fanin_min, the wide rule's from it on."""
import pytest

import pair_fanin_graphs as fg
import pair_graphs as pg

_G = {}


def _graph(name):
    if name not in _G:
        _G[name] = (fg.CASES.get(name) or fg.REFUSED[name])[0]()
    return _G[name]


def _comp(g, l=4):
    return pg.composed_in_degrees(g, l)


@pytest.mark.parametrize("name", list(fg.CASES))
def test_the_model_chooses_what_the_case_says(name):
    g, want = _graph(name), fg.CASES[name][1]
    assert 6 <= g.n_levels <= 10 and max(int(g.level_off[l + 1] - g.level_off[l]) for l in range(g.n_levels)) <= 41
    assert fg.choose_pairs(g) == want and any(b for (_, b) in want)
    comp = _comp(g)
    assert sum(c > fg.LIGHT_MAX for c in comp) == dict(want)[4] and max(comp) <= fg.BIG_MAX and min(comp) >= 1
    # the gates: without the form, and below its threshold, exactly the narrow rule's choice -- which pairs other levels, never level 4
    narrow = [(l, 0) for l in pg.expected_pairs(g)]
    assert fg.choose_pairs(g, pair_fanin=0) == narrow == fg.choose_pairs(g, pair_fanin_min=2) and 4 not in dict(narrow)
    assert fg.choose_pairs(g, pair_min=len(want) + 1) == []
    gated = fg.choose_pairs(g, pair_fanin_max_big=fg.DEFAULT_MAX_BIG)
    assert gated == (want if dict(want)[4] <= fg.DEFAULT_MAX_BIG else narrow) and fg.choose_pairs(g, pair_fanin_max_indeg=8) == narrow


def test_composed_in_degrees_at_the_limits():
    for n in (9, 10, 11, 31, 32):
        assert max(_comp(_graph(f"one-big-{n}"))) == n
    g = _graph("one-big-33")
    assert max(_comp(g)) == 33 and all(l not in (3, 4, 5) for (l, _) in fg.choose_pairs(g))      # levels 3 and 4: single launches, in no pair
    # uneven quarters: (n * p) >> 2 for p = 0..4
    assert [[(n * p) >> 2 for p in range(5)] for n in (9, 10, 11)] == [[0, 2, 4, 6, 9], [0, 2, 5, 7, 10], [0, 2, 5, 8, 11]]
    # a column of 32 composed in-edges is one slot block's worth at most; 1, 8, 9 big rows around the inline boundary
    assert fg.BIG_MAX <= 64 and [dict(fg.CASES[f"big-rows-{n}"][1])[4] for n in (1, 8, 9)] == [fg.BIG_INLINE - 7, fg.BIG_INLINE, fg.BIG_INLINE + 1]


def test_which_level_is_the_fan_in_level():
    ins = {n: pg.in_lists(_graph(n)) for n in ("earlier-fanin", "later-fanin", "both-fanin")}

    def dmax(n, l):
        return max(len(ins[n][v]) for v in pg.level_vertices(_graph(n), l))
    assert dmax("earlier-fanin", 3) == 12 and dmax("earlier-fanin", 4) <= 2
    assert dmax("later-fanin", 3) <= 2 and dmax("later-fanin", 4) == 12                     # ranks ru2 / rv2 up to 11
    assert dmax("both-fanin", 3) == 9 and dmax("both-fanin", 4) == 10                        # ru1 / rv1 up to 8, ru2 / rv2 up to 9


def test_shared_and_unused_middle_cells():
    g = _graph("shared-middle")
    ins = pg.in_lists(g)
    used = [m for v in pg.level_vertices(g, 4) for (m, _) in ins[v]]
    assert used.count(0) > 10 and used.count(1) > 10 and 3 not in used and int(g.level_off[4] - g.level_off[3]) == 4


@pytest.mark.parametrize("seed", fg.TIE_SEEDS)
def test_tie_orders_walk_different_edges(seed):
    g = fg.tie_graph(seed)
    plain, ref, ranks = pg.solve_colourless(g), pg.solve_colourless(g, pairs=(2, 4), order="ref"), pg.solve_colourless(g, pairs=(2, 4), order="ranks")
    assert plain == ref and ranks[0] == ref[0] and ranks[1:] != ref[1:]


def test_planes_and_weights():
    assert [_graph(f"planes-{RP}-w1").R + 1 for RP in fg.PLANES] == list(fg.PLANES) and 1 in fg.PLANES and 33 in fg.PLANES
    assert any(RP % 4 and RP % 2 for RP in fg.PLANES)                                       # a ragged last chunk at chunk sizes 2 and 4
    g = _graph("planes-5-w1")
    assert pg.composed_weights(g, 4, int(g.level_off[4]) + 1) == {2} and set(g.out_w.tolist()) == {1}   # row and column together: w = 4, planes down to r2 - 4

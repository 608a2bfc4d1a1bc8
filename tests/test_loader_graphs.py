"""CPU: tests/loader_graphs.py before any GPU test relies on it.  drop_edges keeps what it should in the order it had; every member of
the valid families has the property its name claims, and the oracle alone (tests/oracle_py.py) answers NEG_INF for every graph whose
sink is cut off and something else for EVERY dead_ends member -- a family that lost its sink would pass every device comparison
trivially; every entry of defects() differs from the base graph in the one stated place, gives the base's bytes back when that place is
restored, and is refused by the contract as tests/loader_graphs.py restates it (contract_violation) with the code and the text that
tests/test_gpu_loader_contract.py expects of the library."""
import re

import numpy as np
import pytest

import graphgen
import loader_graphs as lg
import oracle_py as orc
from dipgenie_amd.capi import DpGraphArrays
from paths_model import NEG_INF, PathModel

FAMILIES = lg.valid_families()
MEMBERS = [(fam, name) for fam, members in FAMILIES.items() for name in members]
_REF = {}


def oracle(fam, name):
    if (fam, name) not in _REF:
        _REF[(fam, name)] = orc.dp_solve(FAMILIES[fam][name], want_digest=True)
    return _REF[(fam, name)]


def _edges(g):
    src = lg.sources(g)
    return list(zip(src.tolist(), g.out_dst.tolist(), g.out_w.tolist()))


# ---------------------------------------------------------------------------------------------- drop_edges
def test_drop_edges_keeps_the_rest_in_adjacency_order():
    g = graphgen.random_levelized(9841, n_levels=8, max_width=6, R=2)
    before = _edges(g)
    assert len(set(before)) < len(before)                # parallel edges: copies of one (u, v, w) are told apart by e alone
    for pred in (lambda u, v, w, e: e % 3 == 1, lambda u, v, w, e: w == 1, lambda u, v, w, e: u in (1, 5, 6), lambda u, v, w, e: False, lambda u, v, w, e: True):
        d = lg.drop_edges(g, pred)
        want = [x for e, x in enumerate(before) if not pred(*x, e)]
        assert _edges(d) == want
        assert d.out_off[0] == 0 and d.out_off[-1] == len(want) == d.out_dst.size == d.out_w.size and (np.diff(d.out_off) >= 0).all()
        for n in ("level_off", "hom_off", "hom_col", "het_off", "het_col"):
            assert np.array_equal(getattr(d, n), getattr(g, n))
        assert d.R == g.R and lg.contract_violation(d) is None
    assert _edges(g) == before                           # a copy: the graph given is untouched
    # by hand: the second of three edges of vertex 0, and the only edge of vertex 2
    h = DpGraphArrays(1, level_off=[0, 1, 3, 4], out_off=[0, 3, 4, 5, 5], out_dst=[1, 2, 1, 3, 3], out_w=[0, 1, 0, 1, 0], hom_off=np.zeros(5), hom_col=[],
                      het_off=np.zeros(5), het_col=[])
    d = lg.drop_edges(h, lambda u, v, w, e: e in (1, 4))
    assert d.out_off.tolist() == [0, 2, 3, 3, 3] and d.out_dst.tolist() == [1, 1, 3] and d.out_w.tolist() == [0, 0, 1]
    assert d.out_dst.dtype == np.int32 and d.out_w.dtype == np.uint8 and d.out_off.dtype == np.int64
    assert lg.dead_end_vertices(d).tolist() == [2]


def test_prune_keeps_every_path_and_no_dead_end_on_the_way():
    for name, g in FAMILIES["dead_ends"].items():
        p = lg.prune(g)
        if name in lg.ENUMERABLE_DEAD_NAMES:
            assert PathModel(p).all_paths() == PathModel(g).all_paths()
        paths, _ = PathModel(p).sample_paths(np.random.default_rng(1), 50)      # (asserts "no dead end" at every step)
        m = PathModel(g)
        assert all(m.check_path(x) is None for x in paths)


# ---------------------------------------------------------------------------------------------- the valid families
@pytest.mark.parametrize("fam,name", MEMBERS)
def test_members_are_small_and_inside_the_contract(fam, name):
    g = FAMILIES[fam][name]
    assert lg.contract_violation(g) is None
    assert g.n_levels <= 12 and np.diff(g.level_off).max() <= 9
    assert g.R <= 4 or (fam == "max_budget" and g.R == lg.MAX_R and g.n_levels == 6 and np.diff(g.level_off).max() <= 3)


def test_no_edges():
    assert {name: g.n_levels for name, g in FAMILIES["no_edges"].items()} == {"L2": 2, "L5": 5}
    for name, g in FAMILIES["no_edges"].items():
        assert g.out_off[-1] == 0 and not g.out_off.any() and g.out_dst.size == 0 and g.out_w.size == 0
        ref = oracle("no_edges", name)
        assert ref["value"] == NEG_INF and ref["p1"] == [] and ref["p2"] == [] and not ref["digest"][1:].any()
    g = FAMILIES["no_edges"]["L5"]
    assert (np.diff(g.hom_off) + np.diff(g.het_off) > 0).all()         # every transition is a coloured one, with 0 x 0 score deltas


def test_empty_transition():
    cases = lg.empty_transition()
    assert sorted(cut for _, cut in cases.values()) == [1, 1, 3, 3, 6, 6]
    for name, (g, cut) in cases.items():
        lv, indeg = lg.level_of(g), lg.in_degrees(g)
        assert indeg[lv == cut].sum() == 0
        assert all(indeg[lv == l].sum() > 0 for l in range(1, g.n_levels) if l != cut)
        has = (np.diff(g.hom_off) + np.diff(g.het_off)) > 0
        around = has[(lv == cut - 1) | (lv == cut)]
        assert around.all() if name.endswith("_coloured") else not around.any()
        assert has.any()                                     # (the colourless ones keep their colours elsewhere)
        ref = oracle("empty_transition", name)
        assert ref["value"] == NEG_INF and ref["p1"] == [] and ref["p2"] == []
        assert not ref["digest"][cut:].any() and (cut <= 1 or ref["digest"][1:cut].all())


def test_dead_ends_have_dead_ends_and_the_oracle_still_reaches_the_sink():
    members = FAMILIES["dead_ends"]
    assert list(members)[:6] == lg.ENUMERABLE_DEAD_NAMES and len(members) >= 9
    for name, g in members.items():
        dead = lg.dead_end_vertices(g)
        assert dead.size >= 1 and dead.min() >= 1, name                      # inner vertices
        assert lg.reaches_sink(g)[0], name
        assert oracle("dead_ends", name)["value"] != NEG_INF, name          # a condition on the family, not a measurement
    # a level in which every vertex but one is a dead end
    g, l = lg.lonely_level(graphgen.random_levelized(9823, n_levels=9, max_width=9, min_width=3, R=3, p_w1=0.2, p_colour=0.5))
    assert all(np.array_equal(getattr(g, n), getattr(members["lonely_level"], n)) for n in DpGraphArrays.NAMES)
    a, e = int(g.level_off[l]), int(g.level_off[l + 1])
    assert e - a >= 3 and (np.diff(g.out_off)[a:e] == 0).sum() == e - a - 1
    # the best pair of paths of the undamaged graph ran through the vertex that is a dead end now
    whole = lg.enumerable_graph(0)
    value, p, r = lg.best_pair(0)
    v = lg.best_pair_victim()
    assert value == orc.dp_solve(whole)["value"] and (v in p or v in r)
    assert lg.dead_end_vertices(members["best_path_cut"]).tolist() == [v]
    assert oracle("dead_ends", "best_path_cut")["value"] not in (value, NEG_INF)       # (this graph has no second pair worth as much)


def test_max_budget():
    g = FAMILIES["max_budget"]["R4096"]
    assert g.R == 4096 and set(g.out_w.tolist()) == {0, 1}
    planes = [orc.dp_solve(lg.copy_graph(g, R=b))["value"] for b in (0, 2, 3, 10, 4096)]
    assert planes[0] == NEG_INF and NEG_INF < planes[1] < planes[2] < planes[3] == planes[4] == oracle("max_budget", "R4096")["value"]
    assert lg.MAX_BUDGET_PLANES == [0, 1, 2047, 4095, 4096]


# ---------------------------------------------------------------------------------------------- the refusals
def test_the_base_graph_is_valid_and_coloured():
    g = lg.base_graph()
    assert lg.contract_violation(g) is None and lg.contract_violation(lg.padded(g)) is None
    assert np.diff(g.hom_off).max() >= 3 and np.diff(g.het_off).max() >= 2
    assert orc.dp_solve(g)["value"] not in (0, NEG_INF)
    assert PathModel(g).count_paths() >= 4               # (PathModel refuses parallel edges of different weights: there are none)


def test_every_kind_of_refusal_is_listed():
    names = set(lg.defects())
    assert len(names) == 27
    for kind in ("hom", "het"):
        assert {kind + s for s in ("_off_first", "_off_decrease", "_off_beyond_the_end", "_list_swapped", "_list_repeated")} <= names


@pytest.mark.parametrize("name", list(lg.defects()))
def test_a_defect_is_one_defect(name):
    base = lg.padded(lg.base_graph())
    bad, rc, regex = lg.defects()[name]
    _, _, edits = lg.defect_edits()[name]
    touched = {}
    for arr, at, value in edits:
        touched.setdefault(arr, []).append(at)
    for n in DpGraphArrays.NAMES:
        a, b = getattr(base, n), getattr(bad, n)
        assert a.dtype == b.dtype and a.size == b.size                       # physically as long as the base graph's
        assert np.flatnonzero(a != b).tolist() == sorted(touched.get(n, [])), (name, n)
    assert (bad.R != base.R) == ("R" in touched)
    for kind in ("hom", "het"):                              # zero slack behind the ids, beyond the largest offset any defect writes
        off, col = getattr(bad, kind + "_off"), getattr(bad, kind + "_col")
        true_n = int(getattr(base, kind + "_off")[-1])
        assert off[-1] == true_n and col.size == true_n + lg.COL_SLACK and not col[true_n:].any() and off.max() < col.size
    assert bad.out_off[-1] == base.out_off[-1] == bad.out_dst.size == bad.out_w.size
    # refused by the contract, with the code and the text expected of the library
    got = lg.contract_violation(bad)
    assert got is not None and got[0] == rc and re.search(regex, got[1]), (name, got)
    # and loadable but for that: the edit undone gives the base's bytes
    for arr, at, value in edits:
        if arr == "R":
            bad.R = base.R
        else:
            getattr(bad, arr)[at] = getattr(base, arr)[at]
    assert bad.R == base.R and all(getattr(bad, n).tobytes() == getattr(base, n).tobytes() for n in DpGraphArrays.NAMES)
    assert lg.contract_violation(bad) is None


def test_the_level_that_is_too_wide():
    g, rc, regex = lg.too_wide()
    widths = np.diff(g.level_off)
    assert widths.tolist() == [1, 32769, 1] and g.R == 0 and g.hom_off[-1] == 0 == g.het_off[-1]
    got = lg.contract_violation(g)
    assert got[0] == rc == -5 and re.search(regex, got[1])
    # but for its width the graph is in order: the source's edges enter the level, the level's edges the sink
    lv = lg.level_of(g)
    assert (lv[g.out_dst[:32769]] == 1).all() and (g.out_dst[32769:] == g.n_vertices - 1).all() and (np.diff(g.out_off)[:-1] >= 1).all()
    assert g.out_off[-1] == g.out_dst.size == g.out_w.size == 2 * 32769 and not g.out_w.any()

"""CPU: tests/objective_model.py -- the distinct-colour objective of a pair of paths, stated twice.

A hand-written graph whose counts are written out below, then the two forms against each other and the identities of the
definition on random graphs under the colourings of graphgen.recolour."""
import numpy as np
import pytest

import graphgen
from dipgenie_amd.capi import DpGraphArrays
from objective_model import ObjectiveRanks, objective_sets, objective_sets_many, path_colours
from paths_model import PathModel


def hand_graph():
    """Five levels {0}, {1, 2}, {3, 4}, {5, 6}, {7}; edges 0->1, 0->2, 1->3, 1->4, 2->4, 3->5, 4->6, 5->7, 6->7.
    Hom colour 5 sits on the vertices 1, 3 and 5 of the path 0-1-3-5-7; id 9 is a hom colour (vertices 1, 2) and a het colour
    (vertices 1, 6)."""
    base = DpGraphArrays(1, level_off=np.array([0, 1, 3, 5, 7, 8], np.int32), out_off=np.array([0, 2, 4, 5, 6, 7, 8, 9, 9], np.int64),
                         out_dst=np.array([1, 2, 3, 4, 4, 5, 6, 7, 7], np.int32), out_w=np.array([0, 0, 0, 1, 0, 0, 0, 0, 0], np.uint8),
                         hom_off=np.zeros(9, np.int64), hom_col=np.zeros(0, np.int32), het_off=np.zeros(9, np.int64), het_col=np.zeros(0, np.int32))
    hom = [[7], [5, 9], [9], [5], [20, 30], [5, 20], [], []]
    het = [[], [9, 40, 43], [40], [41, 42], [50, 51, 52], [], [9, 43], [60]]
    return graphgen._with_colours(base, [np.array(x, np.int64) for x in hom], [np.array(x, np.int64) for x in het])


def test_hand_written_graph():
    g = hand_graph()
    m = PathModel(g)
    p, q, p2 = [0, 1, 3, 5, 7], [0, 2, 4, 6, 7], [0, 1, 4, 6, 7]
    assert all(m.check_path(x) is None for x in (p, q, p2))
    # Hom(p) = {5, 7, 9, 20} (5 three times over), Hom(q) = {7, 9, 20, 30}: shared {7, 9, 20}, single {5, 30}
    # Het(p) = {9, 40, 41, 42, 43, 60}, Het(q) = {9, 40, 43, 50, 51, 52, 60}: single {41, 42, 50, 51, 52}, both {9, 40, 43, 60}
    assert path_colours(m, p) == ({5, 7, 9, 20}, {9, 40, 41, 42, 43, 60})
    assert objective_sets(m, p, q) == (3, 2, 5, 4)
    # Hom(p2) = {5, 7, 9, 20, 30}: shared with p {5, 7, 9, 20}, single {30}; Het(p2) = {9, 40, 43, 50, 51, 52, 60}: as q's
    assert objective_sets(m, p, p2) == (4, 1, 5, 4)
    ranks = ObjectiveRanks(g)
    assert (ranks.n_hom, ranks.n_het) == (5, 9)
    assert ranks.many(np.array([[p, q], [p, p2], [q, p]])).tolist() == [[3, 2, 5, 4], [4, 1, 5, 4], [3, 2, 5, 4]]
    assert ranks.bitmap_bytes() == 16


POOL = 200
VARIANTS = {
    "default": dict(),
    "hom_only": dict(hom_only=True),
    "het_only": dict(het_only=True),
    "shared": dict(shared=True),
    "spread_ids": dict(id_map=graphgen.spread_ids(POOL)),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("seed", [4101, 4102, 4103])
def test_forms_agree_and_identities_hold(seed, variant):
    topo = graphgen.random_levelized(seed, n_levels=14, max_width=6, R=3)
    g = graphgen.recolour(topo, seed + 50, p_empty=0.4, p_short=0.3, long_range=(20, 60), pool=POOL, **VARIANTS[variant])
    m = PathModel(g)
    paths, _ = m.sample_pairs(np.random.default_rng(seed), 40)
    a = objective_sets_many(m, paths)
    b = ObjectiveRanks(g).many(paths)
    assert np.array_equal(a, b)
    assert a.sum() > 0
    if variant == "hom_only":
        assert (a[:, 2:] == 0).all()
    if variant == "het_only":
        assert (a[:, :2] == 0).all()
    # symmetric in the two paths
    assert np.array_equal(ObjectiveRanks(g).many(paths[:, ::-1]), a)
    assert np.array_equal(objective_sets_many(m, paths[:, ::-1]), a)
    # a path with itself
    same = np.stack([paths[:, 0], paths[:, 0]], axis=1)
    s = objective_sets_many(m, same)
    assert np.array_equal(ObjectiveRanks(g).many(same), s)
    for row, p in zip(s, paths[:, 0]):
        hom, het = path_colours(m, p)
        assert tuple(row) == (len(hom), 0, 0, len(het))
    # shared + single = the union, per kind
    for row, (p, q) in zip(a, paths):
        (hp, tp), (hq, tq) = path_colours(m, p), path_colours(m, q)
        assert row[0] + row[1] == len(hp | hq) and row[2] + row[3] == len(tp | tq)

"""CPU: the oracle's whole-path output (orc_dp_paths_diploid) against an independent model, and everything that
tests/test_gpu_trace_walk.py relies on in the scripted graphs of tests/trace_graphs.py -- from the arrays and the references alone, so
that the GPU test cannot become vacuous when the script changes.

Classes.  A hop is ((rank, weight, single in-edge) of the first path, the same of the second, merged) with ranks capped at 2
(trace_graphs.hop_classes), computed from the oracle's path and the in-edge order.  On every level 2..L-2 of every graph it must be one
of the two orientations that the script means there (trace_graphs.EXPECT).  Inside one graph every scripted class shows at every
t % 8; a class keeps one orientation on even and the other on odd slots there (the rails swap sides per level and the paths are dealt
anew at every merged level, 13 levels apart), the mirrored graph has them the other way round, so the family shows every orientation
of every class on every slot t = 1..119 (asserted: 55 | 56 and 111 | 112, the batch edges, among them).  Six more graphs run the classes
in another order (trace_graphs.CLASSES_ALT), so that what follows a merged cell or a tie level varies.  t = 0 is the sink, one vertex: a class shows there as far as a merged
destination can (ranks n | n + 1 of one in-edge list, both weights).  A tie level's tie is decoded by the hop that leaves it, one slot
on: tie levels are therefore asserted at t = 55, 56 and 57."""
import copy
import hashlib
import os
import time

import numpy as np
import pytest

import graphgen
import oracle_py as orc
import trace_graphs as tg
import trace_model
from dipgenie_amd.capi import DpGraphArrays
from loader_graphs import contract_violation
from paths_model import NEG_INF, PathModel, edge_list

HERE = os.path.dirname(os.path.abspath(__file__))

# sha256 over R and the eight arrays of every graph of a group, in order (test_sweep_variant_graphs._digest per graph)
PINNED = {
    "narrow": "4ffa8ac9c8fa955d4e4f901a04bef5722b65be4b202d7677733e900ab73d58f6",
    "wide": "dc16ae87e9531466131de6322ef4f9f31f20fc55737486b13108afd329ecea37",
    "ranked": "800cae272fb118fd25f60630fe27f35a4e4cb38681a6426833bdd393afd26f0c",
}
_HOPS = {}


def _digest(names):
    h = hashlib.sha256()
    for name in names:
        g = tg.graph(name)[0]
        h.update(str(g.R).encode())
        for n in DpGraphArrays.NAMES:
            a = getattr(g, n)
            h.update(n.encode())
            h.update(str(a.dtype).encode())
            h.update(a.tobytes())
    return h.hexdigest()


def hops(name):
    """(classes, uncapped ranks) of the oracle's path at budget R"""
    if name not in _HOPS:
        g = tg.graph(name)[0]
        _HOPS[name] = tg.hop_classes(g, tg.oracle_at(name, g.R)[1])
    return _HOPS[name]


def test_the_arrays_are_pinned():
    got = {"narrow": _digest(tg.NARROW), "wide": _digest(tg.WIDE), "ranked": _digest(tg.RANKED)}
    assert got == PINNED, got


@pytest.mark.parametrize("name", tg.ALL)
def test_the_oracles_path_is_the_scripted_optimum(name):
    g, info = tg.graph(name)
    assert contract_violation(g) is None and g.n_levels == tg.N_LEVELS
    m = PathModel(g)
    key, paths = tg.oracle_at(name, g.R)
    value, s_het, p1, p2 = key
    assert value == 2 * (g.n_levels - 1)                                     # the ideal value: both colours on every level
    for h in range(2):
        assert m.check_path(paths[h]) is None, (h, m.check_path(paths[h]))
    score = m.score(paths[0], paths[1])
    assert score == (value, s_het, len(p1) - 1, len(p2) - 1) and score[2] + score[3] == g.R, (score, key)
    assert edge_list(m, paths[0]) == sorted(p1) and edge_list(m, paths[1]) == sorted(p2)
    # the script at every level: rails (or a twin) everywhere, and the hop that was meant
    cls, _ = hops(name)
    altered = {x[0] for x in info.get("wide", [])} | {info["rank"][0]} if "rank" in info else {x[0] for x in info.get("wide", [])}
    for l in range(2, g.n_levels - 1):
        if l in altered:                                                     # (a variant's long in-edge list: asserted by in-degree below)
            continue
        assert cls[l] in tg.EXPECT[info["cls"][l]], (name, l, tg.slot(l), info["cls"][l], cls[l])
    assert cls[1] == ((0, 0, 1), (0, 0, 1), 0) or name.endswith("-wide")     # level 1: one in-edge each (many parallel ones in wide())


def test_every_class_on_every_slot():
    at_mod8, at_slot, sink, top_rank, follows = {}, {}, set(), 0, {}
    for name in tg.NARROW:
        g, info = tg.graph(name)
        cls, ranks = hops(name)
        inside = {}
        for l in range(2, g.n_levels - 1):
            t, c = tg.slot(l), info["cls"][l]
            inside.setdefault(c, set()).add(t % 8)
            follows.setdefault(name in tg.ALT, set()).add((c, info["cls"][l + 1]))
            if name in tg.ALT:                                               # (the family-wide table below is the family's alone)
                continue
            at_mod8.setdefault((c, cls[l]), set()).add(t % 8)
            at_slot.setdefault((c, cls[l]), set()).add(t)
            top_rank = max(top_rank, max(ranks[l]))
        assert set(inside) == set(tg.CLASSES) and all(s == set(range(8)) for s in inside.values()), (name, inside)
        if name in tg.FAMILY:
            sink.add(cls[g.n_levels - 1])
    wanted = {(c, k) for c in tg.CLASSES for k in tg.EXPECT[c]}
    assert set(at_mod8) == wanted
    for ck in sorted(wanted):
        assert at_mod8[ck] == set(range(8)), (ck, at_mod8[ck])
        assert at_slot[ck] == set(range(1, 120)), (ck, sorted(at_slot[ck]))  # every slot but the sink's and level 1's: 55 | 56 and 111 | 112 among them
    assert top_rank == 3                                                     # a rank beyond 2: the in-edge list proper, not its first extra entry
    # the sink: a merged destination, ranks n | n + 1 with n = 0, 1 and 2 or more, each combination of weights
    assert all(c[2] == 1 for c in sink)
    assert {(c[0][0], c[1][0]) for c in sink} >= {(0, 1), (1, 2), (2, 2)}     # (and equal ranks where level L - 2 is merged: parallel edges M -> sink)
    assert {(c[0][1], c[1][1]) for c in sink} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    # the second order: what leaves a merged cell, a tie level, and what leads into a merged level differ from the family's
    # (follows: the class of a level and of the level above it, which the walk decodes one step earlier)
    for c in ("merge", "tie"):
        after = [{b for a, b in follows[alt] if a == c} for alt in (False, True)]
        assert after[0] and after[1] and not (after[0] & after[1]), (c, after)
    assert len(follows[True] - follows[False]) >= 12, sorted(follows[True] - follows[False])
    table = {c: sorted(len(at_slot[(c, k)]) for k in tg.EXPECT[c]) for c in tg.CLASSES}
    print("levels per class and orientation over the family:", table)


def test_tie_levels_are_real():
    slots = set()
    for name in tg.ALL:
        g, info = tg.graph(name)
        m = PathModel(g)
        key, paths = tg.oracle_at(name, g.R)
        assert len(info["twins"]) >= 8, name
        lower = 0
        for l, (twin, orig) in info["twins"].items():
            rows = [h for h in range(2) if int(paths[h][l]) in (twin, orig)]
            assert len(rows) == 1, (name, l)
            h = rows[0]
            assert int(paths[h][l]) == min(twin, orig)                       # the rule's choice: the smaller predecessor
            lower += twin < orig
            other = paths.copy()
            other[h][l] = twin + orig - int(paths[h][l])
            assert m.check_path(other[h]) is None and m.score(other[0], other[1]) == m.score(paths[0], paths[1]), (name, l)
            assert m.hom[twin] == m.hom[orig] and m.succ[twin] == m.succ[orig]
            slots.add(tg.slot(l))
        assert 0 < lower < len(info["twins"]), name                          # twins on either side of their original
    assert {55, 56, 57, 1, 111, 112} <= slots


def test_budgets_matter():
    for name in tg.NARROW:
        g = tg.graph(name)[0]
        values = [tg.oracle_at(name, b)[0][0] for b in range(g.R + 1)]
        assert NEG_INF not in values and values == sorted(values), name
        assert 4 * len(set(values)) >= 3 * len(values), (name, len(set(values)), len(values))
        assert 50 <= g.R <= 60
    for name in tg.WIDE + tg.RANKED:                                         # (relaxation counts grow with the squared in-degree: a subset)
        g = tg.graph(name)[0]
        values = [tg.oracle_at(name, b)[0][0] for b in (0, g.R // 2, g.R)]
        assert NEG_INF not in values and len(set(values)) == 3, (name, values)


def test_the_variants_keep_the_path_and_have_the_in_degrees():
    for phi, name in zip(tg.WIDE_PHIS, tg.WIDE):
        g, info = tg.graph(name)
        base = f"phi{phi}"
        assert np.array_equal(g.level_off, tg.graph(base)[0].level_off) and g.R == tg.graph(base)[0].R
        levels = [l for l, _, _ in info["wide"]]
        assert levels[0] == 1 and levels[1:3] == [tg.N_LEVELS - 1 - 56, tg.N_LEVELS - 1 - 55] and levels[3] in info["merged"] and levels[4] == tg.N_LEVELS - 1
        for l, u, v in info["wide"]:
            assert tg.in_degree(g, v) >= 256 and g.level_off[l] <= v < g.level_off[l + 1]
        deg = np.bincount(g.out_dst, minlength=g.n_vertices)
        wide_levels = {int(np.searchsorted(g.level_off, v, side="right") - 1) for v in np.flatnonzero(deg > 255)}
        assert wide_levels == set(levels)                                    # wide -> wide at 56 | 55, narrow on either side of every other one
        for b in (0, g.R // 2, g.R):
            assert np.array_equal(tg.oracle_at(name, b)[1], tg.oracle_at(base, b)[1]), (name, b)
            assert tg.oracle_at(name, b)[0] == tg.oracle_at(base, b)[0]
        # with lattice_chunk_cells = 1 every wide level is a chunk's last level (where a launch's walk starts) and, but for the sink, which
        # shares its chunk with the levels before it, also its first (where the state is handed on): wide -> wide across a chunk edge at 66 | 65
        ch = tg.chunks(g, 1)
        for l in levels:
            assert any(last == l for _, last in ch), (name, l)
            assert l == tg.N_LEVELS - 1 or (l, l) in ch, (name, l, ch)
        assert any(first < last for first, last in ch)                       # (and narrow levels share chunks: walks of several levels between them)
    base = f"phi{tg.RANK_PHI}"
    for name, indeg in (("rank254", 255), ("rank254-wide", 256)):
        g, info = tg.graph(name)
        l, u, v = info["rank"]
        deg = np.bincount(g.out_dst, minlength=g.n_vertices)
        assert deg[v] == indeg and np.delete(deg, v).max() < 255
        paths = tg.oracle_at(name, g.R)[1]
        h = [int(paths[0][l]), int(paths[1][l])].index(v)                    # the vertex is on the path, its predecessor the last in-edge
        assert hops(name)[1][l][h] == indeg - 1 and hops(name)[0][l][h][0] == 2
        for b in (0, g.R // 2, g.R):
            assert np.array_equal(tg.oracle_at(name, b)[1], tg.oracle_at(base, b)[1]), (name, b)


def _model_equals_oracle(g, budgets):
    """(budgets at which a pair of paths was compared, cells on those paths that only the rule's order decided)"""
    n = n_tied = 0
    for b in budgets:
        gb = copy.copy(g)
        gb.R = b
        value, paths = orc.dp_paths(gb)
        stats = {}
        mvalue, mpaths = trace_model.dp_paths(gb, stats)
        assert value == mvalue == orc.dp_solve(gb)["value"], b
        assert (paths is None) == (mpaths is None) and (paths is None or np.array_equal(paths, mpaths)), b
        n += paths is not None
        n_tied += stats.get("tied", 0)
    return n, n_tied


def test_the_model_equals_the_oracle():
    t0 = time.time()
    for name in ("phi0", "phi6m", "phi11", "alt6"):
        g = tg.graph(name)[0]
        n, n_tied = _model_equals_oracle(g, (0, g.R // 2, g.R))
        assert n == 3 and n_tied >= 8, (name, n, n_tied)                     # (the tie levels, and the two orders of the rails below a merged level)
    # small random graphs: only those count on which at least one pair of paths was compared (an unreachable sink compares nothing)
    n_random = n_paths = n_tied = n_tied_graphs = n_drawn = 0
    for seed in range(40):
        g = graphgen.random_levelized(31000 + seed, n_levels=4 + seed % 27, max_width=5, R=seed % 5, p_w1=0.15, dup_edges=True)
        assert g.n_levels <= 30 and np.diff(g.level_off).max() <= 5 and g.R <= 4
        n, tied = _model_equals_oracle(g, range(g.R + 1))
        n_drawn += 1
        n_random += n > 0
        n_paths += n
        n_tied += tied
        n_tied_graphs += tied > 0
    for dpg in ("toy2_R2.dpg", "toy1_k5w3_R2.dpg"):
        g = DpGraphArrays.load(os.path.join(HERE, "golden", dpg))
        assert _model_equals_oracle(g, range(g.R + 1))[0] >= 1
    print(f"{n_drawn} random graphs drawn, {n_random} with a path compared, {n_paths} paths, {n_tied} tied cells on them in {n_tied_graphs} graphs, "
          f"{time.time() - t0:.1f} s")
    assert n_random >= 20 and n_paths >= 2 * n_random, (n_random, n_paths)
    assert n_tied_graphs >= n_random // 2 and n_tied >= 2 * n_random, (n_tied, n_tied_graphs)   # the tie-break decides on most of them


def test_an_unreachable_sink_gives_no_path():
    g = graphgen.random_levelized(9900 + 11, n_levels=2, R=2)
    cut = DpGraphArrays(2, **{n: getattr(g, n) for n in DpGraphArrays.NAMES})
    cut.out_off = np.zeros_like(g.out_off)                                   # no edge at all
    cut.out_dst, cut.out_w = np.zeros(0, np.int32), np.zeros(0, np.uint8)
    assert orc.dp_paths(cut) == (NEG_INF, None) and trace_model.dp_paths(cut) == (NEG_INF, None)

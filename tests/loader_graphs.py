"""Graphs for the contract of dg_dp_load_graph -- TEST INFRASTRUCTURE, pinned on the CPU by tests/test_loader_graphs.py.

Two kinds.  Valid graphs that tests/graphgen.py cannot draw, because its generators give every vertex but the sink an out-edge: graphs
without any edge, graphs with a level that no edge enters, graphs with dead-end vertices, and one toy at the largest R the loader
accepts.  And defects(): copies of one hand-made graph with exactly one defect each, with the code and the text the loader must refuse
them with -- and contract_violation(), the loader's contract restated in plain Python, which says the same.

No defect graph lets a reader leave the caller's memory, whether the loader checks what it should or not: every array is at least as long
as the base graph's, hom_col and het_col carry COL_SLACK zeros behind their last id (more than the largest offset a defect writes), and
off[nV] / out_off[nV] keep their true values."""
import functools

import numpy as np

import graphgen
from dipgenie_amd.capi import DpGraphArrays
from paths_model import PathModel, strip_colours
from test_gpu_score_paths import ENUMERABLE

MAX_R, MAX_K = 4096, 32768                              # the limits include/dipgenie_hip.h states
COL_SLACK = 16


def copy_graph(g, R=None, **replace):
    arrs = {n: np.array(getattr(g, n), copy=True) for n in DpGraphArrays.NAMES}
    arrs.update(replace)
    return DpGraphArrays(g.R if R is None else R, **arrs)


def sources(g):
    """the source vertex of every out-edge"""
    return np.repeat(np.arange(g.n_vertices), np.diff(g.out_off))


def drop_edges(g, pred):
    """a copy of g without the out-edges e = (u -> v, w) for which pred(u, v, w, e) holds; the others keep their adjacency order"""
    src = sources(g)
    keep = np.array([not pred(int(src[e]), int(g.out_dst[e]), int(g.out_w[e]), e) for e in range(g.out_dst.size)], bool)
    off = np.zeros(g.n_vertices + 1, np.int64)
    np.cumsum(np.bincount(src[keep], minlength=g.n_vertices), out=off[1:])
    return copy_graph(g, out_off=off, out_dst=g.out_dst[keep], out_w=g.out_w[keep])


def level_of(g):
    return np.repeat(np.arange(g.n_levels), np.diff(g.level_off))


def in_degrees(g):
    return np.bincount(g.out_dst, minlength=g.n_vertices)


def dead_end_vertices(g):
    """the vertices before the sink's level that have no out-edge"""
    return np.flatnonzero(np.diff(g.out_off)[:int(g.level_off[-2])] == 0)


# ---------------------------------------------------------------------------------------------- valid families
def no_edges():
    """E = 0 at L = 2 (colourless) and at L = 5 (every vertex coloured: four coloured transitions without a score delta)"""
    a = graphgen.random_levelized(9801, widths=[1, 1], R=2, p_colour=0.0)
    b = graphgen.random_levelized(9802, widths=[1, 3, 2, 4, 1], R=3, p_colour=1.0)
    return {"L2": drop_edges(a, lambda u, v, w, e: True), "L5": drop_edges(b, lambda u, v, w, e: True)}


def empty_transition():
    """name -> (graph, cut): no edge enters level `cut` -- level 1, a middle level, the sink's -- once with colours on every vertex of
    levels cut - 1 and cut, once with none on either (the transition then has no score deltas at all)"""
    base = graphgen.random_levelized(9811, n_levels=7, max_width=5, min_width=2, R=3, p_colour=1.0, max_list=3)
    lv = level_of(base)
    out = {}
    for where, cut in (("first", 1), ("middle", 3), ("sink", base.n_levels - 1)):
        g = drop_edges(base, lambda u, v, w, e: lv[v] == cut)
        out[where + "_coloured"] = (g, cut)
        out[where + "_colourless"] = (strip_colours(g, [cut - 1, cut]), cut)
    return out


def reaches_sink(g):
    """bool [nV]: a path leads from the vertex to the sink"""
    ok = np.zeros(g.n_vertices, bool)
    ok[g.n_vertices - 1] = True
    for u in range(g.n_vertices - 2, -1, -1):
        ok[u] = ok[g.out_dst[g.out_off[u]:g.out_off[u + 1]]].any()
    return ok


def cheapest_path(g):
    """a source -> sink path with the fewest recombinations (the smallest ids among equals), as a list of vertices"""
    INF = 10 ** 9
    cost = np.full(g.n_vertices, INF, np.int64)
    nxt = np.full(g.n_vertices, -1, np.int64)
    cost[g.n_vertices - 1] = 0
    for u in range(g.n_vertices - 2, -1, -1):
        for e in range(int(g.out_off[u]), int(g.out_off[u + 1])):
            c = cost[g.out_dst[e]] + g.out_w[e]
            if c < cost[u] or (c == cost[u] and c < INF and g.out_dst[e] < nxt[u]):
                cost[u], nxt[u] = c, g.out_dst[e]
    assert cost[0] < INF
    path = [0]
    while path[-1] != g.n_vertices - 1:
        path.append(int(nxt[path[-1]]))
    return path


def make_dead_ends(g, victims):
    victims = set(int(v) for v in victims)
    return drop_edges(g, lambda u, v, w, e: u in victims)


def _every_nth(g, n, spare):
    """every n-th inner vertex (levels 1 .. L - 2) that is not spared"""
    inner = [v for v in range(1, int(g.level_off[-2])) if v not in spare]
    return inner[n - 1::n]


def enumerable_graph(q):
    seed, n_levels, extra, p_w1, p_colour = ENUMERABLE[q]
    return graphgen.random_levelized(seed, n_levels=n_levels, max_width=4, R=3, extra_edges=extra, p_w1=p_w1, p_colour=p_colour)


@functools.lru_cache(maxsize=None)
def best_pair(q):
    """brute force on the undamaged enumerable graph q: (value, p, r) of the first pair of paths in enumeration order that is worth the
    most within its R"""
    g = enumerable_graph(q)
    m = PathModel(g)
    paths = m.all_paths()
    rec = [m.recombinations(p) for p in paths]
    best = None
    for a, p in enumerate(paths):
        for b in range(a, len(paths)):
            if rec[a] + rec[b] <= g.R:
                v = m.score(p, paths[b])[0]
                if best is None or v > best[0]:
                    best = (v, p, paths[b])
    return best


N_ENUMERABLE_DEAD = len(ENUMERABLE) + 1


@functools.lru_cache(maxsize=None)
def dead_ends_enumerable(i):
    """the dead_ends members made of the five enumerable graphs: i = 0..4, graph i with every third inner vertex off its cheapest path a
    dead end; i = 5: graph 0 with a vertex of its best pair of paths a dead end (the first one whose loss the sink survives)"""
    if i < len(ENUMERABLE):
        g = enumerable_graph(i)
        return make_dead_ends(g, _every_nth(g, 3, set(cheapest_path(g))))
    g = enumerable_graph(0)
    _, p, r = best_pair(0)
    for v in list(p[1:-1]) + list(r[1:-1]):
        d = make_dead_ends(g, [v])
        if reaches_sink(d)[0] and 2 * PathModel(d).recombinations(cheapest_path(d)) <= d.R:
            return d
    raise AssertionError("every vertex of the best pair is a cut vertex")


def best_pair_victim():
    """the vertex that dead_ends_enumerable(5) turned into a dead end"""
    g, d = enumerable_graph(0), dead_ends_enumerable(5)
    gone = np.flatnonzero((np.diff(g.out_off) > 0) & (np.diff(d.out_off) == 0))
    assert gone.size == 1
    return int(gone[0])


def lonely_level(g):
    """(graph, level): g with every vertex but one of its widest inner level a dead end; the one lies on the cheapest path"""
    keep = cheapest_path(g)
    widths = np.diff(g.level_off)
    l = 1 + int(np.argmax(widths[1:-1]))
    return make_dead_ends(g, [v for v in range(int(g.level_off[l]), int(g.level_off[l + 1])) if v != keep[l]]), l


@functools.lru_cache(maxsize=None)
def dead_ends():
    """name -> graph: inner vertices without out-edges, the sink still reachable within R (test_loader_graphs.py holds the oracle to it)"""
    out = {f"enum{i}": dead_ends_enumerable(i) for i in range(len(ENUMERABLE))}
    out["best_path_cut"] = dead_ends_enumerable(len(ENUMERABLE))
    for name, seed, kw, n in (("random_a", 9821, dict(n_levels=12, max_width=9, R=4, p_colour=0.5), 3),
                              ("random_b", 9822, dict(n_levels=8, max_width=9, min_width=4, R=2, p_w1=0.15, extra_edges=2.5, p_colour=0.3), 2)):
        g = graphgen.random_levelized(seed, **kw)
        out[name] = make_dead_ends(g, _every_nth(g, n, set(cheapest_path(g))))
    out["lonely_level"] = lonely_level(graphgen.random_levelized(9823, n_levels=9, max_width=9, min_width=3, R=3, p_w1=0.2, p_colour=0.5))[0]
    return out


ENUMERABLE_DEAD_NAMES = [f"enum{i}" for i in range(len(ENUMERABLE))] + ["best_path_cut"]


def prune(g):
    """g without the edges into vertices that do not reach the sink: the same source -> sink paths, and PathModel.sample_paths never
    walks into a dead end"""
    ok = reaches_sink(g)
    return drop_edges(g, lambda u, v, w, e: not ok[v])


def max_budget():
    """R = 4096 on six levels of width <= 3, both weights on its edges"""
    return graphgen.random_levelized(9831, widths=[1, 3, 2, 3, 3, 1], R=MAX_R, p_w1=0.5, p_colour=0.8, extra_edges=1.0)


MAX_BUDGET_PLANES = [0, 1, 2047, 4095, 4096]


def valid_families():
    """family -> {name: graph}"""
    return {"no_edges": no_edges(), "empty_transition": {k: g for k, (g, _) in empty_transition().items()}, "dead_ends": dict(dead_ends()),
            "max_budget": {"R4096": max_budget()}}


# ---------------------------------------------------------------------------------------------- the refusals
def _csr(lists, dtype):
    off = np.zeros(len(lists) + 1, np.int64)
    off[1:] = np.cumsum([len(x) for x in lists])
    return off, np.array([c for x in lists for c in x], dtype)


def base_graph():
    """Ten vertices on the levels {0}, {1, 2, 3}, {4, 5, 6}, {7, 8}, {9}, R = 2, made by hand for defects():
      * vertex 1 lists 4 twice in a row, vertex 2 lists 5 twice with an edge to 6 in between (parallel edges of equal weight);
      * 4, 5, 6 send weight 0 to 7 and weight 1 to 8 only, so that one of them may take over the others' edges;
      * the hom ids of 4, 5, 7 and the het ids of 4, 5, 6 ascend across the vertices, so that one list may run into the next."""
    adj = [[(1, 0), (2, 0), (3, 1)], [(4, 0), (4, 0), (5, 1)], [(5, 0), (6, 1), (5, 0)], [(6, 0), (4, 1)],
           [(7, 0), (8, 1)], [(8, 1), (7, 0)], [(8, 1)], [(9, 0)], [(9, 0), (9, 0)], []]
    hom = [[], [1, 4], [2], [], [1, 2, 5], [7], [], [8, 9], [1], []]
    het = [[], [20], [21, 23], [22], [20, 21], [24], [25, 27], [], [22, 24], []]
    out_off, out_dst = _csr([[v for v, _ in a] for a in adj], np.int32)
    _, out_w = _csr([[w for _, w in a] for a in adj], np.uint8)
    hom_off, hom_col = _csr(hom, np.int32)
    het_off, het_col = _csr(het, np.int32)
    return DpGraphArrays(2, level_off=np.array([0, 1, 4, 7, 9, 10], np.int32), out_off=out_off, out_dst=out_dst, out_w=out_w,
                         hom_off=hom_off, hom_col=hom_col, het_off=het_off, het_col=het_col)


def _edits(g):
    """name -> (rc, regex of the message, [(array or "R", index, new value), ...])"""
    nV, L = g.n_vertices, g.n_levels
    e4 = int(g.out_off[4])                                # the edge 4 -> 7
    nxt = r"does not go to the next level"
    out = {
        "edge_same_level": (-1, rf"edge 4->5 {nxt}", [("out_dst", e4, 5)]),
        "edge_earlier_level": (-1, rf"edge 4->2 {nxt}", [("out_dst", e4, 2)]),
        "edge_two_levels_ahead": (-1, rf"edge 4->9 {nxt}", [("out_dst", e4, 9)]),
        "edge_to_minus_one": (-1, rf"edge 4->-1 {nxt}", [("out_dst", e4, -1)]),
        "edge_to_nV": (-1, rf"edge 4->{nV} {nxt}", [("out_dst", e4, nV)]),
        "weight_2": (-1, r"edge weight 2 > 1", [("out_w", e4, 2)]),
        "weight_255": (-1, r"edge weight 255 > 1", [("out_w", e4, 255)]),
        "parallel_adjacent": (-5, r"parallel edges with different weights into vertex 4\b", [("out_w", int(g.out_off[1]) + 1, 1)]),
        "parallel_separated": (-5, r"parallel edges with different weights into vertex 5\b", [("out_w", int(g.out_off[2]) + 2, 1)]),
        "out_off_first": (-1, r"out_off must start at 0", [("out_off", 0, 1)]),
        # vertex 5's list would end before it starts; vertex 4 takes over the edges of 5 and 6, all of them legal for it
        "out_off_decrease": (-1, r"out_off not monotone at 5\b", [("out_off", 5, int(g.out_off[6]) + 1)]),
        "level_empty": (-1, r"level 2 is empty", [("level_off", 3, int(g.level_off[2]))]),
        "level_off_first": (-1, r"level_off must span \[0, n_vertices\]", [("level_off", 0, 1)]),
        "level_off_last": (-1, r"level_off must span \[0, n_vertices\]", [("level_off", L, nV - 1)]),
        "two_sources": (-1, r"level 0 must hold exactly the source vertex", [("level_off", 1, 2)]),
        "R_negative": (-1, r"bad sizes \(V=10 L=5 R=-1\)", [("R", 0, -1)]),
        "R_4097": (-1, r"bad sizes \(V=10 L=5 R=4097\)", [("R", 0, MAX_R + 1)]),
    }
    for kind in ("hom", "het"):
        off, col = getattr(g, kind + "_off"), getattr(g, kind + "_col")
        n = int(off[nV])
        a4 = int(off[4])
        assert off[5] - a4 >= 2 and off[6] > off[5] and off[2] > off[1]
        out[kind + "_off_first"] = (-1, r"colour offsets must start at 0", [(kind + "_off", 0, 1)])
        # vertex 5's list would end before it starts; vertex 4's runs on through the ids of 5 and of the next vertex, ascending still
        out[kind + "_off_decrease"] = (-1, r"colour offsets not monotone at 5\b", [(kind + "_off", 5, int(off[6]) + 1)])
        # past the end of the ids and on: seen from vertex 1 (its end), 2 (both ends) and 3 (its start); the device names whichever lane
        # comes first.  A loader that tested only "end < start" would walk vertex 1's list out of the id array (into the slack, here)
        out[kind + "_off_beyond_the_end"] = (-1, r"colour offsets not monotone at [123]\b", [(kind + "_off", 2, n + 8), (kind + "_off", 3, n + 10)])
        out[kind + "_list_swapped"] = (-1, r"colour list of vertex 4 is not sorted-unique", [(kind + "_col", a4, int(col[a4 + 1])), (kind + "_col", a4 + 1, int(col[a4]))])
        out[kind + "_list_repeated"] = (-1, r"colour list of vertex 4 is not sorted-unique", [(kind + "_col", a4 + 1, int(col[a4]))])
    return out


def padded(g):
    """g with COL_SLACK zeros behind the ids of hom_col and het_col (the offsets do not know of them)"""
    return copy_graph(g, hom_col=np.concatenate([g.hom_col, np.zeros(COL_SLACK, np.int32)]), het_col=np.concatenate([g.het_col, np.zeros(COL_SLACK, np.int32)]))


def defect_edits(g=None):
    return _edits(base_graph() if g is None else g)


def defects(g=None):
    """name -> (bad graph, rc, regex): padded(g) with the one defect the name says (g: base_graph())"""
    g = base_graph() if g is None else g
    out = {}
    for name, (rc, regex, edits) in _edits(g).items():
        bad = padded(g)
        for arr, at, value in edits:
            if arr == "R":
                bad.R = value
            else:
                getattr(bad, arr)[at] = value
        out[name] = (bad, rc, regex)
    return out


def too_wide():
    """(graph, rc, regex): source, a level of 32,769 vertices, sink; every vertex of the level has its edge from the source and to the
    sink; colourless, R = 0"""
    k = MAX_K + 1
    nV = k + 2
    out_off = np.zeros(nV + 1, np.int64)
    out_off[1:k + 2] = k + np.arange(k + 1)
    out_off[k + 2] = 2 * k
    g = DpGraphArrays(0, level_off=np.array([0, 1, k + 1, nV], np.int32), out_off=out_off, out_dst=np.concatenate([np.arange(1, k + 1), np.full(k, k + 1)]).astype(np.int32),
                      out_w=np.zeros(2 * k, np.uint8), hom_off=np.zeros(nV + 1, np.int64), hom_col=np.zeros(COL_SLACK, np.int32), het_off=np.zeros(nV + 1, np.int64),
                      het_col=np.zeros(COL_SLACK, np.int32))
    return g, -5, rf"level width {k} exceeds the supported {MAX_K}"


def contract_violation(g):
    """The contract of dg_dp_load_graph in plain Python: None for a graph it accepts, else (rc, message) of a refusal the loader may
    answer with -- where one defect shows at several places, the first in the order the host-side construction looks at them."""
    nV, L, R = g.n_vertices, g.n_levels, g.R
    lo, oo = g.level_off.tolist(), g.out_off.tolist()
    if nV < 2 or L < 2 or R < 0 or R > MAX_R:
        return -1, f"dg_dp_load_graph: bad sizes (V={nV} L={L} R={R})"
    if lo[0] != 0 or lo[L] != nV:
        return -1, "level_off must span [0, n_vertices]"
    if lo[1] != 1:
        return -1, "level 0 must hold exactly the source vertex"
    for l in range(L):
        if lo[l + 1] <= lo[l]:
            return -1, f"level {l} is empty"
    if max(np.diff(lo)) > MAX_K:
        return -5, f"level width {max(np.diff(lo))} exceeds the supported {MAX_K}"
    if oo[0] != 0:
        return -1, "out_off must start at 0"
    E = oo[nV]
    lv = level_of(g)
    weight_of = {}
    parallel = None
    for u in range(nV):
        if oo[u] < 0 or oo[u + 1] < oo[u] or oo[u + 1] > E:
            return -1, f"out_off not monotone at {u}"
        for e in range(oo[u], oo[u + 1]):
            v, w = int(g.out_dst[e]), int(g.out_w[e])
            if v < 0 or v >= nV or lv[v] != lv[u] + 1:
                return -1, f"edge {u}->{v} does not go to the next level"
            if w > 1:
                return -1, f"edge weight {w} > 1"
            if weight_of.setdefault((u, v), w) != w and parallel is None:
                parallel = v
    if parallel is not None:
        return -5, f"parallel edges with different weights into vertex {parallel}: tie order would be schedule dependent"
    longest = {}
    for kind in ("hom", "het"):
        if getattr(g, kind + "_off")[0] != 0:
            return -1, "colour offsets must start at 0"
    for v in range(nV):
        for kind in ("hom", "het"):
            off, col = getattr(g, kind + "_off").tolist(), getattr(g, kind + "_col")
            if off[v] < 0 or off[v + 1] < off[v] or off[v + 1] > off[nV]:
                return -1, f"colour offsets not monotone at {v}"
            ids = col[off[v]:off[v + 1]].tolist()
            if any(b <= a for a, b in zip(ids, ids[1:])):
                return -1, f"colour list of vertex {v} is not sorted-unique"
            longest[kind] = max(longest.get(kind, 0), len(ids))
    if 2 * longest["hom"] + 4 * longest["het"] > 65535 or max(longest.values()) > 16383:
        return -5, "colour lists too long for uint16 score deltas"
    return None

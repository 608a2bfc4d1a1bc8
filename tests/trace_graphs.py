"""Scripted DP graphs that steer the traceback walkers (dg_dp_trace.hip) -- TEST INFRASTRUCTURE.

Two rails A and B, one per haplotype, carry the hom colours 1 and 2; source, sink and the vertex of a merged level carry both; every other
vertex (a decoy) is colourless.  A transition scores 2 exactly when both levels show both colours, so a pair of paths reaches the ideal
value 2 * (n_levels - 1) only by riding the two rails at every level, and the script -- not chance -- decides what the walk meets there.

An inner level is [d0, d1, (low twin), rail, rail, (high twin), d4, d5]: the rails swap sides from level to level; a merged level is
[d0, d1, M, d4, d5].  In-edges of a vertex are ranked by source position, then adjacency order, so edges from d0 / d1 into a rail vertex
push its rail predecessor to rank 1, 2 or 3, and an edge from d4 / d5 adds an in-edge behind it.  Every decoy has a weight-0 chain of its
own, every rail vertex a weight-0 escape edge to d4 (rail A) or d5 (rail B): a budget below R leaves the rails somewhere, and each
budget answers differently.  R is the number of weight-1 rail hops.

The hop into destination level l has class CLASSES[(n_levels - 1 - l + phi) % P]: n_levels - 1 - l is the slot t of an unsegmented walk
(batches of 56 levels: slots 55 | 56 and 111 | 112 are batch edges).  P = 13 is coprime to the walkers' 8-step unroll, so one graph
shows every class at every t % 8; the family (phi = 0..P-1, each also mirrored: the rails' roles p, q exchanged) puts every class, in
both orientations, on every slot.  Level 1 (all edges leave the source) is always scripted "single".

A tie level gives one rail vertex a twin with the same colours, in-edges and out-edges, right below or right above the rails: the two
predecessors of the next level's cell tie, and only the rule of approximator.cpp:657-659 (smaller pred_i, then smaller pred_j) decides.

CLASSES_ALT is the same cycle in another order (six more graphs): what lies one level ahead of a merged cell or a tie level varies.

chunks() restates how the library packs levels into lattice chunks, so that the tests can say which levels begin and end a chunk.

wide(), rank254(): variants by paths_model.repeat_edge -- parallel edges of equal weight, so neither widths nor the oracle's path change."""
import numpy as np

from dipgenie_amd.capi import DpGraphArrays
from paths_model import repeat_edge

N_LEVELS = 122                         # 121 destination levels: batches of 56 + 56 + 9
P = 13
CLASSES = ["plain", "tie", "p_rank1", "q_rank1", "both_rank1", "p_rank2", "q_rank2_w1", "both_rank2_p_w1", "both_w1", "p_rank1_w1", "merge",
           "single", "q_w1"]
# the same classes in another order: the walkers load one level ahead, and in CLASSES the hop that leaves a merged cell is always
# p_rank1_w1, the one into a merged level always follows single, the one that leaves a tie level is always plain.  (Kept in both orders:
# behind a tie level neither single, p_rank1_w1 nor merge -- the twin adds an in-edge; behind a merged level neither both_w1 nor q_w1 --
# a detour over d4 | d5 would cost what the rail costs.)
CLASSES_ALT = ["plain", "q_w1", "tie", "both_w1", "p_rank2", "merge", "both_rank1", "single", "q_rank2_w1", "p_rank1", "p_rank1_w1", "q_rank1",
               "both_rank2_p_w1"]
assert sorted(CLASSES_ALT) == sorted(CLASSES)
PHIS = list(range(P))
FAMILY = [f"phi{phi}{m}" for phi in PHIS for m in ("", "m")]
ALT = [f"alt{phi}{m}" for phi in (1, 6, 11) for m in ("", "m")]
NARROW = FAMILY + ALT
WIDE_PHIS = (0, 4, 9)
WIDE = [f"phi{phi}-wide" for phi in WIDE_PHIS]
RANK_PHI = 2
_CACHE = {}


def class_of_level(phi, l, order=CLASSES):
    return "single" if l == 1 else order[(N_LEVELS - 1 - l + phi) % P]


def _spec(name, p, q, occ, mirror):
    """the hop of one class: n = low-decoy in-edges in front of each rail's predecessor, w = the rail hops' weights, hi = an in-edge from
    d4 / d5 behind it"""
    n, w, hi = {"A": 0, "B": 0}, {"A": 0, "B": 0}, {"A": 0, "B": 0}
    if name in ("plain", "tie"):
        hi[p] = hi[q] = 1
    elif name == "p_rank1":
        n[p], hi[q] = 1, 1
    elif name == "q_rank1":
        n[q], hi[p] = 1, 1
    elif name == "both_rank1":
        n[p] = n[q] = 1
    elif name == "p_rank2":
        n[p], hi[q] = 2 + occ % 2, 1
    elif name == "q_rank2_w1":
        n[q], w[q], hi[p] = 2, 1, 1
    elif name == "both_rank2_p_w1":
        n[p], n[q], w[p] = 2, 3, 1
    elif name == "both_w1":
        w[p] = w[q] = hi[p] = hi[q] = 1
    elif name == "p_rank1_w1":
        n[p], w[p] = 1, 1                      # (no in-edge from d4 / d5 here: the level before may be merged, and a detour M | d5 -> rail would tie)
    elif name == "merge":
        n[p] = (occ + mirror) % 2              # (the mirrored graph has the other count on the same level)
    elif name == "q_w1":
        w[q], hi[p], hi[q] = 1, 1, 1
    else:
        assert name == "single"
    return n, w, hi


def build(phi, mirror=False, order=CLASSES):
    """(DpGraphArrays with R = the scripted recombinations, info): info["twins"] = {level: (twin vertex, its original)}, info["merged"] =
    the merged levels, info["roles"] = per level {role: vertex}, info["cls"] = per level the class name (None for level 0)"""
    p, q = ("B", "A") if mirror else ("A", "B")
    L = N_LEVELS
    cls = [None] + [class_of_level(phi, l, order) for l in range(1, L)]
    occ, seen = [0] * L, {}
    for l in range(1, L):
        occ[l] = seen.get(cls[l], 0)
        seen[cls[l]] = occ[l] + 1
    # ---- vertices ----
    layout, twin_of = [["S"]], {}
    for l in range(1, L - 1):
        if cls[l] == "merge":
            layout.append(["d0", "d1", "M", "d4", "d5"])
            continue
        rails = ["A", "B"] if l % 2 == 0 else ["B", "A"]
        low, high = [], []
        if cls[l] == "tie":
            twin_of[l] = "AB"[occ[l] % 2]
            (low if (occ[l] // 2) % 2 == 0 else high).append("T")
        layout.append(["d0", "d1"] + low + rails + high + ["d4", "d5"])
    layout.append(["S"])
    level_off = np.zeros(L + 1, np.int32)
    level_off[1:] = np.cumsum([len(x) for x in layout])
    roles = [{role: int(level_off[l]) + pos for pos, role in enumerate(layout[l])} for l in range(L)]
    nV = int(level_off[-1])

    def at(l, rail):
        """the vertices that stand for a rail on level l, in position order"""
        r = roles[l]
        if "S" in r:
            return [r["S"]]
        if "M" in r:
            return [r["M"]]
        return sorted([r[rail]] + ([r["T"]] if twin_of.get(l) == rail else []))

    def decoy(l, d):
        return roles[l].get(d, roles[l].get("S"))

    # ---- edges, level by level; a source's adjacency order is the order in which its edges are made here ----
    edges, R = [], 0
    for l in range(1, L):
        n, w, hi = _spec(cls[l], p, q, occ[l], int(mirror))
        last, joined = l == L - 1, len(at(l, "A")) == 1 and at(l, "A") == at(l, "B")
        if joined and at(l - 1, "A") == at(l - 1, "B"):
            w["A"] = w["B"] = w[p]                                           # one vertex to one vertex: parallel edges carry equal weights
        R += w["A"] + w["B"]
        for d in ("d0", "d1", "d4", "d5"):                                   # chains (the high decoys reach the sink)
            if not last or d in ("d4", "d5"):
                edges.append((decoy(l - 1, d), decoy(l, d), 0))
        for rail in ("A", "B"):
            for u in at(l - 1, rail):
                for v in at(l, rail):
                    edges.append((u, v, w[rail]))
        if l > 1:
            for rail in ((p,) if joined else ("A", "B")):                    # low decoys in front of the rail predecessor: d0 weight 0, d1 weight 1
                srcs = {0: [], 1: ["d1" if occ[l] % 2 else "d0"], 2: ["d0", "d1"], 3: ["d0", "d0", "d1"]}[n[rail]]
                for d in srcs:
                    for v in at(l, rail):
                        edges.append((roles[l - 1][d], v, int(d == "d1")))
            if not joined:
                for rail, d in (("A", "d4"), ("B", "d5")):                   # a high decoy behind it
                    if hi[rail]:
                        for v in at(l, rail):
                            edges.append((roles[l - 1][d], v, 1))
            if not last:
                for rail, d in (("A", "d4"), ("B", "d5")):                   # escapes
                    for u in at(l - 1, rail):
                        edges.append((u, roles[l][d], 0))
    out = [[] for _ in range(nV)]
    weight = {}
    for u, v, wt in edges:
        assert weight.setdefault((u, v), wt) == wt, (u, v)
        out[u].append((v, wt))
    out_off = np.zeros(nV + 1, np.int64)
    out_off[1:] = np.cumsum([len(o) for o in out])
    hom = [[] for _ in range(nV)]
    for l in range(L):
        for role, v in roles[l].items():
            rail = twin_of.get(l) if role == "T" else role
            hom[v] = {"A": [1], "B": [2], "M": [1, 2], "S": [1, 2]}.get(rail, [])
    hom_off = np.zeros(nV + 1, np.int64)
    hom_off[1:] = np.cumsum([len(x) for x in hom])
    g = DpGraphArrays(R, level_off=level_off, out_off=out_off, out_dst=np.array([v for o in out for v, _ in o], np.int32),
                      out_w=np.array([wt for o in out for _, wt in o], np.uint8), hom_off=hom_off, hom_col=np.array([c for x in hom for c in x], np.int32),
                      het_off=np.zeros(nV + 1, np.int64), het_col=np.zeros(0, np.int32))
    info = dict(phi=phi, mirror=mirror, cls=cls, roles=roles, merged=[l for l in range(1, L - 1) if "M" in roles[l]],
                twins={l: (roles[l]["T"], roles[l][rail]) for l, rail in twin_of.items()})
    return g, info


# ---------------------------------------------------------------------------------------------- variants with long in-edge lists
def in_degree(g, v):
    return int((g.out_dst == v).sum())


def first_edge(g, u, v):
    for e in range(int(g.out_off[u]), int(g.out_off[u + 1])):
        if g.out_dst[e] == v:
            return e
    raise KeyError((u, v))


def _fill(g, u, v, indeg):
    """g with the edge u -> v repeated until v has `indeg` in-edges"""
    return repeat_edge(g, first_edge(g, u, v), indeg - in_degree(g, v))


def wide_spots(info):
    """(level, source, destination) of the rail-A edges that wide() repeats: into the levels of slots 56 and 55 (two wide levels in a row),
    level 1 (a chunk's l_lo), a merged level and the sink"""
    roles, L = info["roles"], N_LEVELS

    def rail(l):
        r = roles[l]
        return r.get("A", r.get("M", r.get("S")))
    merged = [l for l in info["merged"] if l not in (L - 1 - 55, L - 1 - 56)]
    return [(l, rail(l - 1), rail(l)) for l in (1, L - 1 - 56, L - 1 - 55, merged[len(merged) // 2], L - 1)]


def wide(phi):
    """build(phi) with five levels made wide (in-degree 256 + level % 7 >= 256): the general walker's wide branch, wide -> wide, wide -> narrow
    and narrow -> wide hops, at a batch edge, at both ends of the walk and on a merged level"""
    g, info = build(phi)
    spots = wide_spots(info)
    for l, u, v in spots:
        g = _fill(g, u, v, 256 + l % 7)
    return g, dict(info, wide=spots)


def rank_spot(info):
    """(level, decoy source, rail-A vertex) of a both_rank1 hop near the middle: that vertex has two in-edges, the decoy's first"""
    ls = [l for l in range(2, N_LEVELS - 1) if info["cls"][l] == "both_rank1"]
    l = ls[len(ls) // 2]
    d = "d1" if (len(ls) // 2) % 2 else "d0"                                 # (build() alternates the decoy by occurrence, counted from level 1 upwards)
    return l, info["roles"][l - 1][d], info["roles"][l]["A"]


def rank254(indeg):
    """build(RANK_PHI) with a lower-positioned decoy's edge into a rail vertex repeated until that vertex has `indeg` in-edges: 255 is the
    largest in-degree of a narrow level (the rail predecessor is the last entry, rank 254), 256 makes the level wide"""
    g, info = build(RANK_PHI)
    l, u, v = rank_spot(info)
    assert in_degree(g, v) == 2 and g.out_dst[first_edge(g, u, v)] == v
    return _fill(g, u, v, indeg), dict(info, rank=(l, u, v))


def graph(name):
    """(graph, info) by name: NARROW, WIDE, "rank254" (in-degree 255) and "rank254-wide" (in-degree 256) -- built once"""
    if name not in _CACHE:
        if name.startswith("rank254"):
            _CACHE[name] = rank254(256 if name.endswith("-wide") else 255)
        elif name.endswith("-wide"):
            _CACHE[name] = wide(int(name[3:-5]))
        else:
            _CACHE[name] = build(int(name[3:].rstrip("m")), name.endswith("m"), CLASSES_ALT if name.startswith("alt") else CLASSES)
    return _CACHE[name]


RANKED = ["rank254", "rank254-wide"]
ALL = NARROW + WIDE + RANKED


_ORACLE = {}


def oracle_at(name, b):
    """the oracle on graph(name)'s arrays with g.R = b (as test_gpu_budgets.oracle_per_budget solves it): (key, paths) with key = (value,
    s_het, p1, p2) as DpOutcome.key() gives it and paths = int32 [2, n_levels], all -1 where the budget is unreachable -- solved once"""
    import copy

    import oracle_py as orc
    if (name, b) not in _ORACLE:
        g = copy.copy(graph(name)[0])
        g.R = b
        ref = orc.dp_solve(g)
        value, paths = orc.dp_paths(g)
        assert value == ref["value"]
        paths = np.full((2, g.n_levels), -1, np.int32) if paths is None else paths
        paths.setflags(write=False)
        _ORACLE[(name, b)] = ((ref["value"], ref["s_het"], tuple(ref["p1"]), tuple(ref["p2"])), paths)
    return _ORACLE[(name, b)]


def slot(l):
    """the slot of destination level l in an unsegmented walk"""
    return N_LEVELS - 1 - l


# ---------------------------------------------------------------------------------------------- what a path meets, from the arrays alone
def in_edges(g):
    """per vertex the in-edge sources in rank order (source position, then adjacency order) and their weights"""
    src = np.repeat(np.arange(g.n_vertices), np.diff(g.out_off))
    order = np.lexsort((np.arange(src.size), src, g.out_dst))               # by destination, then source id (= position inside a level), then edge number
    off = np.zeros(g.n_vertices + 1, np.int64)
    np.cumsum(np.bincount(g.out_dst, minlength=g.n_vertices), out=off[1:])
    return off, src[order], g.out_w[order]


def hop_classes(g, paths):
    """per destination level l = 1..L-1 (index l; index 0 is None) the hop of the pair of paths `paths` [2, L] as
    ((rank_i, weight_i, single_i), (rank_j, weight_j, single_j), merged): rank = first position of the predecessor in the destination's
    in-edge list, capped at 2; single = the destination has exactly one in-edge; merged = both paths stand on one vertex.  Also the
    uncapped ranks."""
    off, src, w = in_edges(g)
    out, ranks = [None], [None]
    for l in range(1, g.n_levels):
        halves, rk = [], []
        for h in range(2):
            u, v = int(paths[h][l - 1]), int(paths[h][l])
            lst = src[off[v]:off[v + 1]]
            r = int(np.flatnonzero(lst == u)[0])
            rk.append(r)
            halves.append((min(r, 2), int(w[off[v] + r]), int(lst.size == 1)))
        out.append((halves[0], halves[1], int(paths[0][l] == paths[1][l])))
        ranks.append(tuple(rk))
    return out, ranks


def chunks(g, chunk_cells):
    """The lattice chunks of g under option lattice_chunk_cells = chunk_cells, as (first, last) destination levels -- the library's packing
     restated: a level takes (R + 1) * k2 * k2 back-pointer units, twice that where an in-degree exceeds 255, rounded up to
    even; a chunk holds max(chunk_cells rounded up to even, the largest level) units and is closed when the next level does not fit."""
    k2 = np.diff(g.level_off).astype(np.int64)
    deg = np.bincount(g.out_dst, minlength=g.n_vertices)
    units = [0] + [int((((2 if deg[g.level_off[l]:g.level_off[l + 1]].max() > 255 else 1) * (g.R + 1) * k2[l] * k2[l]) + 1) & ~1) for l in range(1, g.n_levels)]
    cap = max((chunk_cells + 1) & ~1, max(units))
    out, first, acc = [], 1, 0
    for l in range(1, g.n_levels):
        if acc > 0 and acc + units[l] > cap:
            out.append((first, l - 1))
            first, acc = l, 0
        acc += units[l]
    out.append((first, g.n_levels - 1))
    return out


def _both(a, b, merged=0):
    return {(a, b, merged), (b, a, merged)}


# what the oracle's path must show on a level of each scripted class (levels 2..L-2), in its two orientations
EXPECT = {
    "plain": _both((0, 0, 0), (0, 0, 0)), "tie": _both((0, 0, 0), (0, 0, 0)),
    "p_rank1": _both((1, 0, 0), (0, 0, 0)), "q_rank1": _both((1, 0, 0), (0, 0, 0)), "both_rank1": _both((1, 0, 0), (1, 0, 0)),
    "p_rank2": _both((2, 0, 0), (0, 0, 0)), "q_rank2_w1": _both((2, 1, 0), (0, 0, 0)), "both_rank2_p_w1": _both((2, 1, 0), (2, 0, 0)),
    "both_w1": _both((0, 1, 0), (0, 1, 0)), "p_rank1_w1": _both((1, 1, 0), (0, 0, 1)),
    "merge": {((0, 0, 0), (1, 0, 0), 1), ((1, 0, 0), (2, 0, 0), 1)},         # (one in-edge list: the first path's predecessor always ranks first)
    "single": _both((0, 0, 1), (0, 0, 1)), "q_w1": _both((0, 1, 0), (0, 0, 0)),
}

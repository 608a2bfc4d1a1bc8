"""Graphs and a plain model for the level-pair form of the sweep (tests/test_pair_graphs.py on the CPU, tests/test_gpu_pair_levels.py
on the GPU) -- test infrastructure.

A level pair (l - 1, l) is swept by ONE launch as a composed transition from level l - 2 (dipgenie_amd/csrc/dg_dp_pairs.hip).  The
graphs here are written out edge by edge, so that every in-degree, composed in-degree and composed in-edge count is what the case
says; expected_pairs() restates the library's eligibility rule and greedy choice from the arrays alone, and solve_colourless() is
the DP on a graph without colours, level by level or with the pairs composed under either tie order."""
import numpy as np

from dipgenie_amd.capi import DpGraphArrays

MAX_COMPOSED = 8          # composed in-degree of a vertex of the later level
MAX_WIDTH = 255           # both levels of a pair
MAX_T = 2047              # in-edges into either level
MAX_INDEG_LEAN = 64       # a column with more in-edges takes the general variant: not lean


def from_edges(R, widths, edges, hom=None, het=None):
    """widths[l] vertices on level l; edges[l] = [(i, j, w), ...] from position i of level l to position j of level l + 1, in the
    adjacency order given (in-edges of a vertex are ranked by source position, then by this order); hom / het: {vertex id: ids}"""
    widths = [int(w) for w in widths]
    assert widths[0] == 1 and widths[-1] == 1 and len(edges) == len(widths) - 1
    level_off = np.zeros(len(widths) + 1, np.int32)
    level_off[1:] = np.cumsum(widths)
    nV = int(level_off[-1])
    out = [[] for _ in range(nV)]
    for l, el in enumerate(edges):
        for (i, j, w) in el:
            assert 0 <= i < widths[l] and 0 <= j < widths[l + 1] and w in (0, 1), (l, i, j, w)
            out[level_off[l] + i].append((int(level_off[l + 1]) + j, w))
    out_off = np.zeros(nV + 1, np.int64)
    out_off[1:] = np.cumsum([len(o) for o in out])
    lists = {}
    for kind, given in (("hom", hom or {}), ("het", het or {})):
        per = [sorted(set(int(x) for x in given.get(v, ()))) for v in range(nV)]
        off = np.zeros(nV + 1, np.int64)
        off[1:] = np.cumsum([len(x) for x in per])
        lists[kind + "_off"] = off
        lists[kind + "_col"] = np.array([c for x in per for c in x], np.int32)
    return DpGraphArrays(R, level_off=level_off, out_off=out_off, out_dst=np.array([d for o in out for (d, _) in o], np.int32),
                         out_w=np.array([w for o in out for (_, w) in o], np.uint8), **lists)


def with_R(g, R):
    return DpGraphArrays(R, **{n: getattr(g, n) for n in DpGraphArrays.NAMES})


def in_lists(g):
    """per vertex its in-edges [(source position in its level, weight), ...] in rank order: source position, then adjacency order"""
    ins = [[] for _ in range(g.n_vertices)]
    for l in range(g.n_levels - 1):
        for u in range(int(g.level_off[l]), int(g.level_off[l + 1])):
            for e in range(int(g.out_off[u]), int(g.out_off[u + 1])):
                ins[int(g.out_dst[e])].append((u - int(g.level_off[l]), int(g.out_w[e])))
    return ins


def level_vertices(g, l):
    return range(int(g.level_off[l]), int(g.level_off[l + 1]))


def composed_in_degrees(g, l, ins=None):
    """of the vertices of level l over the pair (l - 1, l): the sum over a vertex's in-edges p -> v of the in-degree of p"""
    ins = ins or in_lists(g)
    a0 = int(g.level_off[l - 1])
    return [sum(len(ins[a0 + i]) for (i, _) in ins[v]) for v in level_vertices(g, l)]


def composed_in_edges(g, l, ins=None):
    """T' of the pair (l - 1, l): composed in-edges into level l"""
    return sum(composed_in_degrees(g, l, ins))


def expected_pairs(g):
    """the later levels of the pairs the library chooses: greedy from the left, disjoint; both levels lean (no vertex with more than
    64 in-edges) without a dead column, at most 255 wide with at most 2,047 in-edges, composed in-degree 1..8 everywhere"""
    ins = in_lists(g)

    def level_ok(l):
        deg = [len(ins[v]) for v in level_vertices(g, l)]
        return min(deg) >= 1 and max(deg) <= MAX_INDEG_LEAN and len(deg) <= MAX_WIDTH and sum(deg) <= MAX_T
    out, l = [], 2
    while l < g.n_levels:
        if level_ok(l - 1) and level_ok(l) and max(composed_in_degrees(g, l, ins)) <= MAX_COMPOSED:
            out.append(l)
            l += 2
        else:
            l += 1
    return out


def solve_colourless(g, pairs=(), order="ref"):
    """The diploid DP on a graph without colours (every score delta 0), as plain loops.  A cell (i, j, r) of level l takes the best
    of state[l - 1][pi][pj][r - wu - wv] over its row in-edges (rank ru) and column in-edges (rank rv); ties go to (ru asc, rv asc).
    For l in `pairs` the levels (l - 1, l) are composed instead: the candidates are (ru2, ru1) x (rv2, rv1) read from level l - 2, ties
    go by order "ref" = (ru2, rv2, ru1, rv1) -- the level-by-level order -- or "ranks" = (ru2, ru1, rv2, rv1), the order of ranks
    within the composed lists; the winner writes the back-pointer of its cell and of the middle cell it came through.  Returns
    (sink values per plane, p1, p2) with the paths as the oracle lists them: the weight-1 edges and, last, the edge into the sink."""
    assert g.hom_off[-1] == 0 and g.het_off[-1] == 0
    ins, RP, L = in_lists(g), g.R + 1, g.n_levels
    width = [int(g.level_off[l + 1] - g.level_off[l]) for l in range(L)]
    val = {0: {(0, 0, r): 0 for r in range(RP)}}
    bp = {}
    l = 1
    while l < L:
        b0 = int(g.level_off[l])
        if l + 1 in pairs:
            m0, c0 = b0, int(g.level_off[l + 1])
            cur, nxt = val[l - 1], {}
            for i2 in range(width[l + 1]):
                rows = [(ru2, ru1, pi, mi, w2 + w1) for ru2, (mi, w2) in enumerate(ins[c0 + i2]) for ru1, (pi, w1) in enumerate(ins[m0 + mi])]
                rows = [(ru2, ru1, pi, mi, w, ins[c0 + i2][ru2][1]) for (ru2, ru1, pi, mi, w) in rows]
                for j2 in range(width[l + 1]):
                    cols = [(rv2, rv1, pj, mj, w2 + w1, w2) for rv2, (mj, w2) in enumerate(ins[c0 + j2]) for rv1, (pj, w1) in enumerate(ins[m0 + mj])]
                    for r in range(RP):
                        best = None
                        for (ru2, ru1, pi, mi, wu, wu2) in rows:
                            for (rv2, rv1, pj, mj, wv, wv2) in cols:
                                v = cur.get((pi, pj, r - wu - wv))
                                if v is None:
                                    continue
                                tie = (ru2, rv2, ru1, rv1) if order == "ref" else (ru2, ru1, rv2, rv1)
                                key = (-v, tie)
                                if best is None or key < best[0]:
                                    best = (key, v, (ru2, rv2), (mi, mj, r - wu2 - wv2), (ru1, rv1))
                        if best is not None:
                            nxt[(i2, j2, r)] = best[1]
                            bp[(l + 1, i2, j2, r)] = best[2]
                            bp[(l,) + best[3]] = best[4]
            val[l + 1] = nxt
            l += 2
            continue
        cur, nxt = val[l - 1], {}
        for i2 in range(width[l]):
            for j2 in range(width[l]):
                for r in range(RP):
                    best = None
                    for ru, (pi, wu) in enumerate(ins[b0 + i2]):
                        for rv, (pj, wv) in enumerate(ins[b0 + j2]):
                            v = cur.get((pi, pj, r - wu - wv))
                            if v is not None and (best is None or (-v, (ru, rv)) < best[0]):
                                best = ((-v, (ru, rv)), v)
                    if best is not None:
                        nxt[(i2, j2, r)] = best[1]
                        bp[(l, i2, j2, r)] = best[0][1]
        val[l] = nxt
        l += 1
    sink = [val[L - 1].get((0, 0, r)) for r in range(RP)]
    p1, p2 = [], []
    if sink[g.R] is not None:
        i, j, r = 0, 0, g.R
        for lv in range(L - 1, 0, -1):
            ru, rv = bp[(lv, i, j, r)]
            (pi, wu), (pj, wv) = ins[int(g.level_off[lv]) + i][ru], ins[int(g.level_off[lv]) + j][rv]
            a0 = int(g.level_off[lv - 1])
            for (path, p, w, x) in ((p1, pi, wu, i), (p2, pj, wv, j)):
                path += [(a0 + p, int(g.level_off[lv]) + x)] * (int(lv == L - 1) + w)     # (a weight-1 edge into the sink is listed twice)
            i, j, r = pi, pj, r - wu - wv
        p1.reverse()
        p2.reverse()
    return sink, p1, p2


# ---------------------------------------------------------------------------------------------- the cases
def _rand_edges(rng, k, k2, indeg, p_w1):
    """edges of one transition: vertex j of the next level gets indeg(j) distinct sources; every source keeps at least one out-edge
    where the in-degrees leave room (else it is a dead end, which the DP allows)"""
    el = []
    for j in range(k2):
        d = min(int(indeg(j)), k)
        for i in sorted(rng.choice(k, d, replace=False).tolist()):
            el.append((int(i), j, int(rng.random() < p_w1)))
    rng.shuffle(el)                                             # adjacency order is not position order
    return [tuple(int(x) for x in e) for e in el]


def layered(seed, R, widths, indeg, p_w1=0.4, colour_levels=(), n_colours=10):
    """indeg[l](j) = in-degree of position j of level l + 1 (an int serves every position); colour_levels: levels whose vertices carry
    short hom / het lists"""
    rng = np.random.default_rng(seed)
    edges = []
    for l in range(len(widths) - 1):
        f = indeg[l] if callable(indeg[l]) else (lambda j, d=indeg[l]: d)
        edges.append(_rand_edges(rng, widths[l], widths[l + 1], f, p_w1))
    off = np.concatenate([[0], np.cumsum(widths)])
    hom, het = {}, {}
    for l in colour_levels:
        for v in range(int(off[l]), int(off[l + 1])):
            if rng.random() < 0.7:
                hom[v] = rng.integers(0, n_colours, int(rng.integers(1, 4))).tolist()
            if rng.random() < 0.7:
                het[v] = (n_colours + rng.integers(0, n_colours, int(rng.integers(1, 4)))).tolist()
    return from_edges(R, widths, edges, hom, het)


def tie_graph(k, seed, R=2):
    """colourless, in-degree 2 on both levels of the pair (3, 4) (composed in-degree 4) and of the pair (1, 2) where the width allows"""
    return layered(seed, R, [1, k, k, k, k, 1], [1, min(2, k), 2, 2, min(k, 4)], p_w1=0.5)


# width -> a seed on which the two tie orders of solve_colourless walk different paths (tests/test_pair_graphs.py asserts it)
TIE_ORDER_SEEDS = {2: 54, 3: 57, 5: 199}


def plane_shift_graph(R):
    """pair (2, 3): every edge weighs 1 except those that leave position 0, so most composed candidates have weight 1 on all four edges
    (w = 4, source planes down to r2 - 4 < 0) and a few weigh less; the pair (4, 5) mixes weights"""
    rng = np.random.default_rng(77)
    e01 = [(0, j, 0) for j in range(3)]
    e12 = [(int(i), j, int(i != 0)) for j in range(4) for i in sorted(rng.choice(3, 2, replace=False).tolist())]
    e23 = [(int(i), j, int(i != 0)) for j in range(3) for i in sorted(rng.choice(4, 2, replace=False).tolist())]
    e34 = _rand_edges(rng, 3, 3, lambda j: 2, 0.5)
    e45 = _rand_edges(rng, 3, 2, lambda j: 2, 0.5)
    e56 = [(0, 0, 0), (1, 0, 1)]
    return from_edges(R, [1, 3, 4, 3, 3, 2, 1], [e01, e12, e23, e34, e45, e56])


def indeg_limit_graph(mix, total, seed=5):
    """levels (3, 4): every vertex of level 4 has mix[0] in-edges whose sources have mix[1] in-edges each, so its composed in-degree is
    mix[0] * mix[1]; with total = mix[0] * mix[1] + 1 one source of ONE vertex has an in-edge more (composed in-degree 9: no pair)"""
    a, b = mix
    assert total in (a * b, a * b + 1)
    rng = np.random.default_rng(seed)
    k = 9
    e01 = [(0, j, 0) for j in range(k)]
    e12 = _rand_edges(rng, k, k, lambda j: 1, 0.3)              # pair (1, 2): composed in-degree 1
    e23 = _rand_edges(rng, k, k, lambda j: b, 0.3)
    e34 = _rand_edges(rng, k, k, lambda j: a, 0.3)
    if total == a * b + 1:
        i_src = [i for (i, j, w) in e34 if j == 0][0]            # a source of vertex 0 of level 4 ...
        have = {i for (i, j, w) in e23 if j == i_src}
        e23.append((min(set(range(k)) - have), i_src, 0))       # ... gets one in-edge more
    e45 = [(i, 0, i & 1) for i in range(k)]
    return from_edges(3, [1, k, k, k, k, 1], [e01, e12, e23, e34, e45], hom={v: [v % 5] for v in range(1 + 2 * k, 1 + 4 * k)})


def shared_middle_graph(R=3):
    """level 3 has 2 vertices, level 4 has 40 that all come from them (pairs (1, 2) and (3, 4)): many cells of level 4 share a middle
    cell; vertex 1 of level 3 leads only to vertices that the sink's few in-edges do not come from, and level 2 has a dead end"""
    rng = np.random.default_rng(11)
    e01 = [(0, j, 0) for j in range(4)]
    e12 = _rand_edges(rng, 4, 5, lambda j: 2, 0.4)
    e23 = [(0, 0, 0), (1, 0, 1), (2, 1, 0), (3, 1, 1)]            # position 4 of level 2: no successor
    e34 = [(0, j, int(rng.random() < 0.3)) for j in range(30)] + [(1, j, 0) for j in range(20, 40)]
    e45 = [(j, 0, j & 1) for j in range(0, 8)]                   # the sink: 8 in-edges, from vertices reached through vertex 0 of level 3 only
    return from_edges(R, [1, 4, 5, 2, 40, 1], [e01, e12, e23, e34, e45], hom={8: [1, 2], 10: [2], 11: [1]}, het={12: [30], 13: [31]})


# (composed in-edges, destination width): 63 / 64 / 65 / 129 around the 64-slot block, widths 1 and 65
SLOT_BLOCK_CASES = [(63, 33), (64, 33), (65, 65), (129, 65), (8, 1), (5, 1)]
SLOT_BLOCK_R = {(129, 65): 40}      # R + 1 = 41 planes over three slot blocks: the cost model takes the largest chunk size there


def slot_block_graph(t_composed, k_dst, R=18):
    """pair (3, 4) with exactly t_composed composed in-edges into a level of k_dst vertices (in-degree 1 or 2 over sources of in-degree
    1, 2 or 4), behind the pair (1, 2)"""
    rng = np.random.default_rng(1000 + t_composed + k_dst)
    k = 12
    per = [t_composed // k_dst + (1 if j < t_composed % k_dst else 0) for j in range(k_dst)]      # composed in-degree per destination
    assert min(per) >= 1 and max(per) <= 8
    # sources of level 3: positions 0..3 have in-degree 1, 4..7 in-degree 2, 8..11 in-degree 4
    deg3 = [1] * 4 + [2] * 4 + [4] * 4
    split = {1: [1], 2: [2], 3: [1, 2], 4: [4], 5: [1, 4], 6: [2, 4], 7: [1, 2, 4], 8: [4, 4]}
    e34 = []
    for j, c in enumerate(per):
        used = set()
        for d in split[c]:
            i = [q for q in range(k) if deg3[q] == d and q not in used][int(rng.integers(0, 3))]
            used.add(i)
            e34.append((i, j, int(rng.random() < 0.4)))
    e01 = [(0, j, 0) for j in range(k)]
    e12 = _rand_edges(rng, k, k, lambda j: 1, 0.3)
    e23 = _rand_edges(rng, k, k, lambda j: deg3[j], 0.3)
    n_sink = min(k_dst, 8)
    e45 = [(j, 0, j & 1) for j in range(n_sink)]
    nV4 = 1 + 3 * k
    return from_edges(R, [1, k, k, k, k_dst, 1], [e01, e12, e23, e34, e45], hom={v: [v % 7] for v in range(1 + 2 * k, nV4, 2)},
                      het={v: [40 + v % 3] for v in range(1 + 2 * k, nV4 + min(k_dst, 6), 3)})


def parity_graph(n_pairable, coloured, seed=0):
    """a run of n_pairable levels of in-degree <= 2 (levels 1 .. n_pairable, the first transition with source width 1 inside the
    first pair), closed by a level of in-degree 9 unless the run reaches the sink, which then lies inside a pair; coloured: "none",
    "first" (odd levels), "second" (even levels) or "both\""""
    k = 10
    if n_pairable >= 4:
        widths, indeg = [1, k, k, k, 1], [1, 2, 2, 4]                                          # sink: 4 in-edges over sources of in-degree 2
    else:
        widths = [1] + [k] * (n_pairable + 2) + [1]
        indeg = [1] + [2] * (n_pairable - 1) + [9, 1] + [3]
    levels = range(1, len(widths) - 1)
    cl = {"none": (), "first": [l for l in levels if l & 1], "second": [l for l in levels if not l & 1], "both": list(levels)}[coloured]
    return layered(900 + 10 * n_pairable + seed, 4, widths, indeg, colour_levels=cl)

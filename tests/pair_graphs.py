"""Graphs and a plain model for the level-pair form of the sweep (tests/test_pair_graphs.py on the CPU, tests/test_gpu_pair_levels.py
and tests/test_gpu_pair_cells.py on the GPU) -- test infrastructure.

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


DIGEST_PRED_MUL = 0x9E3779B97F4A7C15          # oracle/oracle_dp.cpp: weight of the predecessor term of a level digest


def level_digest(k, cells):
    """the oracle's digest of a level of width k: over its reachable cells {(i, j, r): (value, pred_i, pred_j)}, with t the r-major
    cell index, the sum mod 2^64 of uint32(value + 1) * (t + 1) + DIGEST_PRED_MUL * (((pred_i << 15) | pred_j) + 1) * (t + 1)"""
    d = 0
    for (i, j, r), (v, pi, pj) in cells.items():
        t = (r * k + i) * k + j
        d += ((v + 1) & 0xFFFFFFFF) * (t + 1) + DIGEST_PRED_MUL * (((pi << 15) | pj) + 1) * (t + 1)
    return d & 0xFFFFFFFFFFFFFFFF


def solve_colourless(g, pairs=(), order="ref", want_digest=False):
    """The diploid DP on a graph without colours (every score delta 0), as plain loops.  A cell (i, j, r) of level l takes the best
    of state[l - 1][pi][pj][r - wu - wv] over its row in-edges (rank ru) and column in-edges (rank rv); ties go to (ru asc, rv asc).
    For l in `pairs` the levels (l - 1, l) are composed instead: the candidates are (ru2, ru1) x (rv2, rv1) read from level l - 2, ties
    go by order "ref" = (ru2, rv2, ru1, rv1) -- the level-by-level order -- or "ranks" = (ru2, ru1, rv2, rv1), the order of ranks
    within the composed lists; the winner writes the back-pointer of its cell and of the middle cell it came through.  Returns
    (sink values per plane, p1, p2) with the paths as the oracle lists them: the weight-1 edges and, last, the edge into the sink.
    want_digest: a fourth entry, the per-level digests by the oracle's definition (level_digest) as Python ints -- of a composed pair
    the later level's, whose predecessors are the middle cells, and 0 for the earlier level, which is never materialised."""
    assert g.hom_off[-1] == 0 and g.het_off[-1] == 0
    ins, RP, L = in_lists(g), g.R + 1, g.n_levels
    width = [int(g.level_off[l + 1] - g.level_off[l]) for l in range(L)]
    val = {0: {(0, 0, r): 0 for r in range(RP)}}
    bp = {}
    pred = {}                                                   # level -> {cell: (value, pred_i, pred_j)}
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
                            pred.setdefault(l + 1, {})[(i2, j2, r)] = (best[1], best[3][0], best[3][1])
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
                                best = ((-v, (ru, rv)), v, pi, pj)
                    if best is not None:
                        nxt[(i2, j2, r)] = best[1]
                        bp[(l, i2, j2, r)] = best[0][1]
                        pred.setdefault(l, {})[(i2, j2, r)] = best[1:]
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
    if want_digest:
        return sink, p1, p2, [level_digest(width[lv], pred.get(lv, {})) for lv in range(L)]
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


# ---------------------------------------------------------------------------------------------- the cell-by-cell cases
# tests/test_gpu_pair_cells.py runs every graph below (and those above) with the pair kernel's digest form, so that every cell of a
# later level is compared with the oracle; tests/test_pair_graphs.py holds their properties on the CPU.
COLOUR_MODES = ("neither", "first", "second", "both")


def with_colours(g, levels, seed=0, n_colours=10):
    """g with short hom / het lists, drawn as layered() draws them, on every vertex of the given levels (the other lists stay)"""
    rng = np.random.default_rng(7000 + seed)
    hom = {v: g.hom_col[g.hom_off[v]:g.hom_off[v + 1]].tolist() for v in range(g.n_vertices)}
    het = {v: g.het_col[g.het_off[v]:g.het_off[v + 1]].tolist() for v in range(g.n_vertices)}
    for l in levels:
        for v in level_vertices(g, l):
            if rng.random() < 0.7:
                hom[v] = rng.integers(0, n_colours, int(rng.integers(1, 4))).tolist()
            if rng.random() < 0.7:
                het[v] = (n_colours + rng.integers(0, n_colours, int(rng.integers(1, 4)))).tolist()
    lists = {}
    for kind, given in (("hom", hom), ("het", het)):
        per = [sorted(set(int(x) for x in given[v])) for v in range(g.n_vertices)]
        off = np.zeros(g.n_vertices + 1, np.int64)
        off[1:] = np.cumsum([len(x) for x in per])
        lists[kind + "_off"] = off
        lists[kind + "_col"] = np.array([c for x in per for c in x], np.int32)
    return DpGraphArrays(g.R, level_off=g.level_off, out_off=g.out_off, out_dst=g.out_dst, out_w=g.out_w, **lists)


def coloured(g, l, mode, seed=0):
    """the score-delta routes of the pair (l - 1, l).  A transition scores where either of its levels carries a colour, so: "neither"
    = no colours; "first" = level l - 2 coloured (transition into l - 1 only); "second" = level l coloured (transition into l only);
    "both" = levels l - 2, l - 1 and l coloured"""
    return with_colours(g, {"neither": (), "first": (l - 2,), "second": (l,), "both": (l - 2, l - 1, l)}[mode], seed)


def delta_routes(g, l):
    """(the transition into level l - 1 scores, the transition into level l scores)"""
    has = [any(g.hom_off[v + 1] > g.hom_off[v] or g.het_off[v + 1] > g.het_off[v] for v in level_vertices(g, q)) for q in range(g.n_levels)]
    return (has[l - 2] or has[l - 1], has[l - 1] or has[l])


def _front(k_src, R, rng):
    """levels 0..2 in front of a pair (3, 4): 4 vertices, then k_src vertices of in-degree 1 (the pair (1, 2) while k_src <= 255)"""
    return [[(0, j, 0) for j in range(4)], [(int(rng.integers(0, 4)), j, int(rng.random() < 0.4)) for j in range(k_src)]]


def _pick(rng, k, d, must=None):
    """d distinct positions below k in rising order, `must` among them"""
    s = set() if must is None else {must}
    while len(s) < d:
        s.add(int(rng.integers(0, k)))
    return sorted(s)


def width_limit_graph(role, width, R=3):
    """pair (3, 4) from level 2: the source (2), middle (3) or later (4) level is `width` wide, the other two 6 to 40; in-degree 2 on
    both levels of the pair, the last position of the wide level is used (position 254 at width 255), the sink has 3 in-edges"""
    ks, km, kl = {"source": (width, 7, 9), "middle": (6, width, 40), "later": (6, 7, width)}[role]
    rng = np.random.default_rng(300 + width + len(role))
    e23 = [(i, m, int(rng.random() < 0.4)) for m in range(km) for i in _pick(rng, ks, 2, ks - 1 if m == 0 else None)]
    e34 = [(m, j, int(rng.random() < 0.4)) for j in range(kl) for m in _pick(rng, km, 2, km - 1 if j == 0 else None)]
    e45 = [(0, 0, 0), (1, 0, 1), (kl - 1, 0, 0)]
    return from_edges(R, [1, 4, ks, km, kl, 1], _front(ks, R, rng) + [e23, e34, e45])


def t_limit_graph(T1, R=1):
    """pair (3, 4): 255 x 255 vertices, exactly T1 in-edges into level 3.  Positions 5..254 of level 3 have 8 in-edges and one
    successor each (composed in-degree 8 on level 4); positions 0..4 are dead ends that take the remaining T1 - 2,000 in-edges (9
    and more each: at most 64, so the level stays lean).  The in-edges of position 254 are the delta rows T1 - 8 .. T1 - 1."""
    rng = np.random.default_rng(2047)
    rest = T1 - 2000
    deg = [9, 9, 9, 9, rest - 36] + [8] * 250
    assert sum(deg) == T1 and 9 <= deg[4] <= 16
    e23 = [(i, m, int(rng.random() < 0.4)) for m in range(255) for i in _pick(rng, 16, deg[m])]
    e34 = [(max(j, 5), j, j & 1) for j in range(255)]
    e45 = [(0, 0, 0), (100, 0, 1), (254, 0, 0)]
    return from_edges(R, [1, 4, 16, 255, 255, 1], _front(16, R, rng) + [e23, e34, e45])


def t2_max_graph(R=1):
    """pair (3, 4) with the most in-edges the later level can have: 255 vertices x 8 in-edges over sources of in-degree 1 = 2,040
    (every in-edge adds at least 1 to the composed in-degree, so 2,047 into the later level cannot be reached under the limit of 8)"""
    rng = np.random.default_rng(2040)
    e23 = [(int(rng.integers(0, 16)), m, int(rng.random() < 0.4)) for m in range(255)]
    e34 = [(m, j, int(rng.random() < 0.4)) for j in range(255) for m in _pick(rng, 255, 8, 254 if j == 254 else None)]
    e45 = [(0, 0, 0), (100, 0, 1), (254, 0, 0)]
    return from_edges(R, [1, 4, 16, 255, 255, 1], _front(16, R, rng) + [e23, e34, e45])


def lean_limit_graph(n, R=3):
    """pair (3, 4): position 0 of level 3 is a dead end with n in-edges (64: the level is lean; 65: it takes the general variant and
    nothing is paired with it); the other five have 2 in-edges, the 8 vertices of level 4 come from two of those (composed 4)"""
    rng = np.random.default_rng(64)
    e23 = [(i, 0, i & 1) for i in range(n)] + [(i, m, int(rng.random() < 0.4)) for m in range(1, 6) for i in _pick(rng, 70, 2)]
    e34 = [(1 + m, j, int(rng.random() < 0.4)) for j in range(8) for m in _pick(rng, 5, 2)]
    e45 = [(0, 0, 0), (1, 0, 1), (7, 0, 0)]
    return from_edges(R, [1, 4, 70, 6, 8, 1], _front(70, R, rng) + [e23, e34, e45])


def dead_column_graph(dead, R=3):
    """pair (3, 4) of in-degree 2 on both levels; dead: position 3 of the middle level has no in-edge (and no successor)"""
    rng = np.random.default_rng(33)
    e23 = [(i, m, int(rng.random() < 0.4)) for m in range(7) for i in _pick(rng, 6, 2) if not (dead and m == 3)]
    e34 = [(m, j, int(rng.random() < 0.4)) for j in range(9) for m in _pick(rng, 7, 2, 3 if j == 0 else None)]
    if dead:
        e34 = [(m, j, w) for (m, j, w) in e34 if m != 3] + [(4, 0, 1)]          # vertex 0 of level 4 keeps two in-edges
        e34 = sorted(set(e34), key=lambda e: (e[1], e[0]))
    e45 = [(0, 0, 0), (1, 0, 1), (8, 0, 0)]
    return from_edges(R, [1, 4, 6, 7, 9, 1], _front(6, R, rng) + [e23, e34, e45])


def wide_budget_graph(R=4096):
    """R + 1 = 4,097 planes (bit 12 of the plane count, beside the source width from bit 13 on) on levels at most 3 wide: pairs
    (1, 2), (3, 4), (5, 6), mixed weights"""
    rng = np.random.default_rng(4096)
    widths = [1, 2, 3, 3, 2, 3, 1]
    edges = [[(0, 0, 0), (0, 1, 1)]] + [_rand_edges(rng, widths[l], widths[l + 1], lambda j: 2, 0.5) for l in range(1, 6)]
    return from_edges(R, widths, edges)


def _bundles(n, k, first, wbit):
    """n in-edges as bundles of parallel edges over the k source positions, starting at position `first`: [(position, weight)];
    the edges of a bundle share their weight (the loader refuses parallel edges of different weights), bundles alternate by wbit"""
    size = [n // k + (1 if q < n % k else 0) for q in range(k)]
    return [((first + q) % k, ((first + q) >> wbit) & 1) for q in range(k) for _ in range(size[q])]


RANK_MIXES = [(8, 1), (4, 2), (2, 4), (1, 8)]


def rank_graph(mix, R=6):
    """pair (3, 4), composed in-degree 8 = a in-edges into every vertex of level 4 over middle vertices of b in-edges each, as bundles
    of parallel edges from 3 (into level 3) and 4 (into level 4) positions: the ranks run up to a - 1 and b - 1 whatever the widths,
    and bundles of weight 0 and of weight 1 come from neighbouring positions"""
    a, b = mix
    e01 = [(0, j, 0) for j in range(3)]
    e12 = [(j, (j + 1) % 3, j & 1) for j in range(3)]
    e23 = [(i, m, w) for m in range(4) for (i, w) in _bundles(b, 3, m % 3, 0)]
    e34 = [(m, j, w) for j in range(4) for (m, w) in _bundles(a, 4, j, 0)]
    e45 = [(j, 0, j & 1) for j in range(4)]
    return from_edges(R, [1, 3, 3, 4, 4, 1], [e01, e12, e23, e34, e45])


def composed_weights(g, l, v, ins=None):
    """the set of w2 + w1 over the composed in-edges of vertex v (a vertex id) of level l"""
    ins = ins or in_lists(g)
    return {w2 + w1 for (m, w2) in ins[v] for (_, w1) in ins[int(g.level_off[l - 1]) + m]}


PLANE_RPS = [1, 2, 3, 4, 5, 7, 19, 41]
PLANE_WEIGHTS = {"w1": 1.0, "w0": 0.0, "mixed": 0.5}


def plane_graph(RP, weights):
    """pairs (1, 2), (3, 4), (5, 6) of in-degree 2 on RP planes; every edge weighs 1 ("w1": a composed candidate reads plane r2 - 4,
    and level l is reachable from plane 2 l on), 0 ("w0") or either ("mixed")"""
    rng = np.random.default_rng(500 + RP)
    widths = [1, 3, 4, 3, 3, 2, 1]
    edges = [_rand_edges(rng, widths[l], widths[l + 1], lambda j: 2, PLANE_WEIGHTS[weights]) for l in range(6)]
    return from_edges(RP - 1, widths, edges)


def delta_bound_pair_graph(M=10922):
    """levels {0}, {1, 2}, {3, 4}, {5, 6}, {7, 8}, {9}, two disjoint chains, all weights 0, R = 1; pairs (1, 2) and (3, 4).  With a =
    arange(M): the hom lists of the chain vertices alternate a, a + M along a chain and between the chains, the het lists are
    disjoint blocks of M ids.  From level 2 on, the two chain edges of a transition then score 2 M + 4 M = 6 M = 65,532 against each
    other with M = 10,922, the largest lists colour_lists_fit_delta accepts with both kinds: both transitions of the pair (3, 4)."""
    a = list(range(M))
    edges = [[(0, 0, 0), (0, 1, 0)]] + [[(0, 0, 0), (1, 1, 0)]] * 3 + [[(0, 0, 0), (1, 0, 0)]]
    hom, het = {}, {}
    for l in (2, 3, 4):
        for c in (0, 1):
            v = 1 + 2 * (l - 1) + c
            hom[v] = [x + M * ((l + c) & 1) for x in a]
            het[v] = [x + M * (2 + 2 * l + c) for x in a]
    return from_edges(1, [1, 2, 2, 2, 2, 1], edges, hom, het)


N_RANDOM = 42


def random_layered(seed):
    """9..15 levels of width 1..40, in-degrees 1..4 mixed inside a level, p_w1 in {0, 0.4, 1} and R in 0..24 by the seed; a level of
    in-degree 9 at a place the seed chooses, so that runs of pairs start at odd and at even levels.  Every vertex has an in-edge, so
    a level has a reachable cell as soon as R covers the lightest pair of paths into it: with p_w1 = 1 that is 2 per level, so those
    graphs have at most 13 levels and R >= 2 (levels - 1); with p_w1 = 0, R is 0..3."""
    rng = np.random.default_rng(8000 + seed)
    p_w1 = (0.0, 0.4, 1.0)[seed % 3]
    L = 9 + (seed // 3) % (5 if p_w1 == 1.0 else 7)
    R = {0.0: (seed // 3) % 4, 0.4: [8, 13, 24, 5, 18][(seed // 3) % 5], 1.0: min(24, 2 * (L - 1) + (seed // 3) % 3)}[p_w1]
    widths = [1] + [int(rng.integers(1, 41)) for _ in range(L - 2)] + [1]
    block = 2 + seed % 5
    widths[block - 1] = max(widths[block - 1], 9)
    indeg = []
    for l in range(L - 1):
        if l + 1 == block:
            indeg.append(9)
        else:
            top = int(rng.integers(1, 5))
            indeg.append(lambda j, top=top, s=int(rng.integers(0, 4)): 1 + (j + s) % top)
    return layered(8000 + seed, R, widths, indeg, p_w1=p_w1)


# seed -> expected_pairs(random_layered(seed)), written out (tests/test_pair_graphs.py compares)
RANDOM_PAIRS = {
    0: [4, 7], 1: [2, 5, 7], 2: [2, 7], 3: [2, 4, 7, 9], 4: [2, 4, 8], 5: [4, 6, 8], 6: [2, 5, 7, 9], 7: [2, 6, 8, 10], 8: [2, 4, 7, 9],
    9: [2, 4, 11], 10: [4, 6, 8, 10], 11: [2, 5, 9, 11], 12: [2, 7, 9, 11], 13: [2, 4, 7, 9, 11], 14: [2, 5, 8, 10, 12],
    15: [4, 6, 8, 10, 12], 16: [2, 5, 7, 9, 11, 13], 17: [2, 6, 8], 18: [2, 4, 7, 9, 13], 19: [2, 5, 8, 10, 12, 14], 20: [4, 6, 8],
    21: [2, 5, 8], 22: [2, 8], 23: [2, 4, 7, 10], 24: [2, 4, 9], 25: [4, 6, 9], 26: [2, 5, 7, 9, 11], 27: [2, 6, 8, 10], 28: [2, 4, 7, 10],
    29: [2, 4, 8, 12], 30: [4, 6, 8, 10], 31: [2, 5, 7, 9, 11], 32: [2, 6, 8], 33: [2, 4, 7, 9, 11], 34: [2, 4, 8, 11], 35: [5, 7, 9],
    36: [2, 5, 10, 12], 37: [2, 6, 8, 10, 12], 38: [2, 4, 7, 9], 39: [2, 4, 8, 10, 12, 14], 40: [4, 7, 10, 12, 14], 41: [2, 6, 8, 10],
}


def long_graph():
    return layered(4242, 5, [1] + [10] * 7 + [1], [1, 2, 2, 2, 2, 2, 2, 4], colour_levels=(2, 3, 5, 8))     # pairs (1,2) (3,4) (5,6) (7,8)


def _cell_cases():
    """name -> (builder, the later levels of the pairs the library must choose); every graph has at least one pair"""
    c = {}

    def modes(name, build, pairs, l=4):
        for q, mode in enumerate(COLOUR_MODES):
            c[f"{name}/{mode}"] = (lambda build=build, mode=mode, q=q: coloured(build(), l, mode, q), pairs)
    # field limits.  (The source level of a pair has no width limit of its own -- a source position has 15 bits -- so 256 sources are
    # paired as well; the later level cannot have more than 255 x 8 = 2,040 in-edges.)
    modes("width-source-255", lambda: width_limit_graph("source", 255), [2, 4])
    modes("width-source-256", lambda: width_limit_graph("source", 256), [4])
    modes("width-middle-255", lambda: width_limit_graph("middle", 255), [2, 4])
    modes("width-later-255", lambda: width_limit_graph("later", 255), [2, 4])
    modes("t1-2047", lambda: t_limit_graph(2047), [2, 4])
    modes("t2-2040", t2_max_graph, [2, 4])
    modes("lean-64", lambda: lean_limit_graph(64), [2, 4])
    modes("planes-4097", wide_budget_graph, [2, 4, 6])
    c["live-columns"] = (lambda: dead_column_graph(False), [2, 4])
    c["delta-bound"] = (delta_bound_pair_graph, [2, 4])
    for mix in RANK_MIXES:
        modes(f"rank-{mix[0]}x{mix[1]}", lambda mix=mix: rank_graph(mix), [2, 4])
    for RP in PLANE_RPS:
        for w in PLANE_WEIGHTS:
            modes(f"plane-{RP}-{w}", lambda RP=RP, w=w: plane_graph(RP, w), [2, 4, 6])
    for seed in range(N_RANDOM):
        c[f"random-{seed}"] = (lambda seed=seed: random_layered(seed), RANDOM_PAIRS[seed])
    # the graphs of tests/test_gpu_pair_levels.py
    for k, seed in TIE_ORDER_SEEDS.items():
        c[f"tie-{k}"] = (lambda k=k, seed=seed: tie_graph(k, seed), [2, 4])
    for R in (1, 2, 3, 4, 18):
        c[f"plane-shift-{R}"] = (lambda R=R: plane_shift_graph(R), [2, 4, 6])
    for mix in RANK_MIXES:
        c[f"indeg-{mix[0]}x{mix[1]}"] = (lambda mix=mix: indeg_limit_graph(mix, 8), [2, 4])
    for R in (3, 0, 1):
        c[f"shared-middle-{R}"] = (lambda R=R: shared_middle_graph(R), [2, 4])
    for t, k in SLOT_BLOCK_CASES:
        c[f"slots-{t}-{k}"] = (lambda t=t, k=k: slot_block_graph(t, k, R=SLOT_BLOCK_R.get((t, k), 18)), [2, 4])
    for n, pairs in ((1, [4]), (2, [2, 5]), (3, [2, 6]), (4, [2, 4])):
        for mode in ("none", "first", "second", "both"):
            c[f"parity-{n}-{mode}"] = (lambda n=n, mode=mode: parity_graph(n, mode), pairs)
    c["long"] = (long_graph, [2, 4, 6, 8])
    return c


CELL_CASES = _cell_cases()

# name -> (builder, the pairs that remain, the level at which the twin's pair is refused: neither it nor its predecessor may lie in a pair)
REFUSED_TWINS = {
    "width-middle-256": (lambda: width_limit_graph("middle", 256), [2, 5], 4),
    "width-later-256": (lambda: width_limit_graph("later", 256), [2], 4),
    "t1-2048": (lambda: coloured(t_limit_graph(2048), 4, "both"), [2, 5], 4),
    "lean-65": (lambda: lean_limit_graph(65), [2, 5], 4),
    "dead-column": (lambda: dead_column_graph(True), [2, 5], 4),
    **{f"indeg-{a}x{b}+1": (lambda a=a, b=b: indeg_limit_graph((a, b), 9), [2], 4) for (a, b) in RANK_MIXES},
}

# Paired later levels without a reachable cell (digest 0): with every edge of weight 1, level l is reachable from plane 2 l on, so the
# "w1" plane graphs below 13 planes cannot have one at their later pairs -- there the pin is that every cell is declared unreachable
# (source rows in the front padding).  Everywhere else a paired later level has a non-zero digest.
UNREACHABLE_PAIRED = {
    **{f"plane-{RP}-w1/{m}": [2, 4, 6] for RP in (1, 2, 3, 4) for m in COLOUR_MODES},
    **{f"plane-{RP}-w1/{m}": [4, 6] for RP in (5, 7) for m in COLOUR_MODES},
    **{f"plane-1-mixed/{m}": [4, 6] for m in COLOUR_MODES}, **{f"plane-2-mixed/{m}": [6] for m in COLOUR_MODES},
    "plane-shift-1": [6],                                       # (two planes, and nearly every edge of that graph weighs 1)
}


def budgets_checked(g):
    """the budgets a case reads out and solves the oracle for: all of 0..R -- except on the 4,097-plane graph, where R + 1 oracle
    solves of cost ~R each are minutes: there 0..16 (its paths weigh at most 12), the middle and the last two"""
    return list(range(g.R + 1)) if g.R <= 64 else list(range(17)) + [g.R // 2 - 1, g.R // 2, g.R - 1, g.R]

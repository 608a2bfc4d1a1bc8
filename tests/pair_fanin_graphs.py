"""Graphs and a plain model of the pairing rule for fan-in pairs -- level pairs whose later level has rows of composed in-degree 9..32
(dipgenie_amd/csrc/dg_dp_pairs.hip, dp_sweep_pair_coop_kernel) -- test infrastructure of tests/test_pair_fanin_graphs.py (CPU) and
tests/test_gpu_pair_fanin.py (GPU).  Built on tests/pair_graphs.py: graphs are written out edge by edge, parallel edges included, so
every in-degree, rank and composed in-degree is what the case says.

Every graph has the levels 0 {source}, 1, 2 (a light pair), 3 and 4 (THE pair of the case), 5 .. (a tail), sink."""
import numpy as np

import pair_graphs as pg

LIGHT_MAX = 8             # composed in-degree of a light row
BIG_MAX = 32              # ... of a big row
BIG_INLINE = 8            # big rows whose position rides in the kernel arguments
DEFAULT_MAX_BIG = 4        # option pair_fanin_max_big as shipped (the measured gate)


def choose_pairs(g, pair_min=1, pair_fanin=1, pair_fanin_min=1, pair_fanin_max_big=255, pair_fanin_max_indeg=BIG_MAX):
    """The library's choice restated from the arrays: [(later level, big rows)].  Greedy from the left and disjoint, both levels lean
    without a dead column, at most 255 wide with at most 2,047 in-edges; every composed in-degree at most 8 (narrow rule) or at most 32
    with the rows above 8 counted as big, at most pair_fanin_max_big of them and none above pair_fanin_max_indeg (wide rule).  The wide rule's choice is taken as a whole, and only if it holds at least
    pair_fanin_min pairs with a big row; else the narrow rule's.  Fewer than pair_min pairs: none."""
    ins = pg.in_lists(g)

    def level_ok(l):
        deg = [len(ins[v]) for v in pg.level_vertices(g, l)]
        return min(deg) >= 1 and max(deg) <= pg.MAX_INDEG_LEAN and len(deg) <= pg.MAX_WIDTH and sum(deg) <= pg.MAX_T
    comp = {l: pg.composed_in_degrees(g, l, ins) for l in range(2, g.n_levels) if level_ok(l - 1) and level_ok(l)}

    def greedy(limit):
        out, l = [], 2
        while l < g.n_levels:
            if l in comp and max(comp[l]) <= limit and (limit == LIGHT_MAX or max(comp[l]) <= LIGHT_MAX or sum(c > LIGHT_MAX for c in comp[l]) <= pair_fanin_max_big):
                out.append((l, sum(c > LIGHT_MAX for c in comp[l])))
                l += 2
            else:
                l += 1
        return out
    chosen = greedy(LIGHT_MAX)
    if pair_fanin:
        wide = greedy(min(pair_fanin_max_indeg, BIG_MAX))
        if sum(1 for (_, b) in wide if b) >= max(pair_fanin_min, 1):
            chosen = wide
    return chosen if len(chosen) >= max(pair_min, 1) else []


def pair_profile(g, rc, **rule):
    """the pair profile a run at the forced chunk size rc must show"""
    chosen = choose_pairs(g, **rule)
    out = {}
    for name, n in ((f"dp_sweep_pair_kernel<{rc}>", sum(1 for (_, b) in chosen if not b)), (f"dp_sweep_pair_coop_kernel<{rc}>", sum(1 for (_, b) in chosen if b))):
        if n:
            out[name] = n
    return out


def _spread(n, k, first=0):
    """n in-edges over k source positions from `first` on, as bundles of parallel edges: [position, ...] in rising rank order"""
    size = [n // k + (1 if q < n % k else 0) for q in range(k)]
    return sorted((first + q) % k for q in range(k) for _ in range(size[q]))


def fanin_graph(R, mid_deg, later, ks=5, seed=0, weights="mixed", tail=0, colours=True):
    """Pair (3, 4).  mid_deg[m] = in-degree of position m of level 3 (bundles over the ks positions of level 2); later[j] = the middle
    positions of the in-edges of position j of level 4 (repeats = parallel edges), so its composed in-degree is sum(mid_deg[m] for m in
    later[j]).  The edges of a bundle share their weight: weights "w0" / "w1" / "mixed" (by source position and destination) / "random" (drawn per bundle).  Levels
    1 and 2 have in-degree 1 and 2 (a light pair); `tail` levels of in-degree 1 follow level 4; the sink takes every vertex of the last."""
    rng = np.random.default_rng(9000 + seed)
    km, kl = len(mid_deg), len(later)

    wtab = rng.integers(0, 2, (64, 64))

    def w(i, j):
        return {"w0": 0, "w1": 1, "mixed": (i + j + seed) & 1, "random": int(wtab[i, j])}[weights]
    e01 = [(0, j, w(0, j)) for j in range(ks)]
    e12 = [(i, j, w(i, j)) for j in range(ks) for i in pg._pick(rng, ks, min(2, ks))]
    e23 = [(i, m, w(i, m)) for m in range(km) for i in _spread(mid_deg[m], ks, m)]
    e34 = [(m, j, w(m, j + 1)) for j in range(kl) for m in sorted(later[j])]
    widths, edges, k = [1, ks, ks, km, kl], [e01, e12, e23, e34], kl
    for _ in range(tail):
        edges.append([(j, j, w(j, 0)) for j in range(k)])
        widths.append(k)
    edges.append([(j, 0, w(j, 1)) for j in range(k)])
    widths.append(1)
    g = pg.from_edges(R, widths, edges)
    return pg.with_colours(g, (2, 3, 4), seed) if colours else g


def one_big(n, R=6, **kw):
    """one row of composed in-degree n among light rows: n = a in-edges over middle vertices of in-degree 1..3 (uneven quarters for
    9, 10, 11), or over two middle vertices of in-degree 16 (and 17) for 32 (33)"""
    if n >= 31:
        mid_deg = [16, n - 16, 1, 2]
        big = [0, 1]
    else:
        mid_deg = [1, 2, 3, 1, 2, 3]
        big, left = [], n
        while left:                                                 # greedily 3, 3, ... over parallel edges into the in-degree-3 vertices
            d = min(3, left)
            big.append({3: 2, 2: 1, 1: 0}[d] + (3 if len(big) & 1 else 0))
            left -= d
    later = [[0], big, [1, 2], [len(mid_deg) - 1] * 2]
    if n >= 31:
        later += [[2]] * 30                                         # the sink's composed in-degree goes beyond 32: level 4 pairs with level 3 or with nothing
    return fanin_graph(R, mid_deg, later, **kw)


def many_big(n_big, R=4, **kw):
    """n_big rows of composed in-degree 9..12 (1, 8, 9: the inline boundary) between light rows, 40 rows at most"""
    mid_deg = [1, 2, 3, 4]
    later = []
    for j in range(n_big):
        later += [[3, 3, j & 3] + [2] * (j % 2), [j & 3]]              # big: 4 + 4 + (1..4) [+ 3]; then a light row
    return fanin_graph(R, mid_deg, later, **kw)


def earlier_is_fanin(R=5, **kw):
    """level 3 holds a vertex of in-degree 12 (a fan-in level: cooperative when launched alone), level 4 has in-degree <= 2"""
    return fanin_graph(R, [12, 1, 2, 9], [[0], [0, 1], [2], [3, 2], [1]], **kw)


def later_is_fanin(R=5, **kw):
    """level 3 has in-degree <= 2, level 4 a vertex of in-degree 12 (ranks ru2 up to 11) and one of in-degree 9"""
    return fanin_graph(R, [1, 2, 2, 1], [[0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3], [1], [0] * 5 + [3] * 4, [2, 3]], **kw)


def both_are_fanin(R=5, **kw):
    """a vertex of in-degree 9 on level 3 (ranks ru1 up to 8) below a vertex of in-degree 10 on level 4 (ru2 up to 9): composed 9 + 9 + 8 x 1 = 26"""
    return fanin_graph(R, [9, 1, 2, 1], [[0, 0, 1, 1, 1, 1, 3, 3, 3, 3], [2], [0, 2], [1, 3]], **kw)


def shared_middle(R=3, **kw):
    """two middle vertices of in-degree 5 and 6 feed 30 rows (composed 5, 6, 10, 11, 12: many cells share a middle cell); a third middle
    vertex feeds nothing the sink's side reaches with a better value than its neighbours, and a fourth has no successor at all"""
    later = [[0], [1], [0, 0], [0, 1], [1, 1]] * 6
    return fanin_graph(R, [5, 6, 2, 3], later + [[2]], **kw)


def tie_graph(seed, R=2):
    """colourless: every candidate of a plane ties, so the walk shows the order alone; middle in-degrees 3, rows of composed 9 and 12"""
    return fanin_graph(R, [3, 3, 3, 3], [[0, 1, 2], [1, 2, 3, 0], [3, 0, 1], [2]], ks=4, seed=seed, weights="random", colours=False)


# seeds on which the level-by-level order (ru2, rv2, ru1, rv1) and the order of ranks within the composed lists walk different edges
# (tests/test_pair_fanin_graphs.py asserts it)
TIE_SEEDS = (0, 40)

PLANES = (1, 2, 3, 5, 19, 33)          # R + 1: below the plane shift of 4, ragged last chunks for the chunk sizes 2 and 4


def _cases():
    """name -> (builder, [(later level, big rows)] expected of choose_pairs under pair_min = pair_fanin_min = 1)"""
    c = {}
    for n in (9, 10, 11, 31, 32):
        c[f"one-big-{n}"] = (lambda n=n: one_big(n, seed=n), [(2, 0), (4, 3 if n >= 31 else 1)])  # (31, 32: the two halves of 16 are big rows too)
    for nb in (1, 8, 9):
        c[f"big-rows-{nb}"] = (lambda nb=nb: many_big(nb, seed=nb), [(2, 0), (4, nb)])
    c["big-rows-20-tail"] = (lambda: many_big(20, seed=20, tail=2), [(2, 0), (4, 20), (6, 0)])
    c["earlier-fanin"] = (earlier_is_fanin, [(2, 0), (4, 3)])
    c["later-fanin"] = (later_is_fanin, [(2, 0), (4, 2)])
    c["both-fanin"] = (both_are_fanin, [(2, 0), (4, 2)])
    c["shared-middle"] = (shared_middle, [(2, 0), (4, 18)])
    for s in TIE_SEEDS:
        c[f"tie-{s}"] = (lambda s=s: tie_graph(s), [(2, 0), (4, 3)])
    for RP in PLANES:
        c[f"planes-{RP}-w1"] = (lambda RP=RP: one_big(11, R=RP - 1, seed=RP, weights="w1"), [(2, 0), (4, 1)])
        c[f"planes-{RP}-mixed"] = (lambda RP=RP: many_big(3, R=RP - 1, seed=RP), [(2, 0), (4, 3)])
    return c


CASES = _cases()

# composed in-degree 33: no pair at level 4 (level 3 and level 4 run as single launches)
REFUSED = {"one-big-33": (lambda: one_big(33, seed=33), 4)}

"""Graphs and a plain model of the pairing rule for wide pairs -- level pairs in which the source, middle or later level holds 256..1,023
vertices, swept by dp_sweep_pair_wide_kernel / dp_sweep_pair_coop_wide_kernel from records with 10-bit positions
(dipgenie_amd/csrc/dg_dp_pairs.hip) -- test infrastructure of tests/test_pair_wide_graphs.py (CPU) and tests/test_gpu_pair_wide.py (GPU).

Most graphs are the small graphs of tests/pair_graphs.py and tests/pair_fanin_graphs.py made wide by widen(): dead-end vertices put IN FRONT
of a level, so that the small graph's own vertices -- the ones every path to the sink runs through -- sit at the highest positions of
the level (bits 8 and 9 set from 768 vertices of padding on) and at the highest score-delta rows.  A dead end has one in-edge and no
out-edge: it is reachable, holds values, and nothing wins through it, so in-edge ranks and the walk are those of the small graph.

Every graph has the levels 0 {source}, 1, 2 (the source level of THE pair), 3 and 4 (the pair), 5 .. (a tail), sink."""
import numpy as np

import pair_fanin_graphs as fg
import pair_graphs as pg

NARROW_WIDTH = 255        # widest level of the narrow layout (8-bit positions); its source level has 15 bits
WIDE_WIDTH = 1023         # widest level of the wide layout (10-bit positions), the source level included
WIDE_BIG_INLINE = 4       # big rows of a wide pair whose position rides in the kernel arguments
RCS = (1, 2, 4)           # chunk sizes of the four pair kernels (a wide light kernel at 8 was measured and left out: DESIGN.md s3.3)


def _width(g, l):
    return int(g.level_off[l + 1] - g.level_off[l])


def choose_pairs(g, pair_min=1, pair_fanin=1, pair_fanin_min=1, pair_fanin_max_big=fg.DEFAULT_MAX_BIG, pair_fanin_max_indeg=fg.BIG_MAX,
                 pair_wide=1, pair_wide_min=1, pair_wide_fanin=1, pair_wide_max_width=WIDE_WIDTH):
    """The library's choice restated from the arrays: [(later level, big rows, wide layout)].

    Greedy from the left and disjoint.  Both levels of a pair are lean without a dead column and have at most 2,047 in-edges; every
    composed in-degree is at most 8, or (fan-in rule) at most pair_fanin_max_indeg with at most pair_fanin_max_big rows above 8.
    Narrow rule: middle and later level at most 255 wide.  Wide rule: at most pair_wide_max_width; a pair takes the wide layout exactly
    when one of its three levels exceeds 255 -- then the source level too is at most pair_wide_max_width wide -- except that a source
    beyond pair_wide_max_width over two narrow levels keeps the narrow layout; a wide-layout pair has big rows only under pair_wide_fanin.
    Under either width rule, the choice with big rows replaces the one without as a whole if it holds at least pair_fanin_min pairs with
    a big row.  The wide rule's choice replaces the narrow rule's as a whole if it holds at least pair_wide_min pairs in the wide layout.
    Fewer than pair_min pairs: none."""
    ins = pg.in_lists(g)
    cap = min(pair_wide_max_width, WIDE_WIDTH)

    def level_ok(l):
        deg = [len(ins[v]) for v in pg.level_vertices(g, l)]
        return min(deg) >= 1 and max(deg) <= pg.MAX_INDEG_LEAN and sum(deg) <= pg.MAX_T
    comp = {l: pg.composed_in_degrees(g, l, ins) for l in range(2, g.n_levels) if level_ok(l - 1) and level_ok(l)}

    def greedy(fanin, wide):
        out, l = [], 2
        while l < g.n_levels:
            k0, k1, k2 = _width(g, l - 2), _width(g, l - 1), _width(g, l)
            wide_level = max(k1, k2) > NARROW_WIDTH
            layout = wide_level or (wide and NARROW_WIDTH < k0 <= cap)
            ok = l in comp and not (wide_level and not (wide and max(k0, k1, k2) <= cap))
            if ok:
                big = sum(c > fg.LIGHT_MAX for c in comp[l])
                ok = big == 0 or (fanin and max(comp[l]) <= min(pair_fanin_max_indeg, fg.BIG_MAX) and big <= pair_fanin_max_big and not (layout and not pair_wide_fanin))
            if ok:
                out.append((l, big, bool(layout)))
                l += 2
            else:
                l += 1
        return out

    def with_fanin(wide):
        light, with_big = greedy(False, wide), greedy(True, wide)
        return with_big if pair_fanin and sum(1 for (_, b, _) in with_big if b) >= max(pair_fanin_min, 1) else light
    chosen = with_fanin(False)
    if pair_wide:
        wider = with_fanin(True)
        if sum(1 for (_, _, w) in wider if w) >= max(pair_wide_min, 1):
            chosen = wider
    return chosen if len(chosen) >= max(pair_min, 1) else []


KERNELS = {(False, False): "dp_sweep_pair_kernel", (True, False): "dp_sweep_pair_coop_kernel",
           (False, True): "dp_sweep_pair_wide_kernel", (True, True): "dp_sweep_pair_coop_wide_kernel"}


def pair_profile(g, **rule):
    """{kernel name without its chunk size: launches} a run must show"""
    out = {}
    for (_, big, wide) in choose_pairs(g, **rule):
        name = KERNELS[(big > 0, wide)]
        out[name] = out.get(name, 0) + 1
    return out


def widen(g, pads, colour_pads=0):
    """g with pads[l] dead ends in front of level l: each takes one in-edge of weight (its position & 1) from the vertex of level l - 1 with
    the fewest in-edges (the first of them), listed last in that vertex's adjacency.  The vertices of g keep their order, in-edge ranks
    and colours.  colour_pads: every n-th dead end carries a hom colour of its own kind, so that its transitions score too."""
    L = g.n_levels
    old_w = [_width(g, l) for l in range(L)]
    pad = [int(pads.get(l, 0)) for l in range(L)]
    assert pad[0] == 0 and pad[L - 1] == 0
    ins = pg.in_lists(g)
    edges = [[] for _ in range(L - 1)]
    for l in range(L - 1):
        for i in range(old_w[l]):
            u = int(g.level_off[l]) + i
            for e in range(int(g.out_off[u]), int(g.out_off[u + 1])):
                edges[l].append((i + pad[l], int(g.out_dst[e]) - int(g.level_off[l + 1]) + pad[l + 1], int(g.out_w[e])))
    for l in range(1, L - 1):
        if pad[l]:
            deg = [len(ins[v]) for v in pg.level_vertices(g, l - 1)] if l > 1 else [0]
            # (a padded level l - 1: its dead ends have in-degree 1, the fewest there is)
            src = 0 if pad[l - 1] else pad[l - 1] + int(np.argmin(deg))
            edges[l - 1] += [(src, q, q & 1) for q in range(pad[l])]
    new_off = np.concatenate([[0], np.cumsum([old_w[l] + pad[l] for l in range(L)])])
    hom, het = {}, {}
    for l in range(L):
        for i in range(old_w[l]):
            v = int(g.level_off[l]) + i
            nv = int(new_off[l]) + pad[l] + i
            hom[nv] = g.hom_col[g.hom_off[v]:g.hom_off[v + 1]].tolist()
            het[nv] = g.het_col[g.het_off[v]:g.het_off[v + 1]].tolist()
        if colour_pads:
            for q in range(0, pad[l], colour_pads):
                hom[int(new_off[l]) + q] = [900 + (q // colour_pads) % 7]
    return pg.from_edges(g.R, [old_w[l] + pad[l] for l in range(L)], edges, hom, het)


# which levels are padded: the role of the wide level in the pair (3, 4)
ROLES = {"source": (2,), "middle": (3,), "later": (4,), "all": (2, 3, 4)}


def widened(build, role, width, colour_pads=0):
    """the small graph with the levels of `role` padded to `width` vertices"""
    g = build()
    return widen(g, {l: width - _width(g, l) for l in ROLES[role]}, colour_pads)


def custom(R, ks, km, kl, mid_in, later_in, sink_in, w=None, seed=0, colours=True):
    """Pair (3, 4) written out: mid_in(m) = the source positions (level 2, ks wide) of the in-edges of middle position m, later_in(j) = the
    middle positions of the in-edges of later position j (repeats = parallel edges), sink_in = the later positions the sink comes from.
    Level 1 has 4 vertices, level 2 in-degree 1.  w(i, j): weight of every edge from position i to position j (default: (i + j) & 1)."""
    rng = np.random.default_rng(5000 + seed)
    w = w or (lambda i, j: (i + j) & 1)
    e23 = [(i, m, w(i, m)) for m in range(km) for i in sorted(mid_in(m))]
    e34 = [(m, j, w(m, j)) for j in range(kl) for m in sorted(later_in(j))]
    e45 = [(j, 0, j & 1) for j in sink_in]
    g = pg.from_edges(R, [1, 4, ks, km, kl, 1], pg._front(ks, R, rng) + [e23, e34, e45])
    return pg.with_colours(g, (2, 3, 4), seed) if colours else g


def high_middle_graph(R=4):
    """all three levels 1,023 wide.  Later position j comes from the middle positions 1022 - (j % 200) and 1021 - (j % 200) (822..1022:
    bits 8 and 9 set), middle position m from the sources m and (m + 1) % 1023; the sink comes from the later positions 0, 511 and 1022,
    so BOTH paths of the answer run through middle positions above 767.  Composed in-degree 4 everywhere: 4,092 composed in-edges."""
    return custom(R, 1023, 1023, 1023, lambda m: (m, (m + 1) % 1023), lambda j: (1022 - j % 200, 1021 - j % 200), (0, 511, 1022), seed=1)


# the sink comes from these later positions: composed in-degree beyond 32, so that the sink pairs with nothing and level 4 keeps its digest
MANY_SINK_IN = tuple(range(0, 40, 2))


def width_refused_graph(role, R=3):
    """the middle or the later level 1,024 wide, in-degree 2 on both levels, the last position of the wide level used"""
    km, kl = {"middle": (1024, 40), "later": (7, 1024)}[role]
    return custom(R, 6, km, kl, lambda m: (m % 6, (m + 1) % 6), lambda j: ((j * 7) % km, km - 1 - (j % 5)), MANY_SINK_IN + (kl - 1,), seed=len(role))


def t_limit_graph(T1, T2, R=3, sink_in=(0, 1, 1021, 1022)):
    """middle and later level 1,023 wide with exactly T1 and T2 in-edges (2,047 = the cap: 1,022 vertices of in-degree 2 and one of 3;
    2,048: two of 3).  The vertices of in-degree 3 are the last ones, so their delta rows are the last (2,044 .. 2,046 / 2,047)."""
    def mid_in(m):
        return [m % 16, (m + 1) % 16] + ([(m + 2) % 16] if m >= 1023 - (T1 - 2046) else [])

    def later_in(j):
        # the extra in-edge comes from middle position 0 (in-degree 2), so the composed in-degree stays at most 3 * 2 + 1 = 7
        return [j, (j + 1) % 1021] + ([(j + 2) % 1021] if j >= 1023 - (T2 - 2046) else [])
    return custom(R, 16, 1023, 1023, mid_in, later_in, sink_in, seed=T1 + T2)


def full_block_graph(R=3):
    """later level 320 wide, every vertex of composed in-degree 8 (4 in-edges over middle vertices of in-degree 2): each slot block holds
    exactly 8 whole columns = 64 composed in-edges, 40 blocks, no padding slot anywhere"""
    return custom(R, 8, 300, 320, lambda m: (m % 8, (m + 3) % 8), lambda j: [(j + q * 7) % 300 for q in range(4)], (0, 100, 319), seed=2)


def column_64_graph(R=3):
    """later level 260 wide; its position 259 has 8 in-edges from middle vertices of in-degree 8: a destination column of 64 composed
    in-edges, beyond the 32 of a big row -- the level pairs with nothing"""
    return custom(R, 16, 300, 260, lambda m: [(m + q) % 16 for q in range(8 if m >= 292 else 2)], lambda j: list(range(292, 300)) if j == 259 else [j, j + 1], MANY_SINK_IN + (259,), seed=3)


def two_columns_of_32_graph(R=3):
    """later level 258 wide; positions 256 and 257 (bit 8) are big rows of composed in-degree 32 = 4 in-edges over middle vertices of
    in-degree 8: together one slot block of exactly 64 composed in-edges"""
    return custom(R, 16, 300, 258, lambda m: [(m + q) % 16 for q in range(8 if m >= 292 else 1)],
                  lambda j: list(range(292, 296)) if j == 256 else list(range(296, 300)) if j == 257 else [j], (0, 256, 257), seed=4)


def _cases():
    """name -> (builder, choose_pairs(g) under the test's options: pair_min = pair_wide_min = pair_fanin_min = 1, the shipped gates otherwise)"""
    c = {}
    N, W = False, True
    # widths: each role at 255 (narrow layout), 256, 257 and 1,023 (wide layout); pg.width_limit_graph uses the last position of the level
    for role in ("source", "middle", "later"):
        for width in (255, 256, 257, 1023):
            wide = width > 255
            first = [(2, 0, N)] if role != "source" or not wide else [(2, 0, W)]      # level 2 = the source level: the later level of the pair (1, 2)
            c[f"width-{role}-{width}"] = (lambda role=role, width=width: pg.coloured(pg.width_limit_graph(role, width), 4, "both", width), first + [(4, 0, wide)])
    # a source of 1,024 over two narrow levels keeps the narrow layout (15-bit source positions); level 2 itself pairs with nothing
    c["width-source-1024"] = (lambda: pg.coloured(pg.width_limit_graph("source", 1024), 4, "both", 1024), [(4, 0, N)])
    c["width-all-1023"] = (high_middle_graph, [(2, 0, W), (4, 0, W)])
    c["t-2047-2047"] = (lambda: t_limit_graph(2047, 2047), [(2, 0, N), (4, 0, W)])
    c["full-blocks"] = (full_block_graph, [(2, 0, N), (4, 0, W)])
    c["two-columns-of-32"] = (two_columns_of_32_graph, [(2, 0, N), (4, 2, W)])
    # the small graphs of the narrow pair tests behind 768+ dead ends: ties, shared and unused middle cells, composed in-degree 8, planes and weights
    for role, width in (("source", 300), ("middle", 1023), ("later", 1000), ("all", 800)):
        src = role in ("source", "all")
        for k, seed in pg.TIE_ORDER_SEEDS.items():
            c[f"tie-{k}/{role}"] = (lambda k=k, seed=seed, role=role, width=width: widened(lambda: pg.tie_graph(k, seed), role, width), [(2, 0, src), (4, 0, W)])
        for seed in fg.TIE_SEEDS:
            c[f"tie-big-{seed}/{role}"] = (lambda seed=seed, role=role, width=width: widened(lambda: fg.tie_graph(seed), role, width), [(2, 0, src), (4, 3, W)])
    for role, width in (("middle", 900), ("all", 1023)):
        src = role == "all"
        c[f"shared-middle/{role}"] = (lambda role=role, width=width: widened(pg.shared_middle_graph, role, width, 5), [(2, 0, src), (4, 0, W)])
        c[f"shared-middle-big/{role}"] = (lambda role=role, width=width: widened(lambda: fg.many_big(4, seed=4), role, width, 5), [(2, 0, src), (4, 4, W)])
        for mix in pg.RANK_MIXES:
            c[f"indeg-{mix[0]}x{mix[1]}/{role}"] = (lambda mix=mix, role=role, width=width: widened(lambda: pg.indeg_limit_graph(mix, 8), role, width, 3), [(2, 0, src), (4, 0, W)])
        # 8 against 9: one row of composed in-degree 9 among light rows is a big row
        c[f"one-big-9/{role}"] = (lambda role=role, width=width: widened(lambda: fg.one_big(9, seed=9), role, width, 3), [(2, 0, src), (4, 1, W)])
    c["big-rows-1/later"] = (lambda: widened(lambda: fg.many_big(1, seed=1), "later", 513, 4), [(2, 0, N), (4, 1, W)])
    for RP in PLANES:
        for weights in ("w0", "w1", "mixed"):
            role = ("source", "middle", "later", "all")[(RP + len(weights)) % 4]
            c[f"planes-{RP}-{weights}/{role}"] = (lambda RP=RP, weights=weights, role=role: widened(lambda: fg.fanin_graph(RP - 1, [1, 2, 2, 1], [[0, 1], [1, 2], [3], [2, 3, 0]], seed=RP, weights=weights), role, 770 + RP, 6),
                                                  [(2, 0, role in ("source", "all")), (4, 0, W)])
    return c


PLANES = (3, 4, 5, 7, 8)               # R + 1: plane shifts r2 - 4 < 0 on every graph, ragged last chunks for the chunk sizes 2 and 4

CASES = _cases()

# name -> (builder, choose_pairs(g)): level 4 is the later level of no pair.  Where the sink (level 5) pairs with nothing either, levels 3 and 4
# both run as single launches and show the oracle's digests; big-rows-5 follows the shipped gate of 4 big rows, and its sink pairs with level 4.
REFUSED = {
    "width-middle-1024": (lambda: width_refused_graph("middle"), [(2, 0, False)]),
    "width-later-1024": (lambda: width_refused_graph("later"), [(2, 0, False)]),
    "t1-2048": (lambda: t_limit_graph(2048, 2047, sink_in=MANY_SINK_IN), [(2, 0, False)]),
    "t2-2048": (lambda: t_limit_graph(2047, 2048, sink_in=MANY_SINK_IN), [(2, 0, False)]),
    "column-64": (column_64_graph, [(2, 0, False)]),
    "big-rows-5": (lambda: widened(lambda: fg.many_big(5, seed=5), "later", 600), [(2, 0, False), (5, 1, True)]),
}

"""Random levelized DP graphs (dg_dp_graph layout) for kernel parity tests -- test infrastructure."""
import numpy as np

from dipgenie_amd.capi import DpGraphArrays


def random_levelized(seed, n_levels=12, max_width=9, R=3, p_w1=0.3, p_colour=0.4, n_colours=12, max_list=4,
                     extra_edges=1.5, dup_edges=True, min_width=1, widths=None):
    """Level 0 = {source}, last level = {sink}. Every vertex gets >=1 out-edge (except sink) and edges only
    go to the next level. Parallel edges carry equal weights (the product's documented precondition).
    widths=[1, ..., 1] prescribes every level's width (n_levels, min_width and max_width are then unused) in place of the random
    draw; without it every seeded call gives the arrays it always gave (tests/test_sweep_variant_graphs.py pins four of them by sha256;
    tests/test_colour_graphs.py pins recolour() in the same way)."""
    rng = np.random.default_rng(seed)
    if widths is None:
        widths = [1] + [int(rng.integers(min_width, max_width + 1)) for _ in range(n_levels - 2)] + [1]
    else:
        widths = [int(w) for w in widths]
        n_levels = len(widths)
        assert n_levels >= 2 and widths[0] == 1 and widths[-1] == 1 and min(widths) >= 1, widths
    level_off = np.zeros(n_levels + 1, np.int32)
    level_off[1:] = np.cumsum(widths)
    nV = int(level_off[-1])
    out = [[] for _ in range(nV)]
    for l in range(n_levels - 1):
        a0, k, b0, k2 = level_off[l], widths[l], level_off[l + 1], widths[l + 1]
        wmap = {}
        for i in range(k):
            n_e = 1 + int(rng.poisson(extra_edges))
            for _ in range(n_e):
                j = int(rng.integers(0, k2))
                w = wmap.setdefault((i, j), int(rng.random() < p_w1))
                out[a0 + i].append((b0 + j, w))
                if dup_edges and rng.random() < 0.1:
                    out[a0 + i].append((b0 + j, w))
        # make sure every next-level vertex is reachable from someone, most of the time
        for j in range(k2):
            if rng.random() < 0.9 and not any(d == b0 + j for i in range(k) for (d, _) in out[a0 + i]):
                i = int(rng.integers(0, k))
                w = wmap.setdefault((i, j), int(rng.random() < p_w1))
                out[a0 + i].append((b0 + j, w))
    out_off = np.zeros(nV + 1, np.int64)
    out_off[1:] = np.cumsum([len(o) for o in out])
    out_dst = np.array([d for o in out for (d, _) in o], np.int32)
    out_w = np.array([w for o in out for (_, w) in o], np.uint8)
    hom, het = [], []
    for v in range(nV):
        def lst():
            if rng.random() < p_colour:
                n = int(rng.integers(1, max_list + 1))
                return sorted(set(int(x) for x in rng.integers(0, n_colours, n)))
            return []
        a, b = lst(), lst()
        b = [c + n_colours for c in b]   # HOM and HET colour ids are disjoint in the product
        hom.append(a)
        het.append(b)
    hom_off = np.zeros(nV + 1, np.int64)
    het_off = np.zeros(nV + 1, np.int64)
    hom_off[1:] = np.cumsum([len(x) for x in hom])
    het_off[1:] = np.cumsum([len(x) for x in het])
    return DpGraphArrays(R, level_off=level_off, out_off=out_off, out_dst=out_dst, out_w=out_w,
                         hom_off=hom_off, hom_col=np.array([c for x in hom for c in x], np.int32),
                         het_off=het_off, het_col=np.array([c for x in het for c in x], np.int32))


def random_topological(seed, n=60, R=4, avg_deg=2.0, p_w1=0.4, p_zero_colour=0.5, max_colours=4, span=8, dup=0.15):
    """A DAG whose vertex ids are a topological order (every edge u -> v has u < v), as ExpandedGraph::topologically_reorder
    leaves it for the haploid DP: edges reach up to `span` ids ahead (several depth levels), parallel edges may carry
    DIFFERENT weights (the scatter loop's arrival order then matters), many vertices carry no colour (ties at value 0).
    Returns (out_off, out_dst, out_w, n_colours)."""
    rng = np.random.default_rng(seed)
    out = [[] for _ in range(n)]
    for u in range(n - 1):
        for _ in range(1 + int(rng.poisson(avg_deg - 1))):
            v = int(min(n - 1, u + 1 + rng.integers(0, span)))
            w = int(rng.random() < p_w1)
            out[u].append((v, w))
            if rng.random() < dup:
                out[u].append((v, int(rng.random() < 0.5)))      # parallel edge, independent weight
    out_off = np.zeros(n + 1, np.int64)
    out_off[1:] = np.cumsum([len(o) for o in out])
    out_dst = np.array([v for o in out for (v, _) in o], np.int32)
    out_w = np.array([w for o in out for (_, w) in o], np.uint8)
    ncol = np.where(rng.random(n) < p_zero_colour, 0, rng.integers(1, max_colours + 1, n)).astype(np.int32)
    return out_off, out_dst, out_w, ncol


# ---------------------------------------------------------------------------------------------- colour lists for a given topology
def _with_colours(g, hom, het, R=None):
    """a copy of g whose vertex v carries the sorted-unique id arrays hom[v] and het[v]"""
    arrs = {n: getattr(g, n).copy() for n in DpGraphArrays.NAMES}
    for kind, lists in (("hom", hom), ("het", het)):
        off = np.zeros(g.n_vertices + 1, np.int64)
        off[1:] = np.cumsum([len(x) for x in lists])
        arrs[kind + "_off"] = off
        arrs[kind + "_col"] = np.concatenate(lists).astype(np.int32) if off[-1] else np.zeros(0, np.int32)
    return DpGraphArrays(g.R if R is None else R, **arrs)


def spread_ids(pool):
    """an id map for recolour(): the 2 * pool raw ids spread evenly over the whole non-negative int32 range, 0 and 2^31 - 1 included"""
    return np.round(np.linspace(0, 2 ** 31 - 1, 2 * pool)).astype(np.int64)


def recolour(g, seed, p_empty=0.7, p_short=0.2, long_range=(200, 2000), pool=4000, hom_only=False, het_only=False, id_map=None,
             hom_high=False, shared=False, R=None):
    """A copy of g (same topology, R unless given) with new colour lists.  Every list is empty with probability p_empty, short
    (1..4 ids) with p_short and otherwise long (long_range, inclusive); its ids are drawn without repetition from a pool of `pool`
    raw ids per kind, so that lists of neighbouring levels share ids.  Hom lists take the raw ids 0..pool-1 and het lists
    pool..2*pool-1 (hom_high: the other way round), so the two kinds stay disjoint; id_map, a strictly increasing array of 2 * pool
    non-negative int32 values, then replaces raw id i by id_map[i] (spread_ids).  hom_only / het_only leave the other kind empty.
    shared: every non-empty list of a kind is the same list (the first one drawn).  Lists come out sorted-unique."""
    rng = np.random.default_rng(seed)
    assert not (hom_only and het_only) and 4 <= long_range[0] <= long_range[1] and (long_range[1] <= pool or p_empty + p_short >= 1) and pool >= 4
    if id_map is None:
        id_map = np.arange(2 * pool)
    id_map = np.asarray(id_map, np.int64)
    assert id_map.shape == (2 * pool,) and id_map[0] >= 0 and id_map[-1] <= 2 ** 31 - 1 and (np.diff(id_map) > 0).all()

    def lists(on, base):
        out, first = [], None
        for _ in range(g.n_vertices):
            x = rng.random()
            if not on or x < p_empty:
                out.append(np.zeros(0, np.int64))
                continue
            n = int(rng.integers(1, 5)) if x < p_empty + p_short else int(rng.integers(long_range[0], long_range[1] + 1))
            ids = id_map[base + np.sort(rng.choice(pool, n, replace=False))]
            if shared:
                first = ids if first is None else first
                ids = first
            out.append(ids)
        return out
    hom = lists(not het_only, pool if hom_high else 0)
    het = lists(not hom_only, 0 if hom_high else pool)
    return _with_colours(g, hom, het, R)


def recolour_disjoint_big(g, seed, per_level=2, lengths=(9000, 10000), R=None):
    """A copy of g in which up to per_level vertices of every inner level carry a het list of lengths[0]..lengths[1] ids, all of
    them pairwise disjoint (consecutive blocks of ids), and nothing else carries a colour.  From the second inner level on the
    vertices are out-neighbours of the previous level's, different ones where the edges allow it, so that transitions exist
    whose four vertices all carry a list."""
    rng = np.random.default_rng(seed)
    het = [np.zeros(0, np.int64) for _ in range(g.n_vertices)]
    prev, next_id = [], 0
    for l in range(1, g.n_levels - 1):
        b0, b1 = int(g.level_off[l]), int(g.level_off[l + 1])
        want = min(per_level, b1 - b0)
        chosen = []
        for u in prev:
            cand = [int(v) for v in g.out_dst[g.out_off[u]:g.out_off[u + 1]] if int(v) not in chosen]
            if cand and len(chosen) < want:
                chosen.append(cand[int(rng.integers(0, len(cand)))])
        rest = [v for v in rng.permutation(np.arange(b0, b1)).tolist() if v not in chosen]
        chosen += rest[:want - len(chosen)]
        for v in chosen:
            n = int(rng.integers(lengths[0], lengths[1] + 1))
            het[v] = np.arange(next_id, next_id + n)
            next_id += n
        prev = chosen
    return _with_colours(g, [np.zeros(0, np.int64)] * g.n_vertices, het, R)


def delta_bound_graph(M, hom=True, het=True, only=None):
    """Six vertices on the levels {0}, {1, 2}, {3, 4}, {5}; edges 0->1, 0->2, 1->3, 2->4, 3->5, 4->5, all of weight 0; R = 1.  With
    a = arange(M): Hom(1) = Hom(4) = a, Hom(2) = Hom(3) = a + M, and Het(1..4) are four disjoint blocks of M ids above every hom id.
    The transition (1 -> 3, 2 -> 4) then scores 2 M + 4 M = 6 M, the largest score delta that lists of M ids can give; the optimum is
    10 M with s_het 8 M (2 M / 0 with hom alone, 8 M / 8 M with het alone).  only: the vertices that keep their lists."""
    a = np.arange(M, dtype=np.int64)
    none = np.zeros(0, np.int64)
    keep = (lambda v: True) if only is None else (lambda v: v in only)
    homl = [a + M * {1: 0, 4: 0, 2: 1, 3: 1}[v] if hom and v in (1, 2, 3, 4) and keep(v) else none for v in range(6)]
    hetl = [a + M * (1 + v) if het and v in (1, 2, 3, 4) and keep(v) else none for v in range(6)]
    g = DpGraphArrays(1, level_off=np.array([0, 1, 3, 5, 6], np.int32), out_off=np.array([0, 2, 3, 4, 5, 6, 6], np.int64),
                      out_dst=np.array([1, 2, 3, 4, 5, 5], np.int32), out_w=np.zeros(6, np.uint8),
                      hom_off=np.zeros(7, np.int64), hom_col=np.zeros(0, np.int32), het_off=np.zeros(7, np.int64), het_col=np.zeros(0, np.int32))
    return _with_colours(g, homl, hetl)


def transition_deltas(g, l):
    """Every score delta of the transition l - 1 -> l at once: (delta, symd, coloured) with delta[e, f] = inter + symd and symd[e, f]
    for the out-edges e, f of level l - 1 (in out-edge order, parallel edges included) and coloured[e] = "an end of e carries a
    colour".  Counted with indicator matrices over the ids present (x = the complement of an indicator row):
      |(A_e u A_f) n (B_e u B_f)| = n - xA_e.xA_f - xB_e.xB_f + (xA_e xB_e).(xA_f xB_f)
      |(C_e u C_f) /\\ (D_e u D_f)| = xC_e.xC_f + xD_e.xD_f - 2 (xC_e xD_e).(xC_f xD_f)
    (float32 products of 0 / 1 entries: exact below 2^24 ids).  tests/test_colour_graphs.py checks entries against the oracle's set
    functions."""
    a0, a1, b1 = int(g.level_off[l - 1]), int(g.level_off[l]), int(g.level_off[l + 1])
    src = np.repeat(np.arange(a0, a1), np.diff(g.out_off[a0:a1 + 1])) - a0
    dst = g.out_dst[g.out_off[a0]:g.out_off[a1]].astype(np.int64) - a0

    def complement(off, col):
        ids = np.unique(col[off[a0]:off[b1]])
        x = np.ones((b1 - a0, ids.size), np.float32)
        for v in range(a0, b1):
            x[v - a0, np.searchsorted(ids, col[off[v]:off[v + 1]])] = 0
        return x, ids.size
    xh, n_hom = complement(g.hom_off, g.hom_col)
    xa, xb = xh[src], xh[dst]
    inter = n_hom - xa @ xa.T - xb @ xb.T + (xa * xb) @ (xa * xb).T
    xt, _ = complement(g.het_off, g.het_col)
    xc, xd = xt[src], xt[dst]
    symd = xc @ xc.T + xd @ xd.T - 2 * ((xc * xd) @ (xc * xd).T)
    has = (np.diff(g.hom_off) + np.diff(g.het_off))[a0:b1] > 0
    inter, symd = np.rint(inter).astype(np.int64), np.rint(symd).astype(np.int64)
    return inter + symd, symd, has[src] | has[dst]

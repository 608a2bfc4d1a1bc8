"""Padded graphs: a small graph the numpy models handle, widened with vertices that no path from the source reaches -- TEST
INFRASTRUCTURE, CPU only, for the joint-pass kernels of dg_dp_joint.hip beyond their grid caps.

pad(g, front, back, ...) puts front[l] pad vertices before and back[l] behind the vertices of level l.  A pad has in-edges from pads of
the level before only (pads of level 1 have none), carries a hom and a het list, and may send one edge into a real vertex of the next
level.  Then, in the padded graph G':

  * every cell that holds a pad has F = NEG_INF (nothing reaches it), so its through-value is NEG_INF: it is no alternative, no table
    entry, no cis or trans cell;
  * every real cell has exactly the value it has in G: its in-edge pairs from pads meet a NEG_INF source cell and are skipped, and a real
    vertex has no edge into a pad;
  * the map from old to new ids is monotone inside a level, so every tie-break (value descending, i ascending, j ascending) carries over.

So the device on G' must equal the model on G with the ids remapped (remap_*), field for field, and NEG_INF / absent on every pad.
tests/test_padded_graphs.py checks that claim with the models themselves at small pad counts, and that each of the four full-size shapes
(rows, edges, lanes, deep) still crosses the cap it is named for."""
import numpy as np

import graphgen
from dipgenie_amd.capi import DpGraphArrays
from paths_model import NEG_INF

# the caps of the joint pass, restated once (the kernels stride beyond each of them)
THREADS = 256                                           # dg_dp_joint.hip:57   JT_THREADS
ROW_BLOCKS = 2048                                       # dg_dp_joint.hip:61   JT_ROW_BLOCKS: workgroups of jt_combine_kernel, rows strided
X_BLOCKS = 4096                                         # dg_dp_joint.hip:62   JT_X_BLOCKS: workgroups per row of the recurrences and the seeds
MASK_X_BLOCKS = 4096                                    # dg_dp_pins.hip:104   pins_launch_joint_mask: workgroups per row of jt_pin_mask_kernel
SCORE_Y_BLOCKS = 16384                                  # dg_dp_joint.hip:865  the launch of jt_scores_kernel: rows eu of the matrix, strided
SCORE_X_BLOCKS = 64                                     # dg_dp_joint.hip:865  ... and workgroups along ev
SCAN_CHUNK = 1024                                       # dg_dp_joint.hip:144  jt_out_scan_kernel: vertices per pass of its one workgroup
LANES_PER_ROW = X_BLOCKS * THREADS                      # 2^20 lanes of one row before a lane takes a second (j, r)


def pad(g, front, back, *, pad_indeg, into_real, seed, p_w1=0.3, n_colours=12, max_list=2):
    """-> (g_padded, new_id).  front[l] / back[l]: pads before / behind level l's own vertices (0 on the first and the last level);
    pad_indeg[l] (a list per level or a dict, 0 where absent): in-edges of every pad of level l >= 2, from uniformly drawn pads of level
    l - 1 where that level has any (so parallel edges occur; they share a weight); into_real: the share of the pads that send one edge
    into a uniformly drawn real vertex of the next level; every pad gets a hom and a het list of 1..max_list ids, hom ids below
    n_colours and het ids from n_colours on, as graphgen.random_levelized has them.  new_id: int64 [g.n_vertices], old id -> new id."""
    rng = np.random.default_rng(seed)
    L = g.n_levels
    front, back = [int(x) for x in front], [int(x) for x in back]
    assert len(front) == len(back) == L and front[0] == back[0] == front[-1] == back[-1] == 0 and min(front + back) >= 0
    indeg = [int(pad_indeg.get(l, 0)) if isinstance(pad_indeg, dict) else int(pad_indeg[l]) for l in range(L)]
    old_off = np.asarray(g.level_off, np.int64)
    widths = np.diff(old_off)
    new_off = np.zeros(L + 1, np.int64)
    new_off[1:] = np.cumsum(widths + np.array(front) + np.array(back))
    nV = int(new_off[-1])
    level_of = np.repeat(np.arange(L), widths)
    new_id = new_off[level_of] + np.array(front)[level_of] + (np.arange(g.n_vertices) - old_off[level_of])
    is_pad = np.ones(nV, bool)
    is_pad[new_id] = False
    pads = [np.flatnonzero(is_pad[new_off[l]:new_off[l + 1]]) + new_off[l] for l in range(L)]
    out = [[] for _ in range(nV)]
    for v in range(g.n_vertices):                        # the real vertices keep their out-edges, in their order
        e0, e1 = int(g.out_off[v]), int(g.out_off[v + 1])
        out[int(new_id[v])] = [(int(new_id[d]), int(w)) for d, w in zip(g.out_dst[e0:e1], g.out_w[e0:e1])]
    wmap = {}
    for l in range(2, L):
        if indeg[l] and len(pads[l - 1]) and len(pads[l]):
            src = rng.choice(pads[l - 1], (len(pads[l]), indeg[l]))
            for p, row in zip(pads[l].tolist(), src.tolist()):
                for u in row:
                    out[u].append((p, wmap.setdefault((u, p), int(rng.random() < p_w1))))
    for l in range(1, L - 1):
        real = new_id[old_off[l + 1]:old_off[l + 2]]
        for p in pads[l][rng.random(len(pads[l])) < into_real].tolist():
            d = int(rng.choice(real))
            out[p].append((d, wmap.setdefault((p, d), int(rng.random() < p_w1))))
    out_off = np.zeros(nV + 1, np.int64)
    out_off[1:] = np.cumsum([len(o) for o in out])
    hom = [np.zeros(0, np.int64)] * nV
    het = [np.zeros(0, np.int64)] * nV
    for v in range(g.n_vertices):
        hom[int(new_id[v])] = np.asarray(g.hom_col[g.hom_off[v]:g.hom_off[v + 1]], np.int64)
        het[int(new_id[v])] = np.asarray(g.het_col[g.het_off[v]:g.het_off[v + 1]], np.int64)
    for p in np.flatnonzero(is_pad).tolist():
        hom[p] = np.unique(rng.integers(0, n_colours, int(rng.integers(1, max_list + 1))))
        het[p] = np.unique(rng.integers(0, n_colours, int(rng.integers(1, max_list + 1)))) + n_colours
    hom_off, het_off = np.zeros(nV + 1, np.int64), np.zeros(nV + 1, np.int64)
    hom_off[1:] = np.cumsum([len(x) for x in hom])
    het_off[1:] = np.cumsum([len(x) for x in het])
    gp = DpGraphArrays(g.R, level_off=new_off.astype(np.int32), out_off=out_off, out_dst=np.array([d for o in out for d, _ in o], np.int32),
                       out_w=np.array([w for o in out for _, w in o], np.uint8), hom_off=hom_off, hom_col=np.concatenate(hom).astype(np.int32),
                       het_off=het_off, het_col=np.concatenate(het).astype(np.int32))
    return gp, new_id


# ---------------------------------------------------------------------------------------------- from G to G'
def pad_mask(gp, new_id):
    """bool [gp.n_vertices]: True on the pads"""
    m = np.ones(gp.n_vertices, bool)
    m[new_id] = False
    return m


def _ids(a, new_id):
    """vertex ids through the map; -1 (no vertex, any vertex) stays"""
    a = np.asarray(a, np.int64)
    return np.where(a < 0, a, new_id[np.maximum(a, 0)])


def remap_called(called, new_id):
    return np.ascontiguousarray(_ids(called, new_id), np.int32)


def remap_pins(pins, new_id):
    """(level, vertex1, vertex2, kind) rows; -1 = any vertex"""
    return [(int(l), int(_ids(v1, new_id)), int(_ids(v2, new_id)), int(kind)) for l, v1, v2, kind in pins]


def pad_classes(g, gp, new_id, vertex_class, seed):
    """a class array of G extended over the pads: every pad draws from the classes of its level's real vertices and one class that no
    vertex of G has, so some pad rows carry the called classes and some a class of their own"""
    rng = np.random.default_rng(seed)
    cls = np.asarray(vertex_class, np.int32)
    out = np.zeros(gp.n_vertices, np.int32)
    out[new_id] = cls
    novel = int(cls.max()) + 1
    pads = pad_mask(gp, new_id)
    for l in range(g.n_levels):
        at = np.flatnonzero(pads[gp.level_off[l]:gp.level_off[l + 1]]) + int(gp.level_off[l])
        pool = np.array(sorted(set(cls[g.level_off[l]:g.level_off[l + 1]].tolist())) + [novel], np.int32)
        out[at] = rng.choice(pool, len(at))
    return out


def remap_records(rec, new_id):
    """genotype margin rows [..., 6]: vertex1, vertex2, value, alt_vertex1, alt_vertex2, alt_value"""
    out = np.array(rec, np.int64)
    for f in (0, 1, 3, 4):
        out[..., f] = _ids(out[..., f], new_id)
    return out


def remap_vertex_values(J, gp, new_id):
    """J of G -> J of G': NEG_INF on every pad"""
    out = np.full(gp.n_vertices, NEG_INF, np.int32)
    out[new_id] = J
    return out


def remap_table(off, rows, new_id, own_classes):
    """genotype table rows [n, 5]: class1, class2, vertex1, vertex2, value.  own_classes (vertex_class = None): a class is its vertex's
    id, so it moves with it.  The levels' offsets stay: a pad adds no entry, and the map is monotone inside a level"""
    out = np.array(rows, np.int64).reshape(-1, 5)
    for f in (0, 1, 2, 3) if own_classes else (2, 3):
        out[:, f] = _ids(out[:, f], new_id)
    return np.asarray(off, np.int64), out


def remap_phase(rec, new_id):
    """phase margin rows [n, 8]: level_a, level_b, cis_value, cis_vertex1, cis_vertex2, trans_value, trans_vertex1, trans_vertex2"""
    out = np.array(rec, np.int64).reshape(-1, 8)
    for f in (3, 4, 6, 7):
        out[:, f] = _ids(out[:, f], new_id)
    return out


def embed_through_values(T, g, gp, new_id):
    """per level the through-values of G inside a NEG_INF matrix of G's padded level"""
    out = []
    for l in range(g.n_levels):
        k = int(gp.level_off[l + 1] - gp.level_off[l])
        pos = new_id[g.level_off[l]:g.level_off[l + 1]] - int(gp.level_off[l])
        t = np.full((k, k), NEG_INF, np.int64)
        t[np.ix_(pos, pos)] = np.asarray(T[l], np.int64)
        out.append(t)
    return out


def het_pair(m, cls, levels, seed):
    """a sampled pair of paths whose classes differ on the given levels: drawn from a fixed seed until they do"""
    rng = np.random.default_rng(seed)
    ids = np.arange(m.nV) if cls is None else cls
    for _ in range(10000):
        called, _ = m.sample_paths(rng, 2, p_w0=0.9)
        if all(ids[called[0, l]] != ids[called[1, l]] for l in levels):
            return called
    raise AssertionError("no pair of paths is het on the levels")


# ---------------------------------------------------------------------------------------------- a shape read off the arrays
def widest_level(g):
    return int(np.diff(g.level_off).max())


def vertex_count(g):
    return int(g.level_off[-1])


def in_edge_ranks(g):
    """-> (level, rank) int64 [n_edges] in out-edge order: the level an edge enters and its index among that level's in-edges, which are
    ordered by destination, then by source position, then by their order in the source's adjacency list"""
    src = np.repeat(np.arange(g.n_vertices), np.diff(g.out_off))
    dst = np.asarray(g.out_dst, np.int64)
    order = np.lexsort((np.arange(len(dst)), src, dst))
    level_of = np.repeat(np.arange(g.n_levels), np.diff(g.level_off))
    lvl = level_of[dst]
    first = np.zeros(g.n_levels + 1, np.int64)           # in-edges before level l
    np.cumsum(np.bincount(lvl, minlength=g.n_levels), out=first[1:])
    rank = np.zeros(len(dst), np.int64)
    rank[order] = np.arange(len(dst))
    return lvl, rank - first[lvl]


def real_in_edge_ranks(gp, new_id, level):
    """the ranks of the in-edges of `level` that join two real vertices"""
    pads = pad_mask(gp, new_id)
    src = np.repeat(np.arange(gp.n_vertices), np.diff(gp.out_off))
    lvl, rank = in_edge_ranks(gp)
    return np.sort(rank[(lvl == level) & ~pads[src] & ~pads[gp.out_dst]])


def in_edge_count(g, level):
    lvl, _ = in_edge_ranks(g)
    return int((lvl == level).sum())


def min_recombinations(g):
    """the fewest recombinations of any source -> sink path (a large number if there is none)"""
    best = np.full(g.n_vertices, 1 << 30, np.int64)
    best[0] = 0
    for v in range(g.n_vertices):
        for e in range(int(g.out_off[v]), int(g.out_off[v + 1])):
            d = int(g.out_dst[e])
            best[d] = min(best[d], best[v] + int(g.out_w[e]))
    return int(best[-1])


# ---------------------------------------------------------------------------------------------- the four shapes
ROWS_BASE = dict(widths=[1, 3, 64, 65, 2, 1], R=3, p_w1=0.3, dup_edges=True, extra_edges=1.2, p_colour=0.5)
LANES_BASE = dict(widths=[1, 3, 10, 3, 1], R=3, p_w1=0.3, dup_edges=True, extra_edges=1.2, p_colour=0.5)
LANES_BUDGET = MAX_BUDGET = 4095                        # JT_MAX_PLANES - 1
DEEP_BUDGET = 4
EDGES_LEVEL = 3                                         # the transition of the edges shape that outgrows SCORE_Y_BLOCKS


def rows(small=False):
    """-> (g, g_padded, new_id).  Level 2: 2,020 pads in front and 70 behind, so its 64 real rows 2,020..2,083 lie on both sides of
    ROW_BLOCKS and the workgroups 0..105 of jt_combine_kernel serve a pad row first and a real row (2,048..2,083) second; level 3: 30 in
    front and 2,100 behind, real rows first and pad rows second in the same workgroups.  Pad in-degree 2 keeps the transition into level 3
    near 5,000 in-edges.  small: tens of pads, for the models"""
    g = graphgen.random_levelized(9130, **ROWS_BASE)
    front, back = ([0, 0, 20, 3, 0, 0], [0, 0, 7, 21, 0, 0]) if small else ([0, 0, 2020, 30, 0, 0], [0, 0, 70, 2100, 0, 0])
    gp, new_id = pad(g, front, back, pad_indeg={3: 2}, into_real=0.2, seed=1)
    return g, gp, new_id


def edges(small=False):
    """-> (g, g_padded, new_id).  The base of rows(); level 3 gets 510 pads of in-degree 32 in front -- 16,320 in-edges, so the in-edges of
    its real vertices start 64 below SCORE_Y_BLOCKS and end above it -- and 17 behind, about 17,000 in-edges in all (more than
    SCORE_X_BLOCKS * THREADS = 16,384 along ev too); level 2 gets the 45 pads they come from"""
    g = graphgen.random_levelized(9130, **ROWS_BASE)
    front, back, deg = ([0, 0, 5, 12, 0, 0], [0, 0, 2, 3, 0, 0], 4) if small else ([0, 0, 40, 510, 0, 0], [0, 0, 5, 17, 0, 0], 32)
    gp, new_id = pad(g, front, back, pad_indeg={EDGES_LEVEL: deg}, into_real=0.2, seed=2)
    return g, gp, new_id


def lanes(small=False):
    """-> (g, g_padded, new_id).  Level 2: 250 pads in front and 40 behind, k = 300; at budget 4,095 a row has 300 * 4,096 lanes, more
    than LANES_PER_ROW = 2^20, and the real columns 250..259 lie on both sides of column 256, where j * 4,096 passes it"""
    g = graphgen.random_levelized(9140, **LANES_BASE)
    front, back = ([0, 0, 12, 0, 0], [0, 0, 5, 0, 0]) if small else ([0, 0, 250, 0, 0], [0, 0, 40, 0, 0])
    gp, new_id = pad(g, front, back, pad_indeg={}, into_real=0.3, seed=3)
    return g, gp, new_id


def deep(small=False):
    """-> (g, g, identity).  No pads: 1,200 levels at most 3 wide, about 2,400 vertices, so the scan of jt_out_scan_kernel carries twice
    and every chunk of SCAN_CHUNK vertices holds real edges.  p_w1 = 0.01: a pair of paths fits DEEP_BUDGET (tests/test_padded_graphs.py)"""
    g = graphgen.random_levelized(9150, n_levels=120 if small else 1200, max_width=3, R=4, p_w1=0.01, extra_edges=1.0, p_colour=0.5)
    return g, g, np.arange(g.n_vertices, dtype=np.int64)


SHAPES = dict(rows=rows, edges=edges, lanes=lanes, deep=deep)

"""The genotype table on a levelized DP graph: per level and genotype the best pair of paths through any cell of that genotype --
plain Python and numpy, TEST INFRASTRUCTURE, on top of the through-values T of genotype_margins_model.

Written from the definition, not from any implementation of it.  The genotype of a cell (i, j) is (min(cls i, cls j), max(cls i, cls j)),
classes compared as signed integers; vertex_class = None: every vertex is its own class, its id.  For level l and genotype g

    G_l[g] = max T_l[i][j] over the reachable cells (T != NEG_INF) of genotype g

and the representative cell is the one attaining it with i <= j, among equals the smallest i, then the smallest j (T is symmetric, so
the cells with i <= j are all of them).  A genotype without a reachable cell is not listed; a level lists its genotypes in ascending
(class1, class2).  A row is (class1, class2, vertex1, vertex2, value).

genotype_table is the definition in plain Python; genotype_table_np does the same with numpy over the cells of a level (for the wider
GPU cases) and is pinned to it by tests/test_genotype_table_model.py.  record_from_table / vertex_maxima_from_table read a margin
record and the joint marginals off a table, by the rules the table's definition implies."""
import numpy as np

from paths_model import NEG_INF

FIELDS = ("class1", "class2", "vertex1", "vertex2", "value")


def _cls(vertex_class, v):
    return v if vertex_class is None else int(vertex_class[v])


def genotype_table(m, T, vertex_class=None):
    """-> per level the list of rows (class1, class2, vertex1, vertex2, value), ascending (class1, class2)"""
    out = []
    for l in range(m.L):
        a0, k = int(m.level_off[l]), int(m.level_off[l + 1] - m.level_off[l])
        best = {}
        for i in range(k):                               # ascending (i, j): a strict > keeps the first among equals
            for j in range(i, k):
                t = int(T[l][i][j])
                if t == NEG_INF:
                    continue
                ci, cj = _cls(vertex_class, a0 + i), _cls(vertex_class, a0 + j)
                g = (min(ci, cj), max(ci, cj))
                if g not in best or t > best[g][2]:
                    best[g] = (a0 + i, a0 + j, t)
        out.append([g + best[g] for g in sorted(best)])
    return out


def genotype_table_np(m, T, vertex_class=None):
    """-> (level_off int64 [L + 1], rows int64 [n, 5]); numpy over the cells of a level"""
    ids = np.arange(m.nV, dtype=np.int64) if vertex_class is None else np.asarray(vertex_class, np.int64)
    rows, off = [], [0]
    for l in range(m.L):
        a0, k = int(m.level_off[l]), int(m.level_off[l + 1] - m.level_off[l])
        Tl = np.asarray(T[l], np.int64)
        i, j = np.nonzero(np.triu(np.ones((k, k), bool)) & (Tl != NEG_INF))
        ci, cj = ids[a0 + i], ids[a0 + j]
        lo, hi, t = np.minimum(ci, cj), np.maximum(ci, cj), Tl[i, j]
        order = np.lexsort((j, i, -t, hi, lo))           # by genotype, then value descending, then i, then j
        lo, hi, t, i, j = lo[order], hi[order], t[order], i[order], j[order]
        first = np.ones(len(order), bool)
        first[1:] = (lo[1:] != lo[:-1]) | (hi[1:] != hi[:-1])
        rows.append(np.stack([lo[first], hi[first], a0 + i[first], a0 + j[first], t[first]], axis=1).reshape(-1, 5))
        off.append(off[-1] + int(first.sum()))
    return np.array(off, np.int64), np.concatenate(rows).astype(np.int64).reshape(-1, 5)


def record_from_table(rows, c1, c2, vertex_class=None):
    """rows: one level's table rows; (c1, c2): the called cell.  -> (value or None, alt_vertex1, alt_vertex2, alt_value): value is the
    entry of the called genotype if the called cell is its representative (None otherwise: the table does not hold the cell's own
    value then); the alternative is the entry with the largest value among the other genotypes, ties to the smallest vertex1, then
    the smallest vertex2; (-1, -1, NEG_INF) if there is none"""
    g1, g2 = sorted((_cls(vertex_class, int(c1)), _cls(vertex_class, int(c2))))
    value, alt = None, (-1, -1, NEG_INF)
    for r1, r2, v1, v2, t in (tuple(int(x) for x in r) for r in rows):
        if (r1, r2) == (g1, g2):
            if (v1, v2) == (min(c1, c2), max(c1, c2)):
                value = t
        elif alt[0] < 0 or (-t, v1, v2) < (-alt[2], alt[0], alt[1]):
            alt = (v1, v2, t)
    return (value,) + alt


def vertex_maxima_from_table(m, off, rows, vertex_class=None):
    """per vertex the largest value among the entries of its level whose genotype contains its class (NEG_INF if none): an upper bound
    of J[v], J[v] itself with vertex_class = None"""
    out = np.full(m.nV, NEG_INF, np.int64)
    for l in range(m.L):
        for v in range(int(m.level_off[l]), int(m.level_off[l + 1])):
            c = _cls(vertex_class, v)
            r = rows[int(off[l]):int(off[l + 1])]
            has = (r[:, 0] == c) | (r[:, 1] == c)
            if has.any():
                out[v] = r[has, 4].max()
    return out

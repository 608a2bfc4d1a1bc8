"""Genotype margins on a levelized DP graph: the best pair of paths through every cell of a level, both paths free -- plain Python
and numpy, TEST INFRASTRUCTURE, on top of paths_model.PathModel and the in-edge lists of partner_model.

Written from the definition, not from any implementation of it.  d(u, v -> i, j) = inter + symd of PathModel.delta for the edge pair
(u -> i, w1), (v -> j, w2), whose weight is w1 + w2 (also when both paths take the same edge); parallel edges are one edge.

    F_0[src, src][r] = 0                                            for r = 0..b    (budgets mean "at most")
    F_l[i][j][r] = max F_{l-1}[u][v][r - w1 - w2] + d               over the in-edge pairs with r - w1 - w2 >= 0 and a reachable source cell
    B_{L-1}[sink, sink][r] = 0                                      for r = 0..b
    B_l[i][j][r] = max d + B_{l+1}[i'][j'][r - w1 - w2]             over the out-edge pairs with r - w1 - w2 >= 0 and a reachable destination cell
    T_l[i][j] = max F_l[i][j][r] + B_l[i][j][b - r]                 over r = 0..b with both cells reachable
    V_b = F_{L-1}[sink, sink][b]          J[v] = max_j T_l[v][j]

NEG_INF wherever a maximum has no candidate.  Per level and called cell (c1, c2) the record is (c1, c2, T[c1][c2], a1, a2, T[a1][a2]):
(a1, a2) the cell with the largest T among the reachable cells whose genotype -- the unordered pair of its vertices' classes --
differs from the called cell's; among equals the smallest min(i, j), then the smallest max(i, j); a1 <= a2; (-1, -1, NEG_INF) if
there is none.  vertex_class = None: every vertex is its own class.

through_values is the definition in plain Python; through_values_np does the same with numpy over the cells of a level (for the
wider GPU cases) and is pinned to it by tests/test_genotype_margins_model.py."""
import numpy as np

from partner_model import in_edges
from paths_model import NEG_INF


def _level(m, l):
    return range(int(m.level_off[l]), int(m.level_off[l + 1]))


def through_values(m, b):
    """-> (T, V): T[l][i - a0][j - a0] for every level (lists of lists of ints), V = F[L-1][sink, sink][b]"""
    assert b >= 0
    pred = in_edges(m)
    src, sink = 0, m.nV - 1
    F = [None] * m.L
    F[0] = {(i, j): ([0] * (b + 1) if i == j == src else [NEG_INF] * (b + 1)) for i in _level(m, 0) for j in _level(m, 0)}
    for l in range(1, m.L):
        cur = {}
        for i in _level(m, l):
            for j in _level(m, l):
                row = []
                for r in range(b + 1):
                    cands = [F[l - 1][(u, v)][r - w1 - w2] + sum(m.delta(u, v, i, j)) for u, w1 in pred[i] for v, w2 in pred[j]
                             if r - w1 - w2 >= 0 and F[l - 1][(u, v)][r - w1 - w2] != NEG_INF]
                    row.append(max(cands) if cands else NEG_INF)
                cur[(i, j)] = row
        F[l] = cur
    B = [None] * m.L
    B[m.L - 1] = {(i, j): ([0] * (b + 1) if i == j == sink else [NEG_INF] * (b + 1)) for i in _level(m, m.L - 1) for j in _level(m, m.L - 1)}
    for l in range(m.L - 2, -1, -1):
        cur = {}
        for i in _level(m, l):
            for j in _level(m, l):
                row = []
                for r in range(b + 1):
                    cands = [sum(m.delta(i, j, i2, j2)) + B[l + 1][(i2, j2)][r - w1 - w2] for i2, w1 in m.succ[i].items() for j2, w2 in m.succ[j].items()
                             if r - w1 - w2 >= 0 and B[l + 1][(i2, j2)][r - w1 - w2] != NEG_INF]
                    row.append(max(cands) if cands else NEG_INF)
                cur[(i, j)] = row
        B[l] = cur
    T = []
    for l in range(m.L):
        rows = []
        for i in _level(m, l):
            row = []
            for j in _level(m, l):
                cands = [F[l][(i, j)][r] + B[l][(i, j)][b - r] for r in range(b + 1) if F[l][(i, j)][r] != NEG_INF and B[l][(i, j)][b - r] != NEG_INF]
                row.append(max(cands) if cands else NEG_INF)
            rows.append(row)
        T.append(rows)
    return T, F[m.L - 1][(sink, sink)][b]


def _level_edges(m, l):
    """the edges into level l: (source position, destination position, weight) arrays and the score matrix D[e1, e2]"""
    pred = in_edges(m)
    a0, b0 = int(m.level_off[l - 1]), int(m.level_off[l])
    edges = [(u, i, w) for i in _level(m, l) for u, w in pred[i]]
    D = np.zeros((len(edges), len(edges)), np.int64)
    for x, (u, i, _) in enumerate(edges):
        for y, (v, j, _) in enumerate(edges):
            D[x, y] = sum(m.delta(u, v, i, j))
    e = np.array(edges, np.int64).reshape(-1, 3)
    return e[:, 0] - a0, e[:, 1] - b0, e[:, 2], D


def _relax(src_state, dst_state, s_pos, d_pos, w, D, B1):
    """dst_state[d_pos[x], d_pos[y], r] = max over the edge pairs (x, y) of src_state[s_pos[x], s_pos[y], r - w[x] - w[y]] + D[x, y]"""
    for x in range(len(w)):
        for wt in range(int(w[x]), int(w[x]) + 2):
            ys = np.flatnonzero(w + w[x] == wt)
            if ys.size == 0 or wt >= B1:
                continue
            prev = src_state[s_pos[x], s_pos[ys], :B1 - wt]
            cand = np.full((ys.size, B1), NEG_INF, np.int64)
            cand[:, wt:] = np.where(prev == NEG_INF, NEG_INF, prev + D[x, ys][:, None])
            np.maximum.at(dst_state[d_pos[x]], d_pos[ys], cand)


def through_values_np(m, b):
    """-> (T, V): T[l] = int64 [k, k] per level"""
    B1 = b + 1
    widths = np.diff(m.level_off).astype(int)
    sink = m.nV - 1 - int(m.level_off[m.L - 1])
    edges = [None] + [_level_edges(m, l) for l in range(1, m.L)]
    F = [np.full((k, k, B1), NEG_INF, np.int64) for k in widths]
    F[0][0, 0, :] = 0
    for l in range(1, m.L):
        s_pos, d_pos, w, D = edges[l]
        _relax(F[l - 1], F[l], s_pos, d_pos, w, D, B1)
    T = [None] * m.L
    nxt = np.full((widths[-1], widths[-1], B1), NEG_INF, np.int64)
    nxt[sink, sink, :] = 0
    for l in range(m.L - 1, -1, -1):
        if l < m.L - 1:
            s_pos, d_pos, w, D = edges[l + 1]
            cur = np.full((widths[l], widths[l], B1), NEG_INF, np.int64)
            _relax(nxt, cur, d_pos, s_pos, w, D, B1)
            nxt = cur
        f, bb = F[l], nxt[:, :, ::-1]
        T[l] = np.where((f != NEG_INF) & (bb != NEG_INF), f + bb, NEG_INF).max(axis=2)
    return T, int(F[m.L - 1][sink, sink, b])


def joint_marginals(m, T):
    """J per vertex (a list of ints)"""
    return [int(max(row)) for l in range(m.L) for row in np.asarray(T[l]).tolist()]


def _cls(vertex_class, v):
    return v if vertex_class is None else int(vertex_class[v])


def level_records(m, T, called, vertex_class=None):
    """called = [2][L] vertex ids -> per level (vertex1, vertex2, value, alt_vertex1, alt_vertex2, alt_value)"""
    out = []
    for l in range(m.L):
        a0, k = int(m.level_off[l]), int(m.level_off[l + 1] - m.level_off[l])
        c1, c2 = int(called[0][l]), int(called[1][l])
        geno = {_cls(vertex_class, c1), _cls(vertex_class, c2)}, _cls(vertex_class, c1) == _cls(vertex_class, c2)
        best = (-1, -1, NEG_INF)
        for i in range(k):                               # ascending (min, max): a strict > keeps the first among equals
            for j in range(i, k):
                t = int(T[l][i][j])
                ci, cj = _cls(vertex_class, a0 + i), _cls(vertex_class, a0 + j)
                if t == NEG_INF or (({ci, cj}, ci == cj) == geno):
                    continue
                if t > best[2]:
                    best = (a0 + i, a0 + j, t)
        out.append((c1, c2, int(T[l][c1 - a0][c2 - a0])) + best)
    return out


def genotype_margins_np(m, called, b, vertex_class=None, T=None, V=None):
    """called int [n, 2, L] -> (records int32 [n, L, 6], V, J int32 [nV]); numpy over the cells of a level.  T, V: what
    through_values_np(m, b) gave, if the caller has them"""
    if T is None:
        T, V = through_values_np(m, b)
    called = np.asarray(called, np.int64)
    n = called.shape[0]
    rec = np.zeros((n, m.L, 6), np.int32)
    ids = np.arange(m.nV) if vertex_class is None else np.asarray(vertex_class, np.int64)
    for l in range(m.L):
        a0, k = int(m.level_off[l]), int(m.level_off[l + 1] - m.level_off[l])
        Tl = np.asarray(T[l], np.int64)
        ci = ids[a0:a0 + k]
        lo, hi = np.minimum(ci[:, None], ci[None, :]), np.maximum(ci[:, None], ci[None, :])
        upper = np.triu(np.ones((k, k), bool)) & (Tl != NEG_INF)
        for q in range(n):
            c1, c2 = int(called[q, 0, l]), int(called[q, 1, l])
            g1, g2 = sorted((int(ids[c1]), int(ids[c2])))
            keep = upper & ~((lo == g1) & (hi == g2))
            rec[q, l, :3] = (c1, c2, Tl[c1 - a0, c2 - a0])
            if keep.any():
                at = int(np.argmax(np.where(keep, Tl, NEG_INF - 1)))      # row-major: the first among equals = the smallest i, then j
                rec[q, l, 3:] = (a0 + at // k, a0 + at % k, Tl[at // k, at % k])
            else:
                rec[q, l, 3:] = (-1, -1, NEG_INF)
    J = np.concatenate([np.asarray(T[l], np.int64).max(axis=1) for l in range(m.L)]).astype(np.int32)
    return rec, V, J

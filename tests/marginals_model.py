"""Partner marginals of a given source -> sink path on a levelized DP graph -- plain Python, TEST INFRASTRUCTURE, on top of
paths_model.PathModel and the in-edge lists of partner_model.

Written from the definition, not from any implementation of it.  With `given` fixed, the edge u -> v of weight w into level l is
worth d_l(u, v) = inter + symd of the sources (given[l-1], u) against the destinations (given[l], v); parallel edges are one edge.

    F_0[source][r] = 0                                   for r = 0..b    (budgets mean "at most")
    F_l[v][r] = max F_{l-1}[u][r - w] + d_l(u, v)        over the in-edges of v with r - w >= 0 and a reachable source cell
    B_{L-1}[sink][r] = 0                                 for r = 0..b
    B_{l-1}[u][r] = max d_l(u, v) + B_l[v][r - w]        over the out-edges of u with r - w >= 0 and a reachable destination cell
    M[v] = max F[v][r] + B[v][b - r]                     over r = 0..b with both cells reachable

NEG_INF wherever a maximum has no candidate.  M[v] is the best value(given, q) over all paths q through v with r(q) <= b.  Per
level: best = the vertex with the largest M, the smallest id among equals, and its M; second = the same choice among the other
vertices of the level; (-1, NEG_INF) where no (other) vertex has a reachable M.

partner_marginals is the definition, one query at a time; partner_marginals_batch answers many queries on one graph with numpy over
the queries (same loops over levels, vertices and edges, same tie rule) and is pinned to it by tests/test_marginals_model.py."""
import numpy as np

from partner_model import in_edges
from paths_model import NEG_INF


def level_records(M, level_off):
    """M per vertex -> per level (best_vertex, best_value, second_vertex, second_value)"""
    out = []
    for l in range(len(level_off) - 1):
        order = sorted((v for v in range(int(level_off[l]), int(level_off[l + 1])) if M[v] != NEG_INF), key=lambda v: (-M[v], v))
        best = (order[0], M[order[0]]) if order else (-1, NEG_INF)
        second = (order[1], M[order[1]]) if len(order) > 1 else (-1, NEG_INF)
        out.append(best + second)
    return out


def partner_marginals(m, given, b):
    """-> (M, records): M[v] for every vertex (a list of ints), records[l] = (best_vertex, best_value, second_vertex, second_value)"""
    assert m.check_path(given) is None and b >= 0
    given = [int(v) for v in given]
    pred = in_edges(m)
    level_of = m.level_of

    def d(u, v):
        l = int(level_of[v])
        return sum(m.delta(given[l - 1], u, given[l], v))

    F = [None] * m.nV
    F[0] = [0] * (b + 1)
    for v in range(1, m.nV):                             # ids are level-sorted: every source of an in-edge comes first
        row = []
        for r in range(b + 1):
            cands = [F[u][r - w] + d(u, v) for u, w in pred[v] if r - w >= 0 and F[u][r - w] != NEG_INF]
            row.append(max(cands) if cands else NEG_INF)
        F[v] = row
    B = [None] * m.nV
    B[m.nV - 1] = [0] * (b + 1)
    for u in range(m.nV - 2, -1, -1):
        row = []
        for r in range(b + 1):
            cands = [d(u, v) + B[v][r - w] for v, w in m.succ[u].items() if r - w >= 0 and B[v][r - w] != NEG_INF]
            row.append(max(cands) if cands else NEG_INF)
        B[u] = row
    M = []
    for v in range(m.nV):
        cands = [F[v][r] + B[v][b - r] for r in range(b + 1) if F[v][r] != NEG_INF and B[v][b - r] != NEG_INF]
        M.append(max(cands) if cands else NEG_INF)
    return M, level_records(M, m.level_off)


def partner_marginals_batch(m, given, budgets):
    """given [n, L] valid paths, budgets [n] -> (records int32 [n, L, 4], M int32 [n, nV]).  F and B are computed on planes
    0..max(budgets): a cell of plane r depends on planes <= r only, in either direction, so query q combines F[v][r] with
    B[v][budgets[q] - r] for r <= budgets[q]."""
    given = np.asarray(given, np.int64)
    budgets = np.asarray(budgets, np.int64)
    n, B1 = given.shape[0], int(budgets.max()) + 1 if len(budgets) else 1
    assert given.shape == (n, m.L) and (budgets >= 0).all()
    pred = in_edges(m)
    d = {}                                               # (u, v) -> score of the edge per query [n]
    for l in range(1, m.L):
        hops, inv = np.unique(given[:, l - 1:l + 1], axis=0, return_inverse=True)      # the distinct (given[l-1], given[l]) of the queries
        hops, inv = hops.tolist(), inv.reshape(-1)
        for v in range(int(m.level_off[l]), int(m.level_off[l + 1])):
            for u, _ in pred[v]:
                d[(u, v)] = np.array([sum(m.delta(gu, u, gv, v)) for gu, gv in hops], np.int64)[inv]

    def shifted(T, w, add):
        """T[:, r - w] + add where that cell exists and is reachable, NEG_INF elsewhere"""
        cand = np.full((n, B1), NEG_INF, np.int64)
        prev = T[:, :B1 - w] if w else T
        cand[:, w:] = np.where(prev == NEG_INF, NEG_INF, prev + add[:, None])
        return cand

    F = [None] * m.nV
    F[0] = np.zeros((n, B1), np.int64)
    for v in range(1, m.nV):
        best = np.full((n, B1), NEG_INF, np.int64)
        for u, w in pred[v]:
            best = np.maximum(best, shifted(F[u], w, d[(u, v)]))
        F[v] = best
    B = [None] * m.nV
    B[m.nV - 1] = np.zeros((n, B1), np.int64)
    for u in range(m.nV - 2, -1, -1):
        best = np.full((n, B1), NEG_INF, np.int64)
        for v, w in m.succ[u].items():
            best = np.maximum(best, shifted(B[v], w, d[(u, v)]))
        B[u] = best
    q = np.arange(n)
    M = np.full((n, m.nV), NEG_INF, np.int64)
    for v in range(m.nV):
        for r in range(B1):
            ok = r <= budgets
            f, bb = F[v][:, r], B[v][q, np.where(ok, budgets - r, 0)]
            ok &= (f != NEG_INF) & (bb != NEG_INF)
            M[:, v] = np.where(ok, np.maximum(M[:, v], f + bb), M[:, v])
    rec = np.zeros((n, m.L, 4), np.int32)
    for l in range(m.L):
        a0, k = int(m.level_off[l]), int(m.level_off[l + 1] - m.level_off[l])
        Ml = M[:, a0:a0 + k]
        first = Ml.argmax(axis=1)                        # the first among equals = the smallest id; NEG_INF is below every value
        rest = Ml.copy()
        rest[q, first] = NEG_INF - 1
        second = rest.argmax(axis=1)
        v1, v2 = Ml[q, first], (rest[q, second] if k > 1 else np.full(n, NEG_INF))
        rec[:, l, 0] = np.where(v1 == NEG_INF, -1, a0 + first)
        rec[:, l, 1] = v1
        dead2 = (v2 <= NEG_INF) | (k == 1)
        rec[:, l, 2] = np.where(dead2, -1, a0 + second)
        rec[:, l, 3] = np.where(dead2, NEG_INF, v2)
    return rec, M.astype(np.int32)

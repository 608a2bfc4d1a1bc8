"""The best partner of a given source -> sink path on a levelized DP graph -- plain Python, TEST INFRASTRUCTURE, on top of
paths_model.PathModel.

Written from the definition, not from any implementation of it.  With `given` fixed, the transition into level l over the edge
u -> v of weight w is worth d_l(u, v) = inter + symd of the sources (given[l-1], u) against the destinations (given[l], v): what
PathModel.score adds there for the ordered pair (given, partner).  Parallel edges are one edge.

    S_0[source][r] = 0                                   for r = 0..b    (budgets mean "at most")
    S_l[v][r] = max S_{l-1}[u][r - w] + d_l(u, v)        over the in-edges of v with r - w >= 0 and a reachable source cell,
                NEG_INF if there is none; among equal values the in-edge with the smallest source vertex wins.

The answer is S_{L-1}[sink][b] and the path that the winners lead back along from (sink, b).

best_partner is the definition, one query at a time; best_partners answers many queries on one graph with numpy over the
queries (same loops over levels, vertices and in-edges, same tie-break) and is pinned to best_partner by
tests/test_partner_model.py."""
import numpy as np

from paths_model import NEG_INF


def in_edges(m):
    """per vertex: [(source, weight)] sorted by source, parallel edges merged (cached on the PathModel)"""
    pred = getattr(m, "_pred", None)
    if pred is None:
        pred = [[] for _ in range(m.nV)]
        for u in range(m.nV):
            for v, w in m.succ[u].items():
                pred[v].append((u, w))
        for lst in pred:
            lst.sort()
        m._pred = pred
    return pred


def best_partner(m, given, b):
    """-> (value, partner, planes, ties): value = S[sink][b]; partner = the walked-back path as a tuple (None if value is NEG_INF);
    planes = [S[sink][r] for r = 0..b]; ties = cells on the walked chain where more than one in-edge reached the maximum, i.e.
    where the tie-break decided which vertex the partner goes through"""
    assert m.check_path(given) is None and b >= 0
    given = [int(v) for v in given]
    pred = in_edges(m)
    S = {0: [0] * (b + 1)}                               # vertex -> values per plane, the level at hand
    back = [None] * m.L                                  # per level: vertex -> per plane (source, weight, tied) or None
    for l in range(1, m.L):
        cur, bl = {}, {}
        for v in range(int(m.level_off[l]), int(m.level_off[l + 1])):
            vals, bps = [], []
            for r in range(b + 1):
                best, win, tied = NEG_INF, None, False
                for u, w in pred[v]:                     # ascending source: a strict > keeps the smallest among equals
                    if r - w < 0 or S[u][r - w] == NEG_INF:
                        continue
                    inter, symd = m.delta(given[l - 1], u, given[l], v)
                    cand = S[u][r - w] + inter + symd
                    if cand > best:
                        best, win, tied = cand, (u, w), False
                    elif cand == best:
                        tied = True
                vals.append(best)
                bps.append(None if win is None else (win[0], win[1], tied))
            cur[v], bl[v] = vals, bps
        S, back[l] = cur, bl
    sink = m.nV - 1
    planes = list(S[sink])
    value = planes[b]
    if value == NEG_INF:
        return value, None, planes, 0
    path, v, r, ties = [sink], sink, b, 0
    for l in range(m.L - 1, 0, -1):
        u, w, tied = back[l][v][r]
        ties += tied
        v, r = u, r - w
        path.append(v)
    assert v == 0 and r >= 0
    return value, tuple(reversed(path)), planes, ties


def best_partners(m, given, budgets):
    """given [n, L] valid paths, budgets [n] -> (values int32 [n], partners int32 [n, L], rows of -1 where the value is NEG_INF).
    Every query is computed on planes 0..max(budgets): a cell of plane r depends on planes <= r only, so query q reads plane
    budgets[q]."""
    given = np.asarray(given, np.int64)
    budgets = np.asarray(budgets, np.int64)
    n, B1 = given.shape[0], int(budgets.max()) + 1 if len(budgets) else 1
    assert given.shape == (n, m.L) and (budgets >= 0).all()
    pred = in_edges(m)
    q = np.arange(n)
    S = {0: np.zeros((n, B1), np.int64)}
    back = [None] * m.L                                  # per level: vertex -> (source [n, B1], weight [n, B1])
    for l in range(1, m.L):
        hops, inv = np.unique(given[:, l - 1:l + 1], axis=0, return_inverse=True)      # the distinct (given[l-1], given[l]) of the queries
        hops, inv = hops.tolist(), inv.reshape(-1)
        cur, bl = {}, {}
        for v in range(int(m.level_off[l]), int(m.level_off[l + 1])):
            best = np.full((n, B1), NEG_INF, np.int64)
            src = np.full((n, B1), -1, np.int64)
            wgt = np.zeros((n, B1), np.int64)
            for u, w in pred[v]:
                d = np.array([sum(m.delta(gu, u, gv, v)) for gu, gv in hops], np.int64)[inv]
                cand = np.full((n, B1), NEG_INF, np.int64)
                prev = S[u][:, :B1 - w] if w else S[u]
                cand[:, w:] = np.where(prev == NEG_INF, NEG_INF, prev + d[:, None])
                take = cand > best
                best = np.where(take, cand, best)
                src = np.where(take, u, src)
                wgt = np.where(take, w, wgt)
            cur[v], bl[v] = best, (src, wgt)
        S, back[l] = cur, bl
    sink = m.nV - 1
    values = S[sink][q, budgets].astype(np.int32)
    partners = np.full((n, m.L), -1, np.int32)
    for i in np.flatnonzero(values != NEG_INF):
        v, r = sink, int(budgets[i])
        partners[i, m.L - 1] = v
        for l in range(m.L - 1, 0, -1):
            src, wgt = back[l][v]
            v, r = int(src[i, r]), r - int(wgt[i, r])
            partners[i, l - 1] = v
    return values, partners

"""The joint pass under per-level cell constraints (dg_dp_genotype_margins_pinned / dg_dp_genotype_table_pinned) -- plain Python and
numpy, TEST INFRASTRUCTURE, on top of paths_model.PathModel, the mask of pinned_model and the relaxation of genotype_margins_model.

Written from the definition, not from any implementation of it.  With a pin set P (pinned_model: ordered cells, require / forbid):

    F_l[i][j][r], B_l[i][j][r]   the recurrences of genotype_margins_model, NEG_INF on every plane where cell (i, j) of level l is not allowed
    T_l[i][j | P] = max F_l[i][j][r] + B_l[i][j][b - r]            over r = 0..b with both cells reachable
    V_b(P) = F_{L-1}[sink, sink][b]          J[v] = max_j T_l[v][j | P]   (the ordered row)

T_l[i][j | P] is the best value of any ORDERED pair (p, q) of source -> sink paths that satisfies P with p[l] = i, q[l] = j and
r(p) + r(q) <= b, so T need not be symmetric.  A genotype is unordered: the alternative of a margin record and the entries of the table
take the cells i <= j with the value max(T[i][j], T[j][i]) -- folded(T) -- by the rules of genotype_margins_model.level_records and
genotype_table_model; the called cell's own value is T at the ordered called cell.

pinned_through_values is the definition in plain Python; pinned_through_values_np does the same with numpy over the cells of a level
(for the wider GPU cases); tests/test_pinned_joint_model.py pins both to brute force."""
import numpy as np

from genotype_margins_model import _level, _level_edges, _relax, genotype_margins_np, level_records
from genotype_table_model import genotype_table, genotype_table_np
from partner_model import in_edges
from paths_model import NEG_INF
from pinned_model import allowed_masks, cell_allowed


def _pins(pins):
    return [tuple(int(x) for x in p) for p in pins]


def pinned_through_values(m, b, pins):
    """-> (T, V): T[l][i - a0][j - a0] for every level (lists of lists of ints), V = F[L-1][sink, sink][b]; plain Python"""
    assert b >= 0
    pins = _pins(pins)
    pred = in_edges(m)
    src, sink = 0, m.nV - 1
    dead = [NEG_INF] * (b + 1)
    F = [None] * m.L
    F[0] = {(i, j): ([0] * (b + 1) if i == j == src else list(dead)) for i in _level(m, 0) for j in _level(m, 0)}
    for l in range(1, m.L):
        cur = {}
        for i in _level(m, l):
            for j in _level(m, l):
                row = []
                for r in range(b + 1):
                    cands = [F[l - 1][(u, v)][r - w1 - w2] + sum(m.delta(u, v, i, j)) for u, w1 in pred[i] for v, w2 in pred[j]
                             if r - w1 - w2 >= 0 and F[l - 1][(u, v)][r - w1 - w2] != NEG_INF]
                    row.append(max(cands) if cands and cell_allowed(pins, l, i, j) else NEG_INF)
                cur[(i, j)] = row
        F[l] = cur
    B = [None] * m.L
    B[m.L - 1] = {(i, j): ([0] * (b + 1) if i == j == sink else list(dead)) for i in _level(m, m.L - 1) for j in _level(m, m.L - 1)}
    for l in range(m.L - 2, -1, -1):
        cur = {}
        for i in _level(m, l):
            for j in _level(m, l):
                row = []
                for r in range(b + 1):
                    cands = [sum(m.delta(i, j, i2, j2)) + B[l + 1][(i2, j2)][r - w1 - w2] for i2, w1 in m.succ[i].items() for j2, w2 in m.succ[j].items()
                             if r - w1 - w2 >= 0 and B[l + 1][(i2, j2)][r - w1 - w2] != NEG_INF]
                    row.append(max(cands) if cands and cell_allowed(pins, l, i, j) else NEG_INF)
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


def pinned_through_values_np(m, b, pins):
    """-> (T, V): T[l] = int64 [k, k] per level (the transitions' score matrices are cached on the model)"""
    B1 = b + 1
    widths = np.diff(m.level_off).astype(int)
    sink = m.nV - 1 - int(m.level_off[m.L - 1])
    edges = getattr(m, "_level_edges", None)
    if edges is None:
        edges = m._level_edges = [None] + [_level_edges(m, l) for l in range(1, m.L)]
    masks = allowed_masks(m, _pins(pins))
    F = [np.full((k, k, B1), NEG_INF, np.int64) for k in widths]
    F[0][0, 0, :] = 0
    for l in range(1, m.L):
        s_pos, d_pos, w, D = edges[l]
        _relax(F[l - 1], F[l], s_pos, d_pos, w, D, B1)
        if l in masks:
            F[l][~masks[l]] = NEG_INF
    T = [None] * m.L
    nxt = np.full((widths[-1], widths[-1], B1), NEG_INF, np.int64)
    nxt[sink, sink, :] = 0
    for l in range(m.L - 1, -1, -1):
        if l < m.L - 1:
            s_pos, d_pos, w, D = edges[l + 1]
            cur = np.full((widths[l], widths[l], B1), NEG_INF, np.int64)
            _relax(nxt, cur, d_pos, s_pos, w, D, B1)
            if l in masks:
                cur[~masks[l]] = NEG_INF
            nxt = cur
        f, bb = F[l], nxt[:, :, ::-1]
        T[l] = np.where((f != NEG_INF) & (bb != NEG_INF), f + bb, NEG_INF).max(axis=2)
    return T, int(F[m.L - 1][sink, sink, b])


def folded(T):
    """per level max(T[i][j], T[j][i]): the value of the unordered cell, int64 [k, k]"""
    return [np.maximum(np.asarray(t, np.int64), np.asarray(t, np.int64).T) for t in T]


def pinned_level_records(m, T, called, vertex_class=None):
    """called = [2][L] vertex ids -> per level (vertex1, vertex2, value, alt_vertex1, alt_vertex2, alt_value): the alternative by
    genotype_margins_model.level_records on the folded T, the value at the ORDERED called cell"""
    out = []
    for l, rec in enumerate(level_records(m, folded(T), called, vertex_class)):
        a0 = int(m.level_off[l])
        out.append(rec[:2] + (int(T[l][rec[0] - a0][rec[1] - a0]),) + rec[3:])
    return out


def pinned_genotype_margins_np(m, called, T, V, vertex_class=None):
    """called int [n, 2, L], (T, V) of pinned_through_values_np -> (records int32 [n, L, 6], V, J int32 [nV])"""
    called = np.asarray(called, np.int64)
    rec, V, _ = genotype_margins_np(m, called, None, vertex_class, T=folded(T), V=V)
    for l in range(m.L):
        a0 = int(m.level_off[l])
        rec[:, l, 2] = np.asarray(T[l], np.int64)[called[:, 0, l] - a0, called[:, 1, l] - a0]
    J = np.concatenate([np.asarray(T[l], np.int64).max(axis=1) for l in range(m.L)]).astype(np.int32)
    return rec, V, J


def pinned_genotype_table(m, T, vertex_class=None):
    """genotype_table_model.genotype_table of the folded T"""
    return genotype_table(m, folded(T), vertex_class)


def pinned_genotype_table_np(m, T, vertex_class=None):
    """genotype_table_model.genotype_table_np of the folded T -> (level_off, rows)"""
    return genotype_table_np(m, folded(T), vertex_class)


def brute_force_through_values(m, paths, rec, full, b, pins):
    """T_l[i][j | P] from ALL ordered pairs (p, q) of source -> sink paths that satisfy the pins with r(p) + r(q) <= b: per level
    int64 [k, k], NEG_INF where no such pair passes (i, j).  paths, rec, full: as for pinned_model.brute_force_planes"""
    from pinned_model import brute_force_planes
    _, sat = brute_force_planes(m, paths, rec, full, b, pins)
    P = np.asarray(paths, np.int64)
    r = np.asarray(rec, np.int64)
    ok = sat & (r[:, None] + r[None, :] <= b)
    val = np.where(ok, np.asarray(full, np.int64), NEG_INF)
    T = []
    for l in range(m.L):
        a0, k = int(m.level_off[l]), int(m.level_off[l + 1] - m.level_off[l])
        t = np.full((k, k), NEG_INF, np.int64)
        np.maximum.at(t, (np.broadcast_to(P[:, l][:, None] - a0, val.shape), np.broadcast_to(P[:, l][None, :] - a0, val.shape)), val)
        T.append(t)
    return T

"""Phase margins on a levelized DP graph: cis against trans for neighbouring het levels of a called pair of cells per level -- numpy,
TEST INFRASTRUCTURE, on top of genotype_margins_model._level_edges / _relax.

Written from the definition in include/dipgenie_hip.h (dg_dp_phase_margins), not from any implementation of it.  F and B are the
forward and backward states of genotype_margins_model ("at most r"); c_h[l] = the class of called[h][l]; the het levels are those with
c_0[l] != c_1[l], ascending.  For neighbours (a, e):

    S_e[i][j][r] = B_e[i][j][r]  where (cls i, cls j) = (c_0[e], c_1[e]),  NEG_INF elsewhere
    S_l          = the backward recurrence on S_{l+1}, unchanged                                   for l = e - 1 .. a
    U_a[i][j]    = max F_a[i][j][r] + S_a[i][j][b - r]                                             over r = 0..b with both reachable
    cis   = max U_a over the cells of classes (c_0[a], c_1[a])
    trans = max U_a over the cells of classes (c_1[a], c_0[a])

each with its cell: the largest value, then the smallest position of vertex1, then of vertex2; NEG_INF and -1, -1 if none is
reachable.  A record is (level_a, level_b, cis_value, cis_vertex1, cis_vertex2, trans_value, trans_vertex1, trans_vertex2).
tests/test_phase_margins_model.py pins this file to brute force over all pairs of paths."""
import numpy as np

from genotype_margins_model import _level_edges, _relax
from paths_model import NEG_INF

FIELDS = ("level_a", "level_b", "cis_value", "cis_vertex1", "cis_vertex2", "trans_value", "trans_vertex1", "trans_vertex2")


def joint_states_fb(m, b):
    """-> (F, B, V, edges): int64 [k, k, b + 1] per level, both ways, V = F[L-1][sink, sink][b], and the levels' edge lists.
    Independent of `called`: compute once per (graph, budget) and hand it to phase_margins_np as `states`"""
    B1 = b + 1
    widths = np.diff(m.level_off).astype(int)
    sink = m.nV - 1 - int(m.level_off[m.L - 1])
    edges = [None] + [_level_edges(m, l) for l in range(1, m.L)]
    F = [np.full((k, k, B1), NEG_INF, np.int64) for k in widths]
    F[0][0, 0, :] = 0
    for l in range(1, m.L):
        s_pos, d_pos, w, D = edges[l]
        _relax(F[l - 1], F[l], s_pos, d_pos, w, D, B1)
    B = [np.full((k, k, B1), NEG_INF, np.int64) for k in widths]
    B[m.L - 1][sink, sink, :] = 0
    for l in range(m.L - 2, -1, -1):
        s_pos, d_pos, w, D = edges[l + 1]
        _relax(B[l + 1], B[l], d_pos, s_pos, w, D, B1)
    return F, B, int(F[m.L - 1][sink, sink, b]), edges


def het_levels(m, called, vertex_class=None):
    ids = np.arange(m.nV) if vertex_class is None else np.asarray(vertex_class, np.int64)
    called = np.asarray(called, np.int64)
    return [l for l in range(m.L) if ids[called[0, l]] != ids[called[1, l]]]


def _best(U, mask, a0):
    """(value, vertex1, vertex2) of the largest U under mask; row-major argmax: the first among equals = the smallest i, then j"""
    keep = mask & (U != NEG_INF)
    if not keep.any():
        return NEG_INF, -1, -1
    k = U.shape[0]
    at = int(np.argmax(np.where(keep, U, NEG_INF - 1)))
    return int(U[at // k, at % k]), a0 + at // k, a0 + at % k


def phase_margins_np(m, called, b, vertex_class=None, states=None):
    """called int [2, L] -> (records int32 [m - 1, 8] in the order of FIELDS, V)"""
    F, B, V, edges = states if states is not None else joint_states_fb(m, b)
    B1 = b + 1
    ids = np.arange(m.nV) if vertex_class is None else np.asarray(vertex_class, np.int64)
    called = np.asarray(called, np.int64)
    het = het_levels(m, called, vertex_class)
    out = []
    for a, e in zip(het[:-1], het[1:]):
        e0, ke = int(m.level_off[e]), int(m.level_off[e + 1] - m.level_off[e])
        ce = ids[e0:e0 + ke]
        mask_e = (ce[:, None] == ids[called[0, e]]) & (ce[None, :] == ids[called[1, e]])
        S = np.where(mask_e[:, :, None], B[e], NEG_INF)
        for l in range(e - 1, a - 1, -1):
            s_pos, d_pos, w, D = edges[l + 1]
            k = int(m.level_off[l + 1] - m.level_off[l])
            cur = np.full((k, k, B1), NEG_INF, np.int64)
            _relax(S, cur, d_pos, s_pos, w, D, B1)
            S = cur
        f, s = F[a], S[:, :, ::-1]
        U = np.where((f != NEG_INF) & (s != NEG_INF), f + s, NEG_INF).max(axis=2)
        a0, ka = int(m.level_off[a]), int(m.level_off[a + 1] - m.level_off[a])
        ca = ids[a0:a0 + ka]
        x0, x1 = ids[called[0, a]], ids[called[1, a]]
        cis = _best(U, (ca[:, None] == x0) & (ca[None, :] == x1), a0)
        trans = _best(U, (ca[:, None] == x1) & (ca[None, :] == x0), a0)
        out.append((a, e) + cis + trans)
    return np.array(out, np.int32).reshape(-1, 8), V

"""Genotype margins for several budgets from ONE joint pass (dg_dp_genotype_margins_budgets) -- numpy, TEST INFRASTRUCTURE, on top of
the relaxation of genotype_margins_model and the masks of pinned_model.

The claim: the states mean "at most r", so F_l[i][j][r] and B_l[i][j][r] do not depend on the budget they were computed for, and

    T^b_l[i][j] = max F_l[i][j][r] + B_l[i][j][b - r]               over r = 0..b with both cells reachable
    V_b = F_{L-1}[sink, sink][b]

for every b <= bmax from the states at bmax.  joint_states_np computes F and B once at bmax (with pins: NEG_INF on every plane of a cell
that is not allowed, as pinned_joint_model); sliced_through_values cuts T^b out of them.  tests/test_genotype_budgets_model.py pins the
slices to genotype_margins_model.through_values_np(m, b) and pinned_joint_model.pinned_through_values_np(m, b, pins) for every b."""
import numpy as np

from genotype_margins_model import _level_edges, _relax, genotype_margins_np
from paths_model import NEG_INF
from pinned_joint_model import pinned_genotype_margins_np
from pinned_model import allowed_masks


def joint_states_np(m, bmax, pins=()):
    """-> (F, B): per level int64 [k, k, bmax + 1]"""
    B1 = bmax + 1
    widths = np.diff(m.level_off).astype(int)
    sink = m.nV - 1 - int(m.level_off[m.L - 1])
    edges = [None] + [_level_edges(m, l) for l in range(1, m.L)]
    masks = allowed_masks(m, [tuple(int(x) for x in p) for p in pins])
    F = [np.full((k, k, B1), NEG_INF, np.int64) for k in widths]
    F[0][0, 0, :] = 0
    for l in range(1, m.L):
        s_pos, d_pos, w, D = edges[l]
        _relax(F[l - 1], F[l], s_pos, d_pos, w, D, B1)
        if l in masks:
            F[l][~masks[l]] = NEG_INF
    B = [np.full((k, k, B1), NEG_INF, np.int64) for k in widths]
    B[m.L - 1][sink, sink, :] = 0
    for l in range(m.L - 2, -1, -1):
        s_pos, d_pos, w, D = edges[l + 1]
        _relax(B[l + 1], B[l], d_pos, s_pos, w, D, B1)
        if l in masks:
            B[l][~masks[l]] = NEG_INF
    return F, B


def sliced_through_values(m, F, B, b):
    """-> (T, V) at budget b <= bmax from the states of joint_states_np: T[l] = int64 [k, k]"""
    sink = m.nV - 1 - int(m.level_off[m.L - 1])
    T = []
    for l in range(m.L):
        f, bb = F[l][:, :, :b + 1], B[l][:, :, b::-1]
        T.append(np.where((f != NEG_INF) & (bb != NEG_INF), f + bb, NEG_INF).max(axis=2))
    return T, int(F[m.L - 1][sink, sink, b])


def genotype_margins_budgets_np(m, called, budgets, vertex_class=None, pins=None):
    """called int [n, 2, L], budgets int [n] -> (records int32 [n, L, 6], V int32 [n]): query q by the records of
    genotype_margins_np -- with pins (a list, possibly empty, not None) of pinned_genotype_margins_np -- on the slice at budgets[q]"""
    called = np.asarray(called, np.int64)
    budgets = [int(b) for b in budgets]
    F, B = joint_states_np(m, max(budgets), pins if pins is not None else ())
    rec = np.zeros((len(budgets), m.L, 6), np.int32)
    V = np.zeros(len(budgets), np.int32)
    slices = {}
    for q, b in enumerate(budgets):
        if b not in slices:
            slices[b] = sliced_through_values(m, F, B, b)
        T, V[q] = slices[b]
        if pins is None:
            rec[q] = genotype_margins_np(m, called[q:q + 1], b, vertex_class, T, int(V[q]))[0][0]
        else:
            rec[q] = pinned_genotype_margins_np(m, called[q:q + 1], T, int(V[q]), vertex_class)[0][0]
    return rec, V

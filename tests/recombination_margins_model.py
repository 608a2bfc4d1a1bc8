"""Recombination margins on a levelized DP graph: per transition the best pair of paths that spends 0, 1 or 2 crossovers there -- numpy,
TEST INFRASTRUCTURE, on top of phase_margins_model.joint_states_fb / genotype_margins_model._level_edges.

Written from the definition in include/dipgenie_hip.h (dg_dp_recombination_margins), not from any implementation of it.  F and B are the
forward and backward states of genotype_margins_model ("at most r").  For the transition t = l -> l + 1 and s in {0, 1, 2}:

    E_t[s] = max F_l[i][j][r] + d(i, j -> i', j') + B_{l+1}[i'][j'][b - s - r]
             over the ordered hop pairs (i -> i', w1), (j -> j', w2) of t with w1 + w2 = s, s <= b, and r = 0 .. b - s with both reachable

with the hop pair that attains it: the largest value, then the smallest (i, j, i', j') in that order; NEG_INF and -1 where there is
none.  A record is (level, value[3], from1[3], from2[3], to1[3], to2[3]), 16 words, ids are vertex ids.  Per called pair of cells per
level and transition: s_called = the summed weights of the two called hops (-1 if either is no edge) and called_value = the maximum
above restricted to that ordered hop pair.  tests/test_recombination_margins_model.py pins this file to brute force over all pairs of
paths."""
import numpy as np

from paths_model import NEG_INF
from phase_margins_model import joint_states_fb

FIELDS = ("level", "value", "from1", "from2", "to1", "to2")


def hop_values(F_l, B_n, s_pos, d_pos, w, D, b):
    """-> (val, ws): val[x, y] = the best value of a pair of paths that takes the in-edges x and y (ordered) of the transition, NEG_INF
    if none does; ws[x, y] = w[x] + w[y]"""
    E = len(w)
    ws = (w[:, None] + w[None, :]).astype(np.int64)
    val = np.full((E, E), NEG_INF, np.int64)
    if E == 0:
        return val, ws
    Fx = F_l[s_pos[:, None], s_pos[None, :], :]                            # [E, E, b + 1]
    Bx = B_n[d_pos[:, None], d_pos[None, :], :]
    for s in range(min(2, b) + 1):
        n = b - s + 1
        f, bb = Fx[:, :, :n], Bx[:, :, :n][:, :, ::-1]                       # r = 0 .. b - s against b - s - r
        both = np.where((f != NEG_INF) & (bb != NEG_INF), f + bb, NEG_INF).max(axis=2)
        hit = (ws == s) & (both != NEG_INF)
        val[hit] = both[hit] + D[hit]
    return val, ws


def recombination_margins_np(m, b, called=None, states=None):
    """-> (records int32 [L - 1, 16], called_out int32 [n, L - 1, 2] or None, V).  called: int [n, 2, L] or None"""
    F, B, V, edges = states if states is not None else joint_states_fb(m, b)
    L = m.L
    rec = np.zeros((L - 1, 16), np.int32)
    called = None if called is None else np.asarray(called, np.int64)
    out = None if called is None else np.zeros((called.shape[0], L - 1, 2), np.int32)
    for l in range(L - 1):
        a0, b0 = int(m.level_off[l]), int(m.level_off[l + 1])
        s_pos, d_pos, w, D = edges[l + 1]
        val, ws = hop_values(F[l], B[l + 1], s_pos, d_pos, w, D, b)
        rec[l, 0] = l
        for s in range(3):
            hit = np.argwhere((ws == s) & (val != NEG_INF))
            if hit.size == 0:
                rec[l, 1 + s] = NEG_INF
                rec[l, [4 + s, 7 + s, 10 + s, 13 + s]] = -1
                continue
            best = int(val[hit[:, 0], hit[:, 1]].max())
            tup = min((int(s_pos[x]), int(s_pos[y]), int(d_pos[x]), int(d_pos[y])) for x, y in hit.tolist() if val[x, y] == best)
            rec[l, 1 + s] = best
            rec[l, [4 + s, 7 + s, 10 + s, 13 + s]] = (a0 + tup[0], a0 + tup[1], b0 + tup[2], b0 + tup[3])
        if called is None:
            continue
        edge_of = {(int(s_pos[x]), int(d_pos[x])): x for x in range(len(w))}
        for q in range(called.shape[0]):
            x = edge_of.get((int(called[q, 0, l]) - a0, int(called[q, 0, l + 1]) - b0))
            y = edge_of.get((int(called[q, 1, l]) - a0, int(called[q, 1, l + 1]) - b0))
            out[q, l] = (-1, NEG_INF) if x is None or y is None else (int(ws[x, y]), int(val[x, y]))
    return rec, out, V


def rows(records):
    """a RECOMBINATION_MARGIN record array as int64 [n, 16] in the order of FIELDS"""
    return np.concatenate([np.asarray(records[f], np.int64).reshape(len(records), -1) for f in FIELDS], axis=1)


def remap_rows(rec, new_id):
    """records [n, 16] of a graph as those of its padded graph (tests/padded_graphs.py): the ids through the map, -1 stays"""
    out = np.array(rec, np.int64)
    ids = out[:, 4:]
    out[:, 4:] = np.where(ids < 0, ids, new_id[np.maximum(ids, 0)])
    return out

"""The pair of paths that the diploid DP's lattice decodes to -- plain Python, TEST INFRASTRUCTURE, used only to check the oracle.

A second statement of what oracle/oracle_dp.cpp's orc_dp_paths_diploid computes, written from the rule and not from that code: cells
(r, i, j) of a level are visited with r, then i, then j ascending, the out-edges of the two vertices in adjacency order (eu outer, ev
inner); a candidate replaces what the destination cell holds if its value is strictly larger, or equal with a smaller pred_i, or equal
with the same pred_i and a smaller pred_j (approximator.cpp:657-659).  Every cell keeps the (pred_i, pred_j, source plane) of its
winner; the answer is walked back from the sink cell (R, 0, 0).  The score of a transition is tests/paths_model.py's set statement.

Slow (a 122-level, 6-wide, R = 53 graph takes a few seconds): tests/test_trace_graphs.py runs it on a handful of (graph, budget) points."""
import numpy as np

from paths_model import NEG_INF

_BIG = 2 ** 31 - 1


def dp_paths(g, stats=None):
    """(value, int32 [2, n_levels] vertex ids, row 0 the first path) of g at budget g.R; (NEG_INF, None) where the sink cell (R, 0, 0) is
    unreachable.  stats (a dict) receives "tied": the number of cells on the walked path whose value was offered by more than one
    predecessor cell, so that only the rule's order chose between them"""
    R = g.R
    level_off = [int(x) for x in g.level_off]
    out_off = [int(x) for x in g.out_off]
    out_dst = [int(x) for x in g.out_dst]
    out_w = [int(x) for x in g.out_w]
    L = len(level_off) - 1
    hom = [frozenset(int(c) for c in g.hom_col[g.hom_off[v]:g.hom_off[v + 1]]) for v in range(level_off[-1])]
    het = [frozenset(int(c) for c in g.het_col[g.het_off[v]:g.het_off[v + 1]]) for v in range(level_off[-1])]
    assert level_off[1] == 1
    # a cell is [value, pred_i, pred_j, pred_r, tied]
    cur = [[[[0, _BIG, _BIG, -1, False]]] for _ in range(R + 1)]              # level 0: every plane of the source cell holds 0
    back = [None]
    for l in range(L - 1):
        a0, k = level_off[l], level_off[l + 1] - level_off[l]
        b0, k2 = level_off[l + 1], level_off[l + 2] - level_off[l + 1]
        nxt = [[[[NEG_INF, _BIG, _BIG, -1, False] for _ in range(k2)] for _ in range(k2)] for _ in range(R + 1)]
        delta = {}
        for r in range(R + 1):
            for i in range(k):
                for j in range(k):
                    value = cur[r][i][j][0]
                    if value == NEG_INF:
                        continue
                    u1, v1 = a0 + i, a0 + j
                    for eu in range(out_off[u1], out_off[u1 + 1]):
                        u2, wu = out_dst[eu], out_w[eu]
                        for ev in range(out_off[v1], out_off[v1 + 1]):
                            v2 = out_dst[ev]
                            r2 = r + wu + out_w[ev]
                            if r2 > R:
                                continue
                            d = delta.get((u1, v1, u2, v2))
                            if d is None:
                                d = delta[(u1, v1, u2, v2)] = (len((hom[u1] | hom[v1]) & (hom[u2] | hom[v2])) +
                                                               len((het[u1] | het[v1]) ^ (het[u2] | het[v2])))
                            cand = value + d
                            dst = nxt[r2][u2 - b0][v2 - b0]
                            tied = cand == dst[0] and (i, j) != (dst[1], dst[2])        # (parallel edges offer the same predecessor again: no tie)
                            if cand > dst[0] or (cand == dst[0] and (i < dst[1] or (i == dst[1] and j < dst[2]))):
                                dst[0], dst[1], dst[2], dst[3], dst[4] = cand, i, j, r, tied
                            elif tied:
                                dst[4] = True
        back.append(nxt)
        cur = nxt
    value = cur[R][0][0][0]
    if value == NEG_INF:
        return NEG_INF, None
    paths = np.zeros((2, L), np.int32)
    r, i, j, n_tied = R, 0, 0, 0
    for l in range(L - 1, -1, -1):
        paths[0, l], paths[1, l] = level_off[l] + i, level_off[l] + j
        if l:
            _, i, j, r, tied = back[l][r][i][j]
            n_tied += tied
    if stats is not None:
        stats["tied"] = n_tied
    assert (i, j) == (0, 0) and r >= 0
    return value, paths

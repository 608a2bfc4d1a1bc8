"""Call margins of a pair of paths on a levelized DP graph -- plain Python, TEST INFRASTRUCTURE, on top of marginals_model.

Written from the definition.  (p1, p2) is a pair of source -> sink paths with r1, r2 weight-1 hops, b a budget with r1 + r2 <= b
(the answer of a run at budget b is such a pair, and the best one).  Row 0 describes p1 with p2 given and the partner budget b - r2,
row 1 describes p2 with p1 given and b - r1; M is marginals_model's M for that given path and budget.  Per level l:

    vertex     = p_h[l]                 value     = M[p_h[l]]
    alt_vertex = the vertex of level l with the largest reachable M among those whose class differs from the class of p_h[l],
                 the smallest id among equals; alt_value its M; (-1, NEG_INF) if there is none

vertex_class = None: every vertex is its own class.  call_margins is the definition; call_margins_batch does the same through
marginals_model.partner_marginals_batch (one call for both rows) and is pinned to it by tests/test_call_margins_model.py."""
import numpy as np

from marginals_model import partner_marginals, partner_marginals_batch
from paths_model import NEG_INF


def class_records(M, called, level_off, vertex_class=None):
    """M per vertex, the called vertex per level -> per level (vertex, value, alt_vertex, alt_value)"""
    out = []
    for l in range(len(level_off) - 1):
        c = int(called[l])
        cc = c if vertex_class is None else int(vertex_class[c])
        others = [v for v in range(int(level_off[l]), int(level_off[l + 1]))
                  if (v if vertex_class is None else int(vertex_class[v])) != cc and M[v] != NEG_INF]
        alt = min(others, key=lambda v: (-int(M[v]), v)) if others else None
        out.append((c, int(M[c]), -1 if alt is None else alt, NEG_INF if alt is None else int(M[alt])))
    return out


def partner_budgets(m, p1, p2, b):
    r1, r2 = m.recombinations(p1), m.recombinations(p2)
    assert r1 + r2 <= b, (r1, r2, b)
    return b - r2, b - r1


def call_margins(m, p1, p2, b, vertex_class=None):
    """-> [2][L] records (vertex, value, alt_vertex, alt_value)"""
    b0, b1 = partner_budgets(m, p1, p2, b)
    M0, _ = partner_marginals(m, p2, b0)
    M1, _ = partner_marginals(m, p1, b1)
    return [class_records(M0, p1, m.level_off, vertex_class), class_records(M1, p2, m.level_off, vertex_class)]


def call_margins_batch(m, p1, p2, b, class_arrays):
    """the same for several class arrays at once -> (M int32 [2, nV], [records int32 [2, L, 4] per class array])"""
    _, M = partner_marginals_batch(m, np.array([p2, p1], np.int32), np.array(partner_budgets(m, p1, p2, b), np.int32))
    return M, [np.array([class_records(M[0], p1, m.level_off, cls), class_records(M[1], p2, m.level_off, cls)], np.int32) for cls in class_arrays]


def class_arrays(g, seed):
    """the three kinds the tests use: None, one class for all, and 2..4 classes drawn per level"""
    rng = np.random.default_rng(seed)
    drawn = np.zeros(g.n_vertices, np.int32)
    for l in range(g.n_levels):
        a, e = int(g.level_off[l]), int(g.level_off[l + 1])
        drawn[a:e] = rng.integers(0, rng.integers(2, 5), e - a)
    return [None, np.ones(g.n_vertices, np.int32), drawn]

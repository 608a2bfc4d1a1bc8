"""The diploid DP under per-level cell constraints (dg_dp_run_pinned) -- plain Python and numpy, TEST INFRASTRUCTURE, on top of
paths_model.PathModel and the in-edge lists of partner_model.

Written from the definition, not from any implementation of it.  A pin is (level, vertex1, vertex2, kind): it matches cell (i, j) of
its level -- i the vertex of the first path, j of the second, ORDERED -- if vertex1 is -1 or i and vertex2 is -1 or j.  A cell of a
level is allowed if the level has no require-pin (kind 0) or one of them matches it, and no forbid-pin (kind 1) of the level matches
it.  The forward recurrence is that of genotype_margins_model.through_values with every cell that is not allowed unreachable on
every plane:

    F_0[src, src][r] = 0                                            for r = 0..b    (budgets mean "at most")
    F_l[i][j][r] = max F_{l-1}[u][v][r - w1 - w2] + d               over the in-edge pairs with r - w1 - w2 >= 0 and a reachable source cell,
                   NEG_INF if (i, j) is not allowed on level l

and the answer is the sink's value on every plane 0..b.  pinned_planes is the definition in plain Python; pinned_planes_np does the
same with numpy over the cells of a level (for the wider GPU cases); tests/test_pinned_model.py pins both to brute force."""
import numpy as np

from genotype_margins_model import _level, _level_edges, _relax
from partner_model import in_edges
from paths_model import NEG_INF

REQUIRE, FORBID = 0, 1


def matches(pin, i, j):
    _, v1, v2, _ = pin
    return (v1 == -1 or v1 == i) and (v2 == -1 or v2 == j)


def cell_allowed(pins, l, i, j):
    """is cell (i, j) -- vertex ids -- of level l allowed under the pins"""
    mine = [p for p in pins if p[0] == l]
    req = [p for p in mine if p[3] == REQUIRE]
    if req and not any(matches(p, i, j) for p in req):
        return False
    return not any(matches(p, i, j) for p in mine if p[3] == FORBID)


def pair_satisfies(pins, p, q):
    """does the ordered pair of paths (p, q) pass only allowed cells"""
    return all(cell_allowed(pins, l, int(p[l]), int(q[l])) for l in {pin[0] for pin in pins})


def allowed_masks(m, pins):
    """{level: bool [k, k]} for the pinned levels"""
    out = {}
    for l in sorted({int(p[0]) for p in pins}):
        a0, k = int(m.level_off[l]), int(m.level_off[l + 1] - m.level_off[l])
        mine = [p for p in pins if p[0] == l]
        req = np.zeros((k, k), bool)
        forbid = np.zeros((k, k), bool)
        any_req = False
        for _, v1, v2, kind in mine:
            sel = np.zeros((k, k), bool)
            sel[(slice(None) if v1 == -1 else v1 - a0), (slice(None) if v2 == -1 else v2 - a0)] = True
            if kind == REQUIRE:
                any_req = True
                req |= sel
            else:
                forbid |= sel
        out[l] = (req if any_req else np.ones((k, k), bool)) & ~forbid
    return out


def pinned_planes(m, b, pins):
    """the sink's value on planes 0..b (a list of ints), plain Python"""
    assert b >= 0
    pred = in_edges(m)
    src, sink = 0, m.nV - 1
    pins = [tuple(int(x) for x in p) for p in pins]
    F = {(src, src): [0] * (b + 1)}
    for l in range(1, m.L):
        cur = {}
        for i in _level(m, l):
            for j in _level(m, l):
                row = []
                for r in range(b + 1):
                    cands = [F[(u, v)][r - w1 - w2] + sum(m.delta(u, v, i, j)) for u, w1 in pred[i] for v, w2 in pred[j]
                             if r - w1 - w2 >= 0 and F[(u, v)][r - w1 - w2] != NEG_INF]
                    row.append(max(cands) if cands and cell_allowed(pins, l, i, j) else NEG_INF)
                cur[(i, j)] = row
        F = cur
    return F[(sink, sink)]


def pinned_planes_np(m, b, pins):
    """the same as int64 [b + 1], numpy over the cells of a level (the transitions' score matrices are cached on the model)"""
    B1 = b + 1
    widths = np.diff(m.level_off).astype(int)
    edges = getattr(m, "_level_edges", None)
    if edges is None:
        edges = m._level_edges = [None] + [_level_edges(m, l) for l in range(1, m.L)]
    masks = allowed_masks(m, [tuple(int(x) for x in p) for p in pins])
    prev = np.full((1, 1, B1), 0, np.int64)
    for l in range(1, m.L):
        cur = np.full((widths[l], widths[l], B1), NEG_INF, np.int64)
        s_pos, d_pos, w, D = edges[l]
        _relax(prev, cur, s_pos, d_pos, w, D, B1)
        if l in masks:
            cur[~masks[l]] = NEG_INF
        prev = cur
    sink = m.nV - 1 - int(m.level_off[m.L - 1])
    return prev[sink, sink, :].copy()


def brute_force_planes(m, paths, rec, full, b, pins):
    """max over ALL ordered pairs (p, q) of source -> sink paths that satisfy the pins with r(p) + r(q) <= plane, per plane 0..b;
    NEG_INF where there is none.  paths: all of them; rec: their recombinations; full[a][c] = PathModel.score(paths[a], paths[c])[0].
    -> (planes as a list, sat: bool [n, n], sat[a][c] = the ordered pair (paths[a], paths[c]) satisfies the pins)"""
    pins = [tuple(int(x) for x in p) for p in pins]
    P = np.asarray(paths, np.int64)
    n = len(paths)
    sat = np.ones((n, n), bool)
    for l in sorted({p[0] for p in pins}):
        a0, k = int(m.level_off[l]), int(m.level_off[l + 1] - m.level_off[l])
        tab = np.array([[cell_allowed(pins, l, a0 + i, a0 + j) for j in range(k)] for i in range(k)], bool)
        sat &= tab[P[:, l][:, None] - a0, P[:, l][None, :] - a0]
    rsum = np.asarray(rec, np.int64)[:, None] + np.asarray(rec, np.int64)[None, :]
    planes = []
    for plane in range(b + 1):
        ok = sat & (rsum <= plane)
        planes.append(int(np.asarray(full)[ok].max()) if ok.any() else NEG_INF)
    return planes, sat

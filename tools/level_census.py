#!/usr/bin/env python3
"""Census of the levels of a levelized DP graph: python3 tools/level_census.py graph.dpg
How many transitions are 'pure copies' (every destination vertex has exactly one in-edge, of weight 0, and neither level
carries a colour): their sweep is a permutation of the state and their back-pointers are all (0, 0)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from dipgenie_amd import capi
g = capi.DpGraphArrays.load(sys.argv[1])
lo = np.asarray(g.level_off); L = g.n_levels; nV = g.n_vertices
indeg = np.bincount(g.out_dst, minlength=nV)
src = np.repeat(np.arange(nV), np.diff(g.out_off))
w_in = np.zeros(nV, np.int64); np.add.at(w_in, g.out_dst, g.out_w.astype(np.int64))
col = (np.diff(g.hom_off) + np.diff(g.het_off)) > 0
lvl_of = np.repeat(np.arange(L), np.diff(lo))
max_in = np.zeros(L, np.int64); np.maximum.at(max_in, lvl_of, indeg)
min_in = np.full(L, 1 << 30, np.int64); np.minimum.at(min_in, lvl_of, indeg)
w_lvl = np.zeros(L, np.int64); np.add.at(w_lvl, lvl_of, w_in)
c_lvl = np.zeros(L, np.int64); np.add.at(c_lvl, lvl_of, col.astype(np.int64))
width = np.diff(lo)
pure = (max_in[1:] == 1) & (min_in[1:] == 1) & (w_lvl[1:] == 0) & (c_lvl[1:] == 0) & (c_lvl[:-1] == 0)
same_w = width[1:] == width[:-1]
print(f"levels {L}, transitions {L - 1}")
print(f"pure-copy transitions (in-degree 1 everywhere, weight 0, no colour on either level): {int(pure.sum())} = {100 * pure.mean():.1f} %  (of which width unchanged: {int((pure & same_w).sum())})")
runs = np.diff(np.flatnonzero(np.diff(np.concatenate([[0], pure.astype(np.int8), [0]]))))[::2]
if runs.size: print(f"runs of consecutive pure-copy transitions: {runs.size}, mean length {runs.mean():.2f}, max {runs.max()}; a collapsed chain would have {L - 1 - int(pure.sum()) + runs.size} launches")
nocol = (c_lvl[1:] == 0) & (c_lvl[:-1] == 0)
print(f"colourless transitions: {100 * nocol.mean():.1f} %; max in-degree 1: {100 * (max_in[1:] == 1).mean():.1f} %; weight-free: {100 * (w_lvl[1:] == 0).mean():.1f} %")
# level pairs (dipgenie_amd/csrc/dg_dp_pairs.hip): (l - 1, l) run as one composed launch if both levels are lean (no vertex with more than
# 64 in-edges) without a dead column, narrower than 256 with at most 2,047 in-edges, and every vertex of l has a composed in-degree
# (sum over its in-edges p -> v of the in-degree of p) of at most 8; pairs are chosen greedily left to right, disjoint
comp = np.zeros(nV, np.int64); np.add.at(comp, g.out_dst, indeg[src])
max_comp = np.zeros(L, np.int64); np.maximum.at(max_comp, lvl_of, comp)
t_lvl = np.zeros(L, np.int64); np.add.at(t_lvl, lvl_of, indeg)
lvl_ok = (min_in >= 1) & (max_in <= 64) & (width <= 255) & (t_lvl <= 2047)
n_big = np.zeros(L, np.int64); np.add.at(n_big, lvl_of, (comp > 8).astype(np.int64))
for limit in (4, 8, 16, 32):
    n_pairs, l, fanin = 0, 2, []
    while l < L:
        if lvl_ok[l - 1] and lvl_ok[l] and max_comp[l] <= limit:
            n_pairs += 1
            if n_big[l]: fanin.append(l)
            l += 2
        else: l += 1
    rule = {8: " (the rule of pair_levels)", 32: " (the rule of pair_fanin: rows above 8 are big rows)"}.get(limit, "")
    print(f"level pairs, composed in-degree <= {limit}{rule}: {n_pairs} = {100 * n_pairs / (L - 1):.1f} % of the launches; {L - 1 - n_pairs} launches in all")
    if limit == 32 and fanin:
        fanin = np.array(fanin)
        print(f"  of them with a big row: {fanin.size}; big rows per pair p50 / p90 / p99 {np.percentile(n_big[fanin], [50, 90, 99]).astype(int).tolist()}, largest composed in-degree p50 / p90 {np.percentile(max_comp[fanin], [50, 90]).astype(int).tolist()}")
        # the buckets of the measured gate (options pair_fanin_max_big / pair_fanin_max_indeg), greedy under the full rule: a narrower gate re-pairs the levels around the pairs it excludes
        for lo_b, hi_b in ((1, 1), (2, 4), (5, 16), (17, 64), (65, 255)):
            for lo_d, hi_d in ((9, 16), (17, 24), (25, 32)):
                n = int(((n_big[fanin] >= lo_b) & (n_big[fanin] <= hi_b) & (max_comp[fanin] >= lo_d) & (max_comp[fanin] <= hi_d)).sum())
                if n: print(f"    big rows {lo_b}..{hi_b}, largest composed in-degree {lo_d}..{hi_d}: {n} pairs")
# wide levels and wide pairs (options pair_wide / pair_wide_fanin / pair_wide_max_width): a level wider than 255 pairs only in the wide
# layout, whose three levels -- the source level too -- are at most `cap` wide; everything else as shipped (composed in-degree <= 32, at
# most 4 big rows; greedy from the left)
wide = width > 255
cells = width.astype(np.int64) ** 2
wruns = np.diff(np.flatnonzero(np.diff(np.concatenate([[0], wide.astype(np.int8), [0]]))))[::2]
print(f"levels wider than 255: {int(wide.sum())} of {L - 1} = {100 * wide.sum() / (L - 1):.1f} %, holding {100 * cells[wide].sum() / cells.sum():.1f} % of all cells; widest level {int(width.max())}, most in-edges in one level {int(t_lvl.max())}")
if wruns.size: print(f"  in {wruns.size} runs, mean length {wruns.mean():.1f} (p90 {int(np.percentile(wruns, 90))}, max {int(wruns.max())})")
def greedy(cap, light_wide):
    ok = (min_in >= 1) & (max_in <= 64) & (t_lvl <= 2047)
    out, l = [], 2
    while l < L:
        lv_wide = width[l - 1] > 255 or width[l] > 255
        layout = lv_wide or 255 < width[l - 2] <= cap
        fits = ok[l - 1] and ok[l] and max(width[l - 1], width[l]) <= (cap if cap else 255) and not (lv_wide and width[l - 2] > cap)
        if fits and max_comp[l] <= 32 and n_big[l] <= 4 and not (layout and light_wide and n_big[l]):
            out.append((l, bool(layout) and cap > 0))
            l += 2
        else: l += 1
    return out
base = greedy(0, False)
print(f"level pairs as shipped without wide pairs (composed in-degree <= 32, at most 4 big rows): {len(base)}; {L - 1 - len(base)} launches in all")
for cap in (511, 1023):
    for light_wide in (False, True):
        ch = greedy(cap, light_wide)
        wl = np.array([l for (l, w) in ch if w], np.int64)
        mid_cells = cells[wl - 1].sum() if wl.size else 0
        light = int((max_comp[wl] <= 8).sum()) if wl.size else 0
        src_only = int(((width[wl - 1] <= 255) & (width[wl] <= 255)).sum()) if wl.size else 0      # wide by their source level alone
        print(f"  width <= {cap}{', wide pairs only when light' if light_wide else ''}: {len(ch)} pairs, {L - 1 - len(ch)} launches; {wl.size} in the wide layout ({light} of them light, {src_only} by their source level alone), their middle levels hold {100 * mid_cells / cells.sum():.1f} % of all cells")

"""CPU: graphgen.recolour and the graphs of colour_graphs.py -- that the cases of tests/test_gpu_colour_lists.py reach what their
names claim, from the arrays and the oracle alone, so that the GPU test cannot become vacuous when a seed or the generator
changes.  This file also pins recolour()'s seeded output (sha256, as tests/test_sweep_variant_graphs.py does for
random_levelized)."""
import hashlib

import numpy as np
import pytest

import colour_graphs as cg
import graphgen
import oracle_py as orc
import sweep_variant_graphs as sv
from dipgenie_amd.capi import DpGraphArrays
from paths_model import PathModel

ALL = [(topo, case) for topo in cg.SWEEP_TOPOLOGIES for case in cg.CASES] + [("small", case) for case in cg.PATH_CASES]
# sha256 over R and the eight arrays (name, dtype, bytes)
RECORDED = {
    ("w30", "mixed"): "2201f4bab852cb40a9781f6d255423690518e27b9c7cad65f3438735cae81e14",
    ("lean", "extreme_ids"): "7ed79f3dc6c2c64430b0e9271ffa5ba66634544d7bf224c0ba93b2814a918b70",
    ("small", "disjoint_big"): "d725f1c376586c6fd677b3b4a766f81706f6e2ad2c20f448d5413a3968bd1716",
}


def _digest(g):
    h = hashlib.sha256(str(g.R).encode())
    for n in DpGraphArrays.NAMES:
        a = getattr(g, n)
        h.update(n.encode())
        h.update(str(a.dtype).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def _well_formed(g):
    """sorted-unique lists, hom and het ids disjoint, ids in the non-negative int32 range"""
    for off, col in ((g.hom_off, g.hom_col), (g.het_off, g.het_col)):
        assert off[0] == 0 and off[-1] == col.size and (np.diff(off) >= 0).all() and col.dtype == np.int32
        inner = np.ones(col.size, bool)
        inner[off[:-1][np.diff(off) > 0]] = False                          # the first id of every list has no predecessor in it
        assert (np.diff(col.astype(np.int64), prepend=-1)[inner] > 0).all()
        assert col.size == 0 or col.min() >= 0
    assert np.intersect1d(g.hom_col, g.het_col).size == 0


@pytest.mark.parametrize("topo,case", ALL)
def test_lists_are_well_formed_and_the_topology_is_kept(topo, case):
    g = cg.graph(topo, case)
    _well_formed(g)
    t = cg.topology(topo, big=(case == "disjoint_big"))
    for n in ("level_off", "out_off", "out_dst", "out_w"):
        assert np.array_equal(getattr(g, n), getattr(t, n)), n
    assert g.R == t.R
    if case == "hom_only":
        assert g.het_col.size == 0 and g.hom_col.size > 0
    if case in ("het_only", "disjoint_big"):
        assert g.hom_col.size == 0 and g.het_col.size > 0
    if case == "extreme_ids":                                                # 0 and 2^31 - 1 (what union2x2 starts its running minimum from) are
        both = np.concatenate([g.hom_col, g.het_col])                       # listed, the latter in hom lists on two topologies, in het lists on the others
        assert both.min() == 0 and both.max() == 2 ** 31 - 1
        assert (g.hom_col.max() == 2 ** 31 - 1) == (topo in ("w65", "general"))
    if case == "identical":
        hom, het = cg.lists(g)
        assert all(np.array_equal(x, hom[0]) for x in hom) and all(np.array_equal(x, het[0]) for x in het) and len(hom[0]) == len(het[0]) == 300
    if case == "disjoint_big":
        n = np.diff(g.het_off)
        assert set(np.unique(n)) <= {0} | set(range(9000, 10001)) and np.unique(g.het_col).size == g.het_col.size          # pairwise disjoint
        lvl = np.searchsorted(g.level_off, np.flatnonzero(n), side="right") - 1
        assert np.bincount(lvl).max() <= 2 and len(set(lvl)) == g.n_levels - 2


def test_the_same_seed_gives_the_same_arrays():
    t = cg.topology("lean")
    a, b = graphgen.recolour(t, 77, **cg.CASES["mixed"]), graphgen.recolour(t, 77, **cg.CASES["mixed"])
    assert _digest(a) == _digest(b) != _digest(graphgen.recolour(t, 78, **cg.CASES["mixed"]))
    assert _digest(graphgen.recolour_disjoint_big(t, 5)) == _digest(graphgen.recolour_disjoint_big(t, 5)) != _digest(graphgen.recolour_disjoint_big(t, 6))
    assert _digest(t) == _digest(cg.topology("lean"))                       # (recolour leaves its argument alone)
    for key, want in RECORDED.items():
        assert _digest(cg.graph(*key)) == want, key


def test_generator_arguments():
    t = cg.topology("small")
    g = graphgen.recolour(t, 1, p_empty=0.0, p_short=1.0, pool=50, R=9)
    assert g.R == 9 and set(np.diff(g.hom_off)) <= {1, 2, 3, 4} and set(np.diff(g.het_off)) <= {1, 2, 3, 4}
    assert g.hom_col.max() < 50 <= g.het_col.min() and g.het_col.max() < 100
    g = graphgen.recolour(t, 1, p_empty=0.0, p_short=0.0, long_range=(20, 30), pool=50, hom_high=True)
    assert g.het_col.max() < 50 <= g.hom_col.min() and 20 <= np.diff(g.hom_off).min() <= np.diff(g.hom_off).max() <= 30
    g = graphgen.recolour(t, 1, p_empty=1.0)
    assert g.hom_col.size == g.het_col.size == 0
    m = graphgen.spread_ids(7)
    assert m[0] == 0 and m[-1] == 2 ** 31 - 1 and (np.diff(m) > 0).all() and m.size == 14
    with pytest.raises(AssertionError):
        graphgen.recolour(t, 1, pool=50, long_range=(20, 30), id_map=np.zeros(100, np.int64))           # not increasing


@pytest.mark.parametrize("topo,case", ALL)
def test_the_largest_delta_is_in_the_intended_band(topo, case):
    """over every pair of edges of every transition; the matrix entries are checked against the oracle's two set functions at the
    maximum and at sampled pairs, and one transition of the small graphs entry by entry against PathModel"""
    g = cg.graph(topo, case)
    top, (l, e, f), classes = cg.largest_delta(g)
    lo, hi = cg.BANDS[case]
    print(f"{topo} {case}: largest delta {top} at level {l} edges ({e}, {f}); edge pairs without / with one / with two coloured edges {classes.tolist()}")
    assert lo <= top <= hi, (top, lo, hi)
    if case == "mixed":
        assert (classes > 0).all(), classes                                  # all three pair classes of the delta kernel
    if case in ("long", "identical"):
        assert classes[2] > 0.9 * classes.sum()                              # most vertices coloured
    hom, het = cg.lists(g)
    ptr = lambda x: (np.ascontiguousarray(x, np.int32).ctypes.data if len(x) else None, len(x))
    rng = np.random.default_rng(3)
    for lvl in sorted({l, 1, g.n_levels // 2, g.n_levels - 1}):
        delta, symd, _ = graphgen.transition_deltas(g, lvl)
        a0, a1 = int(g.level_off[lvl - 1]), int(g.level_off[lvl])
        src = np.repeat(np.arange(a0, a1), np.diff(g.out_off[a0:a1 + 1]))
        dst = g.out_dst[g.out_off[a0]:g.out_off[a1]]
        assert np.array_equal(delta, delta.T)
        pairs = [(e, f)] if lvl == l else []
        pairs += [tuple(int(x) for x in rng.integers(0, src.size, 2)) for _ in range(25)]
        for x, y in pairs:
            u1, v1, u2, v2 = int(src[x]), int(src[y]), int(dst[x]), int(dst[y])
            inter = orc.lib.orc_inter_union2x2(*ptr(hom[u1]), *ptr(hom[v1]), *ptr(hom[u2]), *ptr(hom[v2]))
            sd = orc.lib.orc_symdiff_union2x2(*ptr(het[u1]), *ptr(het[v1]), *ptr(het[u2]), *ptr(het[v2]))
            assert (int(delta[x, y]), int(symd[x, y])) == (inter + sd, sd), (lvl, x, y)
    if topo == "small":
        m = PathModel(g)
        lvl = g.n_levels // 2
        delta, symd, _ = graphgen.transition_deltas(g, lvl)
        a0, a1 = int(g.level_off[lvl - 1]), int(g.level_off[lvl])
        src = np.repeat(np.arange(a0, a1), np.diff(g.out_off[a0:a1 + 1]))
        dst = g.out_dst[g.out_off[a0]:g.out_off[a1]]
        for x in range(src.size):
            for y in range(src.size):
                d = m.delta(int(src[x]), int(src[y]), int(dst[x]), int(dst[y]))
                assert (int(delta[x, y]), int(symd[x, y])) == (d[0] + d[1], d[1])


@pytest.mark.parametrize("topo", list(cg.TOPOLOGIES))
def test_oracle_runs_are_affordable_and_not_trivial(topo):
    cases = cg.PATH_CASES if topo == "small" else list(cg.CASES)
    for case in cases:
        g, ref = cg.graph(topo, case), cg.oracle(topo, case)
        print(f"{topo} {case}: oracle {ref['seconds']:.2f} s, value {ref['value']}, s_het {ref['s_het']}, recombinations {sv.recombinations(ref)}")
        assert ref["seconds"] < 10.0
        assert (ref["digest"][1:] != 0).all()                                # every level has a reachable cell
        lo, _ = cg.BANDS[case]
        assert ref["value"] > lo                                             # the optimum crosses transitions of the band
    if topo in cg.VARIANT_TOPOLOGIES or topo == "small":
        for case in cg.PATH_CASES:
            g = cg.graph(topo, case)
            assert len(set(cg.planes(topo, case))) >= 2, cg.planes(topo, case)   # the sink's value depends on the budget
            if topo != "small":
                deg = sv.in_degrees(g)
                kinds = {(bool(d.max() > 64), bool(d.max() > 8)) for d in deg}
                assert max(int(d.max()) for d in deg) <= 255 and (True, True) in kinds and ((False, False) in kinds or (False, True) in kinds), kinds


@pytest.mark.parametrize("M,value,s_het", [(10922, 109220, 87376), (10923, 109230, 87384), (16383, 163830, 131064)])
def test_delta_bound_graph(M, value, s_het):
    g = graphgen.delta_bound_graph(M)
    _well_formed(g)
    assert np.diff(g.hom_off).max() == np.diff(g.het_off).max() == M
    ref = orc.dp_solve(g)
    assert (ref["value"], ref["s_het"]) == (value, s_het) == (10 * M, 8 * M)
    delta, symd, _ = graphgen.transition_deltas(g, 2)                         # the middle transition: edges 1 -> 3 and 2 -> 4
    assert delta[0, 1] == delta.max() == 6 * M and symd[0, 1] == 4 * M
    assert delta[0, 0] == 2 * M                                              # one edge with itself: Hom(1) and Hom(3) are disjoint, Het(1) /\\ Het(3)
    for hom, het, want in ((True, False, (2 * M, 0)), (False, True, (8 * M, 8 * M))):
        ref = orc.dp_solve(graphgen.delta_bound_graph(M, hom=hom, het=het))
        assert (ref["value"], ref["s_het"]) == want
    one = graphgen.delta_bound_graph(M, het=False, only=(1,))
    assert list(np.diff(one.hom_off)) == [0, M, 0, 0, 0, 0] and one.het_col.size == 0

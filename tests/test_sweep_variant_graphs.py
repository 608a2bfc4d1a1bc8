"""CPU: the graph generator's widths= argument, and the properties that tests/test_gpu_sweep_variant_parity.py relies on in the
graphs of sweep_variant_graphs.py -- from the arrays and the oracle alone, so that the GPU test cannot become vacuous when a
seed or the generator changes."""
import hashlib

import numpy as np

import graphgen
import sweep_variant_graphs as sv
from dipgenie_amd.capi import DpGraphArrays

# sha256 over R and the eight arrays (name, dtype, bytes) of seeded calls that other tests make, recorded from the generator as it
# was before it had widths=
RECORDED = [
    (7002, dict(max_width=40, n_levels=60, R=18, p_w1=0.5), "da8e19787c3423cdc01d68cc7a91393c211c1899b9566b462b6748dfdec31adf"),
    (9717, dict(min_width=15, max_width=18, n_levels=40, R=7, p_colour=0.6), "a8ef82915cac3ae846c1bc2e86370cb30e59a8dd9d5b6e53057eeec7e0c4072d"),
    (9112, dict(max_width=3, n_levels=6, R=1, extra_edges=300.0, dup_edges=False), "b109dc09e4a40af6749088dfdff5acbf9101b6ee5ef7fcf6a6d475117eb45b0d"),
    (9900, {}, "1817e4f4f765d3b2d58757103794305cdb42155cbbfe6530a881bef7e357f15f"),
]


def _digest(g):
    h = hashlib.sha256(str(g.R).encode())
    for n in DpGraphArrays.NAMES:
        a = getattr(g, n)
        h.update(n.encode())
        h.update(str(a.dtype).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def test_seeded_calls_give_the_arrays_they_always_gave():
    for seed, kw, want in RECORDED:
        assert _digest(graphgen.random_levelized(seed, **kw)) == want, (seed, kw)


def test_widths_are_prescribed():
    widths = [1, 7, 1, 33, 2, 1]
    g = graphgen.random_levelized(5, widths=widths, R=3, n_levels=99, max_width=2)
    assert list(np.diff(g.level_off)) == widths and g.n_levels == 6 and g.R == 3
    lvl = np.searchsorted(g.level_off, np.arange(g.n_vertices), side="right") - 1
    src = np.repeat(np.arange(g.n_vertices), np.diff(g.out_off))
    assert np.array_equal(lvl[g.out_dst], lvl[src] + 1)                      # edges to the next level only
    assert (np.diff(g.out_off)[:-1] >= 1).all() and g.out_off[-1] == g.out_off[-2]
    assert _digest(g) == _digest(graphgen.random_levelized(5, widths=widths, R=3))
    assert _digest(g) != _digest(graphgen.random_levelized(6, widths=widths, R=3))


def test_the_variant_graphs_have_what_the_gpu_test_needs():
    met = {}
    for fam in sv.FAMILIES:
        cases = [c for c in sv.GRAPHS if sv.family(c) == fam]
        assert {7, 9, 18, 20, 32} <= {sv.GRAPHS[c][3] for c in cases}
        degs = {c: sv.in_degrees(sv.graph(c)) for c in cases}
        refs = {c: sv.oracle_per_budget(c) for c in cases}
        # 1. every level's oracle digest is nonzero (a level without a reachable cell would compare nothing)
        for c in cases:
            assert (refs[c][-1]["digest"][1:] != 0).all(), c
        # 2. a destination level with more than 8 rows of more than 8 in-edges (more heavy rows than ride in the kernel arguments)
        met[fam, 2] = max(int((d > 8).sum()) for c in cases for d in degs[c])
        assert met[fam, 2] > 8
        # 3. a row of 9, 10 or 11 in-edges (uneven quarters of the cooperative split)
        met[fam, 3] = sorted({int(x) for c in cases for d in degs[c] for x in d if 9 <= x <= 11})
        assert met[fam, 3]
        # 4. (general) a vertex of 65..255 in-edges, none above 255 (which would send the level to the generic kernel) -- the lean family's sink has one too
        top = max(int(d.max()) for c in cases for d in degs[c])
        assert 65 <= top <= 255, (fam, top)
        # 5. an optimum of 4 or more recombinations
        met[fam, 5] = max(sv.recombinations(refs[c][-1]) for c in cases)
        assert met[fam, 5] >= 4
        # 6. the sink's value differs between at least three budgets
        met[fam, 6] = max(len({ref["value"] for ref in refs[c]}) for c in cases)
        assert met[fam, 6] >= 3
        assert all(len({ref["value"] for ref in refs[c]}) >= 3 for c in cases)   # (in fact in every graph: the plane comparison is nowhere trivial)
        # 7. every oracle run takes under 2 s
        met[fam, 7] = max(ref["seconds"] for c in cases for ref in refs[c])
        assert met[fam, 7] < 2.0
        # what the expected launch profiles assume: each graph has lean levels without heavy rows and a general level; the lean family lean levels with heavy rows
        for c in cases:
            kinds = {(bool(d.max() > 64), bool(d.max() > 8)) for d in degs[c]}
            assert (True, True) in kinds and (False, False) in kinds, (c, kinds)
            assert fam != "lean" or (False, True) in kinds, (c, kinds)
    # the general family at its plain widths: rows of at most two in-edges, rows of more, dead columns, all in a lean level
    for c in ("general-R7", "general-R9"):
        assert any(d.max() <= 64 and (d == 0).any() and (d > 2).any() and ((d > 0) & (d <= 2)).any() for d in sv.in_degrees(sv.graph(c))), c
    assert any((d == 64).any() for d in sv.in_degrees(sv.graph("general-R9")))          # the largest column that is not giant
    print("conditions met:", {f"{f}.{q}": (round(v, 3) if isinstance(v, float) else v) for (f, q), v in met.items()})

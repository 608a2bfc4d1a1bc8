"""-m gpu: the chain walkers of dg_dp_trace.hip against the oracle's walk, level by level.

dp_answer_paths(b) after dp_run_budgets must EQUAL oracle_py.dp_paths on the same arrays with g.R = b, row for row and vertex for
vertex, and the outcome's key the oracle's key -- on the scripted graphs of tests/trace_graphs.py, where the script decides what the
walk meets on every level: back-pointer ranks 0, 1, 2 and 3 on either haplotype, weight-1 hops on one or both, merged (i == j) cells,
vertices with a single in-edge (the lean walk's all-ones guard word) and levels whose two predecessors tie, each of them on every slot
of the walkers' 8-step unroll and on both sides of the 56-level batches.  tests/test_trace_graphs.py establishes all of that on the
CPU, and pins the oracle's paths to an independent model.

Both walkers (lean_chain 1 / 0) on every narrow graph at every budget; lattices cut into one level per chunk and per segment, so that
every level is the first and the last of a launch with the walk's state carried over, and cut at a fifth and a seventh; chains dealt
to groups of uneven size; the general walker's wide branch (wide -> wide, wide -> narrow, narrow -> wide, at a batch edge, at both
ends of the walk, on a merged level), and an in-edge list of 255 entries (the longest that stays narrow) next to one of 256.  Nothing
the library exposes says which walker ran, so the 255 | 256 pair is compared by its answers only.

Not covered here: the helper prefetch groups (they only issue hints, no result depends on them); lattices with 64-bit level offsets
or RP * k >= 2^24 (the other reasons the lean walk declines -- both need graphs far beyond a few seconds).  No test here damages a
lattice."""
import random

import numpy as np
import pytest

import trace_graphs as tg

pytestmark = pytest.mark.gpu

COMPARED = {"paths": 0}


def spot(g):
    """the budgets that the modes beyond the plain one are checked at"""
    return [0, 1, g.R // 2, g.R - 1, g.R]


def first_difference(name, got, want):
    """where a walked pair of paths leaves the oracle's, seen from the sink (the walk's direction): level, slot, scripted class, the
    oracle's hop into the level above it"""
    g, info = tg.graph(name)
    bad = np.flatnonzero((got != want).any(axis=0))
    if bad.size == 0:
        return None
    l = int(bad[-1])
    hop = tg.hop_classes(g, want)[0][l + 1] if l + 1 < g.n_levels and (want >= 0).all() else None
    return dict(level=l, slot=tg.slot(l), scripted=info["cls"][l], decoded_by_hop_into=l + 1, its_class=info["cls"][l + 1] if l + 1 < g.n_levels else None,
                its_hop=hop, got=got[:, l].tolist(), want=want[:, l].tolist())


def check(ctx, name, budgets, outs, mode):
    """every listed budget of the run that gave `outs`: key and whole paths against the oracle"""
    g = tg.graph(name)[0]
    for b, out in zip(budgets, outs):
        key, want = tg.oracle_at(name, b)
        assert out.key() == key, (name, mode, b, out.key(), key)
        got = ctx.dp_answer_paths(b)
        assert got.shape == (2, g.n_levels) and got.dtype == np.int32
        assert np.array_equal(got, want), (name, mode, b, first_difference(name, got, want))
        COMPARED["paths"] += 1


@pytest.mark.parametrize("lean", [1, 0])
@pytest.mark.parametrize("name", tg.NARROW)
def test_every_budget_both_walkers(gpu_ctx, name, lean):
    g = tg.graph(name)[0]
    budgets = list(range(g.R + 1))
    with gpu_ctx.dp_options(lean_chain=lean):
        gpu_ctx.dp_load_graph(g)
        outs = gpu_ctx.dp_run_budgets(budgets)
        t = gpu_ctx.dp_timing()
        assert (t.n_chunks, t.n_segments) == (1, 1)
        check(gpu_ctx, name, budgets, outs, dict(lean=lean))
    gpu_ctx.dp_load_graph(g)
    print("paths compared so far:", COMPARED["paths"])


@pytest.mark.parametrize("lean", [1, 0])
@pytest.mark.parametrize("name", tg.NARROW)
def test_chunk_and_segment_edges(gpu_ctx, name, lean):
    g = tg.graph(name)[0]
    cells = sum(int(k) * int(k) for k in np.diff(g.level_off)[1:]) * (g.R + 1)       # lattice cells: (R + 1) planes of k2 * k2 per destination level
    budgets = spot(g)
    n_dest = g.n_levels - 1
    modes = [dict(lattice_chunk_cells=1), dict(segment_cells=1)]
    for plane_limit in (1, 0):
        modes += [dict(lattice_chunk_cells=max(2, cells // 5), plane_limit=plane_limit), dict(segment_cells=max(1, cells // 7), plane_limit=plane_limit)]
    for mode in modes:
        with gpu_ctx.dp_options(lean_chain=lean, **mode):
            gpu_ctx.dp_load_graph(g)
            outs = gpu_ctx.dp_run_budgets(budgets)
            t = gpu_ctx.dp_timing()
            # the chunks that trace_graphs.chunks() derives from the level sizes: at 1 every level but the sink's (one cell per plane, it joins the
            # level before it) is a chunk of its own; a segment is one chunk
            want = len(tg.chunks(g, mode.get("lattice_chunk_cells", mode.get("segment_cells"))))
            assert want >= (n_dest - 2 if mode in modes[:2] else 5), (mode, want)
            assert t.n_chunks == want and t.n_segments == (want if "segment_cells" in mode else 1), (mode, t.n_chunks, t.n_segments, want)
            check(gpu_ctx, name, budgets, outs, dict(lean=lean, **mode))
    gpu_ctx.dp_load_graph(g)
    print("paths compared so far:", COMPARED["paths"])


@pytest.mark.parametrize("lean", [1, 0])
@pytest.mark.parametrize("name", ["phi0", "phi3m", "phi7", "phi12m"])
def test_chain_placement(gpu_ctx, name, lean):
    """1, 8, 9 and 17 budgets in shuffled order (the host deals the chains into at most 8 groups: one group, eight of one chain, then groups of
    uneven size and more chains than groups), then a plain run; every chain's path, found by its budget"""
    g = tg.graph(name)[0]
    rnd = random.Random(g.R * 7 + lean)
    with gpu_ctx.dp_options(lean_chain=lean):
        gpu_ctx.dp_load_graph(g)
        for n in (1, 8, 9, 17):
            budgets = rnd.sample(range(g.R + 1), n)
            outs = gpu_ctx.dp_run_budgets(budgets)
            check(gpu_ctx, name, budgets, outs, dict(lean=lean, n=n, budgets=budgets))
        out = gpu_ctx.dp_run()
        check(gpu_ctx, name, [g.R], [out], dict(lean=lean, plain_run=True))
    gpu_ctx.dp_load_graph(g)
    print("paths compared so far:", COMPARED["paths"])


@pytest.mark.parametrize("name", tg.WIDE + tg.RANKED)
def test_wide_levels_and_the_longest_narrow_list(gpu_ctx, name):
    g = tg.graph(name)[0]
    budgets = spot(g)
    leans = [1, 0] if name == "rank254" else [1]         # lean_chain = 1 is the default: a graph with a wide level goes to the general walker by itself
    for lean in leans:
        for mode in ({}, dict(lattice_chunk_cells=1)):
            with gpu_ctx.dp_options(lean_chain=lean, **mode):
                gpu_ctx.dp_load_graph(g)
                outs = gpu_ctx.dp_run_budgets(budgets)
                t = gpu_ctx.dp_timing()
                if mode:                                 # the chunks in which tests/test_trace_graphs.py places every wide level first and last
                    assert t.n_chunks == len(tg.chunks(g, 1)) > 30 and t.n_segments == 1, (name, t.n_chunks, len(tg.chunks(g, 1)))
                else:
                    assert (t.n_chunks, t.n_segments) == (1, 1)
                check(gpu_ctx, name, budgets, outs, dict(lean=lean, **mode))
    if name.startswith("rank254"):                       # 255 in-edges and 256: the same vertices (both are the base graph's walk)
        other = "rank254-wide" if name == "rank254" else "rank254"
        for b in budgets:
            assert np.array_equal(tg.oracle_at(name, b)[1], tg.oracle_at(other, b)[1])
    gpu_ctx.dp_load_graph(g)
    print("paths compared so far:", COMPARED["paths"])

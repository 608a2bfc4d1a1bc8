"""-m gpu: the level-pair kernels against the oracle, cell by cell.

tests/test_gpu_pair_levels.py sees a pair launch through the answer and the sink's planes only.  Here every graph of
pair_graphs.CELL_CASES (tests/test_pair_graphs.py holds their properties on the CPU) runs under pair_min = 1 at every chunk size of
Context.dp_pair_variants(), forced by option test_force_pair_rc:
  digest = 1, pair_digest = 1: the pair launches stay and take the kernel's digest form.  dp_level_digest equals the oracle's at every
      level that is not the earlier level of a pair (value, middle row and middle column of EVERY reachable cell of a later level,
      and which cells are reachable), is exactly 0 at the earlier levels (never materialised) and non-zero at the later ones
      (pair_graphs.UNREACHABLE_PAIRED lists the planes that cannot reach one); value, s_het and both edge lists equal the oracle's;
  digest = 0 (the instantiations the product runs): dp_run_budgets over the budgets 0..R equals the oracle solved per budget.
Every run must show exactly the expected pair launches, all of the forced chunk size, and single launches for the remaining levels:
no case passes unpaired.  All comparisons are integer equality."""
import re

import numpy as np
import pytest

import oracle_py as orc
import pair_graphs as pg
from dipgenie_amd import capi

pytestmark = pytest.mark.gpu

PAIR_VARIANTS = capi.Context.dp_pair_variants()
RCS = [int(re.fullmatch(r"dp_sweep_pair_kernel<(\d+)>", name).group(1)) for name in PAIR_VARIANTS]
_LAUNCHED = {1: set(), 0: set()}                            # pair kernels launched by this module with digests on / off, for the last test
_GRAPHS, _ORACLE, _PER_BUDGET = {}, {}, {}                  # per case name; solved once


def _graph(name, build):
    if name not in _GRAPHS:
        _GRAPHS[name] = build()
    return _GRAPHS[name]


def _oracle(name, g):
    if name not in _ORACLE:
        _ORACLE[name] = orc.dp_solve(g, want_digest=True)
    return _ORACLE[name]


def _per_budget(name, g):
    if name not in _PER_BUDGET:
        _PER_BUDGET[name] = {b: _answer_of(orc.dp_solve(pg.with_R(g, b))) for b in pg.budgets_checked(g)}
    return _PER_BUDGET[name]


def _answer_of(ref):
    return (ref["value"], ref["s_het"], ref["p1"], ref["p2"])


def _answer(out):
    return (out.value, out.s_het, out.p1, out.p2)


def _check_profiles(ctx, g, pairs, rc, digest, what):
    """exactly len(pairs) pair launches, all of chunk size rc; every other level a single launch"""
    got, singles, n_launch = ctx.dp_pair_profile(), ctx.dp_launch_profile(), int(ctx.dp_timing().n_forward_launches)
    assert got == ({f"dp_sweep_pair_kernel<{rc}>": len(pairs)} if pairs else {}), (what, got)
    assert sum(singles.values()) == g.n_levels - 1 - 2 * len(pairs) and n_launch == g.n_levels - 1 - len(pairs), (what, singles, n_launch)
    _LAUNCHED[digest].update(got)


def _want_digests(ref, pairs):
    want = ref["digest"].copy()
    want[[l - 1 for l in pairs]] = 0                        # the earlier level of a pair: the 0 of the run's memset
    return want


def _check_digests(ctx, g, ref, pairs, what, unreachable=()):
    got, want = ctx.dp_level_digest(g.n_levels), _want_digests(ref, pairs)
    assert np.array_equal(got[1:], want[1:]), (what, "first level that differs", 1 + int(np.argmax(got[1:] != want[1:])))
    assert [l for l in pairs if got[l] == 0] == list(unreachable), what


def _digest_run(ctx, g, ref, pairs, rc, what, unreachable=(), passes=1, **opts):
    with ctx.dp_options(pair_min=1, digest=1, pair_digest=1, test_force_pair_rc=rc, **opts):
        ctx.dp_load_graph(g)
        for _ in range(passes):
            out = ctx.dp_run()
            assert _answer(out) == _answer_of(ref), what
            _check_digests(ctx, g, ref, pairs, what, unreachable)
            _check_profiles(ctx, g, pairs, rc, 1, what)


def _budget_run(ctx, g, per_budget, pairs, rc, what, **opts):
    with ctx.dp_options(pair_min=1, digest=0, test_force_pair_rc=rc, **opts):
        ctx.dp_load_graph(g)
        outs = ctx.dp_run_budgets(list(per_budget))
        _check_profiles(ctx, g, pairs, rc, 0, what)
    for b, out in zip(per_budget, outs):
        assert _answer(out) == per_budget[b], (what, "budget", b)


def test_the_chunk_sizes_are_the_pair_variants(gpu_ctx):
    assert PAIR_VARIANTS == gpu_ctx.dp_pair_variants() and RCS == sorted(set(RCS)) and len(RCS) >= 1
    g = pg.long_graph()
    with gpu_ctx.dp_options(pair_min=1):
        gpu_ctx.dp_solve(g)
        free = gpu_ctx.dp_pair_profile()
        for n in (3, 8, max(RCS) + 1):                      # no chunk size of the pair kernel: the cost model stays in charge
            assert n not in RCS
            with gpu_ctx.dp_options(test_force_pair_rc=n):
                gpu_ctx.dp_solve(g)
                assert gpu_ctx.dp_pair_profile() == free and sum(free.values()) == 4


@pytest.mark.parametrize("digest", [1, 0])
@pytest.mark.parametrize("name", list(pg.CELL_CASES))
def test_every_cell_of_a_paired_level(gpu_ctx, name, digest):
    build, pairs = pg.CELL_CASES[name]
    g = _graph(name, build)
    assert len(pairs) >= 1
    for rc in RCS:
        if digest:
            _digest_run(gpu_ctx, g, _oracle(name, g), pairs, rc, (name, rc), pg.UNREACHABLE_PAIRED.get(name, ()))
        else:
            _budget_run(gpu_ctx, g, _per_budget(name, g), pairs, rc, (name, rc))


@pytest.mark.parametrize("name", list(pg.REFUSED_TWINS))
def test_refused_twins_run_that_level_singly(gpu_ctx, name):
    """the pairs that remain are launched; the refused level and the one before it carry the oracle's (non-zero) digests, which only
    single launches write"""
    build, pairs, refused = pg.REFUSED_TWINS[name]
    g = _graph(name, build)
    ref = _oracle(name, g)
    assert refused not in pairs and refused - 1 not in pairs and ref["digest"][refused] != 0 and ref["digest"][refused - 1] != 0
    for rc in RCS:
        _digest_run(gpu_ctx, g, ref, pairs, rc, (name, rc))
    _budget_run(gpu_ctx, g, _per_budget(name, g), pairs, RCS[0], name)


def test_replays_leave_the_accumulator_to_the_memset(gpu_ctx):
    """plain launches, the default batch, batches of 3 levels (the pair (3, 4) straddles a batch edge and runs as two single launches,
    so level 3 has its digest); three passes each: the second and third replay the captured batches and must not add to the first's"""
    g = pg.long_graph()
    ref = _oracle("long", g)
    for gb, pairs in ((0, [2, 4, 6, 8]), (-1, [2, 4, 6, 8]), (3, [2, 6, 8])):
        for rc in RCS:
            _digest_run(gpu_ctx, g, ref, pairs, rc, ("long", gb, rc), passes=3, graph_batch=gb)


NT_CASES = [f"rank-{a}x{b}/both" for a, b in pg.RANK_MIXES] + ["plane-19-mixed/both", "plane-41-w1/first", "plane-7-w0/second", "plane-3-mixed/neither"]


@pytest.mark.parametrize("name", NT_CASES)
def test_non_temporal_back_pointer_stores(gpu_ctx, name):
    """bp_nt_min_cells = 1: every level streams the back-pointers of its own cells non-temporally"""
    build, pairs = pg.CELL_CASES[name]
    g = _graph(name, build)
    for rc in RCS:
        _digest_run(gpu_ctx, g, _oracle(name, g), pairs, rc, (name, rc), pg.UNREACHABLE_PAIRED.get(name, ()), bp_nt_min_cells=1)
        _budget_run(gpu_ctx, g, _per_budget(name, g), pairs, rc, (name, rc), bp_nt_min_cells=1)


def test_every_pair_variant_was_compared():
    """runs last in the module: with digests on and with them off, the names launched above are all of dp_pair_variants()"""
    for digest in (1, 0):
        assert _LAUNCHED[digest] == set(PAIR_VARIANTS), (digest, sorted(_LAUNCHED[digest]))

"""-m gpu: fan-in pairs -- level pairs whose later level has rows of composed in-degree 9..32, swept by dp_sweep_pair_coop_kernel -- against
the oracle.  Every graph of pair_fanin_graphs.CASES (tests/test_pair_fanin_graphs.py holds their properties on the CPU) runs under
pair_min = pair_fanin_min = 1 and pair_fanin_max_big = 255 at each chunk size (test_force_pair_rc = 1, 2, 4):
  digest = 1, pair_digest = 1: every level that is not the earlier level of a pair shows the oracle's digest (value, reachability and
      middle cell of EVERY cell of a later level), the earlier levels the 0 of the run's memset; value, s_het and both edge lists equal;
  digest = 0 (the instantiations the product runs): dp_run_budgets over every budget 0..R equals the oracle solved per budget -- the
      walks pin the back-pointers of both levels.
The pair profile must be the one the model of the pairing rule gives.  All comparisons are integer equality."""
import numpy as np
import pytest

import oracle_py as orc
import pair_fanin_graphs as fg
import pair_graphs as pg

pytestmark = pytest.mark.gpu

RCS = (1, 2, 4)
FORCED = dict(pair_min=1, pair_fanin_min=1, pair_fanin_max_big=255)      # (the shipped gate of 4 big rows: test_the_gates)
_G, _ORACLE, _PER_BUDGET = {}, {}, {}


def _graph(name):
    if name not in _G:
        _G[name] = (fg.CASES.get(name) or fg.REFUSED[name])[0]()
    return _G[name]


def _oracle(name):
    if name not in _ORACLE:
        _ORACLE[name] = orc.dp_solve(_graph(name), want_digest=True)
    return _ORACLE[name]


def _answer_of(ref):
    return (ref["value"], ref["s_het"], ref["p1"], ref["p2"])


def _answer(out):
    return (out.value, out.s_het, out.p1, out.p2)


def _per_budget(name):
    if name not in _PER_BUDGET:
        g = _graph(name)
        _PER_BUDGET[name] = [_answer_of(orc.dp_solve(pg.with_R(g, b))) for b in range(g.R + 1)]
    return _PER_BUDGET[name]


def _check_profiles(ctx, g, rc, what, **rule):
    want, chosen = fg.pair_profile(g, rc, **rule), fg.choose_pairs(g, **rule)
    got, singles, n_launch = ctx.dp_pair_profile(), ctx.dp_launch_profile(), int(ctx.dp_timing().n_forward_launches)
    assert got == want, (what, got, want)
    assert sum(singles.values()) == g.n_levels - 1 - 2 * len(chosen) and n_launch == g.n_levels - 1 - len(chosen), (what, singles, n_launch)
    return chosen


def _digest_run(ctx, name, rc, **opts):
    g, ref = _graph(name), _oracle(name)
    with ctx.dp_options(digest=1, pair_digest=1, test_force_pair_rc=rc, **FORCED, **opts):
        ctx.dp_load_graph(g)
        out = ctx.dp_run()
        chosen = _check_profiles(ctx, g, rc, (name, rc), **FORCED)
        got, want = ctx.dp_level_digest(g.n_levels), ref["digest"].copy()
    want[[l - 1 for (l, _) in chosen]] = 0                              # the earlier level of a pair is never materialised
    assert np.array_equal(got[1:], want[1:]), (name, rc, "first level that differs", 1 + int(np.argmax(got[1:] != want[1:])))
    assert _answer(out) == _answer_of(ref), (name, rc)
    return chosen


def _budget_run(ctx, name, rc, **opts):
    g, want = _graph(name), _per_budget(name)
    with ctx.dp_options(digest=0, test_force_pair_rc=rc, **FORCED, **opts):
        ctx.dp_load_graph(g)
        outs = ctx.dp_run_budgets(list(range(g.R + 1)))
        _check_profiles(ctx, g, rc, (name, rc), **FORCED)
    for b, out in enumerate(outs):
        assert _answer(out) == want[b], (name, rc, "budget", b)


@pytest.mark.parametrize("digest", [1, 0])
@pytest.mark.parametrize("name", list(fg.CASES))
def test_every_cell_and_every_walk(gpu_ctx, name, digest):
    for rc in RCS:
        if digest:
            chosen = _digest_run(gpu_ctx, name, rc)
            assert chosen == fg.CASES[name][1] and any(b for (_, b) in chosen)
        else:
            _budget_run(gpu_ctx, name, rc)


@pytest.mark.parametrize("name", list(fg.REFUSED))
def test_refused_neighbour_runs_both_levels_singly(gpu_ctx, name):
    """composed in-degree 33: levels 3 and 4 carry the oracle's (non-zero) digests, which only single launches write"""
    refused, ref = fg.REFUSED[name][1], _oracle(name)
    assert ref["digest"][refused] != 0 and ref["digest"][refused - 1] != 0
    for rc in RCS:
        chosen = _digest_run(gpu_ctx, name, rc)
        assert all(l not in (refused - 1, refused, refused + 1) for (l, _) in chosen)
    _budget_run(gpu_ctx, name, RCS[0])


@pytest.mark.parametrize("name", ["big-rows-9", "both-fanin", "planes-19-mixed"])
def test_non_temporal_stores_batches_and_replays(gpu_ctx, name):
    """every level streaming its back-pointers non-temporally; plain launches and replayed batches (three passes)"""
    for rc in RCS:
        _digest_run(gpu_ctx, name, rc, bp_nt_min_cells=1)
        _budget_run(gpu_ctx, name, rc, bp_nt_min_cells=1)
    g, ref = _graph(name), _oracle(name)
    for gb in (0, -1):
        with gpu_ctx.dp_options(graph_batch=gb, **FORCED):
            gpu_ctx.dp_load_graph(g)
            for _ in range(3):
                assert _answer(gpu_ctx.dp_run()) == _answer_of(ref), (name, gb)
                assert sum(gpu_ctx.dp_pair_profile().values()) == len(fg.CASES[name][1])


@pytest.mark.parametrize("name", ["one-big-9", "big-rows-20-tail", "earlier-fanin"])
def test_the_gates(gpu_ctx, name):
    """pair_fanin 0, and the default pair_fanin_min (4,096 fan-in pairs): the pairs of the narrow rule, chosen as without the form;
    a free cost model launches a cooperative pair kernel of some chunk size; the refusals of light pairs hold for fan-in pairs"""
    g, ref = _graph(name), _oracle(name)
    for opts, rule in ((dict(pair_min=1, pair_fanin=0), dict(pair_fanin=0)), (dict(pair_min=1), dict(pair_fanin_min=4096))):
        with gpu_ctx.dp_options(test_force_pair_rc=1, **opts):
            gpu_ctx.dp_load_graph(g)
            assert _answer(gpu_ctx.dp_run()) == _answer_of(ref)
            chosen = _check_profiles(gpu_ctx, g, 1, (name, opts), **rule)
            assert chosen == [(l, 0) for l in pg.expected_pairs(g)]
    with gpu_ctx.dp_options(pair_min=1, pair_fanin_min=1, test_force_pair_rc=2):          # the shipped gate: at most DEFAULT_MAX_BIG big rows
        gpu_ctx.dp_load_graph(g)
        assert _answer(gpu_ctx.dp_run()) == _answer_of(ref)
        gated = _check_profiles(gpu_ctx, g, 2, (name, "gate"), pair_min=1, pair_fanin_min=1, pair_fanin_max_big=fg.DEFAULT_MAX_BIG)
        assert (4 in dict(gated)) == (dict(fg.CASES[name][1])[4] <= fg.DEFAULT_MAX_BIG)
    with gpu_ctx.dp_options(**FORCED):
        gpu_ctx.dp_load_graph(g)
        assert _answer(gpu_ctx.dp_run()) == _answer_of(ref)
        free = gpu_ctx.dp_pair_profile()
        assert sum(n for k, n in free.items() if k.startswith("dp_sweep_pair_coop_kernel<")) == sum(1 for (_, b) in fg.CASES[name][1] if b)
    for opts in (dict(digest=1), dict(segment_cells=300), dict(test_force_rc=2), dict(adaptive_rc=0), dict(fast=0)):
        with gpu_ctx.dp_options(**FORCED, **opts):
            gpu_ctx.dp_load_graph(g)
            assert _answer(gpu_ctx.dp_run()) == _answer_of(ref), opts
            assert not gpu_ctx.dp_pair_profile(), opts
            assert opts != dict(segment_cells=300) or int(gpu_ctx.dp_timing().n_segments) > 1

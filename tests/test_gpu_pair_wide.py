"""-m gpu: wide pairs -- level pairs with a source, middle or later level of 256..1,023 vertices, swept by dp_sweep_pair_wide_kernel and
dp_sweep_pair_coop_wide_kernel from records with 10-bit positions -- against the oracle.  Every graph of pair_wide_graphs.CASES
(tests/test_pair_wide_graphs.py holds their properties on the CPU) runs under pair_min = pair_wide_min = pair_fanin_min = 1 and the
shipped gates at each chunk size (test_force_pair_rc = 1, 2, 4):
  digest = 1, pair_digest = 1: every level that is not the earlier level of a pair shows the oracle's digest (value, reachability and
      middle cell of EVERY cell of a later level), the earlier levels the 0 of the run's memset; value, s_het and both edge lists equal;
  digest = 0 (the instantiations the product runs): dp_run_budgets over every budget 0..R equals the oracle solved per budget -- the
      walks pin the back-pointers of both levels.
The pair profile must be the one the model of the pairing rule gives, kernel by kernel.  All comparisons are integer equality."""
import re

import numpy as np
import pytest

import oracle_py as orc
import pair_fanin_graphs as fg
import pair_graphs as pg
import pair_wide_graphs as wg

pytestmark = pytest.mark.gpu

RCS = wg.RCS
FORCED = dict(pair_min=1, pair_wide_min=1, pair_fanin_min=1)
_G, _ORACLE, _PER_BUDGET = {}, {}, {}


def _graph(name):
    if name not in _G:
        _G[name] = (wg.CASES.get(name) or wg.REFUSED[name])[0]()
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
    """the launches per pair kernel are the model's, all at chunks of rc (rc None: the cost model's choice)"""
    want, chosen = wg.pair_profile(g, **rule), wg.choose_pairs(g, **rule)
    got, singles, n_launch = ctx.dp_pair_profile(), ctx.dp_launch_profile(), int(ctx.dp_timing().n_forward_launches)
    per_kernel = {}
    for name, n in got.items():
        kernel, size = re.fullmatch(r"(\w+)<(\d+)>", name).groups()
        per_kernel[kernel] = per_kernel.get(kernel, 0) + n
        assert int(size) in RCS and (rc is None or int(size) == rc), (what, got)
    assert per_kernel == want, (what, got, want)
    assert sum(singles.values()) == g.n_levels - 1 - 2 * len(chosen) and n_launch == g.n_levels - 1 - len(chosen), (what, singles, n_launch)
    return chosen


def _digest_run(ctx, name, rc, rule=None, **opts):
    g, ref, rule = _graph(name), _oracle(name), rule or {}
    with ctx.dp_options(digest=1, pair_digest=1, test_force_pair_rc=rc or 0, **FORCED, **rule, **opts):
        ctx.dp_load_graph(g)
        out = ctx.dp_run()
        chosen = _check_profiles(ctx, g, rc, (name, rc), **rule)
        got, want = ctx.dp_level_digest(g.n_levels), ref["digest"].copy()
    want[[l - 1 for (l, _, _) in chosen]] = 0                           # the earlier level of a pair is never materialised
    assert np.array_equal(got[1:], want[1:]), (name, rc, "first level that differs", 1 + int(np.argmax(got[1:] != want[1:])))
    assert _answer(out) == _answer_of(ref), (name, rc)
    return chosen


def _budget_run(ctx, name, rc, rule=None, **opts):
    g, want, rule = _graph(name), _per_budget(name), rule or {}
    with ctx.dp_options(digest=0, test_force_pair_rc=rc or 0, **FORCED, **rule, **opts):
        ctx.dp_load_graph(g)
        outs = ctx.dp_run_budgets(list(range(g.R + 1)))
        chosen = _check_profiles(ctx, g, rc, (name, rc), **rule)
    for b, out in enumerate(outs):
        assert _answer(out) == want[b], (name, rc, "budget", b)
    return chosen


@pytest.mark.parametrize("digest", [1, 0])
@pytest.mark.parametrize("name", list(wg.CASES))
def test_every_cell_and_every_walk(gpu_ctx, name, digest):
    for rc in RCS:
        chosen = (_digest_run if digest else _budget_run)(gpu_ctx, name, rc)
        assert chosen == wg.CASES[name][1]


@pytest.mark.parametrize("name", list(wg.REFUSED))
def test_refused_levels_run_singly(gpu_ctx, name):
    """1,024 vertices, 2,048 in-edges, a column of 64 composed in-edges, 5 big rows under the shipped gate of 4: level 4 is the later
    level of no pair; levels 3 and 4 carry the oracle's (non-zero) digests, which only single launches write -- but for big-rows-5,
    whose level 4 is the earlier level of the sink's pair"""
    ref = _oracle(name)
    assert ref["digest"][3] != 0 and ref["digest"][4] != 0
    for rc in RCS:
        chosen = _digest_run(gpu_ctx, name, rc)
        assert chosen == wg.REFUSED[name][1] and all(l not in (3, 4) for (l, _, _) in chosen)
    _budget_run(gpu_ctx, name, RCS[0])


def test_the_big_row_list_beyond_the_inline_ones(gpu_ctx):
    """pair_fanin_max_big 5: the fifth big row of a wide pair comes from the pair's list, the first four ride in the kernel arguments"""
    rule = dict(pair_fanin_max_big=5)
    for rc in RCS:
        assert (4, 5, True) in _digest_run(gpu_ctx, "big-rows-5", rc, rule)
        assert (4, 5, True) in _budget_run(gpu_ctx, "big-rows-5", rc, rule)


@pytest.mark.parametrize("name", ["width-all-1023", "two-columns-of-32", "tie-big-0/all", "planes-7-mixed/source"])
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
                assert sum(gpu_ctx.dp_pair_profile().values()) == len(wg.CASES[name][1])


@pytest.mark.parametrize("name", ["width-middle-257", "width-source-256", "one-big-9/all", "shared-middle-big/middle", "t-2047-2047"])
def test_the_gates(gpu_ctx, name):
    """pair_wide 0, and the default pair_wide_min (1,024 wide pairs): the pairs of the earlier rules, chosen as without the form.  No big
    rows in a wide pair under pair_wide_fanin 0, nothing wider than pair_wide_max_width.  pair_wide_rc sets the chunk size of the wide
    pairs alone.  The refusals of narrow pairs hold for wide pairs."""
    g, ref = _graph(name), _oracle(name)
    earlier = [(l, b, False) for (l, b) in fg.choose_pairs(g, pair_fanin_max_big=fg.DEFAULT_MAX_BIG)]
    for opts, rule in ((dict(pair_wide=0), dict(pair_wide=0)), (dict(pair_wide_min=1024), dict(pair_wide_min=1024))):
        with gpu_ctx.dp_options(test_force_pair_rc=1, **{**FORCED, **opts}):
            gpu_ctx.dp_load_graph(g)
            assert _answer(gpu_ctx.dp_run()) == _answer_of(ref)
            assert _check_profiles(gpu_ctx, g, 1, (name, opts), **rule) == earlier and not any(w for (_, _, w) in earlier)
    for rule in (dict(pair_wide_fanin=0), dict(pair_wide_max_width=511), dict(pair_wide_max_width=256)):
        chosen = _digest_run(gpu_ctx, name, 2, rule)
        assert all(not (w and b) for (_, b, w) in chosen) or "pair_wide_fanin" not in rule
        _budget_run(gpu_ctx, name, 4, rule)
    for rc in RCS:
        with gpu_ctx.dp_options(pair_wide_rc=rc, **FORCED):
            gpu_ctx.dp_load_graph(g)
            assert _answer(gpu_ctx.dp_run()) == _answer_of(ref)
            _check_profiles(gpu_ctx, g, None, (name, "pair_wide_rc", rc))
            for kernel_rc, n in gpu_ctx.dp_pair_profile().items():
                kernel, size = re.fullmatch(r"(\w+)<(\d+)>", kernel_rc).groups()
                assert "wide" not in kernel or int(size) == rc, (name, rc, kernel_rc)
    for opts in (dict(digest=1), dict(segment_cells=300), dict(test_force_rc=2), dict(adaptive_rc=0), dict(fast=0)):
        with gpu_ctx.dp_options(**FORCED, **opts):
            gpu_ctx.dp_load_graph(g)
            assert _answer(gpu_ctx.dp_run()) == _answer_of(ref), opts
            assert not gpu_ctx.dp_pair_profile(), opts
            assert opts != dict(segment_cells=300) or int(gpu_ctx.dp_timing().n_segments) > 1

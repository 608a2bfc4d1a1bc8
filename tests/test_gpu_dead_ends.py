"""-m gpu: dead-end vertices through the backward recurrences.  No generator of tests/graphgen.py leaves an inner vertex without an
out-edge, so the entry points that walk the graph from the sink -- dg_dp_partner_marginals, dg_dp_best_partners, dg_dp_call_margins,
dg_dp_genotype_margins, dg_dp_genotype_table -- have met none: a vertex that no scatter from the next level reaches must still hold
NEG_INF, a by-source edge list may be empty.

Integers only: every comparison is exact.  The graphs are the dead_ends family of tests/loader_graphs.py (the oracle alone reaches the
sink of every member: tests/test_loader_graphs.py); the yardsticks are the models of tests/test_gpu_marginals.py, test_gpu_partner.py,
test_gpu_call_margins.py, test_gpu_genotype_margins.py and test_gpu_genotype_table.py, pinned to brute force on the enumerable members by
their own CPU tests.  Given paths are samples of PathModel.sample_paths on the graph pruned of the edges into vertices that cannot
reach the sink (the same paths, and no walk strands).  After every call the preceding run's planes and level digests are as they were."""
import numpy as np
import pytest

import loader_graphs as lg
from call_margins_model import call_margins_batch, class_arrays
from marginals_model import partner_marginals_batch
from partner_model import best_partners
from paths_model import NEG_INF, PathModel
from test_gpu_genotype_margins import _called, _compare as compare_margins
from test_gpu_genotype_table import _compare as compare_table

pytestmark = pytest.mark.gpu

MEMBERS = lg.dead_ends()
N_GIVEN = 30
_CASES = {}


def case(name):
    """graph, model, dead-end vertices, given paths, budgets 0..R + 1 in turn, class arrays -- computed once"""
    if name not in _CASES:
        g = MEMBERS[name]
        m = PathModel(g)
        sampler = PathModel(lg.prune(g))
        rng = np.random.default_rng(61)
        a, _ = sampler.sample_paths(rng, N_GIVEN // 2)
        b, _ = sampler.sample_paths(rng, N_GIVEN - N_GIVEN // 2, 0.9)
        given = np.concatenate([a, b])
        assert all(m.check_path(p) is None for p in given)
        budgets = (np.arange(N_GIVEN) % (g.R + 2)).astype(np.int32)
        _CASES[name] = (g, m, lg.dead_end_vertices(g), given, budgets, class_arrays(g, 71))
    return _CASES[name]


class RunState:
    """load, run every budget with level digests; same() then says whether the run's planes and digests are still what they were"""

    def __init__(self, ctx, g):
        self.ctx, self.g = ctx, g
        ctx.dp_load_graph(g)
        self.outs = [o.key() for o in ctx.dp_run_budgets(range(g.R + 1))]
        self.planes = ctx.dp_budget_values().copy()
        self.digest = ctx.dp_level_digest(g.n_levels).copy()
        assert self.digest[1:].any() and self.planes[g.R] != NEG_INF

    def same(self):
        return np.array_equal(self.ctx.dp_budget_values(), self.planes) and np.array_equal(self.ctx.dp_level_digest(self.g.n_levels), self.digest)


ROUTES = {"lds": ({}, 1), "device_memory": ({"partner_wide": 2}, 2)}


@pytest.mark.parametrize("name", list(MEMBERS))
def test_partner_marginals_and_best_partners(gpu_ctx, name):
    g, m, dead, given, budgets, _ = case(name)
    records, M = partner_marginals_batch(m, given, budgets)
    values, partners = best_partners(m, given, budgets)
    reach = values != NEG_INF
    assert reach.any() and np.array_equal(M[:, -1], values) and (M[:, dead] == NEG_INF).all() and budgets.max() == g.R + 1
    want = np.zeros((len(given), 4), np.int64)
    for i in range(len(given)):
        want[i] = m.score(given[i], partners[i]) if reach[i] else (NEG_INF, 0, m.recombinations(given[i]), 0)
    with gpu_ctx.dp_options(digest=1):
        run = RunState(gpu_ctx, g)
        for route, (opts, number) in ROUTES.items():
            with gpu_ctx.dp_options(**opts):
                levels, vertex_values = gpu_ctx.dp_partner_marginals(given, budgets, want_vertices=True)
                assert gpu_ctx.dp_partner_route()[0] == number and run.same()
                rec, rows = gpu_ctx.dp_best_partners(given, budgets)
                assert gpu_ctx.dp_partner_route()[0] == number and run.same()
            bad = np.argwhere(vertex_values != M)
            assert bad.size == 0, (name, route, bad[:5], vertex_values[tuple(bad[:5].T)], M[tuple(bad[:5].T)])
            assert (vertex_values[:, dead] == NEG_INF).all()               # (implied; said once more for the vertices this file is about)
            got = np.stack([levels[f] for f in ("best_vertex", "best_value", "second_vertex", "second_value")], axis=-1)
            bad = np.argwhere((got != records).any(axis=-1))
            assert bad.size == 0, (name, route, bad[:5], got[tuple(bad[:5].T)], records[tuple(bad[:5].T)])
            got = np.stack([rec["value"], rec["s_het"], rec["r1"], rec["r2"]], axis=1)
            bad = np.flatnonzero((got != want).any(axis=1))
            assert bad.size == 0, (name, route, bad[:5], got[bad[:5]], want[bad[:5]])
            assert np.array_equal(rows, partners), (name, route, np.flatnonzero((rows != partners).any(axis=1))[:5])
            assert not np.isin(rows[reach], dead).any()
        assert [o.key() for o in gpu_ctx.dp_run_budgets(range(g.R + 1))] == run.outs


@pytest.mark.parametrize("name", list(MEMBERS))
def test_call_margins(gpu_ctx, name):
    g, m, dead, _, _, classes = case(name)
    fields = ("vertex", "value", "alt_vertex", "alt_value")
    with gpu_ctx.dp_options(digest=1):
        run = RunState(gpu_ctx, g)
        for b in range(g.R + 1):
            got = [gpu_ctx.dp_call_margins(b, cls, want_paths=True) for cls in classes]
            assert run.same()
            paths = got[0][1]
            assert np.array_equal(paths, gpu_ctx.dp_answer_paths(b))
            if run.planes[b] == NEG_INF:
                assert (paths == -1).all()
                for levels, _ in got:
                    assert (np.stack([levels[f] for f in fields], axis=-1) == (-1, NEG_INF, -1, NEG_INF)).all()
                continue
            assert not np.isin(paths, dead).any()
            _, want = call_margins_batch(m, paths[0], paths[1], b, classes)
            for kind, ((levels, _), rec) in enumerate(zip(got, want)):
                rows = np.stack([levels[f] for f in fields], axis=-1)
                bad = np.argwhere((rows != rec).any(axis=-1))
                assert bad.size == 0, (name, b, kind, bad[:5], rows[tuple(bad[:5].T)], rec[tuple(bad[:5].T)])
                assert (levels["value"] == run.planes[b]).all() and not np.isin(levels["alt_vertex"], dead).any()


@pytest.mark.parametrize("name", list(MEMBERS))
def test_genotype_margins(gpu_ctx, name):
    g, m, dead, _, _, classes = case(name)
    sampler = PathModel(lg.prune(g))
    rng = np.random.default_rng(81)
    with gpu_ctx.dp_options(digest=1):
        run = RunState(gpu_ctx, g)
        for b in range(g.R + 1):
            best = gpu_ctx.dp_answer_paths(b) if run.planes[b] != NEG_INF else None
            T, V = compare_margins(gpu_ctx, g, m, b, _called(sampler, rng, best), classes, name)      # (with want_vertices=True)
            assert V == run.planes[b] and run.same()
            _, _, J = gpu_ctx.dp_genotype_margins(_called(sampler, rng), b, None, want_vertices=True)
            assert (J[dead] == NEG_INF).all() and (V == NEG_INF or J.max() == V)


@pytest.mark.parametrize("name", list(MEMBERS))
def test_genotype_table(gpu_ctx, name):
    g, m, dead, _, _, classes = case(name)
    state = 4 * (np.diff(g.level_off).astype(np.int64) ** 2)
    with gpu_ctx.dp_options(digest=1):
        run = RunState(gpu_ctx, g)
        for b in (0, g.R):
            whole = compare_table(gpu_ctx, g, m, b, [None, classes[2]], name)
            assert gpu_ctx.dp_genotype_stats()["n_segments"] == 1 and run.same()
            off, rows = whole[0]
            assert not np.isin(rows[:, 2:4], dead).any()                   # no cell of a dead-end vertex is a reachable genotype
            with gpu_ctx.dp_options(joint_state_bytes=int(2.5 * state.mean()) * (b + 1)):
                parts = compare_table(gpu_ctx, g, m, b, [None, classes[2]], (name, "segments"))
                assert 2 <= gpu_ctx.dp_genotype_stats()["n_segments"] <= g.n_levels and run.same()
            assert all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(whole, parts))

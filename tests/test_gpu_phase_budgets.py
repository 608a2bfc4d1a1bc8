"""-m gpu: dg_dp_phase_margins_budgets / Context.dp_phase_margins_budgets -- the phase margins of many called pairs, each at a budget of
its own, from one joint pass with a pool of seeded states.

Integers only: every comparison is exact.  Every query is held against tests/phase_margins_model.py (pinned to brute force by
tests/test_phase_margins_model.py) AND against the one-query call; the statistics against the slot plan of tests/phase_budgets_model.py
(pinned to a per-query simulation by tests/test_phase_budgets_model.py, which also asserts, on the CPU, that the query lists used here
share seeds, part ways, re-seed freed slots and hold swapped orders)."""
import numpy as np
import pytest

import graphgen
from dipgenie_amd import capi
from paths_model import NEG_INF, PathModel
from phase_budgets_model import STATS, plan
from phase_margins_model import FIELDS, joint_states_fb, phase_margins_np
from test_gpu_genotype_margins import wide_case
from test_phase_budgets_model import BUDGETS, SEEDS, case, query_lists

pytestmark = pytest.mark.gpu

MAX_QUERIES = 256                                       # the limit include/dipgenie_hip.h states
MAX_PLANES = 4096
_STATES = {}


def _rows(records):
    assert (records["reserved"] == 0).all()
    return np.stack([records[f] for f in FIELDS], axis=-1).reshape(-1, len(FIELDS))


def states(seed, m, b):
    """the model's F, B, V of (graph, budget): computed once, shared, left unchanged"""
    if (seed, b) not in _STATES:
        _STATES[seed, b] = joint_states_fb(m, b)
    return _STATES[seed, b]


def check_call(ctx, tag, m, called, budgets, cls, model_states=None, singles=True):
    """one call; every query against the model (where model_states(b) gives its states) and the one-query call; the plan's statistics"""
    got, best = ctx.dp_phase_margins_budgets(called, budgets, cls)
    stats = ctx.dp_phase_budget_stats()
    assert len(got) == len(budgets) == len(best)
    for q, b in enumerate(budgets):
        if model_states is not None:
            want, V = phase_margins_np(m, called[q], int(b), cls, model_states(int(b)))
            assert best[q] == V and len(got[q]) == len(want), (tag, q, b, best[q], V, len(got[q]), len(want))
            bad = np.flatnonzero((_rows(got[q]) != want).any(axis=-1))
            assert bad.size == 0, (tag, q, b, bad[:5], _rows(got[q])[bad[:5]], want[bad[:5]])
        if singles:
            one, V1 = ctx.dp_phase_margins(called[q], int(b), cls)
            assert best[q] == V1 and np.array_equal(got[q], one), (tag, q, b)
    want_stats = plan(called, cls)["stats"]
    assert {k: stats[k] for k in STATS} == want_stats, (tag, stats, want_stats)
    assert stats["peak_bytes"] > 0
    return got, best, stats


@pytest.mark.parametrize("kind", ["own classes", "two classes"])
@pytest.mark.parametrize("seed", SEEDS)
def test_device_equals_model_and_the_one_query_call(gpu_ctx, seed, kind):
    g, m, two, per_budget = case(seed)
    cls = two if kind == "two classes" else None
    gpu_ctx.dp_load_graph(g)
    gpu_ctx.dp_run_budgets(range(g.R + 1))
    planes = gpu_ctx.dp_budget_values().copy()
    fit = [b for b in range(g.R + 1) if planes[b] != NEG_INF]
    assert len(fit) >= 2
    lists = dict(query_lists(seed, cls))
    lists["answers"] = (np.stack([gpu_ctx.dp_answer_paths(b) for b in fit]), np.asarray(fit, np.int32))
    for name, (called, budgets) in lists.items():
        got, best, stats = check_call(gpu_ctx, (seed, kind, name), m, called, budgets, cls, lambda b: states(seed, m, b))
        assert stats["segments"] == 1
        if name == "same":                              # one live slot throughout: the one-query call's backward launches on S
            gpu_ctx.dp_phase_margins(called[0], 5, cls)
            assert stats["slot_levels"] == gpu_ctx.dp_phase_stats()["seeded_launches"] == stats["backward_launches"] and stats["max_live_slots"] == 1
            assert np.array_equal(got[1], got[3]) and best[1] == best[3]
        if name == "mixed":                             # the queries with 0 and 1 het level: an empty range, the value all the same
            assert len(got[1]) == 0 == len(got[4]) and best[1] == best[2] and best[4] == best[0] and len(got[0]) >= 2
        if name == "answers":                           # the run's own answers are optimal pairs: cis is the plane in every record
            for q, b in enumerate(fit):
                assert best[q] == planes[b] and (got[q]["cis_value"] == planes[b]).all() and (got[q]["trans_value"] <= planes[b]).all()
            assert sum(len(r) for r in got) >= 1


@pytest.mark.parametrize("seed", [9301, 9304])
def test_shuffling_the_queries_permutes_the_answers(gpu_ctx, seed):
    g, m, two, _ = case(seed)
    gpu_ctx.dp_load_graph(g)
    gpu_ctx.dp_run_budgets(range(g.R + 1))
    fit = [b for b in range(g.R + 1) if gpu_ctx.dp_budget_values()[b] != NEG_INF]
    assert len(fit) >= 2
    answers = (np.ascontiguousarray(np.stack([gpu_ctx.dp_answer_paths(b) for b in fit]), np.int32), np.asarray(fit, np.int32))
    rng = np.random.default_rng(seed)
    for cls in (None, two):
        lists = dict(query_lists(seed, cls))
        lists["answers"] = answers
        for name in ("sampled", "mixed", "answers"):
            called, budgets = lists[name]
            got, best = gpu_ctx.dp_phase_margins_budgets(called, budgets, cls)
            stats = gpu_ctx.dp_phase_budget_stats()
            assert sum(len(r) for r in got) >= 1, name
            perm = rng.permutation(len(budgets))
            while (perm == np.arange(len(budgets))).all():  # (a short list: drawn again until it moves a query)
                perm = rng.permutation(len(budgets))
            got2, best2 = gpu_ctx.dp_phase_margins_budgets(np.ascontiguousarray(called[perm]), budgets[perm], cls)
            stats2 = gpu_ctx.dp_phase_budget_stats()
            for x, q in enumerate(perm):
                assert np.array_equal(got2[x], got[q]) and best2[x] == best[q], (name, x, q)
            assert {k: stats2[k] for k in STATS} == {k: stats[k] for k in STATS} and stats2["segments"] == stats["segments"], name


def test_segments_change_nothing_but_segments(gpu_ctx):
    g, m, two, _ = case(9302)
    gpu_ctx.dp_load_graph(g)
    called, budgets = query_lists(9302, two)["mixed"]
    out = {}
    for name, nbytes in (("every level", 1), ("default", 0)):
        with gpu_ctx.dp_options(joint_state_bytes=nbytes):
            out[name] = gpu_ctx.dp_phase_margins_budgets(called, budgets, two)
        out[name + " stats"] = gpu_ctx.dp_phase_budget_stats()
    assert sum(len(r) for r in out["default"][0]) >= 4
    for a, b in zip(out["every level"][0], out["default"][0]):
        assert np.array_equal(a, b)
    assert np.array_equal(out["every level"][1], out["default"][1])
    assert out["every level stats"]["segments"] == g.n_levels and out["default stats"]["segments"] == 1
    for f in STATS:
        assert out["every level stats"][f] == out["default stats"][f]


def test_the_call_leaves_the_run_and_the_other_statistics_alone(gpu_ctx):
    g, m, two, per_budget = case(9303)
    gpu_ctx.dp_load_graph(g)
    gpu_ctx.dp_run_budgets(range(g.R + 1))
    planes = gpu_ctx.dp_budget_values().copy()
    paths = [gpu_ctx.dp_answer_paths(b).copy() for b in range(g.R + 1)]
    gpu_ctx.dp_genotype_margins(paths[g.R], g.R, two)
    gpu_ctx.dp_phase_margins(paths[g.R], g.R, two)
    genotype_stats, phase_stats = gpu_ctx.dp_genotype_stats(), gpu_ctx.dp_phase_stats()
    called, budgets = query_lists(9303, two)["mixed"]
    got, best = gpu_ctx.dp_phase_margins_budgets(called, budgets, two)
    assert sum(len(r) for r in got) >= 4
    assert gpu_ctx.dp_genotype_stats() == genotype_stats and gpu_ctx.dp_phase_stats() == phase_stats
    assert np.array_equal(gpu_ctx.dp_budget_values(), planes)
    for b in range(g.R + 1):
        assert np.array_equal(gpu_ctx.dp_answer_paths(b), paths[b])


def test_a_budget_nobody_fits_beside_budgets_that_fit(gpu_ctx):
    """every edge weighs 1, so a pair of paths spends 2 (L - 1) = 10: budgets 0 and 9 fit nobody, 10 and 12 do.  The unanswered queries
    get NEG_INF / -1 records with the levels the model names, beside their neighbours' answers"""
    g = graphgen.random_levelized(9611, widths=[1, 3, 4, 3, 4, 1], R=3, p_w1=1.0, dup_edges=True, extra_edges=1.2, p_colour=0.5)
    m = PathModel(g)
    gpu_ctx.dp_load_graph(g)
    P, _ = m.sample_paths(np.random.default_rng(1), 2)
    P[1, 1:-1] = [v + 1 if v + 1 < g.level_off[l + 2] else v - 1 for l, v in enumerate(P[0, 1:-1])]      # het on every inner level
    rng = np.random.default_rng(2)
    while True:                                         # a pair of real paths with at least two het levels: within budget 10 it is its own cis
        Q, rec = m.sample_paths(rng, 2)
        if (Q[0] != Q[1]).sum() >= 2:
            break
    assert int(rec.sum()) == 10
    called = np.ascontiguousarray(np.stack([P, Q, Q[::-1], P, Q]), np.int32)
    budgets = np.asarray([0, 10, 12, 9, 0], np.int32)
    st = {int(b): joint_states_fb(m, int(b)) for b in set(budgets.tolist())}
    got, best, stats = check_call(gpu_ctx, "weight 1", m, called, budgets, None, lambda b: st[b])
    assert best.tolist()[0] == best.tolist()[3] == best.tolist()[4] == NEG_INF and best[1] != NEG_INF and best[2] != NEG_INF
    for q in (0, 3, 4):
        assert len(got[q]) == (3 if q != 4 else len(got[1])) and (got[q]["cis_value"] == NEG_INF).all() and (got[q]["trans_vertex1"] == -1).all()
    for q in (1, 2):
        assert len(got[q]) >= 1 and (got[q]["cis_value"] != NEG_INF).all()
    assert np.array_equal(got[4][["level_a", "level_b"]], got[1][["level_a", "level_b"]])


def _wide_called(m, seed):
    """a sampled pair of paths whose rows differ on all three inner levels: drawn from a fixed seed until they do"""
    rng = np.random.default_rng(seed)
    while True:
        called, rec = m.sample_paths(rng, 2, p_w0=0.9)
        if (called[0, 1:-1] != called[1, 1:-1]).all():
            return called


def test_wider_than_any_tile_against_the_one_query_call(gpu_ctx):
    g, m, planes = wide_case(gpu_ctx)
    A, B = _wide_called(m, 77), _wide_called(m, 78)
    shared = A.copy()
    shared[:, 1] = B[:, 1]                              # the seeds of A above level 1, another cell there
    called = np.ascontiguousarray(np.stack([A, B, shared, A]), np.int32)
    budgets = np.asarray([3, 18, 18, 18], np.int32)
    got, best, stats = check_call(gpu_ctx, "wide", m, called, budgets, None)
    assert best[1] == best[2] == best[3] == planes[18] and [len(r) for r in got] == [2, 2, 2, 2]
    assert stats["max_live_slots"] == 2 and stats["seed_keys"] < 8
    for q in (1, 3):                                    # a pair of real paths spends at most 2 (L - 1) = 8 <= 18: it is within its own cis
        assert (got[q]["cis_value"] != NEG_INF).all() and (got[q]["cis_value"] <= best[q]).all()


def test_256_queries_are_answered_and_257_refused(gpu_ctx):
    g, m, two, per_budget = case(9305)
    gpu_ctx.dp_load_graph(g)
    few = np.stack([per_budget[b] for b in BUDGETS] + [per_budget[2][::-1]])
    pick = np.arange(MAX_QUERIES) % len(few)
    called = np.ascontiguousarray(few[pick], np.int32)
    budgets = np.asarray([(0, 2, 5, 3)[x] for x in pick], np.int32)
    got, best, stats = check_call(gpu_ctx, "256", m, called, budgets, two, singles=False)
    singles = [gpu_ctx.dp_phase_margins(few[x], (0, 2, 5, 3)[x], two) for x in range(len(few))]
    for q, x in enumerate(pick):
        assert np.array_equal(got[q], singles[x][0]) and best[q] == singles[x][1], q
    assert stats["queries"] == MAX_QUERIES and stats["records"] == sum(len(r) for r in got) >= MAX_QUERIES
    more = np.concatenate([called, called[:1]])
    with pytest.raises(capi.DgError, match=rf"rc=-5.*dg_dp_phase_margins_budgets.*\b{MAX_QUERIES + 1}\b.*\b{MAX_QUERIES}\b"):
        gpu_ctx.dp_phase_margins_budgets(more, np.concatenate([budgets, budgets[:1]]), two)
    assert gpu_ctx.dp_phase_budget_stats() == stats


def test_errors_and_layout(gpu_ctx):
    g, m, two, per_budget = case(9300)
    L = g.n_levels
    call = capi.lib.dg_dp_phase_margins_budgets
    fresh = capi.Context(0)
    try:
        with pytest.raises(capi.DgError, match=r"rc=-6.*dg_dp_phase_margins_budgets: no graph loaded"):
            fresh.dp_phase_margins_budgets(np.zeros((1, 2, L), np.int32), [0])
    finally:
        fresh.close()
    gpu_ctx.dp_load_graph(g)
    called, budgets = query_lists(9300, None)["mixed"]
    n = len(budgets)
    want, V = gpu_ctx.dp_phase_margins_budgets(called, budgets)
    stats = gpu_ctx.dp_phase_budget_stats()
    total = sum(len(r) for r in want)
    assert total >= 4
    out = np.full((n * (L - 1), 10), -7, np.int32)
    off = np.full(n + 1, -7, np.int64)
    best = np.full(n, -7, np.int32)
    ptr = lambda a: a.ctypes.data if a is not None else None

    def raw(p, b, count=n, records=out, off_=off, best_=best):
        return call(gpu_ctx.h, ptr(p), ptr(b), count, None, ptr(records), ptr(off_), ptr(best_))

    def untouched():
        return (out == -7).all() and (off == -7).all() and (best == -7).all()

    bad = called.copy()
    bad[2, 1, 2] = g.level_off[3]                        # query 2, row 1, level 2: the first vertex of level 3
    bad[3, 0, 1] = 0                                     # (a later one too: the first is named)
    with pytest.raises(capi.DgError, match=r"rc=-1.*dg_dp_phase_margins_budgets.*query 2 row 1 level 2\b"):
        gpu_ctx.dp_phase_margins_budgets(bad, budgets)
    assert raw(bad, budgets) == -1 and untouched()
    neg = budgets.copy()
    neg[1], neg[4] = -1, -3
    with pytest.raises(capi.DgError, match=r"rc=-1.*dg_dp_phase_margins_budgets.*query 1\b.*budget -1"):
        gpu_ctx.dp_phase_margins_budgets(called, neg)
    assert raw(called, neg) == -1 and untouched()
    assert raw(None, budgets) == -1 and raw(called, None) == -1 and raw(called, budgets, records=None) == -1 and untouched()
    assert raw(called, budgets, off_=None) == -1 and raw(called, budgets, best_=None) == -1 and untouched()
    assert raw(called, budgets, count=0) == -1 and raw(called, budgets, count=-1) == -1 and untouched()
    assert raw(called, budgets, count=MAX_QUERIES + 1) == -5 and untouched()           # refused before a query is read
    big = budgets.copy()
    big[3] = MAX_PLANES
    with pytest.raises(capi.DgError, match=rf"rc=-5.*dg_dp_phase_margins_budgets.*\b{MAX_PLANES + 1}\b.*\b{MAX_PLANES}\b"):
        gpu_ctx.dp_phase_margins_budgets(called, big)
    assert raw(called, big) == -5 and untouched()
    assert gpu_ctx.dp_phase_budget_stats() == stats      # a refused call leaves the statistics too
    with pytest.raises(ValueError):
        gpu_ctx.dp_phase_margins_budgets(called[:, :, :-1], budgets)
    with pytest.raises(ValueError):
        gpu_ctx.dp_phase_margins_budgets(called[0], budgets[:1])
    with pytest.raises(ValueError):
        gpu_ctx.dp_phase_margins_budgets(called, budgets[:-1])
    with pytest.raises(ValueError):
        gpu_ctx.dp_phase_margins_budgets(called, budgets, np.zeros(g.n_vertices - 1, np.int32))
    with pytest.raises(capi.DgError, match=r"rc=-1.*dg_dp_get_phase_budget_stats"):
        capi._check(capi.lib.dg_dp_get_phase_budget_stats(gpu_ctx.h, np.zeros(10, np.int64).ctypes.data, 9), "dg_dp_get_phase_budget_stats")
    # the raw call writes ten words per record -- the eight fields and two zeros -- the offsets, and nothing behind the last record
    assert raw(called, budgets) == 0 and off[0] == 0 and np.array_equal(np.diff(off), [len(r) for r in want]) and np.array_equal(best, V)
    assert np.array_equal(out[:total, :8], np.concatenate([_rows(r) for r in want])) and (out[:total, 8:] == 0).all() and (out[total:] == -7).all()

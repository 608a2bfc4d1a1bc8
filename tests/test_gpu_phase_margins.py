"""-m gpu: dg_dp_phase_margins / Context.dp_phase_margins -- cis against trans for every pair of neighbouring het levels of a called
pair, from the joint pass with one more rolling backward state.

Integers only: every comparison is exact.  The yardstick is tests/phase_margins_model.py, itself pinned to brute force by
tests/test_phase_margins_model.py; the tests without a model hold every record against dp_run_pinned (plane b of the run that requires
the ordered class pair at both levels is cis, with the classes at the first level swapped it is trans) and dp_score_paths."""
import numpy as np
import pytest

import graphgen
from dipgenie_amd import capi
from paths_model import NEG_INF, PathModel
from phase_margins_model import FIELDS, het_levels, joint_states_fb, phase_margins_np
from test_gpu_genotype_margins import wide_case

pytestmark = pytest.mark.gpu

SEEDS = range(9300, 9306)
BUDGETS = (0, 2, 5)
MAX_PLANES = 4096                                       # the limit include/dipgenie_hip.h states
_CASES = {}


def case(seed):
    """graph, model, the two-class array and one sampled pair of paths per budget, in the draw order the floors below were derived with"""
    if seed not in _CASES:
        g = graphgen.random_levelized(seed, widths=[1] + [3, 5, 2, 4, 6, 3] * 4 + [1], R=3, p_w1=0.3, dup_edges=True, extra_edges=1.2, p_colour=0.5)
        m = PathModel(g)
        rng = np.random.default_rng(seed)
        two = rng.integers(0, 2, g.n_vertices).astype(np.int32)
        called = {b: m.sample_paths(rng, 2, p_w0=0.9)[0] for b in BUDGETS}
        _CASES[seed] = (g, m, two, called)
    return _CASES[seed]


def _rows(records):
    assert (records["reserved"] == 0).all()
    return np.stack([records[f] for f in FIELDS], axis=-1).reshape(-1, len(FIELDS))


@pytest.mark.parametrize("seed", SEEDS)
def test_device_equals_model(gpu_ctx, seed):
    g, m, two, called = case(seed)
    gpu_ctx.dp_load_graph(g)
    for b in BUDGETS:
        states = joint_states_fb(m, b)
        for kind, cls in enumerate((None, two)):
            want, V = phase_margins_np(m, called[b], b, cls, states)
            got, best = gpu_ctx.dp_phase_margins(called[b], b, cls)
            assert best == V and len(got) == len(want), (seed, b, kind, best, V, len(got), len(want))
            bad = np.flatnonzero((_rows(got) != want).any(axis=-1))
            assert bad.size == 0, (seed, b, kind, bad[:5], _rows(got)[bad[:5]], want[bad[:5]])
            stats = gpu_ctx.dp_phase_stats()
            assert stats["records"] == len(want) == stats["readout_launches"] and stats["het_levels"] == len(het_levels(m, called[b], cls))
            if len(want):                                # the second backward launch runs between the first and the last het level only
                assert stats["seeded_launches"] == want[-1, 1] - want[0, 0]
            else:
                assert stats["seeded_launches"] == 0


def test_the_set_is_not_vacuous():
    """over budgets 2 and 5 of all six seeds (computed on the CPU, so that the floors hold however the tests are selected): the model
    gives 84 records with a reachable trans, 32 with cis == trans, 13 with trans > cis, 75 whose levels are not adjacent, and at least
    one reachable trans in each of the 24 cases"""
    trans = equal = better = far = 0
    smallest = None
    for seed in SEEDS:
        g, m, two, called = case(seed)
        for b in BUDGETS[1:]:
            states = joint_states_fb(m, b)
            for cls in (None, two):
                want, _ = phase_margins_np(m, called[b], b, cls, states)
                has = want[:, 5] != NEG_INF
                trans += int(has.sum())
                equal += int((want[:, 2] == want[:, 5])[has].sum())
                better += int((want[:, 5] > want[:, 2]).sum())
                far += int((want[:, 1] - want[:, 0] > 1).sum())
                smallest = int(has.sum()) if smallest is None else min(smallest, int(has.sum()))
    print(f"reachable trans {trans}, cis == trans {equal}, trans > cis {better}, level_b - level_a > 1 {far}, fewest reachable trans in a case {smallest}")
    assert trans >= 40 and equal >= 15 and better >= 5 and far >= 30 and smallest >= 1


def _class_cells(g, cls, level, x0, x1):
    """the ordered cells (i, j) of `level` with (cls i, cls j) = (x0, x1)"""
    ids = np.arange(g.n_vertices) if cls is None else cls
    vs = np.arange(g.level_off[level], g.level_off[level + 1])
    return [(int(i), int(j)) for i in vs[ids[vs] == x0] for j in vs[ids[vs] == x1]]


def _pinned_value(ctx, g, cls, b, a, xa, e, xe):
    """plane b of the run that requires the ordered class pair xa at level a and xe at level e"""
    pins = [(lvl, i, j, capi.PIN_REQUIRE) for lvl, x in ((a, xa), (e, xe)) for i, j in _class_cells(g, cls, lvl, *x)]
    assert 2 <= len(pins) <= 72
    return ctx.dp_run_pinned(pins, [b])[0].value


@pytest.mark.parametrize("seed", SEEDS)
def test_every_record_is_a_pinned_run(gpu_ctx, seed):
    g, m, two, called = case(seed)
    gpu_ctx.dp_load_graph(g)
    b = 2
    for cls in (None, two):
        ids = np.arange(g.n_vertices) if cls is None else cls
        records, best = gpu_ctx.dp_phase_margins(called[b], b, cls)
        assert len(records) >= 1
        for r in records:
            a, e = int(r["level_a"]), int(r["level_b"])
            xa = (ids[called[b][0, a]], ids[called[b][1, a]])
            xe = (ids[called[b][0, e]], ids[called[b][1, e]])
            assert r["cis_value"] == _pinned_value(gpu_ctx, g, cls, b, a, xa, e, xe), (seed, a, e)
            assert r["trans_value"] == _pinned_value(gpu_ctx, g, cls, b, a, xa[::-1], e, xe), (seed, a, e)
            for which, x in (("cis", xa), ("trans", xa[::-1])):          # the reported cell is one of its class pair, -1 where there is none
                v1, v2 = int(r[which + "_vertex1"]), int(r[which + "_vertex2"])
                if r[which + "_value"] == NEG_INF:
                    assert (v1, v2) == (-1, -1)
                else:
                    assert (v1, v2) in _class_cells(g, cls, a, *x)
            assert max(r["cis_value"], r["trans_value"]) <= best


def _wide_called(m):
    """a sampled pair of paths whose rows differ on all three inner levels: drawn from a fixed seed until they do"""
    rng = np.random.default_rng(77)
    while True:
        called, rec = m.sample_paths(rng, 2, p_w0=0.9)
        if (called[0, 1:-1] != called[1, 1:-1]).all():
            return called, int(rec.sum())


def test_wider_than_any_tile_against_pinned_runs(gpu_ctx):
    g, m, planes = wide_case(gpu_ctx)
    b = 18
    called, r = _wide_called(m)
    records, best = gpu_ctx.dp_phase_margins(called, b)
    assert best == planes[b] and len(records) == 2
    assert records["level_a"].tolist() == [1, 2] and records["level_b"].tolist() == [2, 3]
    score = int(gpu_ctx.dp_score_paths(called[None])[0]["value"])
    for rec in records:
        a, e = int(rec["level_a"]), int(rec["level_b"])
        xa, xe = (called[0, a], called[1, a]), (called[0, e], called[1, e])
        assert rec["cis_value"] == _pinned_value(gpu_ctx, g, None, b, a, xa, e, xe)
        assert rec["trans_value"] == _pinned_value(gpu_ctx, g, None, b, a, xa[::-1], e, xe)
        if rec["cis_value"] != NEG_INF:                  # own classes: the one cell of the pair
            assert (rec["cis_vertex1"], rec["cis_vertex2"]) == xa
        if r <= b:
            assert rec["cis_value"] >= score
        assert max(rec["cis_value"], rec["trans_value"]) <= best
    print(f"wide: r1 + r2 = {r}, score {score}, V {best}, records {_rows(records).tolist()}")


@pytest.mark.parametrize("which", ["levels26", "wide"])
def test_segments_change_nothing(gpu_ctx, which):
    if which == "wide":
        g, m, _ = wide_case(gpu_ctx)
        b, cls = 18, None
        called, _ = _wide_called(m)
    else:
        g, m, cls, per_budget = case(9302)
        gpu_ctx.dp_load_graph(g)
        b = 5
        called = per_budget[b]
    got = {}
    for name, nbytes in (("every level", 1), ("default", 0)):
        with gpu_ctx.dp_options(joint_state_bytes=nbytes):
            got[name] = gpu_ctx.dp_phase_margins(called, b, cls)
        got[name + " stats"] = gpu_ctx.dp_phase_stats()
    assert len(got["default"][0]) >= 2
    assert np.array_equal(got["every level"][0], got["default"][0]) and got["every level"][1] == got["default"][1]
    assert got["every level stats"]["segments"] == g.n_levels and got["default stats"]["segments"] == 1
    for f in ("het_levels", "records", "seeded_launches", "readout_launches"):
        assert got["every level stats"][f] == got["default stats"][f]
    widest = int(np.diff(g.level_off).max())
    assert got["default stats"]["peak_bytes"] >= 4 * 4 * widest * widest * (b + 1)      # B and S, two states of the widest level each


def test_the_call_leaves_the_run_and_the_genotype_statistics_alone(gpu_ctx):
    g, m, two, _ = case(9303)
    gpu_ctx.dp_load_graph(g)
    gpu_ctx.dp_run_budgets(range(g.R + 1))
    planes = gpu_ctx.dp_budget_values().copy()
    paths = [gpu_ctx.dp_answer_paths(b).copy() for b in range(g.R + 1)]
    gpu_ctx.dp_genotype_margins(paths[g.R], g.R, two)
    stats = gpu_ctx.dp_genotype_stats()
    n_records = 0
    for b in range(g.R + 1):
        if planes[b] == NEG_INF:
            continue
        records, best = gpu_ctx.dp_phase_margins(paths[b], b, two)
        assert best == planes[b] and (records["cis_value"] == planes[b]).all()      # the run's own answer is an optimal pair
        assert (records["trans_value"] <= planes[b]).all()
        n_records += len(records)
    assert n_records >= 1
    assert np.array_equal(gpu_ctx.dp_budget_values(), planes)
    for b in range(g.R + 1):
        assert np.array_equal(gpu_ctx.dp_answer_paths(b), paths[b])
    assert gpu_ctx.dp_genotype_stats() == stats


def test_a_budget_nobody_fits(gpu_ctx):
    """every edge weighs 1: at b = 0 no pair fits.  DG_OK, NEG_INF / -1 in every record, the levels as the model names them"""
    g = graphgen.random_levelized(9611, widths=[1, 3, 4, 3, 4, 1], R=3, p_w1=1.0, dup_edges=True, extra_edges=1.2, p_colour=0.5)
    m = PathModel(g)
    gpu_ctx.dp_load_graph(g)
    called, _ = m.sample_paths(np.random.default_rng(1), 2)
    called[1, 1:-1] = [v + 1 if v + 1 < g.level_off[l + 2] else v - 1 for l, v in enumerate(called[0, 1:-1])]      # het on every inner level
    want, V = phase_margins_np(m, called, 0)
    got, best = gpu_ctx.dp_phase_margins(called, 0)
    assert best == V == NEG_INF and len(got) == 3 and np.array_equal(_rows(got), want)
    assert (got["cis_value"] == NEG_INF).all() and (got["trans_vertex1"] == -1).all()


def test_errors_and_layout(gpu_ctx):
    assert capi.PHASE_MARGIN.itemsize == 40 and capi.PHASE_MARGIN.names == FIELDS + ("reserved",)
    g, m, two, per_budget = case(9300)
    L = g.n_levels
    call = capi.lib.dg_dp_phase_margins
    fresh = capi.Context(0)
    try:
        with pytest.raises(capi.DgError, match=r"rc=-6.*dg_dp_phase_margins: no graph loaded"):
            fresh.dp_phase_margins(np.zeros((2, L), np.int32), 0)
    finally:
        fresh.close()
    gpu_ctx.dp_load_graph(g)
    called = np.ascontiguousarray(per_budget[2], np.int32)
    want, V = gpu_ctx.dp_phase_margins(called, 2)
    stats = gpu_ctx.dp_phase_stats()
    assert len(want) >= 2
    out = np.full((L - 1, 10), -7, np.int32)
    n, best = capi.C.c_int64(-7), capi.C.c_int32(-7)

    def raw(p, b, records=out, n_ref=capi.C.byref(n), best_ref=capi.C.byref(best)):
        return call(gpu_ctx.h, p.ctypes.data if p is not None else None, b, None, records.ctypes.data if records is not None else None, n_ref, best_ref)

    def untouched():
        return (out == -7).all() and n.value == -7 and best.value == -7

    bad = called.copy()
    bad[1, 2] = g.level_off[3]                           # row 1, level 2: the first vertex of level 3
    bad[1, 3] = 0                                        # (a later one too: the first is named)
    with pytest.raises(capi.DgError, match=r"rc=-1.*dg_dp_phase_margins.*row 1 level 2\b"):
        gpu_ctx.dp_phase_margins(bad, 2)
    assert raw(bad, 2) == -1 and untouched()
    bad = called.copy()
    bad[0, 0] = -1
    with pytest.raises(capi.DgError, match=r"rc=-1.*row 0 level 0\b"):
        gpu_ctx.dp_phase_margins(bad, 2)
    with pytest.raises(capi.DgError, match=r"rc=-1.*dg_dp_phase_margins.*budget -1"):
        gpu_ctx.dp_phase_margins(called, -1)
    assert raw(called, -1) == -1 and untouched()
    assert raw(None, 2) == -1 and raw(called, 2, records=None) == -1 and raw(called, 2, n_ref=None) == -1 and raw(called, 2, best_ref=None) == -1 and untouched()
    with pytest.raises(capi.DgError, match=rf"rc=-5.*dg_dp_phase_margins.*\b{MAX_PLANES + 1}\b.*\b{MAX_PLANES}\b"):
        gpu_ctx.dp_phase_margins(called, MAX_PLANES)
    assert raw(called, MAX_PLANES) == -5 and untouched()
    assert gpu_ctx.dp_phase_stats() == stats             # a refused call leaves the statistics too
    with pytest.raises(ValueError):
        gpu_ctx.dp_phase_margins(called[:, :-1], 2)
    with pytest.raises(ValueError):
        gpu_ctx.dp_phase_margins(called[None], 2)
    with pytest.raises(ValueError):
        gpu_ctx.dp_phase_margins(called, 2, np.zeros(g.n_vertices - 1, np.int32))
    # the raw call writes ten words per record -- the eight fields and two zeros -- and only n_records of them
    assert raw(called, 2) == 0 and n.value == len(want) and best.value == V
    assert np.array_equal(out[:len(want), :8], _rows(want)) and (out[:len(want), 8:] == 0).all() and (out[len(want):] == -7).all()
    # fewer than two het levels: no record, DG_OK, and the best value all the same
    for het in (0, 1):
        same = np.stack([called[0], called[0]])
        if het:
            same[1, 1] = called[0, 1] + (1 if called[0, 1] + 1 < g.level_off[2] else -1)
        got, best1 = gpu_ctx.dp_phase_margins(same, 2)
        assert len(got) == 0 and best1 == V
        s = gpu_ctx.dp_phase_stats()
        assert (s["het_levels"], s["records"], s["seeded_launches"], s["readout_launches"], s["segments"]) == (het, 0, 0, 0, stats["segments"])
    out[:] = -7
    assert raw(np.stack([called[0], called[0]]), 2) == 0 and n.value == 0 and best.value == V and (out == -7).all()

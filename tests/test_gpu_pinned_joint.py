"""-m gpu: dg_dp_genotype_margins_pinned / dg_dp_genotype_table_pinned -- the joint pass on the DP that per-level cell constraints
leave: the through-value of every ordered cell, the margin records, the joint marginals and the genotype table under pins.

Integers only: every comparison is exact.  The yardstick is tests/pinned_joint_model.py, itself pinned to brute force by
tests/test_pinned_joint_model.py; the tests on the widest graph need no model: they hold the calls against dp_run_pinned and the
unpinned table."""
import numpy as np
import pytest

import graphgen
from call_margins_model import class_arrays
from dipgenie_amd import capi
from paths_model import NEG_INF, PathModel
from pinned_joint_model import pinned_genotype_margins_np, pinned_genotype_table_np, pinned_through_values_np
from pinned_model import FORBID, REQUIRE, cell_allowed
from test_gpu_genotype_margins import BUDGETS, _called, _rows, wide_case
from test_gpu_genotype_table import _entry_rows
from test_gpu_score_paths import ENUMERABLE
from test_partner_model import enumerable_graph
from test_pinned_model import pin_sets, random_pins

pytestmark = pytest.mark.gpu

WIDTHS = [[1, 2, 1], [1, 3, 64, 65, 2, 1], [1, 63, 64, 1], [1, 70, 5, 70, 1], [1, 257, 1]]


def _n_levels(pins):
    return len({int(p[0]) for p in pins})


def _compare(ctx, g, m, b, pins, called, classes, tag):
    """records, best_value, vertex_values, level_off and every entry of the table against the numpy model, for each class array; the
    statistics of a call with one segment: every pinned level is masked once forward and once backward"""
    T, V = pinned_through_values_np(m, b, pins)
    for kind, cls in enumerate(classes):
        want, _, J = pinned_genotype_margins_np(m, called, T, V, cls)
        levels, best, vv = ctx.dp_genotype_margins_pinned(pins, called, b, cls, want_vertices=True)
        assert ctx.dp_genotype_pin_stats() == dict(pins=len(pins), mask_launches=2 * _n_levels(pins)), (tag, ctx.dp_genotype_pin_stats())
        assert levels.shape == (len(called), g.n_levels) and best == V, (tag, b, kind, best, V)
        bad = np.argwhere((_rows(levels) != want).any(axis=-1))
        assert bad.size == 0, (tag, b, kind, pins[:6], bad[:5], _rows(levels)[tuple(bad[:5].T)], want[tuple(bad[:5].T)])
        assert np.array_equal(vv, J), (tag, b, kind, np.flatnonzero(vv != J)[:5])
        want_off, want_rows = pinned_genotype_table_np(m, T, cls)
        off, entries, best2, levels2 = ctx.dp_genotype_table_pinned(pins, b, cls, called)
        assert ctx.dp_genotype_pin_stats() == dict(pins=len(pins), mask_launches=2 * _n_levels(pins))
        rows = _entry_rows(entries)
        assert best2 == V and np.array_equal(off, want_off), (tag, b, kind, off, want_off)
        assert len(entries) == off[-1] == ctx.dp_genotype_stats()["entries"]
        bad = np.flatnonzero((rows != want_rows).any(axis=1))
        assert bad.size == 0, (tag, b, kind, pins[:6], bad[:5], rows[bad[:5]], want_rows[bad[:5]])
        assert np.array_equal(_rows(levels2), want), (tag, b, kind)
        if V != NEG_INF:
            assert (np.maximum.reduceat(rows[:, 4], off[:-1]) == V).all()
        else:
            assert len(entries) == 0 and (off == 0).all() and (vv == NEG_INF).all()
    return T, V


@pytest.mark.parametrize("q", range(len(ENUMERABLE)))
def test_device_equals_model_on_the_enumerable_graphs(gpu_ctx, q):
    g = enumerable_graph(q)
    m = PathModel(g)
    gpu_ctx.dp_load_graph(g)
    rng = np.random.default_rng(40 + q)
    classes = class_arrays(g, 21 + q)
    asymmetric = 0
    for n, (tag, pins) in enumerate(pin_sets(q)):
        for b in (range(4) if n < 14 else [n % 4]):      # every budget for the composed sets, one each for the single cells
            T, V = _compare(gpu_ctx, g, m, b, pins, _called(m, rng), classes if n < 14 else classes[2:], (q, tag))
            asymmetric += any(not np.array_equal(t, t.T) for t in T)
    assert asymmetric >= 1


def _edge_sets(g, m, rng):
    """pins on the first and last row and column and on the 64th and 65th column of the widest inner level, wildcards on either side,
    many pins on one level, every inner level pinned"""
    L = g.n_levels
    widths = np.diff(g.level_off).astype(int)
    wide = 1 + int(np.argmax(widths[1:-1]))
    a0, a1 = int(g.level_off[wide]), int(g.level_off[wide + 1])
    pick = lambda l: int(rng.integers(g.level_off[l], g.level_off[l + 1]))
    cols = [a0 + c for c in (63, 64) if a0 + c < a1]
    return {
        "forbid edges": [(wide, a0, -1, FORBID), (wide, -1, a0, FORBID), (wide, a1 - 1, -1, FORBID), (wide, -1, a1 - 1, FORBID)] + [(wide, -1, c, FORBID) for c in cols],
        "require edges": [(wide, a0, -1, REQUIRE), (wide, -1, a1 - 1, REQUIRE), (wide, a1 - 1, a0, REQUIRE)] + [(wide, -1, c, REQUIRE) for c in cols],
        "wildcard left": [(wide, -1, pick(wide), REQUIRE), (L - 2, -1, pick(L - 2), FORBID)],
        "wildcard right": [(wide, pick(wide), -1, FORBID), (1, pick(1), -1, REQUIRE), (1, pick(1), -1, REQUIRE)],
        "many": [(wide, pick(wide), pick(wide), REQUIRE) for _ in range(70)] + [(wide, pick(wide), pick(wide), FORBID) for _ in range(5)],
        "every level": random_pins(m, rng, L - 2, 3),
    }


@pytest.mark.parametrize("w", range(len(WIDTHS)))
def test_device_equals_model_on_prescribed_widths(gpu_ctx, w):
    """budgets 0, 1, 2, 7, 18: 1, 2, 3, 8 and 19 planes stride the flattened (j, r) of a row unevenly.  Every pin set meets every kind of
    recombination weight (the 257-wide level, whose model is the slow part, meets p_w1 = 0.3 alone); the budgets take turns over the sets"""
    lowered = asymmetric = unsat = 0
    for k, p_w1 in enumerate((0.0, 0.3, 1.0)):
        if max(WIDTHS[w]) > 200 and k != 1:
            continue
        g = graphgen.random_levelized(9100 + 10 * w + k, widths=WIDTHS[w], R=3, p_w1=p_w1, dup_edges=True, extra_edges=0.6 if max(WIDTHS[w]) > 200 else 1.2, p_colour=0.5)
        m = PathModel(g)
        gpu_ctx.dp_load_graph(g)
        rng = np.random.default_rng(50 + w)
        classes = class_arrays(g, 31 + w)
        sets = list(_edge_sets(g, m, rng).items())
        for n, b in enumerate(BUDGETS):
            free = gpu_ctx.dp_genotype_margins(_called(m, rng)[:1], b)[1]
            for x in range(2):
                tag, pins = sets[(2 * n + x + k) % len(sets)]
                T, V = _compare(gpu_ctx, g, m, b, pins, _called(m, rng), classes if b in (2, 18) else classes[2:], (w, p_w1, tag))
                assert V <= free
                lowered += NEG_INF < V < free
                unsat += V == NEG_INF and free != NEG_INF
                asymmetric += any(not np.array_equal(t, t.T) for t in T)
    if max(WIDTHS[w]) >= 63:
        assert asymmetric >= 1 and lowered >= 1, (asymmetric, lowered, unsat)


def _same(a, c):
    return len(a) == len(c) and all(np.array_equal(x, y) for x, y in zip(a, c))


def test_no_pins_is_the_unpinned_call(gpu_ctx):
    """n_pins = 0: every output and every statistic of the twin, and no mask launch"""
    g = graphgen.random_levelized(9130, widths=[1, 3, 64, 65, 2, 1], R=3, p_w1=0.3, dup_edges=True, extra_edges=1.2, p_colour=0.5)
    m = PathModel(g)
    gpu_ctx.dp_load_graph(g)
    called = _called(m, np.random.default_rng(3))
    none = np.zeros((0, 4), np.int32)
    for b in (0, 2, 7):
        for cls in (None, class_arrays(g, 51)[2]):
            for nbytes in (0, 1):
                with gpu_ctx.dp_options(joint_state_bytes=nbytes):
                    gpu_ctx.dp_genotype_margins_pinned([(2, -1, int(g.level_off[2]), FORBID)], called, b, cls)      # so that zeros below are this call's
                    want = gpu_ctx.dp_genotype_margins(called, b, cls, want_vertices=True)
                    stats = gpu_ctx.dp_genotype_stats()
                    assert _same(want, gpu_ctx.dp_genotype_margins_pinned(none, called, b, cls, want_vertices=True))
                    assert gpu_ctx.dp_genotype_stats() == stats and gpu_ctx.dp_genotype_pin_stats() == dict(pins=0, mask_launches=0)
                    assert _same(want, gpu_ctx.dp_genotype_margins_pinned([], called, b, cls, want_vertices=True))
                    gpu_ctx.dp_genotype_table_pinned([(2, -1, int(g.level_off[2]), FORBID)], b, cls)
                    assert gpu_ctx.dp_genotype_pin_stats() == dict(pins=1, mask_launches=2)
                    want = gpu_ctx.dp_genotype_table(b, cls, called)
                    stats = gpu_ctx.dp_genotype_stats()
                    assert _same(want, gpu_ctx.dp_genotype_table_pinned(none, b, cls, called))
                    assert gpu_ctx.dp_genotype_stats() == stats and gpu_ctx.dp_genotype_pin_stats() == dict(pins=0, mask_launches=0)
                    assert _same(gpu_ctx.dp_genotype_table(b, cls), gpu_ctx.dp_genotype_table_pinned(none, b, cls))


def _segments(g, b, nbytes):
    """first levels of the segments: levels are packed greedily while their forward states (4 * width^2 * (b + 1) bytes) fit nbytes, at
    least one level per segment (include/dipgenie_hip.h)"""
    state = 4 * (np.diff(g.level_off).astype(np.int64) ** 2) * (b + 1)
    seg, acc = [0], 0
    for l in range(g.n_levels):
        if l > seg[-1] and acc + state[l] > nbytes:
            seg.append(l)
            acc = 0
        acc += state[l]
    return seg


def test_segments_change_nothing(gpu_ctx):
    """joint_state_bytes = 1, ragged and default: identical outputs; one pinned level is a segment's first, one its last, one inside;
    a pinned level is masked after every forward launch that writes it and once after its backward launch"""
    g = graphgen.random_levelized(9801, widths=[1, 8, 8, 8, 8, 40, 8, 8, 8, 1], R=3, p_w1=0.3, dup_edges=True, extra_edges=1.2, p_colour=0.5)
    m = PathModel(g)
    L, b = g.n_levels, 7
    gpu_ctx.dp_load_graph(g)
    ragged = 4 * 1600
    seg = _segments(g, b, ragged)
    assert seg == [0, 4, 5, 6]
    pinned = [6, 3, 2, 7]                                # a segment's first level, a segment's last, two inside
    assert pinned[0] in seg and pinned[1] + 1 in seg and all(l not in seg and l + 1 not in seg for l in pinned[2:])
    rng = np.random.default_rng(98)
    pick = lambda l: int(rng.integers(g.level_off[l], g.level_off[l + 1]))
    pins = [p for l in pinned for p in ((l, pick(l), -1, FORBID), (l, -1, pick(l), FORBID), (l, pick(l), pick(l), FORBID))]
    called = _called(m, rng)
    cls = class_arrays(g, 52)[2]
    got = {}
    for name, nbytes in (("every level", 1), ("ragged", ragged), ("default", 0)):
        with gpu_ctx.dp_options(joint_state_bytes=nbytes):
            got[name] = list(gpu_ctx.dp_genotype_margins_pinned(pins, called, b, cls, want_vertices=True))
            first = _segments(g, b, nbytes if nbytes else 8 << 30)
            assert gpu_ctx.dp_genotype_stats()["n_segments"] == len(first)
            # pass 1 writes levels 1 .. the last segment's first level (if there are two segments or more), a segment's recompute the
            # levels behind its first one
            writes = sum((len(first) > 1 and l <= first[-1]) + (l not in first) for l in pinned)
            assert gpu_ctx.dp_genotype_pin_stats() == dict(pins=len(pins), mask_launches=writes + len(pinned)), (name, writes)
            got[name] += list(gpu_ctx.dp_genotype_table_pinned(pins, b, cls, called))
            assert gpu_ctx.dp_genotype_pin_stats() == dict(pins=len(pins), mask_launches=writes + len(pinned)), (name, writes)
    for name in ("ragged", "default"):
        assert _same(got["every level"], got[name]), name
    _compare(gpu_ctx, g, m, b, pins, called, [cls], "segments")
    assert gpu_ctx.dp_genotype_margins(called, b, cls)[1] >= got["default"][1]


def _require_cell(pins, l, v1, v2):
    """P + require (l, v1, v2) as one pin set whose only allowed cell of level l is (v1, v2) -- None if P does not allow the cell (a
    second require-pin of a level widens it, so P's own require-pins of the level go)"""
    pins = [tuple(int(x) for x in p) for p in pins]
    if not cell_allowed(pins, l, v1, v2):
        return None
    return [p for p in pins if not (p[0] == l and p[3] == REQUIRE)] + [(l, v1, v2, REQUIRE)]


@pytest.mark.parametrize("b", [2, 18])
def test_wider_than_any_tile_without_a_model(gpu_ctx, b):
    """widths [1, 130, 300, 129, 1]: T(cell | P) is dp_run_pinned(P + require-ordered(cell)), best_value is dp_run_pinned(P), requiring
    both orders of a cell gives its entry in the unpinned table, T(. | P) <= T(.)"""
    g, m, planes = wide_case(gpu_ctx)
    L = g.n_levels
    answer = gpu_ctx.dp_answer_paths(b)
    rng = np.random.default_rng(60 + b)
    pick = lambda l: int(rng.choice(np.setdiff1d(np.arange(g.level_off[l], g.level_off[l + 1]), answer[:, l])))      # (never a vertex of the answer)
    # the answer's ordered cell of a level where its paths differ goes (its mirror stays, and the mirrored answer satisfies the rest), a
    # column of level 1, a row of level 3, and half the rows of level 1 required, the answer's two among them
    lf = next(l for l in range(1, L - 1) if answer[0][l] != answer[1][l])
    P = ([(lf, int(answer[0][lf]), int(answer[1][lf]), FORBID), (1, -1, pick(1), FORBID), (3, pick(3), -1, FORBID), (1, int(answer[0][1]), -1, REQUIRE), (1, int(answer[1][1]), -1, REQUIRE)]
         + [(1, pick(1), -1, REQUIRE) for _ in range(60)])
    off_u, entries_u, free = gpu_ctx.dp_genotype_table(b)
    rows_u = _entry_rows(entries_u)
    assert free == planes[b] != NEG_INF
    J_u = gpu_ctx.dp_genotype_margins(answer, b, want_vertices=True)[2]
    # 14 queries x 3 inner levels = 42 cells: the answer in both orders, reachable cells of the unpinned table, random cells
    called = np.zeros((14, 2, L), np.int32)
    called[:, :, L - 1] = g.n_vertices - 1
    called[0], called[1] = answer, answer[::-1]
    for q in range(2, 14):
        for l in range(1, L - 1):
            if q < 9:
                e = rows_u[int(rng.integers(off_u[l], off_u[l + 1]))]
                called[q, :, l] = (e[2], e[3]) if q % 2 else (e[3], e[2])
            else:
                called[q, :, l] = (pick(l), pick(l))
    off, entries, best, levels = gpu_ctx.dp_genotype_table_pinned(P, b, None, called)
    levels2, best2, J = gpu_ctx.dp_genotype_margins_pinned(P, called, b, want_vertices=True)
    assert gpu_ctx.dp_genotype_pin_stats() == dict(pins=len(P), mask_launches=2 * _n_levels(P))
    assert best == best2 and np.array_equal(_rows(levels), _rows(levels2))
    assert best == gpu_ctx.dp_run_pinned(P, [b])[0].value and NEG_INF < best <= free
    reached = refused = 0
    for q in range(14):
        for l in range(1, L - 1):
            c1, c2 = int(called[q, 0, l]), int(called[q, 1, l])
            pins = _require_cell(P, l, c1, c2)
            want = NEG_INF if pins is None else gpu_ctx.dp_run_pinned(pins, [b])[0].value
            assert levels["value"][q, l] == want, (q, l, c1, c2, levels[q, l], want)
            reached += want != NEG_INF
            refused += pins is None
    assert reached >= 10 and refused >= 1
    assert levels["value"][0, lf] == NEG_INF and levels["value"][1, lf] == free      # the ordered forbid: T is not symmetric
    # T(. | P) <= T(.): every cell the pinned table lists is listed by the unpinned one with at least its value; J likewise
    rows = _entry_rows(entries)
    assert 0 < len(rows) < len(rows_u) and (np.maximum.reduceat(rows[:, 4], off[:-1]) == best).all()
    key_u = rows_u[:, 2] * g.n_vertices + rows_u[:, 3]
    at = np.searchsorted(key_u, rows[:, 2] * g.n_vertices + rows[:, 3])
    assert (key_u[at] == rows[:, 2] * g.n_vertices + rows[:, 3]).all() and (rows[:, 4] <= rows_u[at, 4]).all() and (rows[:, 4] < rows_u[at, 4]).any()
    assert (J <= J_u).all() and (J < J_u).any()
    # both orders of a cell required: the optimum is that cell's entry in the unpinned table
    for l in range(1, L - 1):
        for x in rng.integers(off_u[l], off_u[l + 1], 3):
            e = rows_u[int(x)]
            _, v = gpu_ctx.dp_genotype_margins_pinned(capi.genotype_pins(l, int(e[2]), int(e[3])), answer, b)
            assert v == e[4], (l, e, v)


def test_the_calls_leave_a_run_alone(gpu_ctx):
    g = graphgen.random_levelized(9401, n_levels=30, max_width=9, R=4, p_colour=0.5)
    m = PathModel(g)
    gpu_ctx.dp_load_graph(g)
    rng = np.random.default_rng(5)
    budgets = list(range(g.R + 1))
    called = _called(m, rng)
    cls = class_arrays(g, 9401)[2]
    run_pins = random_pins(m, rng, 4, 2)
    joint_pins = random_pins(m, rng, 6, 2)

    def snapshot():
        return ([(o.value, o.s_het, tuple(o.p1), tuple(o.p2)) for o in outs], gpu_ctx.dp_budget_values().tolist(), [gpu_ctx.dp_answer_paths(b).tolist() for b in budgets],
                gpu_ctx.dp_pin_stats(), [getattr(gpu_ctx.dp_timing(), f) for f, _ in capi.DpTiming._fields_])

    outs = gpu_ctx.dp_run_pinned(run_pins, budgets)
    before = snapshot()
    first = list(gpu_ctx.dp_genotype_margins_pinned(joint_pins, called, g.R, cls, want_vertices=True)) + list(gpu_ctx.dp_genotype_table_pinned(joint_pins, g.R, cls, called))
    assert snapshot() == before
    with pytest.raises(capi.DgError, match=r"rc=-6\): dg_dp_call_margins: the last run was dg_dp_run_pinned"):      # still "the last run"
        gpu_ctx.dp_call_margins(g.R)
    assert gpu_ctx.dp_genotype_margins_pinned(run_pins, called, g.R)[1] == before[1][g.R]
    outs = gpu_ctx.dp_run_budgets(budgets)
    before = snapshot()
    again = list(gpu_ctx.dp_genotype_margins_pinned(joint_pins, called, g.R, cls, want_vertices=True)) + list(gpu_ctx.dp_genotype_table_pinned(joint_pins, g.R, cls, called))
    assert _same(first, again) and snapshot() == before
    levels, _ = gpu_ctx.dp_call_margins(g.R)             # and the unpinned run is still an unpinned run
    assert (levels["value"] == before[1][g.R]).all()


def test_an_unsatisfiable_set_is_an_answer(gpu_ctx):
    g = graphgen.random_levelized(9400, widths=[1, 65, 65, 65, 1], R=3, p_w1=0.3, extra_edges=1.2, p_colour=0.5)
    m = PathModel(g)
    gpu_ctx.dp_load_graph(g)
    L = g.n_levels
    indeg = np.bincount(g.out_dst, minlength=g.n_vertices)
    dead = int(next(v for v in range(int(g.level_off[1]), int(g.level_off[2])) if indeg[v] == 0))     # a vertex nothing reaches
    a0 = int(g.level_off[1])
    called = _called(m, np.random.default_rng(8))
    for pins in ([(1, dead, -1, REQUIRE)], [(2, -1, -1, REQUIRE), (1, -1, dead, REQUIRE)], [(1, a0, -1, REQUIRE), (1, -1, a0 + 1, REQUIRE), (1, a0, -1, FORBID), (1, -1, a0 + 1, FORBID)],
                 [(3, -1, -1, FORBID)]):
        for b in (0, 3):
            levels, best, J = gpu_ctx.dp_genotype_margins_pinned(pins, called, b, want_vertices=True)
            assert best == NEG_INF and (J == NEG_INF).all()
            want = np.concatenate([called.transpose(0, 2, 1), np.broadcast_to(np.array([NEG_INF, -1, -1, NEG_INF]), (len(called), L, 4))], axis=-1)
            assert np.array_equal(_rows(levels), want)
            off, entries, best, levels2 = gpu_ctx.dp_genotype_table_pinned(pins, b, None, called)
            assert best == NEG_INF and len(entries) == 0 and (off == 0).all() and off.shape == (L + 1,) and np.array_equal(_rows(levels2), want)
            ptr, cnt, bv = capi.C.c_void_p(77), capi.C.c_int64(-7), capi.C.c_int32(-7)
            p = np.array(pins, np.int32)
            assert capi.lib.dg_dp_genotype_table_pinned(gpu_ctx.h, p.ctypes.data, len(p), b, None, None, 0, None, off.ctypes.data, capi.C.byref(ptr), capi.C.byref(cnt), capi.C.byref(bv)) == 0
            assert ptr.value is None and cnt.value == 0 and bv.value == NEG_INF
    assert gpu_ctx.dp_genotype_margins(called, 3)[1] != NEG_INF


def test_errors_name_the_entry_point_and_write_nothing(gpu_ctx):
    g = enumerable_graph(1)
    m = PathModel(g)
    gpu_ctx.dp_load_graph(g)
    L = g.n_levels
    a0, a1 = int(g.level_off[1]), int(g.level_off[2])
    good = (1, a0, -1, REQUIRE)
    called = _called(m, np.random.default_rng(6))
    n = len(called)
    gpu_ctx.dp_genotype_table_pinned([good], 2, None, called)
    stats, pin_stats = gpu_ctx.dp_genotype_stats(), gpu_ctx.dp_genotype_pin_stats()
    bad = [((0, 0, 0, REQUIRE), "level 0"), ((L - 1, -1, -1, REQUIRE), f"level {L - 1}"), ((-3, -1, -1, FORBID), "level -3"), ((1, a1, -1, REQUIRE), f"vertex1 {a1}"),
           ((1, -1, a0 - 1, REQUIRE), f"vertex2 {a0 - 1}"), ((1, -2, -1, FORBID), "vertex1 -2"), ((1, a0, a0, 2), "kind 2"), ((1, a0, a0, -1), "kind -1")]
    rec = np.full((n, L, 8), -7, np.int32)
    vv = np.full(g.n_vertices, -7, np.int32)
    off = np.full(L + 1, -7, np.int64)
    ptr, cnt, best = capi.C.c_void_p(77), capi.C.c_int64(-7), capi.C.c_int32(-7)

    def margins(p, n_pins, b=2, c=called, count=n):
        return capi.lib.dg_dp_genotype_margins_pinned(gpu_ctx.h, p.ctypes.data if p is not None else None, n_pins, c.ctypes.data, count, b, None, rec.ctypes.data, vv.ctypes.data,
                                                      capi.C.byref(best))

    def table(p, n_pins, b=2, c=called, count=n):
        return capi.lib.dg_dp_genotype_table_pinned(gpu_ctx.h, p.ctypes.data if p is not None else None, n_pins, b, None, c.ctypes.data, count, rec.ctypes.data, off.ctypes.data,
                                                    capi.C.byref(ptr), capi.C.byref(cnt), capi.C.byref(best))

    def untouched():
        return (rec == -7).all() and (vv == -7).all() and (off == -7).all() and ptr.value == 77 and cnt.value == -7 and best.value == -7

    for call, name in ((margins, "dg_dp_genotype_margins_pinned"), (table, "dg_dp_genotype_table_pinned")):
        for pin, what in bad:
            for at, pins in ((0, [pin, good]), (2, [good, good, pin, (0, 0, 0, 7)])):          # the FIRST offending pin is named
                p = np.array(pins, np.int32)
                assert call(p, len(p)) == -1 and untouched()
                msg = capi.lib.dg_last_error().decode()
                assert msg.startswith(f"{name}: pin {at}: ") and what in msg, msg
        p = np.tile(np.array([good], np.int32), (65537, 1))
        assert call(p, 65537) == -1 and capi.lib.dg_last_error().decode().startswith(f"{name}: n_pins = 65537") and untouched()
        assert call(p, -1) == -1 and capi.lib.dg_last_error().decode().startswith(f"{name}: n_pins = -1") and untouched()
        assert call(None, 3) == -1 and capi.lib.dg_last_error().decode().startswith(f"{name}: null pins") and untouched()
        # the twins' limits, under the new names
        p = np.array([good], np.int32)
        assert call(p, 1, b=-1) == -1 and capi.lib.dg_last_error().decode().startswith(f"{name}: budget -1") and untouched()
        assert call(p, 1, b=4096) == -5 and capi.lib.dg_last_error().decode().startswith(f"{name}: ") and b"4097" in capi.lib.dg_last_error() and untouched()
        many = np.repeat(called[:1], 257, axis=0)
        assert call(p, 1, c=many, count=257) == -5 and capi.lib.dg_last_error().decode().startswith(f"{name}: 257 called") and untouched()
        wrong = called.copy()
        wrong[1, 1, 2] = g.level_off[3]
        assert call(p, 1, c=wrong) == -1 and capi.lib.dg_last_error().decode().startswith(f"{name}: query 1 row 1 level 2") and untouched()
    assert gpu_ctx.dp_genotype_stats() == stats and gpu_ctx.dp_genotype_pin_stats() == pin_stats
    with pytest.raises(capi.DgError, match=r"rc=-1\): dg_dp_genotype_margins_pinned: pin 0: .*level 0"):
        gpu_ctx.dp_genotype_margins_pinned([(0, 0, 0, REQUIRE)], called, 2)
    with pytest.raises(capi.DgError, match=r"rc=-1\): dg_dp_genotype_table_pinned: pin 1: .*kind 2"):
        gpu_ctx.dp_genotype_table_pinned([good, (1, a0, a0, 2)], 2)
    # the limit itself, all duplicates: the answer of one pin
    one = gpu_ctx.dp_genotype_margins_pinned([good], called, 2, want_vertices=True)
    assert _same(one, gpu_ctx.dp_genotype_margins_pinned(np.tile(np.array([good], np.int32), (65536, 1)), called, 2, want_vertices=True))
    assert gpu_ctx.dp_genotype_pin_stats() == dict(pins=65536, mask_launches=2)
    fresh = capi.Context(0)
    try:
        with pytest.raises(capi.DgError, match=r"rc=-6.*dg_dp_genotype_table_pinned: no graph loaded"):
            fresh.dp_genotype_table_pinned([good], 0)
    finally:
        fresh.close()

"""-m gpu: dg_dp_genotype_table / Context.dp_genotype_table -- per level and genotype the best pair of paths through any cell of that
genotype, and that cell; optionally the margin records of dp_genotype_margins from the same pass.

Integers only: every comparison is exact.  The yardstick is tests/genotype_table_model.py, itself pinned to brute force by
tests/test_genotype_table_model.py; the tests on the widest graph need no model: they hold the table against dp_genotype_margins and
the run's planes."""
import numpy as np
import pytest

import graphgen
from call_margins_model import class_arrays
from dipgenie_amd import capi
from genotype_margins_model import through_values_np
from genotype_table_model import FIELDS, genotype_table_np, record_from_table, vertex_maxima_from_table
from paths_model import NEG_INF, PathModel
from test_gpu_genotype_margins import BUDGETS, WIDTHS, _called, _rows, wide_case
from test_gpu_score_paths import ENUMERABLE
from test_partner_model import enumerable_graph

pytestmark = pytest.mark.gpu

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
ENTRY_BYTES = 24


def _entry_rows(entries):
    assert (entries["reserved"] == 0).all()
    assert (entries["vertex1"] <= entries["vertex2"]).all() and (entries["class1"] <= entries["class2"]).all()
    return np.stack([entries[f] for f in FIELDS], axis=-1).astype(np.int64).reshape(-1, 5)


def _signed_classes(g, seed):
    """arbitrary int32 values, both ends of the range among them: the order of the classes is the signed one"""
    return np.random.default_rng(seed).choice(np.array([INT32_MIN, -70000, -1, 0, 5, INT32_MAX], np.int64), g.n_vertices).astype(np.int32)


def _bounds(g, cls):
    """per level A (A + 1) / 2, A = its distinct classes"""
    out = []
    for l in range(g.n_levels):
        a, e = int(g.level_off[l]), int(g.level_off[l + 1])
        A = e - a if cls is None else len(set(np.asarray(cls[a:e]).tolist()))
        out.append(A * (A + 1) // 2)
    return np.array(out, np.int64)


def _compare(ctx, g, m, b, classes, tag, T=None, V=None):
    """level_off, every field of every entry, n_entries and best_value against the numpy model, for each class array -> per class
    array (level_off, rows)"""
    if T is None:
        T, V = through_values_np(m, b)
    out = []
    for kind, cls in enumerate(classes):
        want_off, want = genotype_table_np(m, T, cls)
        off, entries, best = ctx.dp_genotype_table(b, cls)
        rows = _entry_rows(entries)
        assert best == V, (tag, b, kind, best, V)
        assert off.dtype == np.int64 and off.shape == (g.n_levels + 1,) and np.array_equal(off, want_off), (tag, b, kind, off, want_off)
        assert len(entries) == off[-1] == ctx.dp_genotype_stats()["entries"]
        bad = np.flatnonzero((rows != want).any(axis=1))
        assert bad.size == 0, (tag, b, kind, bad[:5], rows[bad[:5]], want[bad[:5]])
        if V != NEG_INF:                                 # on every level the largest value is V_b
            assert (np.maximum.reduceat(rows[:, 4], off[:-1]) == V).all()
        else:
            assert len(entries) == 0 and (off == 0).all()
        assert (off[1:] - off[:-1] <= _bounds(g, cls)).all()
        out.append((off, rows))
    return out


@pytest.mark.parametrize("q", range(len(ENUMERABLE)))
def test_device_equals_model_on_the_enumerable_graphs(gpu_ctx, q):
    g = enumerable_graph(q)
    m = PathModel(g)
    gpu_ctx.dp_load_graph(g)
    for b in range(4):
        _compare(gpu_ctx, g, m, b, class_arrays(g, 21 + q), q)


def _prescribed(w, k):
    return graphgen.random_levelized(9100 + 10 * w + k, widths=WIDTHS[w], R=3, p_w1=(0.0, 0.3, 1.0)[k], dup_edges=True, extra_edges=1.2, p_colour=0.5)


@pytest.mark.parametrize("w", range(len(WIDTHS)))
def test_device_equals_model_on_prescribed_widths(gpu_ctx, w):
    """and facts about these inputs (found with the numpy model), asserted so that the inputs cannot erode: unreachable genotypes
    exist and are left out, the drawn classes fill their bound, several genotypes tie at V_b, p_w1 = 1 at b = 2 is the empty table"""
    for k, p_w1 in enumerate((0.0, 0.3, 1.0)):
        g = _prescribed(w, k)
        m = PathModel(g)
        gpu_ctx.dp_load_graph(g)
        classes = class_arrays(g, 31 + w) + [_signed_classes(g, 61 + w)]
        assert classes[3].min() == INT32_MIN and classes[3].max() == INT32_MAX or g.n_vertices < 20
        for b in BUDGETS:
            got = _compare(gpu_ctx, g, m, b, classes, (w, p_w1))
            n_null, n_drawn = int(got[0][0][-1]), int(got[2][0][-1])
            if p_w1 == 1.0 and b == 2 and len(WIDTHS[w]) >= 4:
                assert n_null == 0                       # every path has L - 1 recombinations: the empty table
            elif max(WIDTHS[w]) >= 63 and n_null:
                assert 0 < n_null < _bounds(g, None).sum()                  # unreachable genotypes are really left out
            if w == 2 and b == 2 and k == 0:
                assert (n_null, int(_bounds(g, None).sum())) == (2105, 4236)
                assert n_drawn == _bounds(g, classes[2]).sum() == 21 and (got[2][0][1:] - got[2][0][:-1]).max() == 10
            if w == 2 and k == 1 and b in (2, 18):       # three levels where two or more genotypes are worth V_b
                off, rows = got[2]
                V = rows[:, 4].max()
                assert sum(int((rows[off[l]:off[l + 1], 4] == V).sum() >= 2) for l in range(g.n_levels)) == 3


def _tables(ctx, g, b, classes, called):
    out = []
    for cls in classes:
        off, entries, best, levels = ctx.dp_genotype_table(b, cls, called)
        out.append((off, entries, best, levels))
    return out


def _same(a, c):
    return all(np.array_equal(x, y) for one, two in zip(a, c) for x, y in zip(one, two))


SMALLEST = dict(genotype_table_tile_keys=256, genotype_table_scan_tiles=64)     # the smallest legal values of the compaction's two sizes


@pytest.mark.parametrize("w", range(len(WIDTHS)))
def test_forced_thresholds_change_nothing(gpu_ctx, w):
    """the graphs, budgets and classes of the test above: genotype_table_lanes at both ends of its range, the compaction's tile and
    scan pass at their smallest, genotype_table_bytes at exactly the largest level's bound; one byte less is refused before anything
    is launched"""
    empty = 0
    for k in range(3):
        g = _prescribed(w, k)
        m = PathModel(g)
        gpu_ctx.dp_load_graph(g)
        classes = class_arrays(g, 31 + w) + [_signed_classes(g, 61 + w)]
        called = _called(m, np.random.default_rng(7))
        for b in BUDGETS:
            want = _tables(gpu_ctx, g, b, classes, called)
            n_last = len(want[-1][1])
            assert gpu_ctx.dp_genotype_stats()["staging_copies"] == (1 if n_last else 0)
            empty += n_last == 0
            for forced in (dict(genotype_table_lanes=1), dict(genotype_table_lanes=64), SMALLEST, dict(SMALLEST, genotype_table_lanes=1)):
                with gpu_ctx.dp_options(**forced):
                    assert _same(want, _tables(gpu_ctx, g, b, classes, called)), (k, b, forced)
            for kind, cls in enumerate(classes):
                bounds = _bounds(g, cls)
                with gpu_ctx.dp_options(genotype_table_bytes=int(bounds.max()) * ENTRY_BYTES, **SMALLEST):
                    assert _same(want[kind:kind + 1], _tables(gpu_ctx, g, b, [cls], called)), (k, b, kind)
                    stats = gpu_ctx.dp_genotype_stats()
                    assert stats["entries"] == len(want[kind][1])
                    assert stats["staging_copies"] > 1 if stats["entries"] else stats["staging_copies"] == 0
                with gpu_ctx.dp_options(genotype_table_bytes=int(bounds.max()) * ENTRY_BYTES - 1):
                    off = np.full(g.n_levels + 1, -7, np.int64)
                    ptr, n, best = capi.C.c_void_p(77), capi.C.c_int64(-7), capi.C.c_int32(-7)
                    rc = capi.lib.dg_dp_genotype_table(gpu_ctx.h, b, cls.ctypes.data if cls is not None else None, None, 0, None, off.ctypes.data, capi.C.byref(ptr),
                                                       capi.C.byref(n), capi.C.byref(best))
                    msg = capi.lib.dg_last_error().decode()
                    l_bad = int(np.argmax(bounds > bounds.max() - 1))
                    assert rc == -5 and f"level {l_bad}:" in msg and str(int(bounds.max())) in msg and str(int(bounds.max()) * ENTRY_BYTES - 1) in msg, msg
                    assert (off == -7).all() and ptr.value == 77 and n.value == -7 and best.value == -7
                    assert gpu_ctx.dp_genotype_stats() == stats
    assert empty >= 1                                    # p_w1 = 1 at the small budgets: the empty table under every forced value too
    assert gpu_ctx.dp_get_option("genotype_table_bytes") == 256 << 20 and gpu_ctx.dp_get_option("genotype_table_lanes") == 0
    assert gpu_ctx.dp_get_option("genotype_table_tile_keys") == 2048 and gpu_ctx.dp_get_option("genotype_table_scan_tiles") == 1024


def test_option_values_are_rounded_into_their_range(gpu_ctx):
    for key, lo, step, hi in (("genotype_table_tile_keys", 256, 256, 2048), ("genotype_table_scan_tiles", 64, 64, 1024)):
        for v, stored in ((1, lo), (lo + step + 1, lo + step), (10 ** 9, hi), (0, hi), (-3, hi)):
            with gpu_ctx.dp_options(**{key: v}):
                assert gpu_ctx.dp_get_option(key) == stored, (key, v)


@pytest.mark.parametrize("b", [2, 18])
def test_wider_than_any_tile(gpu_ctx, b):
    """widths [1, 130, 300, 129, 1]: against dp_genotype_margins and the run's plane without a model at both budgets; at b = 2 the
    NULL-class table also against the numpy model, row for row (every reachable upper-triangle cell and no other).  With the tile at 256
    keys and the scan at 64 tiles per pass the 45,150 keys of the widest level are 177 tiles and three passes of the scan"""
    g, m, planes = wide_case(gpu_ctx)
    V = planes[b]
    assert V != NEG_INF
    rng = np.random.default_rng(70 + b)
    cells = np.array([[[rng.integers(m.level_off[l], m.level_off[l + 1]) for l in range(m.L)] for _ in range(2)] for _ in range(3)], np.int32)
    called = np.concatenate([gpu_ctx.dp_answer_paths(b)[None], cells]).astype(np.int32)
    for cls in (None, class_arrays(g, 41)[2]):
        off, entries, best, levels = gpu_ctx.dp_genotype_table(b, cls, called)
        rows = _entry_rows(entries)
        want, best2, J = gpu_ctx.dp_genotype_margins(called, b, cls, want_vertices=True)
        assert best == best2 == V
        for f in want.dtype.names:                       # the same records, field by field
            assert np.array_equal(levels[f], want[f]), f
        assert (np.maximum.reduceat(rows[:, 4], off[:-1]) == V).all()      # the level maxima equal the plane
        derived = 0
        for q in range(len(called)):                     # every record is derivable from the table
            for l in range(m.L):
                rec = want[q, l]
                got = record_from_table(rows[off[l]:off[l + 1]], int(rec["vertex1"]), int(rec["vertex2"]), cls)
                assert got[1:] == (rec["alt_vertex1"], rec["alt_vertex2"], rec["alt_value"]), (q, l)
                if got[0] is not None:
                    assert got[0] == rec["value"]
                    derived += 1
                else:
                    assert cls is not None or rec["value"] == NEG_INF
        top = vertex_maxima_from_table(m, off, rows, cls)
        assert (J <= top).all()
        if cls is None:                                  # the entries of a level are its reachable upper-triangle cells
            assert derived >= m.L                        # the run's answer is a reachable cell on every level
            assert np.array_equal(top, J)
            assert np.array_equal(rows[:, 0], rows[:, 2]) and np.array_equal(rows[:, 1], rows[:, 3])
            per_level = off[1:] - off[:-1]
            assert per_level[2] > 300 and (per_level <= _bounds(g, None)).all()
            key = rows[:, 2] * g.n_vertices + rows[:, 3]
            assert (np.diff(key) > 0).all()
            reach = J != NEG_INF                         # a cell (v, v') is listed only between reachable vertices, and every reachable vertex is in one
            assert reach[rows[:, 2]].all() and reach[rows[:, 3]].all()
            assert np.array_equal(np.unique(rows[:, 2:4]), np.flatnonzero(reach))
            if b == 2:                                   # a host recount of every level: the model's rows
                T, Vm = through_values_np(m, b)
                want_off, want_rows = genotype_table_np(m, T, None)
                assert Vm == V and np.array_equal(off, want_off) and np.array_equal(rows, want_rows)
        assert 300 * 301 // 2 > 64 * 256 * 2             # more than two passes of the smallest scan over the smallest tiles
        with gpu_ctx.dp_options(**SMALLEST):
            off2, entries2, best3, levels2 = gpu_ctx.dp_genotype_table(b, cls, called)
        assert best3 == best and np.array_equal(off2, off) and np.array_equal(entries2, entries) and np.array_equal(levels2, levels)


def test_segments_change_nothing(gpu_ctx):
    g = _prescribed(2, 1)
    m = PathModel(g)
    gpu_ctx.dp_load_graph(g)
    b = 7
    called = _called(m, np.random.default_rng(3))
    cls = class_arrays(g, 51)[2]
    state = 4 * (np.diff(g.level_off).astype(np.int64) ** 2) * (b + 1)
    got = {}
    for name, nbytes in (("every level", 1), ("ragged", int(2.5 * state.mean())), ("default", 0)):
        with gpu_ctx.dp_options(joint_state_bytes=nbytes):
            got[name] = [gpu_ctx.dp_genotype_table(b, c, called) for c in (None, cls)]
        got[name + " stats"] = gpu_ctx.dp_genotype_stats()
    for name in ("ragged", "default"):
        assert _same(got["every level"], got[name]), name
    assert got["every level stats"]["n_segments"] == g.n_levels == got["every level stats"]["staging_copies"]
    assert 1 < got["ragged stats"]["n_segments"] < g.n_levels and got["ragged stats"]["staging_copies"] == got["ragged stats"]["n_segments"]
    assert got["default stats"]["n_segments"] == 1 == got["default stats"]["staging_copies"]
    for name in ("every level", "ragged", "default"):    # what the table reserves counts: T of the widest level and the staging at least
        assert got[name + " stats"]["peak_bytes"] >= int(state.max()) + 4 * 65 * 65 + ENTRY_BYTES * len(got[name][1][1])


def test_the_call_leaves_the_run_alone_and_the_old_entry_point_as_it_was(gpu_ctx):
    g = graphgen.random_levelized(9401, n_levels=30, max_width=9, R=4, p_colour=0.5)
    m = PathModel(g)
    with gpu_ctx.dp_options(digest=1):
        gpu_ctx.dp_load_graph(g)
        outs = gpu_ctx.dp_run_budgets(range(g.R + 1))
        planes = gpu_ctx.dp_budget_values().copy()
        digest = gpu_ctx.dp_level_digest(g.n_levels).copy()
        paths = [gpu_ctx.dp_answer_paths(b).copy() for b in range(g.R + 1)]
        t = gpu_ctx.dp_timing()
        timing = [getattr(t, f) for f, _ in capi.DpTiming._fields_]
        called = _called(m, np.random.default_rng(5), paths[g.R])
        cls = class_arrays(g, 9401)[2]
        before = gpu_ctx.dp_genotype_margins(called, g.R, cls)
        launches = gpu_ctx.dp_genotype_stats()["launches"]
        assert gpu_ctx.dp_genotype_stats()["entries"] == 0
        first = [gpu_ctx.dp_genotype_table(b, cls, called) for b in (0, g.R, g.R + 3)]
        assert gpu_ctx.dp_genotype_stats()["launches"] > launches           # the table's own kernels are counted in its call
        assert np.array_equal(gpu_ctx.dp_budget_values(), planes) and np.array_equal(gpu_ctx.dp_level_digest(g.n_levels), digest)
        for b in range(g.R + 1):
            assert np.array_equal(gpu_ctx.dp_answer_paths(b), paths[b])
            assert gpu_ctx.dp_genotype_table(b)[2] == planes[b]
        t = gpu_ctx.dp_timing()
        assert [getattr(t, f) for f, _ in capi.DpTiming._fields_] == timing
        again = [gpu_ctx.dp_genotype_table(b, cls, called) for b in (0, g.R, g.R + 3)]
        assert _same(first, again)
        # the launch count of a plain margins call is what it was before any table call
        after = gpu_ctx.dp_genotype_margins(called, g.R, cls)
        assert gpu_ctx.dp_genotype_stats()["launches"] == launches and gpu_ctx.dp_genotype_stats()["entries"] == 0
        assert all(np.array_equal(x, y) for x, y in zip(before, after))
        assert [o.key() for o in gpu_ctx.dp_run_budgets(range(g.R + 1))] == [o.key() for o in outs]
        assert np.array_equal(gpu_ctx.dp_level_digest(g.n_levels), digest)


def test_errors_and_layout(gpu_ctx):
    assert capi.GENOTYPE_ENTRY.itemsize == ENTRY_BYTES and capi.GENOTYPE_ENTRY.names == FIELDS + ("reserved",)
    g = graphgen.random_levelized(9501, widths=[1, 4, 6, 3, 1], R=3, p_colour=0.5)
    m = PathModel(g)
    L = g.n_levels
    call = capi.lib.dg_dp_genotype_table
    fresh = capi.Context(0)
    try:
        with pytest.raises(capi.DgError, match=r"rc=-6.*dg_dp_genotype_table: no graph loaded"):
            fresh.dp_genotype_table(0)
    finally:
        fresh.close()
    gpu_ctx.dp_load_graph(g)
    called = _called(m, np.random.default_rng(6))
    n = len(called)
    rec = np.full((n, L, 8), -7, np.int32)
    off = np.full(L + 1, -7, np.int64)
    ptr, cnt, best = capi.C.c_void_p(77), capi.C.c_int64(-7), capi.C.c_int32(-7)

    def raw(b, p, count, levels, off_=off, ptr_=ptr, cnt_=cnt, best_=best):
        return call(gpu_ctx.h, b, None, p.ctypes.data if p is not None else None, count, levels.ctypes.data if levels is not None else None,
                    off_.ctypes.data if off_ is not None else None, capi.C.byref(ptr_) if ptr_ is not None else None, capi.C.byref(cnt_) if cnt_ is not None else None,
                    capi.C.byref(best_) if best_ is not None else None)

    def untouched():
        return (rec == -7).all() and (off == -7).all() and ptr.value == 77 and cnt.value == -7 and best.value == -7

    assert raw(2, called, n, None) == -1 and untouched()                  # called without levels
    assert raw(2, None, n, rec) == -1 and untouched()                     # levels without called
    assert raw(2, None, n, None) == -1 and raw(2, called, 0, rec) == -1 and raw(2, called, -1, rec) == -1 and untouched()
    assert raw(2, None, 0, None, off_=None) == -1 and raw(2, None, 0, None, ptr_=None) == -1 and untouched()
    assert raw(2, None, 0, None, cnt_=None) == -1 and raw(2, None, 0, None, best_=None) == -1 and untouched()
    assert raw(-1, None, 0, None) == -1 and b"budget -1" in capi.lib.dg_last_error() and untouched()
    assert raw(4096, None, 0, None) == -5 and b"4097" in capi.lib.dg_last_error() and untouched()
    many = np.repeat(called[:1], 257, axis=0)
    assert raw(2, many, 257, np.zeros((257, L, 8), np.int32)) == -5 and b"257" in capi.lib.dg_last_error() and untouched()
    bad = called.copy()
    bad[1, 1, 2] = g.level_off[3]
    assert raw(2, bad, n, rec) == -1 and b"query 1 row 1 level 2" in capi.lib.dg_last_error() and untouched()
    with pytest.raises(ValueError):
        gpu_ctx.dp_genotype_table(2, None, called[:, :, :-1])
    with pytest.raises(ValueError):
        gpu_ctx.dp_genotype_table(2, np.zeros(g.n_vertices - 1, np.int32))
    # the raw call: six words per entry, the last one 0; eight per record
    w_off, w_entries, V, w_levels = gpu_ctx.dp_genotype_table(2, None, called)
    assert raw(2, called, n, rec) == 0 and best.value == V and cnt.value == len(w_entries) == off[-1] and np.array_equal(off, w_off)
    words = np.ctypeslib.as_array(capi.C.cast(ptr, capi.C.POINTER(capi.C.c_int32)), (cnt.value * 6,)).reshape(-1, 6).copy()
    capi.lib.dg_free(ptr)
    assert np.array_equal(words[:, :5], _entry_rows(w_entries)) and (words[:, 5] == 0).all()
    assert np.array_equal(rec[:, :, :6], _rows(w_levels)) and (rec[:, :, 6:] == 0).all()
    want, V2 = gpu_ctx.dp_genotype_margins(called, 2)
    assert V2 == V and np.array_equal(_rows(want), _rows(w_levels))
    # without called the table is the same
    o2, e2, V3 = gpu_ctx.dp_genotype_table(2)
    assert V3 == V and np.array_equal(o2, w_off) and np.array_equal(e2, w_entries)


def test_a_budget_nobody_fits(gpu_ctx):
    """the chain of tests/test_gpu_genotype_margins.py whose one weight-1 edge both paths pay: no pair fits b = 0 or 1"""
    g = graphgen.random_levelized(9601, widths=[1, 1, 1, 1, 1], R=2, p_w1=0.0, dup_edges=False, extra_edges=0.0)
    w = g.out_w.copy()
    w[2] = 1
    g = capi.DpGraphArrays(g.R, **{**{name: getattr(g, name) for name in capi.DpGraphArrays.NAMES}, "out_w": w})
    gpu_ctx.dp_load_graph(g)
    called = np.arange(5, dtype=np.int32)[None, :].repeat(2, axis=0)
    for b in (0, 1):
        off, entries, best, levels = gpu_ctx.dp_genotype_table(b, None, called)
        assert best == NEG_INF and len(entries) == 0 and (off == 0).all() and off.shape == (6,)
        assert (_rows(levels)[0] == np.array([[v, v, NEG_INF, -1, -1, NEG_INF] for v in range(5)])).all()
        ptr, cnt, bv = capi.C.c_void_p(77), capi.C.c_int64(-7), capi.C.c_int32(-7)
        assert capi.lib.dg_dp_genotype_table(gpu_ctx.h, b, None, None, 0, None, off.ctypes.data, capi.C.byref(ptr), capi.C.byref(cnt), capi.C.byref(bv)) == 0
        assert ptr.value is None and cnt.value == 0 and bv.value == NEG_INF
        assert gpu_ctx.dp_genotype_stats()["entries"] == 0 == gpu_ctx.dp_genotype_stats()["staging_copies"]
    off, entries, best = gpu_ctx.dp_genotype_table(2)
    assert best != NEG_INF and off.tolist() == list(range(6))
    assert _entry_rows(entries).tolist() == [[v, v, v, v, best] for v in range(5)]

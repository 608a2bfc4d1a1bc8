"""-m gpu: the joint-pass kernels of dg_dp_joint.hip beyond their grid caps -- rows past JT_ROW_BLOCKS, lanes past JT_X_BLOCKS * 256,
in-edges past the grid of jt_scores_kernel, vertices past one chunk of jt_out_scan_kernel -- on the padded graphs of
tests/padded_graphs.py.

Integers only: every comparison is exact.  The yardstick is the numpy model of each entry point on the small BASE graph with the ids
remapped: pads are reached by nothing, so the device on the padded graph must give every real cell the base graph's value and NEG_INF /
no entry / no alternative on every pad (tests/test_padded_graphs.py checks that claim, and that every shape crosses its cap, on the CPU).
The lanes shape runs at budget 4,095 against the model at 2 (L - 1): beyond that budget nothing changes."""
import numpy as np
import pytest

import oracle_py as orc
import padded_graphs as pg
from call_margins_model import class_arrays
from genotype_budgets_model import genotype_margins_budgets_np
from genotype_margins_model import genotype_margins_np, through_values_np
from genotype_table_model import genotype_table_np
from pair_graphs import with_R
from paths_model import NEG_INF, PathModel
from phase_margins_model import joint_states_fb, phase_margins_np
from pinned_joint_model import pinned_genotype_margins_np, pinned_genotype_table_np, pinned_through_values_np
from pinned_model import FORBID, REQUIRE
from test_gpu_genotype_margins import MAX_PLANES, _called, _rows
from test_gpu_genotype_table import _entry_rows
from test_gpu_phase_margins import _rows as _phase_rows

pytestmark = pytest.mark.gpu

_CASES, _MODELS = {}, {}


class Case:
    """a shape: base graph g and its model m, padded graph gp, the id map, the pads, a 2..4-class and a two-class array on both graphs"""

    def __init__(self, name):
        self.name = name
        self.g, self.gp, self.new_id = pg.SHAPES[name]()
        self.m = PathModel(self.g)
        self.L = self.g.n_levels
        self.pads = pg.pad_mask(self.gp, self.new_id)
        self.cls = class_arrays(self.g, 81)[2]
        self.cls_p = pg.pad_classes(self.g, self.gp, self.new_id, self.cls, 82)
        level_of = np.repeat(np.arange(self.L), np.diff(self.g.level_off))
        self.two = ((np.arange(self.g.n_vertices) - self.g.level_off[level_of]) % 2).astype(np.int32)      # by position: both classes on every level two wide
        self.two_p = pg.pad_classes(self.g, self.gp, self.new_id, self.two, 84)

    def classes(self, kind):
        return {"own": (None, None), "drawn": (self.cls, self.cls_p), "two": (self.two, self.two_p)}[kind]

    def through(self, b):
        """the model's (T, V) of the base graph: computed once per budget, shared, left unchanged"""
        if (self.name, b) not in _MODELS:
            _MODELS[self.name, b] = through_values_np(self.m, b)
        return _MODELS[self.name, b]

    def states(self, b):
        if (self.name, "fb", b) not in _MODELS:
            _MODELS[self.name, "fb", b] = joint_states_fb(self.m, b)
        return _MODELS[self.name, "fb", b]

    def called(self, seed):
        """[2, 2, L] on the base graph: a sampled pair of paths and a list of cells that is no pair of paths"""
        return _called(self.m, np.random.default_rng(seed))

    def real(self, rng, l):
        return int(rng.integers(self.g.level_off[l], self.g.level_off[l + 1]))

    def a_pad(self, l, which=0):
        at = np.flatnonzero(self.pads[self.gp.level_off[l]:self.gp.level_off[l + 1]])
        return int(at[which] + self.gp.level_off[l])


def case(name):
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]


def same_rows(got, want, tag):
    got, want = np.asarray(got, np.int64), np.asarray(want, np.int64)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    bad = np.argwhere((got != want).any(axis=-1))
    assert bad.size == 0, (tag, bad[:5], got[tuple(bad[:5].T)], want[tuple(bad[:5].T)])


def check_margins(c, got, rec, V, J, tag):
    """device records (and vertex values) on the padded graph against the model's of the base graph"""
    levels, best = got[0], got[1]
    assert best == V, (tag, best, V)
    rows = _rows(levels)
    same_rows(rows, pg.remap_records(rec, c.new_id), tag)
    alt = rows[..., 3:5]
    assert not c.pads[alt[alt >= 0]].any(), tag          # no pad is an alternative
    if len(got) > 2:
        want = pg.remap_vertex_values(J, c.gp, c.new_id)
        assert np.array_equal(got[2], want), (tag, np.flatnonzero(got[2] != want)[:5])
        assert (got[2][c.pads] == NEG_INF).all(), tag


def check_table(c, got, off, rows, V, own, tag):
    got_off, entries, best = got[0], got[1], got[2]
    want_off, want = pg.remap_table(off, rows, c.new_id, own_classes=own)
    assert best == V and np.array_equal(got_off, want_off), (tag, best, V, got_off, want_off)
    got_rows = _entry_rows(entries)
    same_rows(got_rows, want, tag)
    assert not c.pads[got_rows[:, 2:4]].any(), tag       # no pad is in the table


def check_phase(c, got, best, want, V, tag):
    assert best == V, (tag, best, V)
    rows = _phase_rows(got)
    same_rows(rows, pg.remap_phase(want, c.new_id), tag)
    cells = rows[:, [3, 4, 6, 7]]
    assert not c.pads[cells[cells >= 0]].any(), tag      # no pad is a cis or a trans vertex


def het_called(c, cls, levels, seed):
    return np.ascontiguousarray(pg.het_pair(c.m, cls, levels, seed), np.int32)


# ---------------------------------------------------------------------------------------------- rows: jt_combine_kernel past JT_ROW_BLOCKS
def rows_pins(c):
    """on real cells of both padded levels: forbid and require, a wildcard each way"""
    rng = np.random.default_rng(85)
    r = c.real
    return ([(2, r(rng, 2), -1, FORBID), (2, -1, r(rng, 2), FORBID), (2, r(rng, 2), r(rng, 2), FORBID), (3, r(rng, 3), r(rng, 3), FORBID)]
            + [(3, r(rng, 3), -1, REQUIRE) for _ in range(20)] + [(3, -1, r(rng, 3), REQUIRE) for _ in range(20)] + [(3, r(rng, 3), r(rng, 3), REQUIRE)])


@pytest.mark.parametrize("b", [0, 2, 7])
def test_rows_genotype_margins(gpu_ctx, b):
    c = case("rows")
    gpu_ctx.dp_load_graph(c.gp)
    T, V = c.through(b)
    called = c.called(86)
    for kind in ("own", "drawn"):
        cls, cls_p = c.classes(kind)
        rec, _, J = genotype_margins_np(c.m, called, b, cls, T, V)
        got = gpu_ctx.dp_genotype_margins(pg.remap_called(called, c.new_id), b, cls_p, want_vertices=True)
        check_margins(c, got, rec, V, J, ("rows", b, kind))
    stats = gpu_ctx.dp_genotype_stats()
    assert stats["n_segments"] == 1 and stats["peak_bytes"] >= 4 * pg.widest_level(c.gp) ** 2 * (b + 1)      # the call ran at the padded width
    assert b == 0 or V != NEG_INF


def test_rows_pinned_margins(gpu_ctx):
    c = case("rows")
    gpu_ctx.dp_load_graph(c.gp)
    b = 7
    pins = rows_pins(c)
    called = c.called(87)
    called_p = pg.remap_called(called, c.new_id)
    T, V = pinned_through_values_np(c.m, b, pins)
    assert NEG_INF < V <= c.through(b)[1] and any(not np.array_equal(t, t.T) for t in T)       # the pins leave an answer, and T is not symmetric
    pins_p = pg.remap_pins(pins, c.new_id) + [(2, c.a_pad(2), -1, FORBID), (3, -1, c.a_pad(3, -1), FORBID)]       # forbidding a pad forbids nothing
    for kind in ("own", "drawn"):
        cls, cls_p = c.classes(kind)
        rec, _, J = pinned_genotype_margins_np(c.m, called, T, V, cls)
        got = gpu_ctx.dp_genotype_margins_pinned(pins_p, called_p, b, cls_p, want_vertices=True)
        check_margins(c, got, rec, V, J, ("rows pinned", kind))
        assert gpu_ctx.dp_genotype_pin_stats() == dict(pins=len(pins_p), mask_launches=4)
    # a required pad alone: nothing satisfies it.  On the base graph that is "every cell of the level forbidden"
    T0, V0 = pinned_through_values_np(c.m, 2, [(2, -1, -1, FORBID)])
    rec, _, J = pinned_genotype_margins_np(c.m, called, T0, V0, c.cls)
    assert V0 == NEG_INF and (rec[..., 2] == NEG_INF).all() and (rec[..., 3] == -1).all()
    for pad_pin in ((2, c.a_pad(2, 5), -1, REQUIRE), (3, -1, c.a_pad(3, -7), REQUIRE)):
        got = gpu_ctx.dp_genotype_margins_pinned([pad_pin], called_p, 2, c.cls_p, want_vertices=True)
        check_margins(c, got, rec, V0, J, ("rows required pad", pad_pin))


def test_rows_nineteen_budgets(gpu_ctx):
    """19 distinct budgets share the 2,048 workgroups: 107 rows each, so every budget strides its rows twenty times"""
    c = case("rows")
    gpu_ctx.dp_load_graph(c.gp)
    budgets = np.random.default_rng(88).permutation(19).astype(np.int32)
    rng = np.random.default_rng(89)
    called = np.array([[[c.real(rng, l) for l in range(c.L)] for _ in range(2)] for _ in budgets], np.int32)
    called[0] = c.m.sample_paths(rng, 2)[0]
    rec, V = genotype_margins_budgets_np(c.m, called, budgets, c.cls)
    levels, best = gpu_ctx.dp_genotype_margins_budgets(pg.remap_called(called, c.new_id), budgets, c.cls_p)
    assert np.array_equal(best, V) and (V != NEG_INF).sum() >= 17
    same_rows(_rows(levels), pg.remap_records(rec, c.new_id), "rows budgets")
    alt = _rows(levels)[..., 3:5]
    assert not c.pads[alt[alt >= 0]].any()


def test_rows_genotype_tables(gpu_ctx):
    c = case("rows")
    gpu_ctx.dp_load_graph(c.gp)
    called = c.called(90)
    called_p = pg.remap_called(called, c.new_id)
    T, V = c.through(7)
    rec, _, _ = genotype_margins_np(c.m, called, 7, c.cls, T, V)
    got = gpu_ctx.dp_genotype_table(7, c.cls_p, called_p)
    check_table(c, got, *genotype_table_np(c.m, T, c.cls), V, False, "rows table")
    check_margins(c, (got[3], got[2]), rec, V, None, "rows table records")
    pins = rows_pins(c)
    Tp, Vp = pinned_through_values_np(c.m, 7, pins)
    rec, _, _ = pinned_genotype_margins_np(c.m, called, Tp, Vp, c.cls)
    got = gpu_ctx.dp_genotype_table_pinned(pg.remap_pins(pins, c.new_id) + [(2, c.a_pad(2), -1, FORBID)], 7, c.cls_p, called_p)
    check_table(c, got, *pinned_genotype_table_np(c.m, Tp, c.cls), Vp, False, "rows pinned table")
    check_margins(c, (got[3], got[2]), rec, Vp, None, "rows pinned table records")
    T, V = c.through(2)                                  # every vertex its own class: 2,195 ranks on the widest level
    got = gpu_ctx.dp_genotype_table(2, None)
    check_table(c, got, *genotype_table_np(c.m, T, None), V, True, "rows table, own classes")
    assert len(got[1]) >= 1000


def test_rows_phase_margins(gpu_ctx):
    """a called pair that is het on both padded levels under two classes; pad rows carry the called classes too, and a class of their own"""
    c = case("rows")
    gpu_ctx.dp_load_graph(c.gp)
    for l in (2, 3):
        at = c.two_p[c.gp.level_off[l]:c.gp.level_off[l + 1]][c.pads[c.gp.level_off[l]:c.gp.level_off[l + 1]]]
        assert (at == 0).sum() >= 100 and (at == 1).sum() >= 100 and (at == 2).sum() >= 100
    pairs = [het_called(c, c.two, (2, 3), 91 + x) for x in range(2)]
    n_records = 0
    for b in (2, 7):
        for kind, pair in (("two", pairs[0]), ("own", pairs[1])):
            cls, cls_p = c.classes(kind)
            want, V = phase_margins_np(c.m, pair, b, cls, c.states(b))
            got, best = gpu_ctx.dp_phase_margins(pg.remap_called(pair, c.new_id), b, cls_p)
            check_phase(c, got, best, want, V, ("rows phase", b, kind))
            n_records += len(want)
            assert any(r[0] <= 2 and r[1] >= 3 for r in want.tolist())      # a seeded state crosses the two wide levels
    assert n_records >= 4
    called = np.stack([pairs[0], pairs[1], pairs[0][::-1], pairs[1]])
    budgets = np.array([7, 2, 2, 0], np.int32)
    got, best = gpu_ctx.dp_phase_margins_budgets(pg.remap_called(called, c.new_id), budgets, c.two_p)
    for q, b in enumerate(budgets.tolist()):
        want, V = phase_margins_np(c.m, called[q], b, c.two, c.states(b))
        check_phase(c, got[q], best[q], want, V, ("rows phase budgets", q, b))


def test_rows_every_level_its_own_segment(gpu_ctx):
    """joint_state_bytes = 1: the first pass and the recompute path see the wide levels"""
    c = case("rows")
    gpu_ctx.dp_load_graph(c.gp)
    found = gpu_ctx.dp_get_option("joint_state_bytes")
    called = c.called(93)
    T, V = c.through(7)
    rec, _, J = genotype_margins_np(c.m, called, 7, c.cls, T, V)
    pair = het_called(c, c.two, (2, 3), 91)
    want, _ = phase_margins_np(c.m, pair, 7, c.two, c.states(7))
    with gpu_ctx.dp_options(joint_state_bytes=1):
        got = gpu_ctx.dp_genotype_margins(pg.remap_called(called, c.new_id), 7, c.cls_p, want_vertices=True)
        assert gpu_ctx.dp_genotype_stats()["n_segments"] == c.L
        ph, best = gpu_ctx.dp_phase_margins(pg.remap_called(pair, c.new_id), 7, c.two_p)
        assert gpu_ctx.dp_phase_stats()["segments"] == c.L
    check_margins(c, got, rec, V, J, "rows segments")
    check_phase(c, ph, best, want, V, "rows segments phase")
    assert gpu_ctx.dp_get_option("joint_state_bytes") == found


# ---------------------------------------------------------------------------------------------- edges: jt_scores_kernel past its grid
def test_edges_genotype_margins(gpu_ctx):
    c = case("edges")
    gpu_ctx.dp_load_graph(c.gp)
    T, V = c.through(2)
    called = c.called(94)
    rec, _, J = genotype_margins_np(c.m, called, 2, c.cls, T, V)
    got = gpu_ctx.dp_genotype_margins(pg.remap_called(called, c.new_id), 2, c.cls_p, want_vertices=True)
    check_margins(c, got, rec, V, J, "edges")
    assert V != NEG_INF


def test_edges_phase_margins(gpu_ctx):
    c = case("edges")
    gpu_ctx.dp_load_graph(c.gp)
    pair = het_called(c, c.two, (2, 3), 95)
    want, V = phase_margins_np(c.m, pair, 2, c.two, c.states(2))
    got, best = gpu_ctx.dp_phase_margins(pg.remap_called(pair, c.new_id), 2, c.two_p)
    check_phase(c, got, best, want, V, "edges phase")
    assert any(r[0] <= 2 and r[1] >= 3 for r in want.tolist())      # the seeded backward pass takes the big transition


# ---------------------------------------------------------------------------------------------- lanes: the recurrences past 2^20 lanes per row
SATURATED = 8                                           # 2 (L - 1) of the lanes shape: no pair of paths spends more


def lanes_case(ctx):
    """loaded with R = 2 (L - 1), so that the run's own plane at R is the value of every budget from there on"""
    c = case("lanes")
    assert SATURATED == 2 * (c.L - 1) and pg.LANES_BUDGET == MAX_PLANES - 1
    ctx.dp_load_graph(with_R(c.gp, SATURATED))
    return c


def test_lanes_genotype_margins(gpu_ctx):
    c = lanes_case(gpu_ctx)
    gpu_ctx.dp_run()
    plane = int(gpu_ctx.dp_budget_values()[SATURATED])
    T, V = c.through(SATURATED)
    called = c.called(96)
    for kind in ("own", "drawn"):
        cls, cls_p = c.classes(kind)
        rec, _, J = genotype_margins_np(c.m, called, SATURATED, cls, T, V)
        got = gpu_ctx.dp_genotype_margins(pg.remap_called(called, c.new_id), pg.LANES_BUDGET, cls_p, want_vertices=True)
        check_margins(c, got, rec, V, J, ("lanes", kind))
        assert got[1] == plane != NEG_INF
        assert gpu_ctx.dp_genotype_stats()["peak_bytes"] >= 4 * 300 * 300 * (pg.LANES_BUDGET + 1)      # one state of level 2 at 4,096 planes: 1.47 GB


def test_lanes_pinned_margins(gpu_ctx):
    """pins on level 2: jt_pin_mask_kernel strides its 300 * 4,096 words per row too"""
    c = lanes_case(gpu_ctx)
    rng = np.random.default_rng(97)
    a0, a1 = int(c.g.level_off[2]), int(c.g.level_off[3])
    pins = [(2, a0 + 7, -1, FORBID), (2, -1, a0 + 2, FORBID), (2, a0 + 6, a0 + 9, FORBID), (2, a0 + 8, a0 + 1, FORBID)]       # columns on both sides of column 256
    called = c.called(98)
    T, V = pinned_through_values_np(c.m, SATURATED, pins)
    rec, _, J = pinned_genotype_margins_np(c.m, called, T, V, c.cls)
    pins_p = pg.remap_pins(pins, c.new_id) + [(2, c.a_pad(2, 3), -1, FORBID)]
    got = gpu_ctx.dp_genotype_margins_pinned(pins_p, pg.remap_called(called, c.new_id), pg.LANES_BUDGET, c.cls_p, want_vertices=True)
    check_margins(c, got, rec, V, J, "lanes pinned")
    assert V != NEG_INF and any(not np.array_equal(t, t.T) for t in T)
    require = [(2, int(rng.integers(a0, a1)), -1, REQUIRE), (2, -1, a1 - 1, REQUIRE)]
    T, V = pinned_through_values_np(c.m, SATURATED, require)
    rec, _, J = pinned_genotype_margins_np(c.m, called, T, V, c.cls)
    got = gpu_ctx.dp_genotype_margins_pinned(pg.remap_pins(require, c.new_id), pg.remap_called(called, c.new_id), pg.LANES_BUDGET, c.cls_p, want_vertices=True)
    check_margins(c, got, rec, V, J, "lanes required")


def test_lanes_budgets(gpu_ctx):
    """8, 100 and 4,095 from one pass at 4,095: the three agree with each other and with the model at 8"""
    c = lanes_case(gpu_ctx)
    budgets = np.array([SATURATED, 100, pg.LANES_BUDGET], np.int32)
    one = c.called(99)[:1]
    called = np.repeat(one, 3, axis=0)
    rec, V = genotype_margins_budgets_np(c.m, called, [SATURATED] * 3, c.cls)
    levels, best = gpu_ctx.dp_genotype_margins_budgets(pg.remap_called(called, c.new_id), budgets, c.cls_p)
    assert np.array_equal(best, V) and best[0] == best[1] == best[2] != NEG_INF
    rows = _rows(levels)
    assert np.array_equal(rows[0], rows[1]) and np.array_equal(rows[0], rows[2])
    same_rows(rows, pg.remap_records(rec, c.new_id), "lanes budgets")


def test_lanes_phase_margins(gpu_ctx):
    c = lanes_case(gpu_ctx)
    pair = het_called(c, c.two, (1, 2, 3), 100)
    want, V = phase_margins_np(c.m, pair, SATURATED, c.two, c.states(SATURATED))
    assert len(want) == 2
    got, best = gpu_ctx.dp_phase_margins(pg.remap_called(pair, c.new_id), pg.LANES_BUDGET, c.two_p)
    check_phase(c, got, best, want, V, "lanes phase")
    called = np.stack([pair, pair[::-1], pair])
    budgets = np.array([pg.LANES_BUDGET, SATURATED, 100], np.int32)
    got, best = gpu_ctx.dp_phase_margins_budgets(pg.remap_called(called, c.new_id), budgets, c.two_p)
    for q in range(3):
        want, V = phase_margins_np(c.m, called[q], SATURATED, c.two, c.states(SATURATED))
        check_phase(c, got[q], best[q], want, V, ("lanes phase budgets", q))
    assert np.array_equal(got[0], got[2])


# ---------------------------------------------------------------------------------------------- deep: jt_out_scan_kernel past one chunk
def test_deep_against_the_models(gpu_ctx):
    c = case("deep")
    b = pg.DEEP_BUDGET
    gpu_ctx.dp_load_graph(c.g)
    T, V = c.through(b)
    assert V != NEG_INF
    called = c.called(101)
    rec, _, J = genotype_margins_np(c.m, called, b, c.cls, T, V)
    got = gpu_ctx.dp_genotype_margins(called, b, c.cls, want_vertices=True)
    check_margins(c, got, rec, V, J, "deep")
    assert gpu_ctx.dp_genotype_stats()["n_segments"] == 1
    found = gpu_ctx.dp_get_option("joint_state_bytes")
    with gpu_ctx.dp_options(joint_state_bytes=800):
        again = gpu_ctx.dp_genotype_margins(called, b, c.cls, want_vertices=True)
        assert gpu_ctx.dp_genotype_stats()["n_segments"] > 100
    check_margins(c, again, rec, V, J, "deep, many segments")
    assert gpu_ctx.dp_get_option("joint_state_bytes") == found
    check_table(c, gpu_ctx.dp_genotype_table(b, c.cls), *genotype_table_np(c.m, T, c.cls), V, False, "deep table")
    budgets = np.array([b, 0, 2, 7], np.int32)
    many = np.concatenate([called, called])
    rec, Vs = genotype_margins_budgets_np(c.m, many, budgets, c.cls)
    levels, best = gpu_ctx.dp_genotype_margins_budgets(many, budgets, c.cls)
    assert np.array_equal(best, Vs)
    same_rows(_rows(levels), rec, "deep budgets")


def test_deep_phase_margins(gpu_ctx):
    c = case("deep")
    b = pg.DEEP_BUDGET
    gpu_ctx.dp_load_graph(c.g)
    pair = np.ascontiguousarray(c.m.sample_paths(np.random.default_rng(102), 2, p_w0=0.9)[0], np.int32)
    want, V = phase_margins_np(c.m, pair, b, c.two, c.states(b))
    assert len(want) >= 100
    got, best = gpu_ctx.dp_phase_margins(pair, b, c.two)
    check_phase(c, got, best, want, V, "deep phase")


def test_deep_run_against_the_oracle(gpu_ctx):
    """the only graph of 1,000 levels and more in the suite"""
    c = case("deep")
    ref = orc.dp_solve(c.g)
    out = gpu_ctx.dp_solve(c.g)
    assert (out.value, out.s_het, out.p1, out.p2) == (ref["value"], ref["s_het"], ref["p1"], ref["p2"])
    assert out.value == c.through(pg.DEEP_BUDGET)[1] and c.g.R == pg.DEEP_BUDGET

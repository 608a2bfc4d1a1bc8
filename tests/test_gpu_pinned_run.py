"""-m gpu: dg_dp_run_pinned / Context.dp_run_pinned -- the run's own DP with some cells of some levels taken out, in every execution
mode of the run: single launches, level pairs, captured batches, lattice segments with and without the plane limit, lattice chunks,
the generic kernel.

Integers only: every comparison is exact.  The yardstick is tests/pinned_model.py, itself pinned to brute force by
tests/test_pinned_model.py; the mode tests need no model: they hold the call against itself under the options that switch the mode
off, and against dp_genotype_margins."""
import numpy as np
import pytest

import graphgen
import pair_graphs as pg
from dipgenie_amd import capi
from paths_model import NEG_INF, PathModel
from pinned_model import FORBID, REQUIRE, pair_satisfies, pinned_planes_np
from test_gpu_score_paths import ENUMERABLE
from test_partner_model import enumerable_graph
from test_pinned_model import pin_sets, random_pins

pytestmark = pytest.mark.gpu


def _key(out):
    return (out.value, out.s_het, out.cells, out.relaxations, tuple(out.p1), tuple(out.p2))


def _budgets(R):
    return list(range(R + 1)) if R <= 3 else [0, 1, R // 2, R]


def _check_answers(ctx, g, pins, budgets, outs, planes):
    """what every pinned run must hold, model or not: the outcome of a budget is its plane's value, the answer paths satisfy every pin
    and score the value within the budget; an unreachable budget has empty lists and paths of -1"""
    for b, out in zip(budgets, outs):
        assert out.value == planes[b], (b, out.value, planes[b])
        paths = ctx.dp_answer_paths(b)
        if out.value == NEG_INF:
            assert out.p1 == [] and out.p2 == [] and (paths == -1).all(), b
            continue
        assert pair_satisfies([tuple(int(x) for x in p) for p in pins], paths[0], paths[1]), (b, pins, paths)
        s = ctx.dp_score_paths(paths[None])[0]
        assert s["value"] == out.value and s["s_het"] == out.s_het and s["r1"] + s["r2"] <= b, (b, s, out.value)


def _check_model(ctx, g, m, pins, tag):
    """one pinned run of the loaded graph g against the model: every plane, every budget's outcome, the answer paths"""
    budgets = _budgets(g.R)
    outs = ctx.dp_run_pinned(pins, budgets)
    planes = ctx.dp_budget_values()
    want = pinned_planes_np(m, g.R, pins)
    assert np.array_equal(planes, want), (tag, pins[:8], planes, want)
    _check_answers(ctx, g, pins, budgets, outs, planes)
    st = ctx.dp_pin_stats()
    if len(pins):
        assert st["pins"] == len(pins) and st["levels"] == len({int(p[0]) for p in pins}) and st["mask_launches"] >= st["levels"], (tag, st)
    return planes


@pytest.mark.parametrize("q", range(len(ENUMERABLE)))
def test_model_on_the_enumerable_graphs(gpu_ctx, q):
    g = enumerable_graph(q)
    m = PathModel(g)
    gpu_ctx.dp_load_graph(g)
    for tag, pins in pin_sets(q):
        _check_model(gpu_ctx, g, m, pins, (q, tag))


# level widths around the mask's block of 64 columns, and planes R + 1 = 1, 2, 4, 19, 33
WIDTHS = [([1, 1, 1, 1, 1], 0), ([1, 2, 2, 2, 1], 1), ([1, 3, 3, 3, 3, 1], 3), ([1, 63, 5, 63, 1], 18), ([1, 64, 64, 1], 32), ([1, 65, 65, 65, 1], 3),
          ([1, 65, 2, 65, 1], 18), ([1, 5, 257, 5, 1], 1)]


@pytest.mark.parametrize("w", range(len(WIDTHS)))
def test_model_on_prescribed_widths(gpu_ctx, w):
    widths, R = WIDTHS[w]
    g = graphgen.random_levelized(9300 + w, widths=widths, R=R, p_w1=0.3 if R > 1 else 0.0, extra_edges=0.6 if max(widths) > 200 else 1.2, p_colour=0.5)
    m = PathModel(g)
    L = g.n_levels
    gpu_ctx.dp_load_graph(g)
    rng = np.random.default_rng(80 + w)
    lo = lambda l: int(g.level_off[l])
    pick = lambda l: int(rng.integers(g.level_off[l], g.level_off[l + 1]))
    wide = 1 + int(np.argmax(widths[1:-1]))
    free = _check_model(gpu_ctx, g, m, [], (w, "none"))
    sets = {
        "first and last": [(1, pick(1), -1, REQUIRE), (L - 2, -1, pick(L - 2), FORBID)],
        "adjacent": [(1, pick(1), -1, REQUIRE), (1, -1, pick(1), REQUIRE), (1, pick(1), pick(1), FORBID), (2, -1, pick(2), REQUIRE), (2, pick(2), -1, REQUIRE)],
        "wildcard left": [(wide, -1, pick(wide), REQUIRE)],
        "wildcard right": [(wide, pick(wide), -1, FORBID)],
        "many": [(wide, pick(wide), pick(wide), REQUIRE) for _ in range(70)] + [(wide, pick(wide), pick(wide), FORBID) for _ in range(5)],
        "last cell": [(wide, lo(wide + 1) - 1, lo(wide + 1) - 1, FORBID), (wide, lo(wide), lo(wide + 1) - 1, FORBID)],
        "random": random_pins(m, rng, L - 2, 3),
    }
    changed = 0
    for tag, pins in sets.items():
        planes = _check_model(gpu_ctx, g, m, pins, (w, tag))
        changed += not np.array_equal(planes, free)
    assert len(sets["many"]) > 64
    assert changed >= 1 or max(widths) == 1


_JOINT = {}


def joint_case(ctx):
    """widths [1, 65, 65, 65, 1], R = 3: graph, T of every cell of levels 1..3 from dp_genotype_margins ([3, 65, 65]), the run's answer
    paths and their margin records -- loaded here, so call it first"""
    if not _JOINT:
        g = graphgen.random_levelized(9400, widths=[1, 65, 65, 65, 1], R=3, p_w1=0.3, extra_edges=1.2, p_colour=0.5)
        ctx.dp_load_graph(g)
        T = np.zeros((3, 65, 65), np.int64)
        cells = [(i, j) for i in range(65) for j in range(65)]
        for c0 in range(0, len(cells), 256):
            part = cells[c0:c0 + 256]
            called = np.zeros((len(part), 2, g.n_levels), np.int32)
            called[:, :, -1] = g.n_vertices - 1
            for n, (i, j) in enumerate(part):
                for l in (1, 2, 3):
                    called[n, 0, l], called[n, 1, l] = g.level_off[l] + i, g.level_off[l] + j
            levels, best = ctx.dp_genotype_margins(called, g.R)
            for n, (i, j) in enumerate(part):
                T[:, i, j] = levels["value"][n, 1:4]
        out = ctx.dp_run_budgets([g.R])[0]
        paths = ctx.dp_answer_paths(g.R)
        rec, best = ctx.dp_genotype_margins(paths, g.R)
        assert best == out.value
        _JOINT.update(g=g, T=T, paths=paths, rec=rec[0], best=best)
    ctx.dp_load_graph(_JOINT["g"])
    return _JOINT


@pytest.mark.parametrize("l", [1, 2, 3])
def test_one_required_cell_is_its_through_value(gpu_ctx, l):
    """no model: one require-pin (i, j) gives T_l[i][j] of dp_genotype_margins, for every cell of the level, unreachable ones included"""
    c = joint_case(gpu_ctx)
    g, T = c["g"], c["T"][l - 1]
    a0 = int(g.level_off[l])
    got = np.array([[gpu_ctx.dp_run_pinned([(l, a0 + i, a0 + j, REQUIRE)])[0].value for j in range(65)] for i in range(65)], np.int64)
    assert np.array_equal(got, T), np.argwhere(got != T)[:5]
    assert (T == NEG_INF).any() and T.max() == c["best"]


def test_forbidding_the_called_cell_gives_the_alternative(gpu_ctx):
    """no model: forbidding the called cell in both orders gives alt_value of dp_genotype_margins (every vertex its own class)"""
    c = joint_case(gpu_ctx)
    g, paths, rec = c["g"], c["paths"], c["rec"]
    lower = 0
    for l in range(1, g.n_levels - 1):
        pins = capi.genotype_pins(l, paths[0][l], paths[1][l], capi.PIN_FORBID)
        out = gpu_ctx.dp_run_pinned(pins)[0]
        assert out.value == rec["alt_value"][l], (l, out.value, rec[l])
        lower += out.value < c["best"]
        _check_answers(gpu_ctx, g, pins, [g.R], [out], gpu_ctx.dp_budget_values())
    assert lower >= 1


def _identity(ctx, g):
    """pins on every inner level at the ordered cell the unpinned answer of budget b passes: the outcome of b is the unpinned one"""
    budgets = list(range(g.R + 1))
    free = ctx.dp_run_budgets(budgets)
    answers = [ctx.dp_answer_paths(b) for b in budgets]
    same = ctx.dp_run_pinned([], budgets)
    assert [_key(o) for o in same] == [_key(o) for o in free]
    for b in budgets:
        if free[b].value == NEG_INF:
            continue
        pins = [(l, answers[b][0][l], answers[b][1][l], REQUIRE) for l in range(1, g.n_levels - 1)]
        outs = ctx.dp_run_pinned(pins, budgets)
        assert _key(outs[b]) == _key(free[b]), b
        assert np.array_equal(ctx.dp_answer_paths(b), answers[b]), b
        for b2 in budgets:                               # the other budgets: what the constrained DP leaves them, never more
            assert outs[b2].value <= free[b2].value


def test_identity(gpu_ctx):
    for seed, kw in [(1, dict(max_width=9, n_levels=40, R=3)), (2, dict(max_width=30, n_levels=12, R=6, p_w1=0.5)), (3, dict(max_width=4, n_levels=300, R=2, p_colour=0.2))]:
        g = graphgen.random_levelized(9500 + seed, **kw)
        gpu_ctx.dp_load_graph(g)
        _identity(gpu_ctx, g)
    with gpu_ctx.dp_options(pair_min=1):
        g = pg.parity_graph(4, "both")
        gpu_ctx.dp_load_graph(g)
        _identity(gpu_ctx, g)
        assert gpu_ctx.dp_pin_stats()["pairs_as_singles"] == len(pg.expected_pairs(g))


def _level_pins(g, rng, levels, kind_of=None):
    """two pins on each listed level: a forbid of a random ordered cell and of a whole random row, or (kind_of(l) = REQUIRE) two rows"""
    pins = []
    for l in levels:
        a0, a1 = int(g.level_off[l]), int(g.level_off[l + 1])
        kind = FORBID if kind_of is None else kind_of(l)
        pins += [(l, int(rng.integers(a0, a1)), int(rng.integers(a0, a1)) if kind == FORBID else -1, kind), (l, int(rng.integers(a0, a1)), -1, kind)]
    return pins


PAIR_GRAPHS = [lambda: pg.parity_graph(4, "both"), lambda: pg.parity_graph(3, "first"), lambda: pg.shared_middle_graph(), lambda: pg.width_limit_graph("later", 255),
               lambda: pg.width_limit_graph("middle", 255)]


@pytest.mark.parametrize("n", range(len(PAIR_GRAPHS)))
def test_pairs(gpu_ctx, n):
    """a pin on the earlier level of a pair: two single launches; on the later level: the pair launch, then the mask"""
    g = PAIR_GRAPHS[n]()
    later = pg.expected_pairs(g)
    assert later
    budgets = list(range(g.R + 1))
    rng = np.random.default_rng(90 + n)
    lp = max(l for l in later if l <= g.n_levels - 2)      # (a pair may end on the sink, which takes no pin)
    cases = {"earlier": [lp - 1], "later": [lp], "both": [lp - 1, lp], "all earlier": [l - 1 for l in later], "all later": [l for l in later if l <= g.n_levels - 2],
             "before": [lp - 2] if lp > 2 else []}
    sets = {tag: _level_pins(g, rng, levels, (lambda l: REQUIRE) if tag in ("both", "all later") else None) for tag, levels in cases.items() if levels}
    want = {}
    with gpu_ctx.dp_options(pair_min=1, pair_levels=0):
        gpu_ctx.dp_load_graph(g)
        for tag, pins in sets.items():
            outs = gpu_ctx.dp_run_pinned(pins, budgets)
            want[tag] = ([_key(o) for o in outs], gpu_ctx.dp_budget_values().copy())
            assert not gpu_ctx.dp_pair_profile() and gpu_ctx.dp_pin_stats()["pairs_as_singles"] == 0
            _check_answers(gpu_ctx, g, pins, budgets, outs, want[tag][1])
    with gpu_ctx.dp_options(pair_min=1):
        gpu_ctx.dp_load_graph(g)
        free = [_key(o) for o in gpu_ctx.dp_run_budgets(budgets)]
        assert sum(gpu_ctx.dp_pair_profile().values()) == len(later)
        changed = 0
        for tag, pins in sets.items():
            outs = gpu_ctx.dp_run_pinned(pins, budgets)
            assert [_key(o) for o in outs] == want[tag][0], tag
            assert np.array_equal(gpu_ctx.dp_budget_values(), want[tag][1]), tag
            split = sum(1 for l in later if (l - 1) in cases[tag])
            st = gpu_ctx.dp_pin_stats()
            assert st["pairs_as_singles"] == split and st["mask_launches"] == len(cases[tag]), (tag, st)
            assert sum(gpu_ctx.dp_pair_profile().values()) == len(later) - split, tag          # the other pairs still ran as pairs
            assert sum(gpu_ctx.dp_launch_profile().values()) == g.n_levels - 1 - 2 * (len(later) - split), tag
            changed += [_key(o) for o in outs] != free
        assert changed >= 1
        assert [_key(o) for o in gpu_ctx.dp_run_budgets(budgets)] == free


def test_batches(gpu_ctx):
    """graph_batch 5: pins on the first and on the last level of a batch and in a batch of their own run those batches plainly; the
    batch cache serves the unpinned runs around a pinned one as before"""
    g = graphgen.random_levelized(9600, max_width=12, n_levels=43, R=4, p_w1=0.4)
    gl = pg.layered(4243, 3, [1] + [10] * 20 + [1], [1] + [2] * 19 + [4], colour_levels=(2, 3, 5, 8, 13))
    for graph, opts in ((g, {}), (gl, dict(pair_min=1))):
        budgets = list(range(graph.R + 1))
        rng = np.random.default_rng(95)
        # batches [1, 6), [6, 11), [11, 16), [16, 21), ...: first level of one, last level of another, one batch with a pin in its middle
        sets = {"first": [6], "last": [10], "own": [13], "mixed": [6, 10, 13, 1, 5], "every": list(range(1, graph.n_levels - 1))}
        pins = {tag: _level_pins(graph, rng, levels) for tag, levels in sets.items()}
        want = {}
        with gpu_ctx.dp_options(graph_batch=0, **opts):
            gpu_ctx.dp_load_graph(graph)
            for tag in sets:
                outs = gpu_ctx.dp_run_pinned(pins[tag], budgets)
                want[tag] = ([_key(o) for o in outs], gpu_ctx.dp_budget_values().copy())
                assert gpu_ctx.dp_pin_stats()["batches_plain"] == 0
                _check_answers(gpu_ctx, graph, pins[tag], budgets, outs, want[tag][1])
        with gpu_ctx.dp_options(graph_batch=5, **opts):
            gpu_ctx.dp_load_graph(graph)
            snap = lambda: ([_key(o) for o in gpu_ctx.dp_run_budgets(budgets)], gpu_ctx.dp_launch_profile(), gpu_ctx.dp_pair_profile(), gpu_ctx.dp_budget_values().tolist())
            first = snap()                                   # captures
            assert snap() == first                           # replays
            for tag in sets:
                outs = gpu_ctx.dp_run_pinned(pins[tag], budgets)
                assert [_key(o) for o in outs] == want[tag][0], tag
                assert np.array_equal(gpu_ctx.dp_budget_values(), want[tag][1]), tag
                assert gpu_ctx.dp_pin_stats()["batches_plain"] == len({(l - 1) // 5 for l in sets[tag]}), tag
                assert snap() == first, tag                  # unpinned, pinned, unpinned
                assert [_key(o) for o in gpu_ctx.dp_run_pinned(pins[tag], budgets)] == want[tag][0], tag      # and pinned again, between replays
        assert want["mixed"][0] != first[0] or want["every"][0] != first[0]


def _cuts(g, units):
    """first levels of the lattice chunks: levels are packed greedily into chunks of `units` 16-bit back-pointers, rounded up to even
    (narrow back-pointers: a cell is one unit, a level an even number of them)"""
    units = max((units + 1) & ~1, max(((int(k) * int(k) * (g.R + 1) + 1) & ~1) for k in np.diff(g.level_off)[1:]))
    cuts, acc = [1], 0
    for l in range(1, g.n_levels):
        k = int(g.level_off[l + 1] - g.level_off[l])
        nu = (k * k * (g.R + 1) + 1) & ~1
        if acc > 0 and acc + nu > units:
            cuts.append(l)
            acc = 0
        acc += nu
    return cuts


@pytest.mark.parametrize("plane_limit", [0, 1])
def test_segments(gpu_ctx, plane_limit):
    """a segmented lattice: the masks apply in the value pass and in every segment's re-sweep; a pin on a segment's last level is in
    the checkpoint; the plane-limited second pass keeps working"""
    g = graphgen.random_levelized(9700, max_width=14, n_levels=120, R=6, p_w1=0.3)
    budgets = list(range(g.R + 1))
    seg_cells = 5000
    cuts = _cuts(g, seg_cells)
    assert len(cuts) >= 4
    rng = np.random.default_rng(97)
    sets = {"last": [c - 1 for c in cuts[1:]], "first": [c for c in cuts[1:-1]], "inside": [c + 1 for c in cuts[1:] if c + 2 < g.n_levels - 1 and c + 1 not in cuts and c + 2 not in cuts][:4],
            "edge pair": [cuts[2] - 1, cuts[2]], "every": list(range(1, g.n_levels - 1))}
    assert all(sets.values())
    pins = {tag: _level_pins(g, rng, levels) + [(levels[0], -1, int(g.level_off[levels[0]]), FORBID)] for tag, levels in sets.items()}
    # (and for the chunked run below: a pin on either side of a chunk edge)
    chunk = 3000
    ccuts = _cuts(g, chunk)
    assert len(ccuts) >= 4
    sets.update({"chunk edge": [ccuts[1] - 1, ccuts[1], ccuts[3] - 1], "chunk first": [ccuts[2]]})
    pins.update({tag: _level_pins(g, rng, sets[tag]) for tag in ("chunk edge", "chunk first")})
    gpu_ctx.dp_load_graph(g)
    free = [_key(o) for o in gpu_ctx.dp_run_budgets(budgets)]
    want = {}
    for tag in sets:
        outs = gpu_ctx.dp_run_pinned(pins[tag], budgets)
        assert gpu_ctx.dp_timing().n_segments == 1
        want[tag] = ([_key(o) for o in outs], gpu_ctx.dp_budget_values().copy())
        _check_answers(gpu_ctx, g, pins[tag], budgets, outs, want[tag][1])
    assert sum(want[tag][0] != free for tag in sets) >= 2
    with gpu_ctx.dp_options(segment_cells=seg_cells, plane_limit=plane_limit):
        gpu_ctx.dp_load_graph(g)
        for tag in sets:
            outs = gpu_ctx.dp_run_pinned(pins[tag], budgets)
            assert gpu_ctx.dp_timing().n_segments == len(cuts), (gpu_ctx.dp_timing().n_segments, cuts)
            assert [_key(o) for o in outs] == want[tag][0], tag
            assert np.array_equal(gpu_ctx.dp_budget_values(), want[tag][1]), tag
            assert gpu_ctx.dp_pin_stats()["mask_launches"] == 2 * len(set(sets[tag])), tag          # once per pass
        assert [_key(o) for o in gpu_ctx.dp_run_budgets(budgets)] == free
    # resident lattice in small chunks, batches of 7 levels cut by the chunk edges
    with gpu_ctx.dp_options(lattice_chunk_cells=chunk, plane_limit=plane_limit, graph_batch=7):
        gpu_ctx.dp_load_graph(g)
        for tag in sets:
            outs = gpu_ctx.dp_run_pinned(pins[tag], budgets)
            tm = gpu_ctx.dp_timing()
            assert tm.n_segments == 1 and tm.n_chunks == len(ccuts), (tm.n_chunks, ccuts)
            assert [_key(o) for o in outs] == want[tag][0], tag
            assert np.array_equal(gpu_ctx.dp_budget_values(), want[tag][1]), tag
            assert gpu_ctx.dp_pin_stats()["mask_launches"] == len(set(sets[tag])), tag
        assert [_key(o) for o in gpu_ctx.dp_run_budgets(budgets)] == free


def test_generic_kernel(gpu_ctx):
    """a graph with in-degrees above 255 (wide back-pointers, the generic kernel): pins on its wide levels, against the model"""
    g = graphgen.random_levelized(9100 + 12, max_width=3, n_levels=6, R=1, extra_edges=300.0, dup_edges=False)
    assert np.bincount(g.out_dst, minlength=g.n_vertices).max() > 255
    m = PathModel(g)
    gpu_ctx.dp_load_graph(g)
    rng = np.random.default_rng(99)
    for n in range(6):
        pins = random_pins(m, rng, 1 + n % 3, 1 + n % 2)
        _check_model(gpu_ctx, g, m, pins, ("generic", n))
        assert any(k.startswith("dp_sweep_kernel") for k in gpu_ctx.dp_launch_profile()), gpu_ctx.dp_launch_profile()
    with gpu_ctx.dp_options(fast=0):                     # every level on the generic kernel
        g2 = enumerable_graph(0)
        gpu_ctx.dp_load_graph(g2)
        for tag, pins in pin_sets(0)[:12]:
            _check_model(gpu_ctx, g2, PathModel(g2), pins, ("fast 0", tag))


def test_unsatisfiable_sets(gpu_ctx):
    g = graphgen.random_levelized(9400, widths=[1, 65, 65, 65, 1], R=3, p_w1=0.3, extra_edges=1.2, p_colour=0.5)
    m = PathModel(g)
    gpu_ctx.dp_load_graph(g)
    budgets = list(range(g.R + 1))
    indeg = np.bincount(g.out_dst, minlength=g.n_vertices)
    dead = int(next(v for v in range(int(g.level_off[1]), int(g.level_off[2])) if indeg[v] == 0))     # a vertex nothing reaches
    a0 = int(g.level_off[1])
    for pins in ([(1, dead, -1, REQUIRE)], [(2, -1, -1, REQUIRE), (1, -1, dead, REQUIRE)], [(1, a0, -1, REQUIRE), (1, -1, a0 + 1, REQUIRE), (1, a0, -1, FORBID), (1, -1, a0 + 1, FORBID)]):
        outs = gpu_ctx.dp_run_pinned(pins, budgets)
        assert (gpu_ctx.dp_budget_values() == NEG_INF).all()
        for b, out in zip(budgets, outs):
            assert out.value == NEG_INF and out.p1 == [] and out.p2 == []
            assert (gpu_ctx.dp_answer_paths(b) == -1).all()
        assert np.array_equal(pinned_planes_np(m, g.R, pins), np.full(g.R + 1, NEG_INF))


def test_errors_leave_the_last_run_alone(gpu_ctx):
    g = enumerable_graph(1)
    gpu_ctx.dp_load_graph(g)
    L = g.n_levels
    a0, a1 = int(g.level_off[1]), int(g.level_off[2])
    good = (1, a0, -1, REQUIRE)
    gpu_ctx.dp_run_pinned([good, (2, -1, int(g.level_off[2]), FORBID)], range(g.R + 1))
    planes, paths, stats = gpu_ctx.dp_budget_values().copy(), gpu_ctx.dp_answer_paths(g.R).copy(), gpu_ctx.dp_pin_stats()
    bad = [((0, 0, 0, REQUIRE), "level 0"), ((L - 1, -1, -1, REQUIRE), f"level {L - 1}"), ((-3, -1, -1, FORBID), "level -3"), ((1, a1, -1, REQUIRE), f"vertex1 {a1}"),
           ((1, -1, a0 - 1, REQUIRE), f"vertex2 {a0 - 1}"), ((1, -2, -1, FORBID), "vertex1 -2"), ((1, a0, a0, 2), "kind 2"), ((1, a0, a0, -1), "kind -1")]
    for pin, what in bad:
        for at, pins in ((0, [pin, good]), (2, [good, good, pin, (0, 0, 0, 7)])):          # the FIRST offending pin is named
            with pytest.raises(capi.DgError, match=rf"rc=-1\): dg_dp_run_pinned: pin {at}: .*{what}") as e:
                gpu_ctx.dp_run_pinned(pins)
            assert np.array_equal(gpu_ctx.dp_budget_values(), planes) and np.array_equal(gpu_ctx.dp_answer_paths(g.R), paths), str(e.value)
    with pytest.raises(capi.DgError, match=r"rc=-1\): dg_dp_run_pinned: n_pins = 65537"):
        gpu_ctx.dp_run_pinned(np.tile(np.array([good], np.int32), (65537, 1)))
    with pytest.raises(capi.DgError, match=r"rc=-1\): dg_dp_run_pinned: budget 9"):
        gpu_ctx.dp_run_pinned([good], [9])
    with pytest.raises(capi.DgError, match="dg_dp_run_pinned: budget 1 listed twice"):
        gpu_ctx.dp_run_pinned([good], [1, 1])
    with gpu_ctx.dp_options(digest=1):
        with pytest.raises(capi.DgError, match=r"rc=-6\): dg_dp_run_pinned: option digest") as e:
            gpu_ctx.dp_run_pinned([good])
    assert np.array_equal(gpu_ctx.dp_budget_values(), planes) and np.array_equal(gpu_ctx.dp_answer_paths(g.R), paths) and gpu_ctx.dp_pin_stats() == stats
    assert gpu_ctx.dp_run_pinned(np.tile(np.array([good], np.int32), (65536, 1)))[0].value == planes[g.R]      # the limit itself, all duplicates
    # the margins of the run's own answer check it against an unconstrained partner DP: refused after a pinned run, back after an unpinned one
    with pytest.raises(capi.DgError, match=r"rc=-6\): dg_dp_call_margins: the last run was dg_dp_run_pinned"):
        gpu_ctx.dp_call_margins(g.R)
    gpu_ctx.dp_run_pinned([], [g.R])                     # no pins: dg_dp_run_budgets
    levels, _ = gpu_ctx.dp_call_margins(g.R)
    assert (levels["value"] == gpu_ctx.dp_budget_values()[g.R]).all()

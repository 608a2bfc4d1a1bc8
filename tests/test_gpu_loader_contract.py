"""-m gpu: the contract of dg_dp_load_graph, on both constructions of the sweep's tables (device kernels: the default; host threads: option
host_tables).

Integers only: every comparison is exact.  The graphs are those of tests/loader_graphs.py, pinned on the CPU by
tests/test_loader_graphs.py: every refusal the loader documents, one defect per graph, must come with its code and its text whichever
construction meets it, and leave no graph loaded; a refused load between two good ones must leave nothing behind; and the valid graphs no
generator draws -- no edges at all, a level without in-edges, dead-end vertices, R = 4096 -- must be answered like the oracle answers
them under every option set that changes which kernels run."""
import re

import numpy as np
import pytest

import graphgen
import loader_graphs as lg
import oracle_py as orc
from dipgenie_amd import capi
from paths_model import NEG_INF, PathModel

pytestmark = pytest.mark.gpu

CONSTRUCTIONS = {"device_tables": 0, "host_tables": 1}
DEFECTS = lg.defects()
FAMILIES = lg.valid_families()
_ORACLE = {}


def oracle(g, key, R=None):
    """the oracle's answer for g (at R, if given), with every level digest -- computed once per key"""
    if (key, R) not in _ORACLE:
        _ORACLE[(key, R)] = orc.dp_solve(g if R is None else lg.copy_graph(g, R=R), want_digest=True)
    return _ORACLE[(key, R)]


def run_equals_oracle(ctx, g, ref, tag, digest=True):
    """a loaded graph: value, s_het, both edge lists, cells, relaxations and (option digest is on) every level digest from level 1 on"""
    out = ctx.dp_run()
    assert (out.value, out.s_het) == (ref["value"], ref["s_het"]), tag
    assert out.p1 == ref["p1"] and out.p2 == ref["p2"], tag
    assert (out.cells, out.relaxations) == (ref["cells"], ref["relaxations"]), tag
    if digest:
        got = ctx.dp_level_digest(g.n_levels)
        assert np.array_equal(got[1:], ref["digest"][1:]), (tag, np.flatnonzero(got[1:] != ref["digest"][1:]) + 1)
    return out


# ---------------------------------------------------------------------------------------------- 1. the refusals
def refused(ctx, bad, rc, regex):
    """the load raises with that code and text, and nothing is loaded afterwards -> the message"""
    with pytest.raises(capi.DgError) as info:
        ctx.dp_load_graph(bad)
    msg = str(info.value)
    assert f"(rc={rc}): " in msg and re.search(regex, msg), msg
    with pytest.raises(capi.DgError, match=r"\(rc=-6\): dg_dp_run: no graph loaded"):
        ctx.dp_run()
    with pytest.raises(capi.DgError, match=r"\(rc=-6\): dg_dp_get_table_digest: no graph loaded"):
        ctx.dp_table_digest()
    with pytest.raises(capi.DgError, match=r"\(rc=-6\)"):
        ctx.dp_level_digest(bad.n_levels)
    return msg


@pytest.mark.parametrize("name", list(DEFECTS))
def test_every_defect_is_refused_alike_by_both_constructions(gpu_ctx, name):
    """with a good graph of as many levels resident and run before each refused load: the refusal must not leave its answers behind"""
    bad, rc, regex = DEFECTS[name]
    base = lg.base_graph()
    msgs = []
    with gpu_ctx.dp_options(digest=1):
        for host_tables in CONSTRUCTIONS.values():
            with gpu_ctx.dp_options(host_tables=host_tables):
                gpu_ctx.dp_load_graph(base)
                run_equals_oracle(gpu_ctx, base, oracle(base, "base"), (name, host_tables))
                msgs.append(refused(gpu_ctx, bad, rc, regex))
    if not name.endswith("_beyond_the_end"):             # one place to name: the same text, word for word
        assert msgs[0] == msgs[1]


def test_a_level_of_32769_vertices_is_refused_alike_by_both_constructions(gpu_ctx):
    """The width limit: source, 32,769 vertices, sink.  Both constructions refuse before any state is planned, so the refusal costs
    nothing.  (The other side of the limit is not run: a level of 32,768 vertices is accepted, and its state alone is gigabytes.)"""
    bad, rc, regex = lg.too_wide()
    msgs = []
    for host_tables in CONSTRUCTIONS.values():
        with gpu_ctx.dp_options(host_tables=host_tables):
            msgs.append(refused(gpu_ctx, bad, rc, regex))
    assert msgs[0] == msgs[1]


# ---------------------------------------------------------------------------------------------- 2. a refused load leaves nothing behind
# one refusal of each class: before any upload (the sizes; the level layout; out_off[0]), at the synchronisation in the middle of the
# device construction (an edge, a weight pair, a colour offset), and the width limit
REFUSALS = ["R_4097", "level_empty", "out_off_first", "weight_2", "parallel_adjacent", "hom_off_beyond_the_end", "too_wide"]
RESIDENT = {"larger": lambda: graphgen.random_levelized(9851, n_levels=12, max_width=9, min_width=4, R=4, p_colour=0.6),
            "smaller": lambda: graphgen.random_levelized(9852, widths=[1, 2, 1], R=1, p_colour=0.5)}
_FRESH = {}


def fresh_table_digest():
    """the twelve table digests of the base graph in a context that has never seen a refusal"""
    if not _FRESH:
        ctx = capi.Context(0)
        try:
            ctx.dp_load_graph(lg.base_graph())
            _FRESH.update(ctx.dp_table_digest())
        finally:
            ctx.close()
    return _FRESH


@pytest.mark.parametrize("resident", list(RESIDENT))
@pytest.mark.parametrize("construction", list(CONSTRUCTIONS))
def test_a_refused_load_leaves_nothing_behind(gpu_ctx, construction, resident):
    base, first = lg.base_graph(), RESIDENT[resident]()
    assert (first.n_vertices > 4 * base.n_vertices and first.out_dst.size > 4 * base.out_dst.size and first.R > base.R) if resident == "larger" else \
        (first.n_vertices < base.n_vertices and first.out_dst.size < base.out_dst.size and first.R < base.R)
    want = fresh_table_digest()
    assert len(want) == 12
    with gpu_ctx.dp_options(digest=1, host_tables=CONSTRUCTIONS[construction]):
        for name in REFUSALS:
            bad, rc, regex = lg.too_wide() if name == "too_wide" else lg.defects()[name]
            gpu_ctx.dp_load_graph(first)
            run_equals_oracle(gpu_ctx, first, oracle(first, resident), (name, "before"))
            refused(gpu_ctx, bad, rc, regex)
            gpu_ctx.dp_load_graph(base)
            assert gpu_ctx.dp_table_digest() == want, (name, [t for t, x in gpu_ctx.dp_table_digest().items() if x != want[t]])
            run_equals_oracle(gpu_ctx, base, oracle(base, "base"), (name, "after"))


# ---------------------------------------------------------------------------------------------- 3. the valid families
MODES = {"default": {}, "host_tables": {"host_tables": 1}, "generic_sweep": {"fast": 0}, "plain_launches": {"graph_batch": 0}, "coop_off": {"coop": 0},
         "coop_forced": {"coop": 2}, "no_rowx": {"rowx": 0}, "general_chain": {"lean_chain": 0}, "pairs_forced": {"pair_levels": 1, "pair_min": 1}}
MEMBERS = [(fam, name) for fam, members in FAMILIES.items() for name in members]


@pytest.mark.parametrize("fam,name", MEMBERS)
def test_valid_graphs_no_generator_draws(gpu_ctx, fam, name):
    g = FAMILIES[fam][name]
    ref = oracle(g, (fam, name))
    assert (ref["value"] == NEG_INF) == (fam in ("no_edges", "empty_transition"))
    with gpu_ctx.dp_options(digest=1):
        for mode, opts in MODES.items():
            with gpu_ctx.dp_options(**opts):
                gpu_ctx.dp_load_graph(g)
                run_equals_oracle(gpu_ctx, g, ref, (fam, name, mode))
                if mode == "pairs_forced":               # level digests keep every level a launch of its own: once more without them
                    with gpu_ctx.dp_options(digest=0):
                        gpu_ctx.dp_load_graph(g)
                        run_equals_oracle(gpu_ctx, g, ref, (fam, name, mode, "paired"), digest=False)
                        if fam != "max_budget":
                            assert np.array_equal(gpu_ctx.dp_budget_values(), [oracle(g, (fam, name), b)["value"] for b in range(g.R + 1)])
        tables = []
        for host_tables in CONSTRUCTIONS.values():
            with gpu_ctx.dp_options(host_tables=host_tables):
                gpu_ctx.dp_load_graph(g)
                tables.append(gpu_ctx.dp_table_digest())
        assert tables[0] == tables[1], [t for t in tables[0] if tables[0][t] != tables[1][t]]
        # every budget from one pass (the graph loaded last: the host construction's tables)
        budgets = lg.MAX_BUDGET_PLANES if fam == "max_budget" else list(range(g.R + 1))
        outs = gpu_ctx.dp_run_budgets(budgets)
        planes = gpu_ctx.dp_budget_values()
        assert planes.shape == (g.R + 1,)
        m = PathModel(g)
        for b, out in zip(budgets, outs):
            want = oracle(g, (fam, name), b)
            assert planes[b] == want["value"], (fam, name, b, planes[b], want["value"])
            assert (out.value, out.s_het, out.p1, out.p2) == (want["value"], want["s_het"], want["p1"], want["p2"]), (fam, name, b)
            paths = gpu_ctx.dp_answer_paths(b)
            if want["value"] == NEG_INF:
                assert (paths == -1).all(), (fam, name, b)
            else:
                assert (paths >= 0).all() and m.check_path(paths[0]) is None and m.check_path(paths[1]) is None
                value, s_het, r1, r2 = m.score(paths[0], paths[1])
                assert (value, s_het) == (want["value"], want["s_het"]) and r1 + r2 <= b
        if fam != "max_budget":
            assert (planes != NEG_INF).any() == (fam == "dead_ends")
        else:
            assert planes[0] == NEG_INF and planes[4096] == ref["value"] != NEG_INF and (np.diff(planes.astype(np.int64)) >= 0).all()

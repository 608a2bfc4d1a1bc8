"""-m gpu: the five kernels that read colour lists (dp_edge_flags_kernel, dp_delta_kernel, the finish pass of the traceback,
dp_score_paths_kernel, dp_partner_scores_kernel -- all through union2x2, dg_dp_setops.hpp) on lists that the random generator's
defaults never draw: hundreds to thousands of ids, ids from 0 to 2^31 - 1, score deltas above 255 and above 32,767, and the
uint16 bound of the delta itself.  The graphs are those of colour_graphs.py; tests/test_colour_graphs.py shows on the CPU that they
reach what their names claim.  Integers only: every comparison is exact.

The bound: a score delta is |(Hom u1 u Hom v1) n (Hom u2 u Hom v2)| + |(Het u1 u Het v1) /\\ (Het u2 u Het v2)| and reaches
2 max_hom + 4 max_het (graphgen.delta_bound_graph: 6 M with lists of M ids of both kinds).  A graph is loaded if that fits 16 bits."""
import numpy as np
import pytest

import colour_graphs as cg
import graphgen
import oracle_py as orc
from dipgenie_amd import capi
from partner_model import best_partners
from paths_model import NEG_INF, PathModel
from test_gpu_parity import _dp_both
from test_gpu_score_paths import walked_pairs_score_their_plane
from test_gpu_sweep_variant_parity import every_variant_equals_the_oracle

pytestmark = pytest.mark.gpu

SETTINGS = {"default": {}, "generic": {"fast": 0}, "delta_windows": {"delta_cap_entries": 400}, "delta_overlap": {"delta_overlap": 2},
            "host_tables": {"host_tables": 1}}
SWEEPS = [(topo, case, setting) for topo in cg.SWEEP_TOPOLOGIES for case in cg.CASES
          for setting in (SETTINGS if case in cg.ALL_SETTINGS else ("default", "host_tables"))]


@pytest.mark.parametrize("topo,case,setting", SWEEPS)
def test_sweep_walk_and_finish(gpu_ctx, topo, case, setting):
    """value, s_het, both edge lists, cells, relaxations and every level digest against the oracle"""
    with gpu_ctx.dp_options(**SETTINGS[setting]):
        _dp_both(gpu_ctx, cg.graph(topo, case), ref=cg.oracle(topo, case))


@pytest.mark.parametrize("case", list(cg.CASES))
@pytest.mark.parametrize("topo", cg.SWEEP_TOPOLOGIES)
def test_device_tables_equal_host_tables(gpu_ctx, topo, case):
    digests = []
    for host in (1, 0):
        with gpu_ctx.dp_options(host_tables=host):
            gpu_ctx.dp_load_graph(cg.graph(topo, case))
            digests.append(gpu_ctx.dp_table_digest())
    assert digests[0] == digests[1], [t for t in digests[0] if digests[0][t] != digests[1][t]]


@pytest.mark.parametrize("digest", [1, 0])
@pytest.mark.parametrize("case", cg.PATH_CASES)
@pytest.mark.parametrize("topo", cg.VARIANT_TOPOLOGIES)
def test_every_sweep_variant(gpu_ctx, topo, case, digest):
    every_variant_equals_the_oracle(gpu_ctx, cg.graph(topo, case), cg.oracle(topo, case), cg.planes(topo, case), digest, (topo, case))


def _rows(rec):
    return np.stack([rec["value"], rec["s_het"], rec["r1"], rec["r2"]], axis=1)


@pytest.mark.parametrize("case", cg.PATH_CASES)
def test_score_paths(gpu_ctx, case):
    """the sweep's own walked pair of every budget (all pairs of paths that its edge lists leave open) and sampled pairs, record for
    record against PathModel"""
    g = cg.graph("small", case)
    m = PathModel(g)
    checked = walked_pairs_score_their_plane(gpu_ctx, g, m, case)
    assert [gpu_ctx.dp_budget_values()[b] for b, _, _, _ in checked] == [cg.planes("small", case)[b] for b, _, _, _ in checked]
    assert len(checked) >= 2
    for b, cand, got, hit in checked:
        assert np.array_equal(_rows(got), m.score_many(cand)), (case, b)
    top = max(int(got["value"].max()) for _, _, got, _ in checked)
    assert top > (32767 if case == "disjoint_big" else 255)
    for topo, n in (("small", 300), ("w30", 300)):
        g = cg.graph(topo, case)
        m = PathModel(g)
        rng = np.random.default_rng(11)
        paths = np.concatenate([m.sample_pairs(rng, n // 2)[0], m.sample_pairs(rng, n // 2, 0.9)[0]])
        want = m.score_many(paths)
        gpu_ctx.dp_load_graph(g)
        bad = np.flatnonzero((_rows(gpu_ctx.dp_score_paths(paths)) != want).any(axis=1))
        assert bad.size == 0, (topo, case, bad[:5], want[bad[:5]])
        assert want[:, 0].max() > 255


@pytest.mark.parametrize("case", cg.PATH_CASES)
def test_best_partners(gpu_ctx, case):
    """every path of the graph as the given one, at mixed budgets: records and partner paths against partner_model; and for a path of
    the sweep's answer the partner within what the pair's budget leaves is worth the sweep's plane -- no more, no less"""
    g = cg.graph("small", case)
    m = PathModel(g)
    given = np.array(m.all_paths(), np.int32)
    assert 20 <= len(given) <= 2000, len(given)
    budgets = np.random.default_rng(42).integers(0, g.R + 2, len(given)).astype(np.int32)
    values, partners = best_partners(m, given, budgets)
    reach = values != NEG_INF
    want = np.array([m.score(given[i], partners[i]) if reach[i] else (NEG_INF, 0, m.recombinations(given[i]), 0) for i in range(len(given))], np.int64)
    assert np.array_equal(want[:, 0], values) and reach.any()
    # the 16-bit score of one in-edge, d(given hop, edge): the largest that a query meets
    top = max(sum(m.delta(int(p[l - 1]), u, int(p[l]), v)) for p in given for l in range(1, m.L) for u in range(g.level_off[l - 1], g.level_off[l]) for v in m.succ[u])
    assert top > (32767 if case == "disjoint_big" else 255), top
    gpu_ctx.dp_load_graph(g)
    rec, rows = gpu_ctx.dp_best_partners(given, budgets)
    bad = np.flatnonzero((_rows(rec) != want).any(axis=1))
    assert bad.size == 0, (case, bad[:5], _rows(rec)[bad[:5]], want[bad[:5]])
    assert np.array_equal(rows, partners)
    # the sweep's answer: one pair per reachable budget that is worth its plane
    for b, cand, got, hit in walked_pairs_score_their_plane(gpu_ctx, g, m, case):
        plane = int(gpu_ctx.dp_budget_values()[b])
        for a in (0, 1):
            p, r_p = cand[hit, a], int(got[hit]["r1" if a == 0 else "r2"])
            rec, _ = gpu_ctx.dp_best_partners(cand[hit:hit + 1, a], np.array([b - r_p], np.int32))
            assert int(rec["value"][0]) <= plane and int(rec["value"][0]) == plane, (case, b, a, p)


# ------------------------------------------------------------------------------------- the uint16 bound of the score delta
SMALL = dict(n_levels=12, max_width=9, R=3)


def _still_solves(ctx):
    g = graphgen.random_levelized(9900, **SMALL)
    _dp_both(ctx, g)


@pytest.mark.parametrize("host_tables", [0, 1])
@pytest.mark.parametrize("M,hom,het,value,s_het", [(10922, True, True, 109220, 87376), (16383, False, True, 131064, 131064), (16383, True, False, 32766, 0)])
def test_the_largest_deltas_that_fit_are_accepted(gpu_ctx, M, hom, het, value, s_het, host_tables):
    """6 M = 65,532 with both kinds, 4 M = 65,532 with het lists alone, 2 M with hom lists alone: loaded and solved"""
    g = graphgen.delta_bound_graph(M, hom=hom, het=het)
    ref = orc.dp_solve(g, want_digest=True)
    assert (ref["value"], ref["s_het"]) == (value, s_het)
    with gpu_ctx.dp_options(host_tables=host_tables):
        out = _dp_both(gpu_ctx, g, ref=ref)
    assert (out.value, out.s_het) == (value, s_het)


REJECTED = {
    "both_10923": lambda: graphgen.delta_bound_graph(10923),                                  # 6 M = 65,538
    "both_16383": lambda: graphgen.delta_bound_graph(16383),                                  # 6 M = 98,298
    "one_hom_list_16384": lambda: graphgen.delta_bound_graph(16384, het=False, only=(1,)),
    "one_het_list_16384": lambda: graphgen.delta_bound_graph(16384, hom=False, only=(4,)),
    "all_hom_lists_16384": lambda: graphgen.delta_bound_graph(16384, het=False),
}


@pytest.mark.parametrize("host_tables", [0, 1])
@pytest.mark.parametrize("name", list(REJECTED))
def test_deltas_beyond_16_bits_are_rejected_at_load(gpu_ctx, name, host_tables):
    """never a value, never the run's own "disagree" / "corrupt": the load says "too long", and the context goes on working"""
    g = REJECTED[name]()
    with gpu_ctx.dp_options(host_tables=host_tables):
        try:
            out = gpu_ctx.dp_solve(g)
        except capi.DgError as e:
            text = str(e)
            assert "too long" in text and "dg_dp_load_graph" in text and "disagree" not in text and "corrupt" not in text, text
        else:
            ref = orc.dp_solve(g)
            raise AssertionError(f"{name}: loaded and answered value {out.value} s_het {out.s_het}; the oracle has {ref['value']} / {ref['s_het']}")
        _still_solves(gpu_ctx)

"""TEST INFRASTRUCTURE: the graphs and queries beyond the 16,384 cells of LDS state (widest level x (budget + 1)) that the tests of the
device-memory route (option partner_wide) share -- tests/test_gpu_partner_wide.py, tests/test_gpu_marginals_wide.py and, without a
device, tests/test_partner_wide_model.py, which keeps the shapes on their side of the limit.  Every reference is computed once per
process and never changed."""
import numpy as np

import graphgen
from marginals_model import partner_marginals_batch
from partner_model import best_partners
from paths_model import PathModel

MAX_CELLS = 16384                                        # the LDS route's limit
WIDE_MAX_CELLS = 1 << 24                                 # the device-memory route's


def _mixed(n, top, seed=42):
    """n budgets 0..top, the first four at the top"""
    b = np.random.default_rng(seed).integers(0, top + 1, n).astype(np.int32)
    b[:4] = top
    return b


# name -> (graph, budgets, widest level, widest level x (largest budget + 1))
SHAPES = {
    # one row of 128 planes past the limit: 129 x 128
    "over_one_row": (lambda: graphgen.random_levelized(8820, n_levels=5, max_width=129, min_width=129, R=4, p_colour=0.5, extra_edges=0.5),
                     _mixed(12, 127), 129, 16512),
    # a level wider than the 1,024 vertices of the in-edge stage: every inner level is read from global memory
    "wide1100": (lambda: graphgen.random_levelized(8824, n_levels=5, max_width=1100, min_width=1100, R=4, extra_edges=0.3),
                 np.array([15, 15, 0, 3, 15, 3, 0, 15, 9, 12], np.int32), 1100, 17600),
    # rows of 1,101 planes, longer than any workgroup, and a budget that binds: nearly every edge is a recombination
    "long_rows": (lambda: graphgen.random_levelized(8823, n_levels=1300, max_width=16, min_width=12, R=4, p_w1=0.9),
                  np.array([1100, 1100, 1050, 600, 0], np.int32), 16, 17616),
    # the same rows on 40 levels: the budgets lie on either side of what a path needs
    "long_rows_short": (lambda: graphgen.random_levelized(8825, n_levels=40, max_width=16, min_width=12, R=4, p_w1=0.9),
                        np.array([1100, 1100, 20, 5, 0, 1030], np.int32), 16, 17616),
}
_GRAPH, _PARTNER, _MARGINALS = {}, {}, {}


def given_paths(m, seed, n):
    """half uniform, half biased towards weight-0 edges (as tests/test_gpu_partner.py draws them)"""
    rng = np.random.default_rng(seed)
    a, _ = m.sample_paths(rng, n - n // 2)
    b, _ = m.sample_paths(rng, n // 2, 0.9)
    return np.concatenate([a, b])


def shape(name):
    """graph, model, given paths, budgets"""
    if name not in _GRAPH:
        make, budgets, _, _ = SHAPES[name]
        g = make()
        m = PathModel(g)
        _GRAPH[name] = (g, m, given_paths(m, 41, len(budgets)), budgets)
    return _GRAPH[name]


def partner_ref(name):
    """... and partner_model's values and partners"""
    if name not in _PARTNER:
        g, m, given, budgets = shape(name)
        _PARTNER[name] = (g, m, given, budgets, *best_partners(m, given, budgets))
    return _PARTNER[name]


def marginals_ref(name):
    """... and marginals_model's level records and vertex values"""
    if name not in _MARGINALS:
        g, m, given, budgets = shape(name)
        _MARGINALS[name] = (g, m, given, budgets, *partner_marginals_batch(m, given, budgets))
    return _MARGINALS[name]


def partner_records(m, given, budgets, values, partners):
    """what dg_dp_best_partners' records must hold: the pair (given, partner) as the model scores it"""
    from paths_model import NEG_INF
    want = np.zeros((len(given), 4), np.int64)
    for i in range(len(given)):
        want[i] = m.score(given[i], partners[i]) if values[i] != NEG_INF else (NEG_INF, 0, m.recombinations(given[i]), 0)
    assert np.array_equal(want[:, 0], values) and (want[values != NEG_INF, 3] <= budgets[values != NEG_INF]).all()
    return want

"""CPU: tests/recombination_margins_model.py (recombination margins, written from their definition) against brute force.  On the
enumerable graphs of tests/test_gpu_score_paths.py, for every budget 0..3: E_t[s] of every transition equals the maximum over all
enumerated ordered pairs of paths within the budget whose two hops of that transition weigh s together, with the hop pair the tie rule
names; the largest of the three is V_b; called_out is the brute-force value of the pairs that take exactly the called hops, for an
optimal pair, a sampled pair and cells that are no paths.  This validates the yardstick of tests/test_gpu_recombination_margins.py.
Then, on that file's graphs, floors under the branches worth having, and the padded-graph claim of tests/padded_graphs.py for the
records."""
import numpy as np
import pytest

import padded_graphs as pg
from paths_model import NEG_INF, PathModel
from phase_margins_model import joint_states_fb
from recombination_margins_model import recombination_margins_np, remap_rows
from test_genotype_margins_model import BUDGETS, _called_kinds, case
from test_gpu_phase_margins import BUDGETS as GPU_BUDGETS, SEEDS, case as gpu_case
from test_gpu_score_paths import ENUMERABLE


def _hop_weights(m, P):
    """[n, L - 1]: the weight of every hop of every enumerated path"""
    return np.array([[m.succ[p[l]][p[l + 1]] for l in range(m.L - 1)] for p in P.tolist()], np.int64)


@pytest.mark.parametrize("q", range(len(ENUMERABLE)))
def test_every_value_and_hop_pair_is_the_brute_force_one(q):
    g, m, P, rec, S, model, brute = case(q)
    W = _hop_weights(m, P)
    reachable = [0, 0, 0]
    no_edge = 0
    for b in BUDGETS:
        states = joint_states_fb(m, b)
        V = states[2]
        assert V == model[b][1]
        kinds = _called_kinds(m, P, rec, S, V, b, 100 * q + b)
        records, out, V2 = recombination_margins_np(m, b, np.stack(kinds), states)
        assert V2 == V and records.shape == (m.L - 1, 16) and out.shape == (len(kinds), m.L - 1, 2)
        plain, none, _ = recombination_margins_np(m, b, None, states)
        assert none is None and np.array_equal(plain, records)              # the records do not depend on called
        ok = (rec[:, None] + rec[None, :]) <= b
        for l in range(m.L - 1):
            ws = W[:, l][:, None] + W[:, l][None, :]
            assert records[l, 0] == l
            for s in range(3):
                keep = ok & (ws == s)
                got = tuple(records[l, [1 + s, 4 + s, 7 + s, 10 + s, 13 + s]].tolist())
                if not keep.any():
                    assert got == (NEG_INF, -1, -1, -1, -1), (q, b, l, s)
                    continue
                best = int(S[keep].max())
                p, r = np.nonzero(keep & (S == best))
                want = (best,) + min(zip(P[p, l].tolist(), P[r, l].tolist(), P[p, l + 1].tolist(), P[r, l + 1].tolist()))
                assert got == want, (q, b, l, s)
                assert got[1] <= got[2]                                      # the symmetry of d
                reachable[s] += 1
            assert records[l, 1:4].max() == V, (q, b, l)                     # the closing check
            for which, called in enumerate(kinds):
                hops = [(int(called[h][l]), int(called[h][l + 1])) for h in range(2)]
                if any(v not in m.succ[u] for u, v in hops):
                    assert out[which, l].tolist() == [-1, NEG_INF]
                    continue
                s_called = sum(m.succ[u][v] for u, v in hops)
                keep = (ok & ((P[:, l] == hops[0][0]) & (P[:, l + 1] == hops[0][1]))[:, None] & ((P[:, l] == hops[1][0]) & (P[:, l + 1] == hops[1][1]))[None, :])
                assert out[which, l].tolist() == [s_called, int(S[keep].max()) if keep.any() else NEG_INF], (q, b, l, which)
        if V != NEG_INF:                                                     # the optimal pair: every transition of it is worth V_b
            assert (out[0, :, 1] == V).all() and out[0, :, 0].sum() <= b
        no_edge += int((out[-1, :, 0] == -1).sum())                          # cells that are no paths
    print(f"case {q}: reachable (transition, budget) entries per s {reachable}")
    assert min(reachable) > 0 and no_edge > 0


def test_the_gpu_graphs_are_not_vacuous():
    """over the 450 (seed, budget, transition) cases of tests/test_gpu_recombination_margins.py, computed on the CPU so that the floors
    hold however the tests are selected"""
    s1 = s2 = better = equal = total = 0
    for seed in SEEDS:
        g, m, two, called = gpu_case(seed)
        for b in GPU_BUDGETS:
            records, _, V = recombination_margins_np(m, b)
            v = records[:, 1:4].astype(np.int64)
            total += len(v)
            s1 += int((v[:, 1] != NEG_INF).sum())
            s2 += int((v[:, 2] != NEG_INF).sum())
            better += int((np.maximum(v[:, 1], v[:, 2]) > v[:, 0]).sum())
            equal += int(((v[:, 1] == v[:, 0]) & (v[:, 0] != NEG_INF)).sum())
    print(f"transitions {total}: reachable s = 1 {s1}, s = 2 {s2}, recombining strictly better {better}, value[1] == value[0] {equal}")
    assert total == 450 and s1 >= 150 and s2 >= 120 and better >= 15 and equal >= 5


@pytest.mark.parametrize("shape", sorted(pg.SHAPES))
def test_the_padded_graph_claim_carries_over(shape):
    g, gp, new_id = pg.SHAPES[shape](small=True)
    b = pg.DEEP_BUDGET if shape == "deep" else 3
    want, _, V = recombination_margins_np(PathModel(g), b)
    got, _, Vp = recombination_margins_np(PathModel(gp), b)
    assert Vp == V != NEG_INF
    assert np.array_equal(got, remap_rows(want, new_id))
    ids = got[:, 4:]
    assert not pg.pad_mask(gp, new_id)[ids[ids >= 0]].any()                 # no pad is in a record
    assert (got[:, 2] != NEG_INF).any() and (got[:, 3] != NEG_INF).any()    # s = 1 and s = 2 are reachable

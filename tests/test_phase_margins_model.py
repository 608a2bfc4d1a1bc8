"""CPU: tests/phase_margins_model.py (phase margins, written from their definition) against brute force.  On the enumerable graphs of
tests/test_gpu_score_paths.py, for every budget 0..3 and three kinds of classes: cis and trans of every pair of neighbouring het
levels equal the maximum over all enumerated ordered pairs of paths with the required ordered classes at both levels, with the cell
the tie rule names; trans is also the value of the pairs that keep the order at the first level and swap it at the second; cis is V_b
for an optimal pair and at least the score of any called pair of paths that fits the budget.  This validates the yardstick of
tests/test_gpu_phase_margins.py.  On graphs this small a sampled pair almost never has a reachable trans: they pin the definition,
the GPU tests' graphs hold the interesting branch."""
import numpy as np
import pytest

from call_margins_model import class_arrays
from paths_model import NEG_INF
from phase_margins_model import het_levels, joint_states_fb, phase_margins_np
from test_genotype_margins_model import BUDGETS, _called_kinds, case
from test_gpu_score_paths import ENUMERABLE


def _brute(P, ok, S, ids, a, e, xa, xe):
    """(value, vertex1, vertex2) at level a of the best ordered pair with classes xa at a and xe at e; ties: smallest vertex1, then vertex2"""
    ca, ce = ids[P[:, a]], ids[P[:, e]]
    keep = ok & (ca[:, None] == xa[0]) & (ca[None, :] == xa[1]) & (ce[:, None] == xe[0]) & (ce[None, :] == xe[1])
    if not keep.any():
        return NEG_INF, -1, -1
    best = int(S[keep].max())
    p, q = np.nonzero(keep & (S == best))
    return (best,) + min(zip(P[p, a].tolist(), P[q, a].tolist()))


@pytest.mark.parametrize("q", range(len(ENUMERABLE)))
def test_cis_and_trans_are_the_brute_force_maxima(q):
    g, m, P, rec, S, model, brute = case(q)
    n_records = n_trans = n_optimal = 0
    for b in BUDGETS:
        states = joint_states_fb(m, b)
        V = states[2]
        assert V == model[b][1]
        ok = (rec[:, None] + rec[None, :]) <= b
        for kind, cls in enumerate(class_arrays(g, 21 + q)):
            ids = np.arange(m.nV) if cls is None else np.asarray(cls, np.int64)
            kinds = _called_kinds(m, P, rec, S, V, b, 100 * q + b)
            for which, called in enumerate(kinds):
                records, V2 = phase_margins_np(m, called, b, cls, states)
                het = het_levels(m, called, cls)
                assert V2 == V and len(records) == max(len(het) - 1, 0)
                if kind == 1:                            # one class for all: no het level
                    assert het == []
                for (a, e, cis, c1, c2, trans, t1, t2), ha, he in zip(records.tolist(), het[:-1], het[1:]):
                    assert (a, e) == (ha, he)
                    xa, xe = (ids[called[0][a]], ids[called[1][a]]), (ids[called[0][e]], ids[called[1][e]])
                    assert (cis, c1, c2) == _brute(P, ok, S, ids, a, e, xa, xe), (q, b, kind, which, a, e)
                    assert (trans, t1, t2) == _brute(P, ok, S, ids, a, e, xa[::-1], xe), (q, b, kind, which, a, e)
                    assert trans == _brute(P, ok, S, ids, a, e, xa, xe[::-1])[0]          # the symmetry of d: swap at e instead
                    assert max(cis, trans) <= V
                    n_records += 1
                    n_trans += trans != NEG_INF
                    if which == 0 and V != NEG_INF:      # the optimal pair
                        assert cis == V
                        n_optimal += 1
                if which < len(kinds) - 1:               # real paths: cis is at least their score where they fit the budget
                    r = m.recombinations(called[0]) + m.recombinations(called[1])
                    if r <= b:
                        assert all(rec_[2] >= m.score(called[0], called[1])[0] for rec_ in records.tolist())
    print(f"case {q}: records {n_records}, with a reachable trans {n_trans}, of an optimal pair {n_optimal}")
    assert n_records > 0 and n_optimal > 0

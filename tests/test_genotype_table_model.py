"""CPU: tests/genotype_table_model.py (the genotype table, written from its definition) against brute force.  On the enumerable graphs
of tests/test_gpu_score_paths.py, for every budget 0..3 and three kinds of classes: per level and genotype the entry is the best value
of any enumerated ordered pair of paths whose cell has that genotype, with the smallest (min, max) cell among the best; genotypes no
pair passes through are absent; and the table implies the margin records (level_records) and bounds the joint marginals
(joint_marginals) as its definition says.  The numpy form is the plain one.  This validates the yardstick of
tests/test_gpu_genotype_table.py.  Cases 5..10 are the same graphs with dead-end vertices (tests/loader_graphs.py): the yardstick of
tests/test_gpu_dead_ends.py."""
import numpy as np
import pytest

from call_margins_model import class_arrays
from genotype_margins_model import joint_marginals, level_records
from genotype_table_model import genotype_table, genotype_table_np, record_from_table, vertex_maxima_from_table
from paths_model import NEG_INF
from test_genotype_margins_model import BUDGETS, _called_kinds, case
from test_partner_model import DEAD_ENDS
from test_gpu_score_paths import ENUMERABLE


def _c(cls, v):
    return int(v) if cls is None else int(cls[v])


@pytest.mark.parametrize("q", [*range(len(ENUMERABLE)), *DEAD_ENDS])
def test_every_entry_is_the_brute_force_best_of_its_genotype(q):
    g, m, P, rec, S, model, brute = case(q)
    listed = absent = 0
    for b in BUDGETS:
        T, V = model[b]
        for kind, cls in enumerate(class_arrays(g, 11 + q)):
            table = genotype_table(m, T, cls)
            assert len(table) == m.L
            for l in range(m.L):
                a0, k = int(m.level_off[l]), int(m.level_off[l + 1] - m.level_off[l])
                # every ordered cell some pair passes through, as (-value, min, max), by genotype: the smallest is the entry
                cands = {}
                for i in range(k):
                    for j in range(k):
                        if brute[b][l][i, j] != NEG_INF:
                            geno = tuple(sorted((_c(cls, a0 + i), _c(cls, a0 + j))))
                            cands.setdefault(geno, []).append((-int(brute[b][l][i, j]), a0 + min(i, j), a0 + max(i, j)))
                want = [geno + (min(c)[1], min(c)[2], -min(c)[0]) for geno, c in sorted(cands.items())]
                assert table[l] == want, (q, b, kind, l)
                assert all(r[0] <= r[1] and r[2] <= r[3] for r in table[l])
                if V != NEG_INF:
                    assert max(r[4] for r in table[l]) == V
                else:
                    assert table[l] == []
                classes = {_c(cls, v) for v in range(a0, a0 + k)}
                listed += len(want)
                absent += len(classes) * (len(classes) + 1) // 2 - len(want)
                if cls is None:                          # the entries are exactly the reachable cells i <= j
                    assert [(r[2], r[3], r[4]) for r in table[l]] == [(a0 + i, a0 + j, int(brute[b][l][i, j])) for i in range(k) for j in range(i, k)
                                                                      if brute[b][l][i, j] != NEG_INF]
    assert listed > 0 and absent > 0


@pytest.mark.parametrize("q", [*range(len(ENUMERABLE)), *DEAD_ENDS])
def test_the_table_implies_the_margin_records_and_bounds_the_marginals(q):
    g, m, P, rec, S, model, brute = case(q)
    own = other = 0
    for b in BUDGETS:
        T, V = model[b]
        J = joint_marginals(m, T)
        for kind, cls in enumerate(class_arrays(g, 11 + q)):
            table = genotype_table(m, T, cls)
            off, rows = genotype_table_np(m, [np.array(t, np.int64) for t in T], cls)
            assert off.tolist() == np.cumsum([0] + [len(t) for t in table]).tolist()
            assert [tuple(r) for r in rows.tolist()] == [r for t in table for r in t], (q, b, kind)
            for called in _called_kinds(m, P, rec, S, V, b, 100 * q + b):
                for l, (c1, c2, value, a1, a2, alt) in enumerate(level_records(m, T, called, cls)):
                    got = record_from_table(table[l], c1, c2, cls)
                    assert got[1:] == (a1, a2, alt), (q, b, kind, l)
                    if got[0] is not None:               # the called cell is the best of its genotype
                        assert got[0] == value
                        own += 1
                    else:
                        assert cls is not None or value == NEG_INF
                        other += 1
            top = vertex_maxima_from_table(m, off, rows, cls)
            assert (np.array(J) <= top).all(), (q, b, kind)
            if cls is None:
                assert top.tolist() == J
    assert own > 0 and other > 0

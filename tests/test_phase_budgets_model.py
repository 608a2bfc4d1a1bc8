"""CPU: tests/phase_budgets_model.py, the slot plan of dg_dp_phase_margins_budgets, against a per-query simulation that shares nothing,
and the floors that keep tests/test_gpu_phase_budgets.py from being vacuous -- computed here, on the CPU, on the query lists that file
runs (query_lists below; the list of the run's own answers needs a device and is not among them)."""
import numpy as np
import pytest

import graphgen
from paths_model import PathModel
from phase_budgets_model import STATS, classes_of, naive_live, plan, query_keys

SEEDS = range(9300, 9306)
BUDGETS = (0, 2, 5)
_CASES = {}


def case(seed):
    """graph, model, the two-class array and one sampled pair of paths per budget: the draws of tests/test_gpu_phase_margins.py"""
    if seed not in _CASES:
        g = graphgen.random_levelized(seed, widths=[1] + [3, 5, 2, 4, 6, 3] * 4 + [1], R=3, p_w1=0.3, dup_edges=True, extra_edges=1.2, p_colour=0.5)
        m = PathModel(g)
        rng = np.random.default_rng(seed)
        two = rng.integers(0, 2, g.n_vertices).astype(np.int32)
        called = {b: m.sample_paths(rng, 2, p_w0=0.9)[0] for b in BUDGETS}
        _CASES[seed] = (g, m, two, called)
    return _CASES[seed]


def _het(c):
    return [l for l in range(c.shape[1]) if c[0, l] != c[1, l]]


def query_lists(seed, cls):
    """name -> (called int32 [n, 2, L], budgets int32 [n]).  Cells need not lie on a path, so the variants are made by hand:
    same     one sampled pair at budgets (0, 2, 5, 2): one key at a time, one slot throughout
    sampled  a different sampled pair per budget
    mixed    the pair P of budget 2 and what shares with it and parts from it: P with one inner het level made hom (the same seed
             above that level, another next het level below it), P with its rows swapped (the same het levels, the classes in the
             other order), a pair without a het level, a pair with one, and the pair of budget 5"""
    g, m, two, called = case(seed)
    P = np.ascontiguousarray(called[2], np.int32)
    het = _het(classes_of(P[None], cls)[0])
    assert len(het) >= 3, (seed, het)
    hom = P.copy()
    hom[1, het[len(het) // 2]] = hom[0, het[len(het) // 2]]
    none = np.stack([P[0], P[0]])
    one = none.copy()
    one[1, het[0]] = P[1, het[0]]
    lists = {
        "same": (np.stack([P] * 4), [0, 2, 5, 2]),
        "sampled": (np.stack([called[b] for b in BUDGETS]), list(BUDGETS)),
        "mixed": (np.stack([P, none, hom, P[::-1], one, called[5]]), [2, 5, 5, 0, 2, 5]),
    }
    return {k: (np.ascontiguousarray(c, np.int32), np.asarray(b, np.int32)) for k, (c, b) in lists.items()}


def all_lists():
    for seed in SEEDS:
        for kind, cls in enumerate((None, case(seed)[2])):
            for name, (called, budgets) in query_lists(seed, cls).items():
                yield (seed, kind, name), called, cls


def test_the_plan_is_the_union_of_the_queries_intervals():
    for tag, called, cls in all_lists():
        p, naive = plan(called, cls), naive_live(called, cls)
        L = called.shape[2]
        keys = [query_keys(c) for c in classes_of(called, cls)]
        for l in range(L):
            assert set(p["live"][l]) == naive[l], (tag, l)
            assert len(set(p["live"][l].values())) == len(p["live"][l])                 # one slot per live key
            for q1, s1 in p["on_slot"][l].items():                                      # two queries on one slot have equal keys
                for q2, s2 in p["on_slot"][l].items():
                    assert (s1 == s2) == (keys[q1][l] == keys[q2][l]), (tag, l, q1, q2)
            assert all(key[0] == l for key in p["created"][l])                          # a key is seeded at its own level ...
            if l:
                assert set(p["created"][l]) == naive[l - 1] - naive[l], (tag, l)        # ... when it is first carried below it
        st = p["stats"]
        assert tuple(st) == STATS
        assert st["slot_levels"] == sum(len(x) for x in naive) and st["max_live_slots"] == max(len(x) for x in naive)
        assert st["slots_allocated"] == st["max_live_slots"]                            # the largest live count is enough
        assert st["seed_keys"] == len(set().union(*naive))
        assert st["backward_launches"] == sum(1 for x in naive if x)
        assert st["records"] == sum(len(r) for r in p["reads"]) == sum(max(len(_het(c)) - 1, 0) for c in classes_of(called, cls))
        assert st["readout_launches"] == sum(1 for r in p["reads"] if r)


def test_one_query_is_the_one_budget_schedule():
    """slot-levels of a single query = the levels between its first and last het level: seeded_launches of dg_dp_phase_margins"""
    for seed in SEEDS:
        g, m, two, called = case(seed)
        for cls in (None, two):
            for b in BUDGETS:
                het = _het(classes_of(called[b][None], cls)[0])
                st = plan(called[b][None], cls)["stats"]
                want = het[-1] - het[0] if len(het) >= 2 else 0
                assert (st["slot_levels"], st["backward_launches"], st["max_live_slots"], st["records"]) == (want, want, int(want > 0), max(len(het) - 1, 0))
            st = plan(*query_lists(seed, cls)["same"][:1], cls)["stats"]
            assert st["max_live_slots"] == 1 and st["queries"] == 4


def test_the_gpu_set_is_not_vacuous():
    """counted over the lists of all six seeds and both class arrays; every floor also holds in at least one single list"""
    part = reseed = swapped = more_keys = shared_levels = 0
    for tag, called, cls in all_lists():
        p = plan(called, cls)
        L = called.shape[2]
        keys = [query_keys(c) for c in classes_of(called, cls)]
        n = len(keys)
        # two queries share a seed and then part ways: one key on some level, keys of different het levels on a level below it
        found = False
        for q1 in range(n):
            for q2 in range(q1 + 1, n):
                both = [l for l in range(L) if l in keys[q1] and l in keys[q2]]
                same = [l for l in both if keys[q1][l] == keys[q2][l]]
                if same and any(l < max(same) and keys[q1][l][0] != keys[q2][l][0] for l in both):
                    found = True
                shared_levels += len(same)
        part += found
        # a freed slot is seeded again at the level it was freed
        found = False
        for l in range(1, L):
            freed = {slot for key, slot in p["live"][l].items() if key not in p["live"][l - 1]}
            if any(p["live"][l - 1][key] in freed for key in p["created"][l]):
                found = True
        reseed += found
        # the same het level with the orders swapped: two slots
        found = False
        for l in range(L):
            for (e, a, b), slot in p["live"][l].items():
                if (e, b, a) in p["live"][l]:
                    assert p["live"][l][(e, b, a)] != slot
                    found = True
        swapped += found
        more_keys += p["stats"]["seed_keys"] > p["stats"]["max_live_slots"]
    print(f"lists with: share then part {part}, a slot re-seeded where it was freed {reseed}, swapped orders {swapped}, more keys than slots {more_keys}; "
          f"levels shared by a pair of queries {shared_levels}")
    assert part >= 6 and reseed >= 12 and swapped >= 6 and more_keys >= 12 and shared_levels >= 100


@pytest.mark.parametrize("n", [1, 7])
def test_no_het_level_no_slot(n):
    g, m, two, called = case(9300)
    same = np.stack([np.stack([called[2][0], called[2][0]])] * n)
    st = plan(same)["stats"]
    assert st == dict(queries=n, records=0, seed_keys=0, slot_levels=0, backward_launches=0, readout_launches=0, max_live_slots=0, slots_allocated=0)

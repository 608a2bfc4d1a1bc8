"""CPU: pins tests/anchor_model.py (the plain restatement that tests/test_gpu_anchor_kernels.py holds dg_anchor_* to) and the
inputs of tests/anchor_cases.py.  The model's key order against hand-written vectors, its ordering stage against every verbatim
dump of the REAL reference in tests/golden/anchors.json; then, per input family, that the input has the property it was made
for, and that a model with the corresponding rule broken gives another answer on it (so a device that breaks the rule cannot
pass the GPU test by accident)."""
import json
import os

import numpy as np
import pytest

import anchor_cases as ac
import anchor_model as am

HERE = os.path.dirname(os.path.abspath(__file__))
ANCH = json.load(open(os.path.join(HERE, "golden", "anchors.json")))


def order_of(lists, n_haps=1):
    return [l for _, _, l in am.filter_and_sort([(0, 0, l) for l in lists], n_haps).occs]


# front 5 and back 7 are shared, so only the key decides; worked out by hand from the ASCII codes ('_' = 0x5F is above every digit)
KEY_VECTORS = [
    ([5, 10, 7], [5, 9, 7]),                    # "10_" < "9_": '1' < '9'
    ([5, 10, 7], [5, 1, 7]),                    # "10_" < "1_": '0' < '_'
    ([5, 100, 7], [5, 99, 7]),                  # '1' < '9'
    ([5, 0, 7], [5, 10, 7]),                    # '0' < '1'
    ([5, 2147483647, 7], [5, 214748364, 7]),    # "2147483647_" < "214748364_": '7' < '_'
    ([5, 7], [5, 7, 3, 7]),                     # "5_7_" is a proper prefix of "5_7_3_7_": the shorter string first
    ([5, 50, 7], [5, 5, 7]),                    # token-level prefix: "5_50_7_" < "5_5_7_" ('0' < '_')
]


@pytest.mark.parametrize("first,second", KEY_VECTORS)
def test_key_order_vectors(first, second):
    assert am.key_of(first) < am.key_of(second)
    assert order_of([first, second]) == [first, second] == order_of([second, first])


def test_stable_up_to_16_unstable_above():
    tie = [[5, 9, 7], [5, 10, 7]]
    rest = [[20 + q, 1, 90] for q in range(15)]
    res = am.filter_and_sort([(0, 0, l) for l in rest[:14] + tie], 1)
    assert res.unstable == [] and [l for _, _, l in res.occs][:2] == [[5, 10, 7], [5, 9, 7]]
    assert am.filter_and_sort([(0, 0, l) for l in rest + tie], 1).unstable == [(0, 0)]
    assert am.filter_and_sort([(0, 0, l) for l in rest + [tie[0], tie[0]]], 1).unstable == []      # identical lists tie harmlessly


def test_filter_compares_as_float32():
    occs = [(0, 0, [1, 2]), (0, 1, [1, 2]), (1, 0, [3]), (1, 2, [4])]
    assert am.filter_and_sort(occs, 3, np.float32(2.0)).dropped == {0}
    assert am.filter_and_sort(occs, 3, np.float32(0.34) * np.float32(3)).dropped == {0}
    assert am.filter_and_sort(occs, 3, np.float32(2.0000002)).dropped == set()
    assert am.filter_and_sort(occs, 3, np.float32(1.0)).dropped == {0, 1}
    assert am.filter_and_sort(occs, 3, np.float32(16777217.0)).dropped == set()


def test_spans_by_hand():
    # steps: vertex 4 over bases 0..2, an empty step (vertex 9), vertex 2 over base 3, vertex 4 again over 4..5, vertex 0 over 6..9
    top = [3, 9, 0, 7, 5, 1, 2, 4, 6, 8]
    got = am.spans(4, [0, 1, 3, 6], [4, 9, 2, 4, 0], [0, 3, 3, 4, 6, 10], top)
    assert got == [[2, 4], [2, 4], [2, 0, 4], [0]]


@pytest.mark.parametrize("name", [n for n, a in ANCH.items() if "dump" in a])
def test_ordering_stage_reproduces_reference_dump(name):
    """the dump's occurrences, per id in (haplotype, shuffled) order -- occurrences of one key are identical lists, so no shuffle
    can change what the reference saw -- through the model's map + sort with the filter off: the dump's order comes back"""
    want = [(int(i), int(h), [int(v) for v in vs.split(",")]) for i, h, vs in (l.split() for l in ANCH[name]["dump"] if not l.startswith("homo"))]
    rng = np.random.default_rng(5)
    shuffled = [want[int(i)] for i in rng.permutation(len(want))]
    shuffled.sort(key=lambda o: o[1])                                           # (stable: shuffled inside a haplotype)
    res = am.filter_and_sort(shuffled, 1 + max(h for _, h, _ in want))
    assert res.unstable == [] and res.occs == want


# ------------------------------------------------------------------------------------------- the GPU tests' inputs, on the CPU
def model_of(case, **kw):
    return am.run(case["k"], case["top"], case["haps"], case["sp_hash"], kw.get("min_shared", case["min_shared"]))


def check_case_is_valid(case):
    assert case["top"].size == case["n_vertices"] and not np.array_equal(case["top"], np.arange(case["n_vertices"]))
    assert np.all(np.diff(case["sp_hash"].astype(object)) > 0) if case["sp_hash"].size > 1 else True
    for hs, ps, sv, ss in case["haps"]:
        assert hs.size == ps.size and ss.size == sv.size + 1 and ss[0] == 0 and np.all(np.diff(ss) >= 0) and sv.size >= 1
        assert np.all(np.diff(ps) >= 0) and (ps.size == 0 or (ps[0] >= 0 and ps[-1] + case["k"] <= ss[-1]))
        assert sv.min() >= 0 and sv.max() < case["n_vertices"]


def test_span_cases_cover_what_they_are_for():
    lengths = set()
    for k in (5, 31, 40):
        for variant in ac.SPAN_VARIANTS:
            case = ac.span_case(k, variant)
            check_case_is_valid(case)
            res = model_of(case)
            assert len(res.occs) == res.n_candidates == sum(h[0].size for h in case["haps"]) and not res.dropped      # every span comes back
            lengths |= {len(l) for _, _, l in res.occs}
            assert {1, 2, k} <= {len(l) for _, _, l in res.occs}
            hs, ps, sv, ss = case["haps"][0]
            assert ps[-1] + k == ss[-1] and np.any(np.isin(ps + k, ss[1:-1]))   # a k-mer ending on the last base, one ending on a step boundary
            assert case["haps"][1][2].size == 1                                 # the one-step haplotype
            if variant == "empty":
                d = np.diff(ss)
                assert d[0] == 0 and d[1] == 0 and d[-1] == 0 and d[-4] == 0 and d[-5] == 0 and d[-3] > 0 and np.any(d[10:-10] == 0)
            if variant.startswith("revisit"):
                # counting the vertices of the walk without looking back beyond the first eight distinct ones (what a count
                # kernel without its look-back branch would do) must disagree with the model where k allows nine vertices
                wrong = 0
                base_vtx = np.repeat(sv, np.diff(ss))
                for p in ps:
                    seen, extra = [], 0
                    for v in base_vtx[p:p + k]:
                        if v in seen[:8]:
                            continue
                        if len(seen) >= 8 and v in seen[8:]:
                            extra += 1
                        else:
                            seen.append(v)
                    wrong += extra > 0
                assert (wrong > 0) == (k > 8), (k, variant, wrong)
                early = sum(1 for p in ps if len(set(base_vtx[p:p + min(k, 8)].tolist())) < min(k, 8) and len(set(base_vtx[p:p + k].tolist())) > 2)
                assert early > 0
    assert {1, 2, 7, 8, 9, 10, 16, 5, 31, 40} <= lengths


@pytest.fixture(scope="module")
def big():
    return ac.big_top()


def numeric_order_model(occs, n_haps):
    """the ordering stage with the keys compared as numbers instead of strings (what a token_cmp without its string rules gives)"""
    out = []
    for r in sorted({o[0] for o in occs}):
        for h in range(n_haps):
            out += [(r, h, l) for l in sorted([l for i, hh, l in occs if i == r and hh == h], key=lambda l: (l[0], l[-1], l))]
    return out


def test_key_order_case_separates_string_from_number_order(big):
    case = ac.key_order_case(big)
    check_case_is_valid(case)
    res = model_of(case)
    assert res.unstable == [] and not res.dropped
    sizes = {}
    for r, h, l in res.occs:
        sizes[(r, h)] = sizes.get((r, h), 0) + 1
    assert max(sizes.values()) == 16 and min(s for s in sizes.values() if s > 1) == 2
    assert res.occs != numeric_order_model(res.occs, 2)
    used = {v for _, _, l in res.occs for v in l[1:-1]}
    assert {0, 9, 10, 11, 99, 100, 101, 999, 1000, ac.BIG_N - 1} <= used
    # front / back really are shared inside the groups that matter: some group holds different lists with equal (front, back)
    ties = {}
    for r, h, l in res.occs:
        ties.setdefault((r, h, l[0], l[-1]), set()).add(tuple(l))
    assert sum(len(s) > 1 for s in ties.values()) >= 40


@pytest.mark.parametrize("where", ["start", "middle", "end"])
def test_boundary_cases_sit_on_the_boundary(big, where):
    for size, tie, unstable in ((16, "different", False), (17, "different", True), (17, "identical", False), (17, "none", False)):
        case = ac.boundary_case(big, size, where, tie)
        check_case_is_valid(case)
        res = model_of(case)
        group = [l for r, h, l in res.occs if (r, h) == (1, 0)]
        assert len(group) == size and (res.unstable == [(1, 0)]) == unstable and (unstable or res.unstable == [])
        if tie != "none":
            at = [q for q in range(size - 1) if (group[q][0], group[q][-1]) == (group[q + 1][0], group[q + 1][-1])]
            assert at == [{"start": 0, "middle": (size - 1) // 2, "end": size - 2}[where]]


def test_boundary_case_5000(big):
    case = ac.boundary_case(big, 5000, "middle", "identical")
    res = model_of(case)
    assert res.unstable == [] and sum(1 for r, h, _ in res.occs if (r, h) == (1, 0)) == 5000


@pytest.mark.parametrize("n_haps,min_shared", ac.FILTER_SETTINGS)
def test_filter_cases_drop_what_they_say(n_haps, min_shared):
    case, must_drop = ac.filter_case(n_haps, min_shared)
    check_case_is_valid(case)
    res = model_of(case)
    assert res.dropped == must_drop
    assert (len(res.occs) == 0) == (n_haps == 1)                                  # 0.999 * 1: every id goes
    if n_haps > 1:
        assert 0 < len(must_drop) < case["sp_hash"].size
        # one step of float32 to either side of the bound changes the answer only where a run length equals it
        assert model_of(case, min_shared=np.float32(np.ceil(min_shared)) + np.float32(0.5)).dropped < must_drop


def test_join_and_large_cases():
    for n_sp in (0, 1, 2, 3, 255, 256, 257, 65536, 65537):
        case = ac.join_case(n_sp)
        check_case_is_valid(case)
        res = model_of(case, min_shared=ac.INF)
        assert case["haps"][1][0].size == 0
        if n_sp:
            ids = {r for r, _, _ in res.occs}
            assert {0, n_sp - 1} <= ids and res.n_candidates < sum(h[0].size for h in case["haps"])      # both ends hit, absent hashes skipped
        else:
            assert res.occs == []
    case = ac.large_case()
    check_case_is_valid(case)
    res = model_of(case)
    assert 28000 <= res.n_candidates <= 32000 and res.unstable == []
    assert 200 < len(res.dropped) < 1800 and len({r for r, _, _ in res.occs}) + len(res.dropped) == 2000
    assert res.occs != numeric_order_model(res.occs, 4)                           # the key order decides inside its groups too

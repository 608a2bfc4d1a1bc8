"""CPU: the model of the sharded-scoring device operations (tests/shard_ops_model.py) against its brute-force twins on
every case of tests/shard_ops_cases.py, and the cases against a list of wrong kernels: for each plausible mistake (a
signed compare, `<=` for `<`, the owner from the wrong half of the hash, a padding drop that eats a real entry, ...) at
least one case must tell the wrong variant from the model.  The variants live here, never in the product."""
import numpy as np
import pytest
import torch

import shard_ops_cases as cases
import shard_ops_model as model
from shard_ops_model import MAX64

PARTITION, JOIN, MERGE, HIST = cases.partition_cases(), cases.join_cases(), cases.merge_cases(), cases.histogram_cases()


def _signed(x):
    return x - (1 << 64) if x >= (1 << 63) else x


# ------------------------------------------------------------------ the case lists hold what they promise
def test_case_names_are_unique_and_generation_is_deterministic():
    for make in (cases.partition_cases, cases.join_cases, cases.merge_cases):
        a, b = make(), make()
        assert len({c.name for c in a}) == len(a)
        for x, y in zip(a, b):
            assert x.name == y.name and all(np.array_equal(v, getattr(y, k)) for k, v in vars(x).items() if k != "name")
    assert len({c.name for c in HIST}) == len(HIST)


def test_partition_cases_cover_the_issue():
    assert {c.world for c in PARTITION} == set(cases.PARTITION_WORLDS)
    for c in PARTITION:
        assert c.h.dtype == np.uint64 and np.all(c.h[1:] > c.h[:-1])
    for world in cases.PARTITION_WORLDS:
        mine = [c for c in PARTITION if c.world == world]
        assert {0, 1, 2, 1000} <= {c.h.size for c in mine}
        edge = set(int(x) for x in next(c for c in mine if c.name == f"w{world}_boundaries").h)
        assert set(cases.FIXED_HASHES) <= edge
        for r in {1, world // 2, world - 1} - {0, world}:
            b = cases.first_hash_of(r, world)
            assert {b, b - 1, b + 1} <= edge and ((b >> 32) * world) >> 32 == r and (((b - 1) >> 32) * world) >> 32 == r - 1
        assert any(len(set(int(o) for o in model.owner_of(c.h, world))) == 1 and c.h.size > 2 for c in mine)      # all in one range
        assert any(c.h.size and world > c.h.size for c in mine) or world == 1                                   # empty ranges
    assert max(c.world for c in PARTITION) + 1 > 64                                  # more than one block of 64 outputs


def test_join_cases_cover_the_issue():
    assert {(c.d.size, c.h.size, c.base) for c in JOIN} == {(a, b, e) for a in cases.JOIN_NDICT for b in cases.JOIN_N for e in cases.JOIN_BASES}
    seen = set()
    for c in JOIN:
        assert np.all(c.h[1:] > c.h[:-1]) and np.all(c.d[1:] >= c.d[:-1]) and np.all(c.counts0 != 0) and np.all(c.rank0 != 0)
        h, d = [int(x) for x in c.h], [int(x) for x in c.d]
        if not h:
            continue
        hs = set(h)
        seen |= {"below_first"} if any(x < h[0] for x in d) else set()
        seen |= {"above_last"} if any(x > h[-1] for x in d) else set()
        seen |= {"first"} if h[0] in d else set()
        seen |= {"last"} if h[-1] in d else set()
        seen |= {"between"} if any(h[0] < x < h[-1] and x not in hs for x in d) else set()
        seen |= {"hit_low_half", "hit_high_half"} if any(x in hs and x < cases.H63 for x in d) and any(x in hs and x >= cases.H63 for x in d) else set()
        seen |= {"key_0_hit"} if 0 in hs and 0 in d else set()
        seen |= {"key_0_miss"} if 0 not in hs and 0 in d else set()
        seen |= {"key_max_hit"} if MAX64 in hs and MAX64 in d else set()
        seen |= {"key_max_miss"} if MAX64 not in hs and MAX64 in d else set()
        seen |= {"twice_hit"} if any(d.count(x) > 1 for x in set(d) & hs) else set()
        seen |= {"twice_miss"} if any(d.count(x) > 1 for x in set(d) - hs) else set()
    assert seen == {"below_first", "above_last", "first", "last", "between", "hit_low_half", "hit_high_half", "key_0_hit", "key_0_miss",
                    "key_max_hit", "key_max_miss", "twice_hit", "twice_miss"}


def test_merge_cases_cover_the_issue():
    sizes = {c.h.size for c in MERGE}
    assert {0, 1, 2, 3, 1000} <= sizes and any(65000 <= n <= 75000 for n in sizes)
    for c in MERGE:
        assert c.h.size == c.c.size and c.c.dtype == np.int32
        assert int(np.abs(c.c.astype(np.int64)).sum()) < (1 << 31)                    # no sum can reach 2^31
    by = {c.name: c for c in MERGE}
    assert max(np.unique(by["one_hash_5000_times"].h, return_counts=True)[1]) >= 5000
    assert not np.all(np.diff(by["runs8_n70000"].h.astype(np.float64)) >= 0)          # unsorted overall
    pad = by["genuine_max_with_padding"]
    assert int(pad.c[pad.h == np.uint64(MAX64)].sum()) == 3 and int((pad.h == np.uint64(MAX64)).sum()) > 3
    assert np.all(by["only_padding_n64"].h == np.uint64(MAX64)) and not by["only_padding_n64"].c.any()
    per_hash = np.unique(by["runs8_n70000"].h, return_counts=True)[1]
    assert per_hash.min() == 1 and per_hash.max() == 8                               # every hash in 1 to 8 runs


def test_histogram_cases_cover_the_issue():
    assert {(c.hist0.size, c.c.size) for c in HIST} >= {(b, n) for b in cases.HIST_BINS for n in cases.HIST_N}
    allc = np.concatenate([c.c for c in HIST if c.c.size < 10000])
    for lo, hi in ((0, 7), (8, 4095), (4096, 4999), (1 << 20, cases.I32_MAX), (cases.I32_MIN, -1)):
        assert ((allc >= lo) & (allc <= hi)).any()
    assert all(np.all(c.hist0 != 0) for c in HIST)
    assert any(c.c.size >= 100000 and np.all(c.c == c.c[0]) for c in HIST)


# ------------------------------------------------------------------ the model equals its brute-force twin on every case
@pytest.mark.parametrize("c", PARTITION, ids=lambda c: c.name)
def test_partition_model_equals_brute_force(c):
    got = model.partition(c.h, c.world)
    assert got.dtype == np.int64 and got.tolist() == model.brute_partition(c.h, c.world)
    assert got[0] == 0 and got[-1] == c.h.size


@pytest.mark.parametrize("c", JOIN, ids=lambda c: c.name)
def test_join_models_equal_brute_force(c):
    counts, rank1 = c.counts0.copy(), c.rank0.copy()
    for _ in range(2):                                                               # twice into the same outputs: accumulation
        want_counts = model.brute_count_dictionary_into(c.d, c.h, c.c, counts)
        want_rank1 = model.brute_rank_dictionary(c.d, c.h, rank1, c.base)
        both_c, both_r = counts.copy(), rank1.copy()
        model.count_dictionary_into(c.d, c.h, c.c, counts)
        model.rank_dictionary(c.d, c.h, rank1, c.base)
        model.count_rank_dictionary_into(c.d, c.h, c.c, both_c, both_r, c.base)
        assert counts.tolist() == want_counts and rank1.tolist() == want_rank1
        assert np.array_equal(both_c, counts) and np.array_equal(both_r, rank1)
    assert counts.dtype == np.int32 and rank1.dtype == np.int64


@pytest.mark.parametrize("c", MERGE, ids=lambda c: c.name)
def test_merge_model_equals_brute_force(c):
    uh, uc = model.merge_runs(c.h, c.c)
    bh, bc = model.brute_merge_runs(c.h, c.c)
    assert uh.dtype == np.uint64 and uc.dtype == np.int32
    assert [int(x) for x in uh] == bh and uc.tolist() == bc


def test_merge_model_keeps_what_is_not_padding():
    by = {c.name: c for c in MERGE}
    for name in ("genuine_max_alone", "genuine_max_with_padding", "genuine_max_split_with_padding"):
        uh, uc = model.merge_runs(by[name].h, by[name].c)
        assert int(uh[-1]) == MAX64 and int(uc[-1]) == 3, name
    for name in ("only_padding_n1", "only_padding_n64"):
        assert model.merge_runs(by[name].h, by[name].c)[0].size == 0
    z = by["zero_total_on_largest_ordinary_hash"]
    uh, uc = model.merge_runs(z.h, z.c)
    assert int(uh[-1]) == int(z.h.max()) and int(uc[-1]) == 0 and int((uc == 0).sum()) >= 3
    p = by["padding_on_some_runs"]
    uh, uc = model.merge_runs(p.h, p.c)
    assert int(uh[-1]) == int(p.h[p.h != np.uint64(MAX64)].max()) and int(uc[-1]) == 0      # the padding goes, the zero count in front of it stays


@pytest.mark.parametrize("c", HIST, ids=lambda c: c.name)
def test_histogram_model_equals_brute_force(c):
    hist = c.hist0.copy()
    model.histogram(c.c, hist)
    assert hist.tolist() == model.brute_histogram(c.c, c.hist0)
    assert int(hist.sum() - c.hist0.sum()) == c.c.size


def test_cpu_ops_shim_is_the_model_on_tensors():
    """CpuOps, what the gloo tests inject into ShardedSketch, is the numpy layer and nothing else"""
    ops = model.CpuOps(None)

    def t64(a):
        return torch.from_numpy(a.view(np.int64).copy())
    for c in PARTITION:
        assert np.array_equal(ops.partition(t64(c.h), c.world).numpy(), model.partition(c.h, c.world)), c.name
    for c in JOIN:
        d, h, cnt = t64(c.d), t64(c.h), torch.from_numpy(c.c.copy())
        counts, rank1 = torch.from_numpy(c.counts0.copy()), torch.from_numpy(c.rank0.copy())
        want_c, want_r, zero = c.counts0.copy(), c.rank0.copy(), np.zeros(c.d.size, np.int32)
        ops.count_dictionary_into(d, h, cnt, counts)
        ops.rank_dictionary(d, h, rank1, c.base)
        model.count_rank_dictionary_into(c.d, c.h, c.c, want_c, want_r, c.base)
        model.count_dictionary_into(c.d, c.h, c.c, zero)
        assert np.array_equal(counts.numpy(), want_c) and np.array_equal(rank1.numpy(), want_r), c.name
        assert np.array_equal(ops.count_dictionary(d, h, cnt).numpy(), zero), c.name
    for c in MERGE:
        rh, rc = ops.merge_runs(t64(c.h), torch.from_numpy(c.c.copy()))
        uh, uc = model.merge_runs(c.h, c.c)
        assert np.array_equal(rh.numpy().view(np.uint64), uh) and np.array_equal(rc.numpy(), uc), c.name
    for c in HIST:
        hist, want = torch.from_numpy(c.hist0.copy()), c.hist0.copy()
        ops.histogram(torch.from_numpy(c.c.copy()), hist)
        model.histogram(c.c, want)
        assert np.array_equal(hist.numpy(), want), c.name


# ------------------------------------------------------------------ wrong variants: every one must be caught by a case
def _search(h, key, less):
    lo, hi = 0, len(h)
    while lo < hi:
        mid = (lo + hi) >> 1
        if less(h[mid], key):
            lo = mid + 1
        else:
            hi = mid
    return lo


def _join_variant(c, which, less=lambda a, b: a < b, assign=False, use_base=True):
    """the three join kernels as written (binary search, hit test, update) with one thing wrong; which: count / rank / both"""
    h, cnt = [int(x) for x in c.h], c.c.tolist()
    counts, rank1 = c.counts0.tolist(), c.rank0.tolist()
    for i, key in enumerate(int(x) for x in c.d):
        lo = _search(h, key, less)
        if lo < len(h) and h[lo] == key:
            if which in ("count", "both"):
                counts[i] = cnt[lo] if assign else counts[i] + cnt[lo]
            if which in ("rank", "both"):
                add = (c.base if use_base else 0) + lo + 1
                rank1[i] = add if assign else rank1[i] + add
    return counts, rank1


def _join_model(c, which):
    counts, rank1 = c.counts0.copy(), c.rank0.copy()
    if which in ("count", "both"):
        model.count_dictionary_into(c.d, c.h, c.c, counts)
    if which in ("rank", "both"):
        model.rank_dictionary(c.d, c.h, rank1, c.base)
    return counts.tolist(), rank1.tolist()


def test_join_variant_harness_is_the_model_when_nothing_is_wrong():
    for c in JOIN:
        for which in ("count", "rank", "both"):
            assert _join_variant(c, which) == _join_model(c, which), c.name


JOIN_VARIANTS = {
    "signed key compare": dict(less=lambda a, b: _signed(a) < _signed(b)),
    "<= for < in the search": dict(less=lambda a, b: a <= b),
    "= instead of +=": dict(assign=True),
    "base ignored": dict(use_base=False),
}


@pytest.mark.parametrize("variant,which", [(v, k) for v in sorted(JOIN_VARIANTS) for k in ("count", "rank", "both")
                                           if (v, k) != ("base ignored", "count")])        # (the count kernel takes no base)
def test_join_cases_catch(variant, which):
    caught = [c.name for c in JOIN if _join_variant(c, which, **JOIN_VARIANTS[variant]) != _join_model(c, which)]
    assert caught, f"no join case tells `{variant}` in the {which} kernel from the model"


def _partition_variant(c, owner):
    h = [int(x) for x in c.h]
    return [_search(h, r, lambda x, r: owner(x, c.world) < r) for r in range(c.world + 1)]


PARTITION_VARIANTS = {
    "owner from lo32": lambda x, world: ((x & 0xFFFFFFFF) * world) >> 32,
    "owner with a signed shift": lambda x, world: ((_signed(x) >> 32) * world) >> 32,
    "<= for < in the search": None,
}


def test_partition_variant_harness_is_the_model_when_nothing_is_wrong():
    for c in PARTITION:
        assert _partition_variant(c, lambda x, world: ((x >> 32) * world) >> 32) == model.partition(c.h, c.world).tolist(), c.name


@pytest.mark.parametrize("variant", sorted(PARTITION_VARIANTS))
def test_partition_cases_catch(variant):
    def run(c):
        if variant == "<= for < in the search":
            h = [int(x) for x in c.h]
            return [_search(h, r, lambda x, r: ((x >> 32) * c.world) >> 32 <= r) for r in range(c.world + 1)]
        return _partition_variant(c, PARTITION_VARIANTS[variant])
    caught = [c.name for c in PARTITION if run(c) != model.partition(c.h, c.world).tolist()]
    assert caught, f"no partition case tells `{variant}` from the model"
    assert {c.world for c in PARTITION if c.name in caught} >= set(cases.PARTITION_WORLDS) - {1}      # (world 1 has one owner whatever the half)


def _merge_variant(c, drop):
    pairs = sorted(zip([int(x) for x in c.h], c.c.tolist()), key=lambda p: p[0])
    out = []
    for x, n in pairs:
        if out and out[-1][0] == x:
            out[-1][1] += n
        else:
            out.append([x, n])
    if out and drop(out):
        out.pop()
    return [p[0] for p in out], [p[1] for p in out]


MERGE_VARIANTS = {
    "padding drop applied to any zero-count tail": lambda out: out[-1][1] == 0,
    "padding drop that ignores the count": lambda out: out[-1][0] == MAX64,
    "no padding drop": lambda out: False,
    "every zero count dropped": None,
}


def test_merge_variant_harness_is_the_model_when_nothing_is_wrong():
    for c in MERGE:
        uh, uc = model.merge_runs(c.h, c.c)
        assert _merge_variant(c, lambda out: out[-1][0] == MAX64 and out[-1][1] == 0) == ([int(x) for x in uh], uc.tolist()), c.name


@pytest.mark.parametrize("variant", sorted(MERGE_VARIANTS))
def test_merge_cases_catch(variant):
    def run(c):
        if variant == "every zero count dropped":
            h, v = _merge_variant(c, lambda out: False)
            keep = [i for i in range(len(h)) if v[i] != 0]
            return [h[i] for i in keep], [v[i] for i in keep]
        return _merge_variant(c, MERGE_VARIANTS[variant])
    caught = []
    for c in MERGE:
        uh, uc = model.merge_runs(c.h, c.c)
        if run(c) != ([int(x) for x in uh], uc.tolist()):
            caught.append(c.name)
    assert caught, f"no merge case tells `{variant}` from the model"


def _hist_variant(c, clamp):
    out = np.append(c.hist0, np.int64(0))                                            # one word behind the last bin: where a clamp at n_bins lands
    n_bins = c.hist0.size
    idx = clamp(c.c.astype(np.int64), n_bins)
    idx = np.where(idx < 0, n_bins, idx)                                             # (out of bounds below: anywhere but a bin of the model)
    out += np.bincount(idx, minlength=n_bins + 1)
    return out[:n_bins].tolist()


HIST_VARIANTS = {
    "clamp at n_bins instead of n_bins - 1": lambda c, n_bins: np.clip(c, 0, n_bins),
    "no negative clamp": lambda c, n_bins: np.minimum(c, n_bins - 1),
    "clamp one bin early": lambda c, n_bins: np.clip(c, 0, n_bins - 2),
    "counts of 4096 and more all into the last bin": lambda c, n_bins: np.where(c >= 4096, n_bins - 1, np.clip(c, 0, n_bins - 1)),
}


def test_histogram_variant_harness_is_the_model_when_nothing_is_wrong():
    for c in HIST:
        hist = c.hist0.copy()
        model.histogram(c.c, hist)
        assert _hist_variant(c, lambda v, n_bins: np.clip(v, 0, n_bins - 1)) == hist.tolist(), c.name


@pytest.mark.parametrize("variant", sorted(HIST_VARIANTS))
def test_histogram_cases_catch(variant):
    caught = []
    for c in HIST:
        hist = c.hist0.copy()
        model.histogram(c.c, hist)
        if _hist_variant(c, HIST_VARIANTS[variant]) != hist.tolist():
            caught.append(c.name)
    assert caught, f"no histogram case tells `{variant}` from the model"
    if variant == "clamp at n_bins instead of n_bins - 1":
        assert {c.hist0.size for c in HIST if c.name in caught} == set(cases.HIST_BINS)       # the off-by-one shows at every n_bins


def test_histogram_not_accumulating_is_caught():
    """`=` for `+=` on the histogram words: every case presets hist to non-zero"""
    for c in HIST:
        hist = c.hist0.copy()
        model.histogram(c.c, hist)
        assert not np.array_equal(hist - c.hist0, hist)

"""Named, seeded inputs for the device operations of the read-sharded scoring path -- TEST INFRASTRUCTURE.

Every generator returns a list of SimpleNamespace cases with a unique `name`; the arrays of a case are a function of its
name alone.  tests/test_shard_ops_cases.py checks the model (tests/shard_ops_model.py) on them and that they tell a list
of wrong variants from the model; tests/test_gpu_shard_ops.py runs them through the kernels.  Hashes are uint64 arrays
(the tests reinterpret them as int64 tensors, as the device path holds them), counts int32."""
import zlib
from types import SimpleNamespace as Case

import numpy as np

from shard_ops_model import MAX64

H63 = 1 << 63
FIXED_HASHES = (0, H63 - 1, H63, MAX64)
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _u64(values):
    return np.array(sorted(set(int(v) for v in values)), dtype=np.uint64)


def _random_hashes(rng, n, lo=0, hi=MAX64):
    return rng.integers(lo, hi, n, dtype=np.uint64, endpoint=True)


# ------------------------------------------------------------------ partition
PARTITION_WORLDS = (1, 2, 3, 5, 7, 8, 63, 64, 65, 4096)


def first_hash_of(r, world):
    """the smallest hash owned by range r: ceil(r * 2^32 / world) << 32 (2^64 for r = world)"""
    return (-(-(r << 32) // world)) << 32


def _boundary_ranges(world):
    rng = _rng("partition ranges", world)
    rs = {0, 1, world // 2, world - 2, world - 1, 62, 63, 64, 65, 127, 128, 4031, 4032} | set(int(x) for x in rng.integers(0, world, 6))
    return sorted(r for r in rs if 0 <= r < world)


def partition_cases():
    cases = [Case(name="fixed_hashes_w3", world=3, h=_u64(FIXED_HASHES))]
    for world in PARTITION_WORLDS:
        rng = _rng("partition", world)
        edge = list(FIXED_HASHES)
        for r in _boundary_ranges(world):
            b = first_hash_of(r, world)
            edge += [b, b + 1, b + 0x7FFFFFFF, b + 0x80000000, b + 0xFFFFFFFF]        # the first hi32 of range r, differing lo32
            if b:
                edge += [b - 1, b - 0x80000000, b - (1 << 32)]                         # the last hi32 of range r - 1, differing lo32
        cases.append(Case(name=f"w{world}_boundaries", world=world, h=_u64(edge)))
        r = world // 2
        cases.append(Case(name=f"w{world}_one_range", world=world,
                          h=_u64(_random_hashes(rng, 40, first_hash_of(r, world), first_hash_of(r + 1, world) - 1))))
        uni = _random_hashes(rng, 1003)
        for n in (0, 1, 2, 1000):
            cases.append(Case(name=f"w{world}_uniform_n{n}", world=world, h=_u64(uni[:n])))
        cases.append(Case(name=f"w{world}_last_hash_only", world=world, h=_u64([MAX64])))
    return cases


# ------------------------------------------------------------------ dictionary joins
JOIN_NDICT = (0, 1, 255, 256, 257, 1000)
JOIN_N = (0, 1, 2, 1000)
JOIN_BASES = (0, 7, 1 << 40)


def _join_list(flavour, n, rng):
    """the sorted distinct list the kernels search: `inner` keeps clear of 0 and 2^64 - 1 (so that keys exist below the
    first and above the last entry) and straddles 2^63; `edge` has 0 and 2^64 - 1 as its first and last entry"""
    if flavour == "inner":
        must = {0: [], 1: [H63 + 11], 2: [H63 - 7, H63 + 11]}.get(n, [H63 - 7, H63 - 1, H63, H63 + 11, 1 << 20, MAX64 - (1 << 20)])
    else:
        must = {0: [], 1: [MAX64], 2: [0, MAX64]}.get(n, [0, 1, H63 - 1, H63, MAX64 - 1, MAX64])
    vals = set(must)
    while len(vals) < n:
        vals |= set(int(x) for x in _random_hashes(rng, n - len(vals), (1 << 20) + 1, MAX64 - (1 << 20) - 1))
    return _u64(vals)


def _join_keys(h, n_dict, rng):
    """sorted dictionary of n_dict keys (duplicates allowed): the edges first, the rest hits and misses half and half"""
    hs = [int(x) for x in h]
    must = [0, MAX64, H63 - 1, H63]
    if hs:
        must += [hs[0], hs[-1], hs[len(hs) // 2]]
        must += [hs[0] - 1] if hs[0] > 0 else []
        must += [hs[-1] + 1] if hs[-1] < MAX64 else []
        for i in sorted(set(int(x) for x in rng.integers(0, len(hs), 4))):
            if i + 1 < len(hs) and hs[i] + 1 < hs[i + 1]:
                must.append(hs[i] + 1)                                               # strictly between neighbours
        must += [hs[len(hs) // 2], hs[0] - 1 if hs[0] > 0 else 5, H63]                  # the same key twice: a hit and misses
    if n_dict <= len(must):
        keys = [must[int(i)] for i in rng.permutation(len(must))[:n_dict]]
    else:
        rest = n_dict - len(must)
        hits = [hs[int(i)] for i in rng.integers(0, len(hs), rest // 2)] if hs else []
        keys = must + hits + [int(x) for x in _random_hashes(rng, rest - len(hits))]
    return np.array(sorted(keys), dtype=np.uint64)


def join_cases():
    cases = []
    for flavour in ("inner", "edge"):
        for n in JOIN_N:
            for n_dict in JOIN_NDICT:
                for base in JOIN_BASES:
                    name = f"{flavour}_ndict{n_dict}_n{n}_base{base}"
                    rng = _rng("join", name)
                    h = _join_list(flavour, n, rng)
                    c = rng.integers(1, 1001, n).astype(np.int32)
                    c[rng.random(n) < 0.1] = 0
                    d = _join_keys(h, n_dict, rng)
                    cases.append(Case(name=name, d=d, h=h, c=c, base=base,
                                      counts0=(1000 + rng.integers(1, 977, n_dict)).astype(np.int32),      # sentinels: never 0
                                      rank0=(10 ** 12 + 3 * np.arange(n_dict, dtype=np.int64) + 1)))
    return cases


# ------------------------------------------------------------------ merge
def _sorted_runs(rng, pool, n_runs, zero_total=()):
    """every hash of `pool` into 1..min(8, n_runs) of n_runs sorted runs; counts 0..1000 (a tenth of them 0; every count
    of a hash in `zero_total` 0).  Returns a list of (hash uint64 [], count int32 []) runs"""
    pool = np.asarray(pool, np.uint64)
    k = rng.integers(1, min(8, n_runs) + 1, pool.size)
    member = np.argsort(np.argsort(rng.random((pool.size, n_runs)), axis=1), axis=1) < k[:, None]
    runs = []
    for r in range(n_runs):
        h = np.sort(pool[member[:, r]])
        c = rng.integers(1, 1001, h.size).astype(np.int32)
        c[rng.random(h.size) < 0.1] = 0
        c[np.isin(h, np.asarray(zero_total, np.uint64))] = 0
        runs.append((h, c))
    return runs


def _padded(run, n_pad):
    return (np.concatenate([run[0], np.full(n_pad, MAX64, np.uint64)]), np.concatenate([run[1], np.zeros(n_pad, np.int32)]))


def _merge_case(name, runs, n=None):
    h = np.concatenate([r[0] for r in runs]) if runs else np.zeros(0, np.uint64)
    c = np.concatenate([r[1] for r in runs]) if runs else np.zeros(0, np.int32)
    if n is not None:
        assert h.size >= n, name
        h, c = h[:n], c[:n]                                                         # (the cut shortens the last runs: still sorted runs)
    return Case(name=name, h=h.astype(np.uint64), c=c.astype(np.int32))


def _one(hashes, counts):
    return (np.array(hashes, np.uint64), np.array(counts, np.int32))


def merge_cases():
    cases = [
        _merge_case("n0", []),
        _merge_case("n1", [_one([H63 + 5], [9])]),
        _merge_case("n1_zero_count", [_one([77], [0])]),
        _merge_case("n2_same_hash", [_one([H63 - 1], [4]), _one([H63 - 1], [6])]),
        _merge_case("n2_descending", [_one([H63], [4]), _one([H63 - 1], [6])]),
        _merge_case("n3_small", small_merge_after_large()),
        _merge_case("only_padding_n1", [_one([MAX64], [0])]),
        _merge_case("only_padding_n64", [_padded(_one([], []), 40), _padded(_one([], []), 24)]),
        _merge_case("genuine_max_alone", [_one([MAX64], [3])]),
        _merge_case("genuine_max_split_with_padding", [_padded(_one([5, H63], [1, 2]), 3), _one([9, MAX64], [4, 3]), _padded(_one([], []), 2)]),
        _merge_case("zero_count_hash_zero", [_one([0, 8], [0, 1]), _one([0, 9], [0, 2])]),
    ]
    for n_runs in (2, 3, 5, 8):
        rng = _rng("merge runs1000", n_runs)
        pool = _random_hashes(rng, int(2600 / (min(8, n_runs) + 1)))                   # about 1,170 entries before the cut to 1,000
        cases.append(_merge_case(f"runs{n_runs}_n1000", _sorted_runs(rng, pool, n_runs), n=1000))
    rng = _rng("merge zero tail")
    pool = np.unique(_random_hashes(rng, 120, 0, MAX64 - 1))
    cases.append(_merge_case("zero_total_on_largest_ordinary_hash", _sorted_runs(rng, pool, 4, zero_total=[pool[-1], pool[3], pool[50]])))
    runs = _sorted_runs(rng, pool, 5, zero_total=[pool[-1], pool[7]])
    cases.append(_merge_case("padding_on_some_runs", [_padded(runs[0], 1), runs[1], _padded(runs[2], 37), runs[3], _padded(runs[4], 200)]))
    runs = _sorted_runs(rng, pool, 3)
    runs[1] = (np.append(runs[1][0], np.uint64(MAX64)), np.append(runs[1][1], np.int32(3)))
    cases.append(_merge_case("genuine_max_with_padding", [_padded(runs[0], 17), runs[1], _padded(runs[2], 5)]))
    rng = _rng("merge repeat5000")
    pool = np.unique(_random_hashes(rng, 200))
    runs = _sorted_runs(rng, pool, 4)
    hot = np.uint64(pool[120])
    for r, m in enumerate((1250, 1, 2500, 1249)):                                       # 5,000 more entries of one hash, kept in sorted position
        h = np.concatenate([runs[r][0], np.full(m, hot, np.uint64)])
        c = np.concatenate([runs[r][1], rng.integers(0, 1001, m).astype(np.int32)])
        order = np.argsort(h, kind="stable")
        runs[r] = (h[order], c[order])
    cases.append(_merge_case("one_hash_5000_times", runs))
    cases.append(large_merge_case())
    return cases


def large_merge_case():
    """about 70,000 entries in 8 sorted runs: several blocks of the radix sort and of the reduce-by-key"""
    rng = _rng("merge runs70000")
    pool = np.unique(_random_hashes(rng, 15600))
    return _merge_case("runs8_n70000", _sorted_runs(rng, pool, 8))


def small_merge_after_large():
    """the 3 entries merged right after large_merge_case() on the same context (stale scratch buffers)"""
    return [_one([H63 + 1, MAX64 - 1], [2, 0]), _one([H63 + 1], [5])]


# ------------------------------------------------------------------ histogram
HIST_BINS = (2, 8, 9, 4096, 4097, 5000)
HIST_N = (1, 63, 64, 65, 255, 256, 257, 8192, 8193, 256 * 8192 + 1)
_HIST_REGIMES = ((0, 7), (8, 4095), (4096, 4999), (5000, I32_MAX), (I32_MIN, -1))


def _hist_counts(rng, n, n_bins):
    regime = rng.choice(5, n, p=(0.40, 0.30, 0.15, 0.13, 0.02))
    c = np.zeros(n, np.int64)
    for q, (lo, hi) in enumerate(_HIST_REGIMES):
        c = np.where(regime == q, rng.integers(lo, hi, n, endpoint=True), c)
    edges = np.array([0, 7, 8, 4095, 4096, 4999, 5000, n_bins - 2, n_bins - 1, n_bins, n_bins + 1, -1, I32_MIN, I32_MAX])
    if n >= 63:
        c[rng.choice(n, edges.size, replace=False)] = edges
    else:                                                                              # (n = 1: one edge value, another for every n_bins)
        c[:] = edges[(np.arange(n) + HIST_BINS.index(n_bins) + 7) % edges.size]
    return c.astype(np.int32)


def _hist0(rng, n_bins):
    return rng.integers(1, 1 << 40, n_bins).astype(np.int64)                          # preset, never 0


def histogram_cases():
    cases = []
    for n_bins in HIST_BINS:
        for n in HIST_N:
            rng = _rng("hist", n_bins, n)
            cases.append(Case(name=f"bins{n_bins}_n{n}", c=_hist_counts(rng, n, n_bins), hist0=_hist0(rng, n_bins)))
    for n_bins, v in ((4096, 3), (4096, 100), (5000, 4500), (4096, 1 << 20)):               # every lane on one bin: register, LDS, global, clamped
        cases.append(Case(name=f"bins{n_bins}_100000_times_{v}", c=np.full(100000, v, np.int32), hist0=_hist0(_rng("hist eq", n_bins, v), n_bins)))
    return cases

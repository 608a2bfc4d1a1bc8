"""The one yardstick for the device operations of the read-sharded scoring path (dg_sketch.hip: dg_sketch_partition_dev,
dg_sketch_merge_runs_dev, dg_sketch_count_dictionary_dev, dg_sketch_rank_dictionary_dev,
dg_sketch_count_rank_dictionary_dev, dg_sketch_histogram_dev) -- TEST INFRASTRUCTURE.

Three layers, all on the CPU:
  * the contract of every entry point as a numpy function on uint64 hashes (`partition`, `merge_runs`,
    `count_dictionary_into`, `rank_dictionary`, `count_rank_dictionary_into`, `histogram`);
  * beside each a brute-force twin in plain Python integers and loops (`brute_*`: no searchsorted, unique or reduceat),
    against which tests/test_shard_ops_cases.py checks the numpy layer;
  * `CpuOps`, the shim with HipOps' methods on CPU tensors that tests/test_dist_gloo.py injects into ShardedSketch; its
    methods are the numpy layer on tensors.
tests/test_gpu_shard_ops.py compares the kernels with the numpy layer on the cases of tests/shard_ops_cases.py."""
import numpy as np
import torch

MAX64 = (1 << 64) - 1            # the hash of the fixed-size exchange's padding entries (count 0)


# ------------------------------------------------------------------ the contracts, numpy
def owner_of(h, world):
    """owner range of uint64 hashes: floor(hi32 * world / 2^32), unsigned throughout (dg_sketch.hip: hash_owner)"""
    h = np.asarray(h, np.uint64)
    return ((h >> np.uint64(32)) * np.uint64(world)) >> np.uint64(32)


def partition(h, world):
    """h: sorted uint64 [n].  int64 [world + 1]: split[r] = first index whose owner is >= r; split[world] = n"""
    return np.searchsorted(owner_of(h, world), np.arange(world + 1, dtype=np.uint64), side="left").astype(np.int64)


def merge_runs(h, c):
    """h uint64 [n], c int32 [n], any order: stable sort by hash, one entry per distinct hash with the sum of its counts.
    After the reduction exactly one trailing (2^64 - 1, 0) entry -- what the padding of the fixed-size exchange collapses
    into -- is dropped and nothing else: zero counts on other hashes stay, and 2^64 - 1 with a non-zero sum stays."""
    h, c = np.asarray(h, np.uint64), np.asarray(c, np.int32)
    if h.size == 0:
        return h[:0].copy(), c[:0].copy()
    order = np.argsort(h, kind="stable")
    hh, cc = h[order], c[order]
    uh, idx = np.unique(hh, return_index=True)
    uc = np.add.reduceat(cc, idx).astype(np.int32)
    if uh[-1] == np.uint64(MAX64) and uc[-1] == 0:
        uh, uc = uh[:-1], uc[:-1]
    return uh.copy(), uc.copy()


def _lookup(d, h):
    """for every key of d: (found in the sorted list h, index of its first occurrence)"""
    d, h = np.asarray(d, np.uint64), np.asarray(h, np.uint64)
    if h.size == 0:
        return np.zeros(d.size, bool), np.zeros(d.size, np.int64)
    pos = np.searchsorted(h, d, side="left")
    hit = (pos < h.size) & (h[np.minimum(pos, h.size - 1)] == d)
    return hit, pos.astype(np.int64)


def count_dictionary_into(d, h, c, out):
    """out[i] += c[idx] where d[i] == h[idx] (h sorted); a miss leaves out[i] as it was"""
    hit, pos = _lookup(d, h)
    out[hit] += np.asarray(c, np.int32)[pos[hit]]


def rank_dictionary(d, h, rank1, base=0):
    """rank1[i] += base + idx + 1 where d[i] == h[idx] (h sorted); a miss leaves rank1[i] as it was"""
    hit, pos = _lookup(d, h)
    rank1[hit] += np.int64(base) + pos[hit] + 1


def count_rank_dictionary_into(d, h, c, out, rank1, base=0):
    """the pair of the two above against the same list"""
    count_dictionary_into(d, h, c, out)
    rank_dictionary(d, h, rank1, base)


def histogram(c, hist):
    """hist[min(max(c, 0), n_bins - 1)] += 1 per entry; n_bins = hist.size.  The clamp at 0 is the guard of
    mult_hist_kernel: a negative count lands in bin 0"""
    n_bins = hist.size
    hist += np.bincount(np.clip(np.asarray(c, np.int64), 0, n_bins - 1), minlength=n_bins).astype(hist.dtype)


# ------------------------------------------------------------------ the same, plain Python integers and loops
def _ints(a):
    return [int(x) for x in np.asarray(a).tolist()]


def brute_partition(h, world):
    owners = [((x >> 32) * world) >> 32 for x in _ints(h)]
    split = []
    for r in range(world + 1):
        first = len(owners)
        for i, o in enumerate(owners):
            if o >= r:
                first = i
                break
        split.append(first)
    return split


def brute_merge_runs(h, c):
    pairs = sorted(zip(_ints(h), _ints(c)), key=lambda p: p[0])          # (sorted() is stable)
    out = []
    for x, v in pairs:
        if out and out[-1][0] == x:
            out[-1][1] += v
        else:
            out.append([x, v])
    if out and out[-1][0] == MAX64 and out[-1][1] == 0:
        out.pop()
    return [p[0] for p in out], [p[1] for p in out]


def _brute_find(h, key):
    for i, x in enumerate(h):
        if x == key:
            return i
    return -1


def brute_count_dictionary_into(d, h, c, out):
    h, c, out = _ints(h), _ints(c), _ints(out)
    for i, key in enumerate(_ints(d)):
        j = _brute_find(h, key)
        if j >= 0:
            out[i] += c[j]
    return out


def brute_rank_dictionary(d, h, rank1, base=0):
    h, rank1 = _ints(h), _ints(rank1)
    for i, key in enumerate(_ints(d)):
        j = _brute_find(h, key)
        if j >= 0:
            rank1[i] += base + j + 1
    return rank1


def brute_histogram(c, hist):
    out = _ints(hist)
    last = len(out) - 1
    for v in np.asarray(c).tolist():
        if v < 0:
            v = 0
        if v > last:
            v = last
        out[v] += 1
    return out


# ------------------------------------------------------------------ the shim of the gloo tests
class CpuOps:
    """test shim for dist_sketch.HipOps: same methods, CPU tensors (uint64 hashes held as int64, like the device path).
    (No count_rank_dictionary method on purpose: ShardedSketch takes its one-pass path where the ops object has one, and
    the gloo tests pin the two-call path; the pair's contract is count_rank_dictionary_into above.)"""
    stream = None

    def __init__(self, orc):
        self.orc = orc

    @staticmethod
    def _u(t):
        return t.numpy().view(np.uint64)

    def sketch_reads(self, bases_t, off_t, k, w):
        b, off = bases_t.numpy().tobytes(), off_t.numpy()
        reads = [b[off[i]:off[i + 1]] for i in range(off.size - 1)]
        h, c = self.orc.sketch_reads(reads, k, w)
        return torch.from_numpy(h.view(np.int64).copy()), torch.from_numpy(c.copy())

    def count_dictionary(self, dict_t, h, c):
        out = torch.zeros(dict_t.numel(), dtype=torch.int32)
        self.count_dictionary_into(dict_t, h, c, out)
        return out

    def count_dictionary_into(self, dict_t, h, c, out):
        count_dictionary_into(self._u(dict_t), self._u(h), c.numpy(), out.numpy())

    def partition(self, h, world):
        return torch.from_numpy(partition(self._u(h), world))

    def merge_runs(self, h, c):
        if h.numel() == 0:
            return h[:0], c[:0]
        uh, uc = merge_runs(self._u(h), c.numpy())
        return torch.from_numpy(uh.view(np.int64).copy()), torch.from_numpy(uc.copy())

    def rank_dictionary(self, dict_t, h, rank1, base=0):
        rank_dictionary(self._u(dict_t), self._u(h), rank1.numpy(), base)

    def histogram(self, c, hist):
        histogram(c.numpy(), hist.numpy())

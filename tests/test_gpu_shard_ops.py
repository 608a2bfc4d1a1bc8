"""GPU (-m gpu): the six device entry points of the read-sharded scoring path (dg_sketch.hip: partition, merge_runs,
count / rank / count_rank dictionary, histogram) against their model (tests/shard_ops_model.py) on the named cases of
tests/shard_ops_cases.py -- whole outputs, the words behind them, n_out, and the inputs after the call -- their refusals,
and a small emulated exchange (worlds 2, 3 and 5 on one context, exact runs and the padded fixed-size blocks of
ShardedSketch) against the oracle on the whole read set.  Every comparison is exact."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import oracle_py as orc
import shard_ops_cases as cases
import shard_ops_model as model
from dipgenie_amd import capi
from dipgenie_amd.dist_sketch import HIST_BINS, HipOps, shard_bounds

pytestmark = pytest.mark.gpu
lib = capi.lib
GUARD = 8                        # words behind every output, preset like the output itself: nothing may touch them
DG_ERR_ARG = -1


@pytest.fixture(scope="module")
def shard():
    ctx = capi.Context(0)
    dev = torch.device("cuda", 0)
    yield SimpleNamespace(ctx=ctx, dev=dev, ops=HipOps(ctx, dev))
    torch.cuda.synchronize()
    ctx.close()


@pytest.fixture(autouse=True)
def on_ops_stream(shard):
    """every call of a test inside `with torch.cuda.stream(ops.stream)`: uploads and library kernels share one stream"""
    with torch.cuda.stream(shard.ops.stream):
        yield
    torch.cuda.synchronize()


def _hashes(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64).copy()).to(dev)


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to(dev)


def _guarded(a, dev, fill):
    """a device copy of `a` with GUARD more words of `fill` behind it"""
    return _dev(np.concatenate([a, np.full(GUARD, fill, a.dtype)]), dev)


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


# ------------------------------------------------------------------ partition
@pytest.mark.parametrize("c", cases.partition_cases(), ids=lambda c: c.name)
def test_partition(shard, c):
    dev, n, world = shard.dev, c.h.size, c.world
    want = model.partition(c.h, world)
    h = _hashes(c.h, dev)
    split = _guarded(np.full(world + 1, -7, np.int64), dev, -7)
    capi._check(lib.dg_sketch_partition_dev(shard.ctx.h, h.data_ptr(), n, world, split.data_ptr()), "dg_sketch_partition_dev")
    through_ops = shard.ops.partition(h, world)
    torch.cuda.synchronize()
    got = split.cpu().numpy()
    assert np.array_equal(got[: world + 1], want) and np.all(got[world + 1:] == -7)
    assert np.array_equal(through_ops.cpu().numpy(), want)
    assert np.array_equal(_u64(h), c.h)


# ------------------------------------------------------------------ dictionary joins
@pytest.mark.parametrize("c", cases.join_cases(), ids=lambda c: c.name)
def test_dictionary_joins(shard, c):
    dev, hd = shard.dev, shard.ctx.h
    nd, n = c.d.size, c.h.size
    d, h, cnt = _hashes(c.d, dev), _hashes(c.h, dev), _dev(c.c, dev)
    counts, rank1 = _guarded(c.counts0, dev, -3), _guarded(c.rank0, dev, -5)          # the two single kernels
    counts2, rank2 = _guarded(c.counts0, dev, -3), _guarded(c.rank0, dev, -5)        # the fused kernel
    want_counts, want_rank1 = c.counts0.copy(), c.rank0.copy()
    for _ in range(2):                                                               # the same call twice into the same outputs
        capi._check(lib.dg_sketch_count_dictionary_dev(hd, d.data_ptr(), nd, h.data_ptr(), cnt.data_ptr(), n, counts.data_ptr()), "dg_sketch_count_dictionary_dev")
        capi._check(lib.dg_sketch_rank_dictionary_dev(hd, d.data_ptr(), nd, h.data_ptr(), n, c.base, rank1.data_ptr()), "dg_sketch_rank_dictionary_dev")
        capi._check(lib.dg_sketch_count_rank_dictionary_dev(hd, d.data_ptr(), nd, h.data_ptr(), cnt.data_ptr(), n, c.base, counts2.data_ptr(), rank2.data_ptr()),
                    "dg_sketch_count_rank_dictionary_dev")
        model.count_dictionary_into(c.d, c.h, c.c, want_counts)
        model.rank_dictionary(c.d, c.h, want_rank1, c.base)
    torch.cuda.synchronize()
    got_c, got_r, got_c2, got_r2 = (t.cpu().numpy() for t in (counts, rank1, counts2, rank2))
    assert np.array_equal(got_c[:nd], want_counts) and np.all(got_c[nd:] == -3)
    assert np.array_equal(got_r[:nd], want_rank1) and np.all(got_r[nd:] == -5)
    assert np.array_equal(got_c2, got_c) and np.array_equal(got_r2, got_r)           # count_rank == count + rank
    hit = np.isin(c.d, c.h)
    assert np.array_equal(got_c[:nd][~hit], c.counts0[~hit]) and np.array_equal(got_r[:nd][~hit], c.rank0[~hit])   # misses: untouched
    assert np.array_equal(_u64(d), c.d) and np.array_equal(_u64(h), c.h) and np.array_equal(cnt.cpu().numpy(), c.c)
    if c.base == 0:                                                                  # what HipOps exposes: base 0, counts from zero
        zc, zr = np.zeros(nd, np.int32), np.zeros(nd, np.int64)
        model.count_rank_dictionary_into(c.d, c.h, c.c, zc, zr)
        r_a, r_b = torch.zeros(nd, dtype=torch.int64, device=dev), torch.zeros(nd, dtype=torch.int64, device=dev)
        c_a = shard.ops.count_dictionary(d, h, cnt)
        shard.ops.rank_dictionary(d, h, r_a)
        c_b = shard.ops.count_rank_dictionary(d, h, cnt, r_b)
        torch.cuda.synchronize()
        assert np.array_equal(c_a.cpu().numpy(), zc) and np.array_equal(c_b.cpu().numpy(), zc)
        assert np.array_equal(r_a.cpu().numpy(), zr) and np.array_equal(r_b.cpu().numpy(), zr)


# ------------------------------------------------------------------ merge
def _merge(shard, h, cnt, n, cap, fill_h=-11, fill_c=-13):
    """dg_sketch_merge_runs_dev into buffers of cap + GUARD preset words; returns (rc, n_out, out_hash int64, out_count)"""
    oh = _dev(np.full(cap + GUARD, fill_h, np.int64), shard.dev)
    oc = _dev(np.full(cap + GUARD, fill_c, np.int32), shard.dev)
    n_out = C.c_int64(77)
    rc = lib.dg_sketch_merge_runs_dev(shard.ctx.h, h.data_ptr(), cnt.data_ptr(), n, oh.data_ptr(), oc.data_ptr(), cap, C.byref(n_out))
    torch.cuda.synchronize()
    return rc, n_out.value, oh.cpu().numpy(), oc.cpu().numpy()


def _check_merge(shard, c):
    dev = shard.dev
    uh, uc = model.merge_runs(c.h, c.c)
    nd, n = uh.size, c.h.size
    h, cnt = _hashes(c.h, dev), _dev(c.c, dev)
    rh, rc_t = shard.ops.merge_runs(h, cnt)                                          # as the product calls it: cap = n
    torch.cuda.synchronize()
    assert rh.numel() == nd and np.array_equal(_u64(rh), uh) and np.array_equal(rc_t.cpu().numpy(), uc)
    rc, n_out, oh, oc = _merge(shard, h, cnt, n, nd)                                 # cap exactly reached
    assert rc == 0 and n_out == nd
    assert np.array_equal(oh[:nd].view(np.uint64), uh) and np.array_equal(oc[:nd], uc)
    assert np.all(oh[nd:] == -11) and np.all(oc[nd:] == -13)
    if nd > 0:                                                                       # cap exceeded by one
        rc, n_out, oh, oc = _merge(shard, h, cnt, n, nd - 1)
        assert rc == DG_ERR_ARG and n_out == 0
        assert f"{nd} distinct exceed capacity {nd - 1}" in lib.dg_last_error().decode()
        assert np.all(oh == -11) and np.all(oc == -13)
    assert np.array_equal(_u64(h), c.h) and np.array_equal(cnt.cpu().numpy(), c.c)


@pytest.mark.parametrize("c", cases.merge_cases(), ids=lambda c: c.name)
def test_merge_runs(shard, c):
    _check_merge(shard, c)


def test_merge_small_call_after_large_on_the_same_context(shard):
    """the scratch buffers of the context are reused: 3 entries right after 70,000 must not see what those left behind"""
    by = {c.name: c for c in cases.merge_cases()}
    _check_merge(shard, by["runs8_n70000"])
    _check_merge(shard, by["n3_small"])
    _check_merge(shard, by["only_padding_n1"])


# ------------------------------------------------------------------ histogram
@pytest.mark.parametrize("c", cases.histogram_cases(), ids=lambda c: c.name)
def test_histogram(shard, c):
    dev, n_bins = shard.dev, c.hist0.size
    cnt = _dev(c.c, dev)
    hist = _guarded(c.hist0, dev, -17)
    want = c.hist0.copy()
    capi._check(lib.dg_sketch_histogram_dev(shard.ctx.h, cnt.data_ptr(), c.c.size, n_bins, hist.data_ptr()), "dg_sketch_histogram_dev")
    model.histogram(c.c, want)
    torch.cuda.synchronize()
    once = hist.cpu().numpy()
    assert np.array_equal(once[:n_bins], want) and np.all(once[n_bins:] == -17)
    shard.ops.histogram(cnt, hist[:n_bins])                                          # again, through HipOps, into the same words
    model.histogram(c.c, want)
    torch.cuda.synchronize()
    twice = hist.cpu().numpy()
    assert np.array_equal(twice[:n_bins], want) and np.all(twice[n_bins:] == -17)
    assert np.array_equal(cnt.cpu().numpy(), c.c)


# ------------------------------------------------------------------ refusals
def test_refusals(shard):
    """bad arguments: DG_ERR_ARG, the message names the entry point, nothing is written"""
    dev, hd = shard.dev, shard.ctx.h
    h = _hashes(np.array([3, 9, 1 << 63], np.uint64), dev)
    cnt = _dev(np.array([1, 2, 3], np.int32), dev)
    o64 = _dev(np.full(16, -21, np.int64), dev)
    o32 = _dev(np.full(16, -23, np.int32), dev)
    H, Cn, O64, O32 = h.data_ptr(), cnt.data_ptr(), o64.data_ptr(), o32.data_ptr()
    n_out = C.c_int64(77)
    N = C.byref(n_out)
    part, hist, merge = lib.dg_sketch_partition_dev, lib.dg_sketch_histogram_dev, lib.dg_sketch_merge_runs_dev
    count, rank, both = lib.dg_sketch_count_dictionary_dev, lib.dg_sketch_rank_dictionary_dev, lib.dg_sketch_count_rank_dictionary_dev
    refused = [
        ("dg_sketch_partition_dev: bad arguments", lambda: part(hd, H, 3, 0, O64)),
        ("dg_sketch_partition_dev: bad arguments", lambda: part(hd, H, 3, 4097, O64)),
        ("dg_sketch_partition_dev: bad arguments", lambda: part(hd, H, 3, 2, None)),
        ("dg_sketch_partition_dev: bad arguments", lambda: part(hd, H, -1, 2, O64)),
        ("dg_sketch_histogram_dev: bad arguments", lambda: hist(hd, Cn, 3, 1, O64)),
        ("dg_sketch_histogram_dev: bad arguments", lambda: hist(hd, Cn, 3, 8, None)),
        ("dg_sketch_merge_runs_dev: null n_out", lambda: merge(hd, H, Cn, 3, O64, O32, 16, None)),
        ("merge: 3 distinct exceed capacity 2", lambda: merge(hd, H, Cn, 3, O64, O32, 2, N)),
        ("dg_sketch_merge_runs_dev: bad arguments", lambda: merge(hd, H, Cn, -1, O64, O32, 16, N)),
        ("dg_sketch_merge_runs_dev: bad arguments", lambda: merge(hd, H, Cn, 3, O64, O32, -1, N)),
        ("dg_sketch_merge_runs_dev: bad arguments", lambda: merge(hd, None, Cn, 3, O64, O32, 16, N)),
        ("dg_sketch_merge_runs_dev: bad arguments", lambda: merge(hd, H, None, 3, O64, O32, 16, N)),
        ("dg_sketch_merge_runs_dev: bad arguments", lambda: merge(hd, H, Cn, 3, None, O32, 16, N)),
        ("dg_sketch_merge_runs_dev: bad arguments", lambda: merge(hd, H, Cn, 3, O64, None, 16, N)),
        ("dg_sketch_count_dictionary_dev: bad arguments", lambda: count(hd, H, -1, H, Cn, 3, O32)),
        ("dg_sketch_count_dictionary_dev: bad arguments", lambda: count(hd, H, 3, H, Cn, -1, O32)),
        ("dg_sketch_count_dictionary_dev: bad arguments", lambda: count(hd, None, 3, H, Cn, 3, O32)),
        ("dg_sketch_count_dictionary_dev: bad arguments", lambda: count(hd, H, 3, None, Cn, 3, O32)),
        ("dg_sketch_count_dictionary_dev: bad arguments", lambda: count(hd, H, 3, H, None, 3, O32)),
        ("dg_sketch_count_dictionary_dev: bad arguments", lambda: count(hd, H, 3, H, Cn, 3, None)),
        ("dg_sketch_rank_dictionary_dev: bad arguments", lambda: rank(hd, H, -1, H, 3, 0, O64)),
        ("dg_sketch_rank_dictionary_dev: bad arguments", lambda: rank(hd, H, 3, H, -1, 0, O64)),
        ("dg_sketch_rank_dictionary_dev: bad arguments", lambda: rank(hd, None, 3, H, 3, 0, O64)),
        ("dg_sketch_rank_dictionary_dev: bad arguments", lambda: rank(hd, H, 3, None, 3, 0, O64)),
        ("dg_sketch_rank_dictionary_dev: bad arguments", lambda: rank(hd, H, 3, H, 3, 0, None)),
        ("dg_sketch_count_rank_dictionary_dev: bad arguments", lambda: both(hd, H, -1, H, Cn, 3, 0, O32, O64)),
        ("dg_sketch_count_rank_dictionary_dev: bad arguments", lambda: both(hd, H, 3, H, Cn, -1, 0, O32, O64)),
        ("dg_sketch_count_rank_dictionary_dev: bad arguments", lambda: both(hd, None, 3, H, Cn, 3, 0, O32, O64)),
        ("dg_sketch_count_rank_dictionary_dev: bad arguments", lambda: both(hd, H, 3, None, Cn, 3, 0, O32, O64)),
        ("dg_sketch_count_rank_dictionary_dev: bad arguments", lambda: both(hd, H, 3, H, None, 3, 0, O32, O64)),
        ("dg_sketch_count_rank_dictionary_dev: bad arguments", lambda: both(hd, H, 3, H, Cn, 3, 0, None, O64)),
        ("dg_sketch_count_rank_dictionary_dev: bad arguments", lambda: both(hd, H, 3, H, Cn, 3, 0, O32, None)),
    ]
    for q, (message, call) in enumerate(refused):
        n_out.value = 77
        rc = call()
        assert rc == DG_ERR_ARG, (q, message, rc)
        assert lib.dg_last_error().decode() == message, (q, message)
        with pytest.raises(capi.DgError, match=message.split(":")[0]):
            capi._check(rc, "entry point")
        torch.cuda.synchronize()
        assert torch.all(o64 == -21) and torch.all(o32 == -23), (q, message)
        assert n_out.value == (77 if "null n_out" in message or "merge" not in message else 0), (q, message)
    # what stays legal: empty sizes with null pointers are no error and write nothing
    assert part(hd, None, 0, 3, O64) == 0
    assert hist(hd, None, 0, 8, O64 + 8 * 8) == 0
    assert merge(hd, None, None, 0, None, None, 0, N) == 0 and n_out.value == 0
    assert count(hd, None, 0, H, Cn, 3, None) == 0 and count(hd, H, 3, None, None, 0, O32) == 0
    assert rank(hd, None, 0, H, 3, 5, None) == 0 and rank(hd, H, 3, None, 0, 5, O64) == 0
    assert both(hd, None, 0, H, Cn, 3, 5, None, None) == 0 and both(hd, H, 3, None, None, 0, 5, O32, O64) == 0
    torch.cuda.synchronize()
    assert o64[:4].tolist() == [0, 0, 0, 0] and torch.all(o64[4:] == -21) and torch.all(o32 == -23)     # (the partition of an empty list: all zero)
    assert np.array_equal(_u64(h), np.array([3, 9, 1 << 63], np.uint64)) and cnt.tolist() == [1, 2, 3]


# ------------------------------------------------------------------ a small emulated exchange
def _read_set(seed):
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    genome = bytes(rng.choice(acgt, 6000).tobytes())
    reads = [genome[s:s + int(ln)] for s, ln in zip(rng.integers(0, len(genome) - 110, 300), rng.integers(90, 111, 300))]
    return reads + [b"", b"ACGT", bytes(rng.choice(acgt, 100).tobytes())]


@pytest.fixture(scope="module", params=[(31, 25), (5, 3)], ids=lambda kw: f"k{kw[0]}w{kw[1]}")
def whole(request):
    """the single-process answer on the whole read set, by the oracle and numpy: computed once per (k, w), never changed"""
    k, w = request.param
    reads = _read_set(11)
    H, Cn = orc.sketch_reads(reads, k, w)
    rng = np.random.default_rng(12)
    D = np.unique(np.concatenate([orc.minimizers(reads[i], k, w)[0] for i in (0, 7, 150, 299)]
                                 + [rng.integers(0, model.MAX64, 40, dtype=np.uint64, endpoint=True), np.array([0, model.MAX64], np.uint64)]))
    hit = np.isin(D, H)
    assert hit.any() and (~hit).sum() >= 40 and H.size > 0
    pos = np.searchsorted(H, D)
    counts = np.where(hit, Cn[np.minimum(pos, H.size - 1)], 0).astype(np.int32)
    ids = np.where(hit, pos, -1).astype(np.int64)
    hist = np.bincount(np.minimum(Cn, HIST_BINS - 1), minlength=HIST_BINS).astype(np.int64)
    for a in (H, Cn, D, counts, ids, hist):
        a.setflags(write=False)
    return dict(k=k, w=w, reads=reads, H=H, C=Cn, D=D, counts=counts, ids=ids, hist=hist)


def _pack_block(h, c, split, W, cap, dev):
    """one sender's [W, 1 + cap, 2] block of the fixed-size exchange, packed exactly as ShardedSketch._score packs it"""
    n = h.numel()
    seg = split[1:] - split[:-1]
    col = torch.arange(cap, device=dev)
    valid = col[None, :] < seg[:, None]
    src = (split[:-1, None] + col[None, :]).clamp_(max=max(n - 1, 0))
    block = torch.empty((W, cap + 1, 2), dtype=torch.int64, device=dev)
    block[:, 0, 0] = torch.where(seg <= cap, seg, torch.full_like(seg, -1))
    block[:, 0, 1] = 0
    if n > 0:
        block[:, 1:, 0] = torch.where(valid, h[src], torch.full((1, 1), -1, dtype=torch.int64, device=dev))
        block[:, 1:, 1] = torch.where(valid, c[src].to(torch.int64), torch.zeros((1, 1), dtype=torch.int64, device=dev))
    else:
        block[:, 1:, 0] = -1; block[:, 1:, 1] = 0
    return block


@pytest.mark.parametrize("fixed_size", [False, True], ids=["exact_runs", "padded_blocks"])
@pytest.mark.parametrize("world", [2, 3, 5])
def test_emulated_exchange(shard, whole, world, fixed_size):
    """ranks emulated one after the other on the one context: per-shard sketch, dictionary counts summed over the shards,
    partition, the exchange (exact runs, or blocks of cap = the longest run padded with (-1, 0)), per-owner merge, ids with
    the owner's base, histogram -- reassembled, all of it equals the single-process answer"""
    dev, ops, hd = shard.dev, shard.ops, shard.ctx.h
    reads, H, Cn, D, k, w = whole["reads"], whole["H"], whole["C"], whole["D"], whole["k"], whole["w"]
    dict_t = _hashes(D, dev)
    counts = torch.zeros(D.size, dtype=torch.int32, device=dev)
    runs = []
    for r in range(world):
        lo, hi = shard_bounds(len(reads), world, r)
        mine = reads[lo:hi]
        off = np.zeros(len(mine) + 1, np.int64)
        np.cumsum([len(x) for x in mine], out=off[1:])
        h, c = ops.sketch_reads(_dev(np.frombuffer(b"".join(mine), np.uint8), dev), _dev(off, dev), k, w)
        h, c = h.clone(), c.clone()
        capi._check(lib.dg_sketch_count_dictionary_dev(hd, dict_t.data_ptr(), D.size, h.data_ptr(), c.data_ptr(), h.numel(), counts.data_ptr()),
                    "dg_sketch_count_dictionary_dev")                                # += : the sum the all-reduce would form
        split = ops.partition(h, world)
        assert np.array_equal(split.cpu().numpy(), model.partition(_u64(h), world))
        runs.append((h, c, split))
    if fixed_size:
        cap = max(int((s[1:] - s[:-1]).max()) for _, _, s in runs)                   # the longest run: every block is full somewhere
        blocks = [_pack_block(h, c, s, world, cap, dev) for h, c, s in runs]
    base, rank1 = 0, torch.zeros(D.size, dtype=torch.int64, device=dev)
    hist = torch.zeros(HIST_BINS, dtype=torch.int64, device=dev)
    for owner in range(world):                                                       # what rank `owner` receives from the all-to-all
        if fixed_size:
            recv = torch.stack([b[owner] for b in blocks])
            assert not bool((recv[:, 0, 0] < 0).any())
            body = recv[:, 1:, :].reshape(-1, 2)
            hh, cc = body[:, 0].contiguous(), body[:, 1].to(torch.int32).contiguous()
            assert hh.numel() == world * cap
        else:
            hh = torch.cat([h[int(s[owner]):int(s[owner + 1])] for h, _, s in runs])
            cc = torch.cat([c[int(s[owner]):int(s[owner + 1])] for _, c, s in runs])
        rh, rc = ops.merge_runs(hh, cc)
        m = rh.numel()
        assert np.array_equal(_u64(rh), H[base: base + m]) and np.array_equal(rc.cpu().numpy(), Cn[base: base + m])
        assert m == 0 or bool(np.all(model.owner_of(H[base: base + m], world) == owner))
        capi._check(lib.dg_sketch_rank_dictionary_dev(hd, dict_t.data_ptr(), D.size, rh.data_ptr(), m, base, rank1.data_ptr()), "dg_sketch_rank_dictionary_dev")
        ops.histogram(rc, hist)
        base += m
    torch.cuda.synchronize()
    assert base == H.size
    assert np.array_equal(counts.cpu().numpy(), whole["counts"])
    assert np.array_equal(rank1.cpu().numpy() - 1, whole["ids"])
    assert np.array_equal(hist.cpu().numpy(), whole["hist"])
    assert np.array_equal(_u64(dict_t), D)

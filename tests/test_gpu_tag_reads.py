"""GPU (-m gpu): dg_sketch_tag_reads against the model (tests/tag_model.py), compared exactly.

Read sets follow the tile arithmetic of tests/test_gpu_sketch_domain.py (TW = 128 windows per tile; a read of n bases has
nwin = n - k - w + 2 windows).  A and B are the minimizer hashes of two sequences from which half of the reads are cut; the first
holds N, the second R, so that both have private hashes at k = 1 too.  Every case runs three ways -- the default LDS limit, a limit
of 4 emissions (nearly every read is sorted instead) and a limit between the reads' emission counts (both routes in one call)."""
import functools

import numpy as np
import pytest

import oracle_py as orc
import tag_model as tm
from dipgenie_amd import capi

pytestmark = pytest.mark.gpu
TW = 128
KW = [(31, 25), (1, 1), (2, 2), (8, 33), (16, 64), (33, 1), (64, 65)]
IDS = [f"k{k}_w{w}" for k, w in KW]
DG_ERR_ARG = -1


def _rnd(rng, n, alpha=b"ACGT"):
    return bytes(rng.choice(np.frombuffer(alpha, np.uint8), max(n, 0)).tobytes())


def _len_for(k, w, nwin):
    return nwin + k + w - 2


def _two_haplotypes(rng, n=3000):
    """H1: random with single N; H2: H1 with substitutions and single R at other places.  Shared and private hashes on both sides."""
    base = bytearray(_rnd(rng, n))
    h1, h2 = bytearray(base), bytearray(base)
    for p in rng.integers(0, n, n // 50):
        h2[p] = b"ACGT"[(b"ACGT".index(h2[p]) + 1) % 4]
    for p in range(150, n, 600):
        h1[p] = ord("N")
        h2[p + 300] = ord("R")
    return bytes(h1), bytes(h2)


def _read_set(rng, k, w, h1, h2):
    lens = [k + w - 2, _len_for(k, w, 1)] + [_len_for(k, w, x) for x in (127, 128, 129, 256, 257, 4 * TW + 37)]
    lens += [int(n) for n in rng.integers(k + w - 2, _len_for(k, w, 300), 150)]
    reads = []
    for i, n in enumerate(lens):                                       # half of them cut from the two sequences, in turn
        if i % 2 == 0:
            src = h1 if i % 4 == 0 else h2
            s = int(rng.integers(0, len(src) - n + 1))
            reads.append(src[s:s + n])
        else:
            reads.append(_rnd(rng, n))
    m = max(300, k + w + 60)
    reads += [h1[150 - m // 2:150 + m // 2], h2[450 - m // 2:450 + m // 2]]   # across the N / the R
    n = _len_for(k, w, 300)
    reads += [_rnd(rng, n, b"ACGTN"), _rnd(rng, n, b"acgt"), _rnd(rng, n, b"acgtACGT"), _rnd(rng, n, b"ACGTRYKM*"), b"N" * n,
              h1[:n].lower(), h2[100:100 + n].lower()]
    # X + Y + X: the second copy starts beyond the first tile (window TW) and re-emits the first copy's hashes
    x = h1[700:700 + k + w + 40]
    y = _rnd(rng, TW + 30)
    reads += [x + y + x, x + y + x + _rnd(rng, 2 * TW) + x, _rnd(rng, k + w + 90) * 3]
    reads += [(u * n)[:n] for u in (b"AC", b"AT", b"ACG", b"AACCGGTT")] + [(_rnd(rng, 7) * n)[:n], (_rnd(rng, 40) * n)[:n]]   # tandem repeats
    reads += [c * n for c in (b"A", b"C", b"G", b"T")]                 # homopolymers
    return reads


@functools.lru_cache(maxsize=None)
def _case(k, w):
    """reads, shuffled lists with duplicates, the model's records and the emissions per read -- computed once, never changed"""
    rng = np.random.default_rng(77_000 + 1000 * k + w)
    h1, h2 = _two_haplotypes(rng)
    reads = _read_set(rng, k, w, h1, h2)
    a, b = orc.minimizers(h1, k, w)[0], orc.minimizers(h2, k, w)[0]
    a = np.concatenate([a, a[::2], a[:7]]); b = np.concatenate([b, b[::3]])
    rng.shuffle(a); rng.shuffle(b)
    want = tm.tag_reads(reads, k, w, a, b)
    want.setflags(write=False)
    emitted = np.array([orc.minimizers(r, k, w)[0].size for r in reads], np.int64)
    return reads, a, b, want, emitted


@pytest.mark.parametrize("k,w", KW, ids=IDS)
def test_tag_reads_three_routes(gpu_ctx, k, w):
    reads, a, b, want, emitted = _case(k, w)
    assert (want[:, 0] > 0).any() and (want[:, 1] > 0).any() and (want[:, 2] > 0).any() and (want[:, 3] > 0).any()
    assert (want[0] == 0).all() and len(reads[0]) == k + w - 2         # the read without a window
    got = gpu_ctx.sketch_tag_reads(reads, k, w, a, b)
    assert got.dtype == np.int32 and got.shape == (len(reads), 4)
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:10]
    assert gpu_ctx.sketch_stat("tag_long_reads") == int((emitted > 1024).sum()) == 0
    assert gpu_ctx.sketch_timing().n_emitted == int(emitted.sum())
    assert gpu_ctx.sketch_stat("tag_dict_distinct") == len(tm.as_set(a) | tm.as_set(b))
    with gpu_ctx.sketch_options(tag_lds_entries=4):
        got4 = gpu_ctx.sketch_tag_reads(reads, k, w, a, b)
        n_long = gpu_ctx.sketch_stat("tag_long_reads")
    assert np.array_equal(got4, want), np.flatnonzero((got4 != want).any(axis=1))[:10]
    assert n_long == int((emitted > 4).sum()) and n_long > len(reads) // 4   # (at w = 64 a read needs ~150 windows for five emissions)
    mid = int(np.median(emitted[emitted > 0]))
    assert 0 < (emitted > mid).sum() < (emitted > 0).sum() and 1 <= mid <= 1024
    with gpu_ctx.sketch_options(tag_lds_entries=mid):
        gotm = gpu_ctx.sketch_tag_reads(reads, k, w, a, b)
        n_long = gpu_ctx.sketch_stat("tag_long_reads")
    assert np.array_equal(gotm, want), np.flatnonzero((gotm != want).any(axis=1))[:10]
    assert n_long == int((emitted > mid).sum())
    assert gpu_ctx.sketch_get_option("tag_lds_entries") == 0


def test_default_limit_boundary(gpu_ctx):
    """the default limit itself (1,024 emissions: the full LDS set of 2,048 slots on one side, the sort on the other): reads of 1,023 ..
    1,026 emissions at k = 33, w = 1 (every k-mer a window), each ending in a copy of its own first 400 bases, so that a third of the
    emissions meet their twin in the set"""
    k, w = 33, 1
    rng = np.random.default_rng(21)
    h1, h2 = _rnd(rng, 1400), _rnd(rng, 1400)
    reads = []
    for i, n in enumerate((1023, 1024, 1025, 1026, 1024, 1025, 3000)):
        src = (h1, h2)[i % 2]
        body = src[:n + k - 1 - 400] if i < 4 else _rnd(rng, n + k - 1 - 400)
        reads.append(body + body[:400])
    emitted = np.array([orc.minimizers(r, k, w)[0].size for r in reads], np.int64)
    assert emitted.tolist() == [1023, 1024, 1025, 1026, 1024, 1025, 3000]
    a, b = orc.minimizers(h1, k, w)[0], orc.minimizers(h2, k, w)[0]
    want = tm.tag_reads(reads, k, w, a, b)
    assert (want[:, 0] < emitted).all() and want[0, 1] > 0 and want[1, 2] > 0
    got = gpu_ctx.sketch_tag_reads(reads, k, w, a, b)
    assert np.array_equal(got, want), (got, want)
    assert gpu_ctx.sketch_stat("tag_long_reads") == int((emitted > 1024).sum()) == 4
    with gpu_ctx.sketch_options(tag_lds_entries=1024):                 # the explicit value is the default
        assert np.array_equal(gpu_ctx.sketch_tag_reads(reads, k, w, a, b), want) and gpu_ctx.sketch_stat("tag_long_reads") == 4
    with gpu_ctx.sketch_options(tag_lds_entries=1023):
        assert np.array_equal(gpu_ctx.sketch_tag_reads(reads, k, w, a, b), want) and gpu_ctx.sketch_stat("tag_long_reads") == 6
    with pytest.raises(capi.DgError):
        gpu_ctx.sketch_set_option("tag_lds_entries", 1025)
    with pytest.raises(capi.DgError):
        gpu_ctx.sketch_set_option("tag_table_bits", 31)


def _bits_for(n_distinct):
    """smallest b >= 1 with 2^b >= n_distinct + 1: one empty slot"""
    b = 1
    while (1 << b) < n_distinct + 1:
        b += 1
    return b


def test_dictionary_edge_cases(gpu_ctx):
    k, w = 31, 25
    reads, a, b, want, _ = _case(k, w)
    chk = lambda x, y: np.array_equal(gpu_ctx.sketch_tag_reads(reads, k, w, x, y), tm.tag_reads(reads, k, w, x, y))
    empty = np.zeros(0, np.uint64)
    for x, y in ((empty, empty), (None, None), (a, empty), (None, b), (a, None), (empty, b)):
        xs = empty if x is None else x
        ys = empty if y is None else y
        got = gpu_ctx.sketch_tag_reads(reads, k, w, xs, ys)            # (an empty list goes down as NULL)
        assert np.array_equal(got, tm.tag_reads(reads, k, w, xs, ys))
    assert gpu_ctx.sketch_tag_reads(reads, k, w, empty, empty)[:, 1:].sum() == 0 and gpu_ctx.sketch_stat("tag_table_slots") >= 1
    got = gpu_ctx.sketch_tag_reads(reads, k, w, a, a)                  # A == B: everything found is `both`
    assert np.array_equal(got, tm.tag_reads(reads, k, w, a, a)) and got[:, 1].sum() == 0 and got[:, 2].sum() == 0 and got[:, 3].sum() > 0
    ends = np.array([0, 2**64 - 1], np.uint64)                         # no value is reserved
    assert chk(np.concatenate([a, ends]), np.concatenate([ends[:1], b]))
    assert chk(ends, ends[::-1]) and chk(ends[1:], ends[:1])
    assert np.array_equal(gpu_ctx.sketch_tag_reads(reads, k, w, np.concatenate([a, ends]), np.concatenate([b, ends])), want)


def test_probe_clusters_and_forced_table_sizes(gpu_ctx):
    """several hundred fillers that agree in their low 32 bits with a real hash, and several hundred that agree in their high 32 bits
    (consecutive low halves): long probe clusters on top of real entries, which must still be found; then the smallest legal table
    (one empty slot: probes wrap around the table's end), and one size smaller, which is an error"""
    k, w = 31, 25
    reads, a, b, want, _ = _case(k, w)
    real = np.unique(np.concatenate([a, b]))
    lo = int(real[3]) & 0xFFFFFFFF
    hi = int(real[5]) & 0xFFFFFFFF00000000
    low_same = np.array([(i << 32) | lo for i in range(1, 401)], np.uint64)
    high_same = np.array([hi | ((int(real[5]) + i) & 0xFFFFFFFF) for i in range(1, 401)], np.uint64)
    fill = np.setdiff1d(np.concatenate([low_same, high_same]), real)
    assert fill.size >= 790
    a2, b2 = np.concatenate([a, fill[::2], fill[::5]]), np.concatenate([fill[1::2], b])
    want2 = tm.tag_reads(reads, k, w, a2, b2)
    assert np.array_equal(want2, want)                                 # fillers are no read's hash
    for opts in ({}, {"tag_lds_entries": 4}):
        with gpu_ctx.sketch_options(**opts):
            assert np.array_equal(gpu_ctx.sketch_tag_reads(reads, k, w, a2, b2), want), opts
    nd = len(tm.as_set(a2) | tm.as_set(b2))
    assert gpu_ctx.sketch_stat("tag_dict_distinct") == nd and gpu_ctx.sketch_stat("tag_table_slots") >= 2 * nd
    # pad to 2^bits - 1 distinct hashes: exactly one empty slot
    bits = _bits_for(nd)
    rng = np.random.default_rng(5)
    pad = np.setdiff1d(rng.integers(0, 2**63, (1 << bits) - 1 - nd + 64, dtype=np.uint64), np.concatenate([a2, b2]))[: (1 << bits) - 1 - nd]
    a3 = np.concatenate([a2, pad])
    nd3 = len(tm.as_set(a3) | tm.as_set(b2))
    assert nd3 == (1 << bits) - 1 and bits >= 2
    want3 = tm.tag_reads(reads, k, w, a3, b2)
    with gpu_ctx.sketch_options(tag_table_bits=bits):
        got = gpu_ctx.sketch_tag_reads(reads, k, w, a3, b2)
        assert gpu_ctx.sketch_stat("tag_table_slots") == 1 << bits and gpu_ctx.sketch_stat("tag_dict_distinct") == nd3
    assert np.array_equal(got, want3)
    out = np.full((len(reads), 4), -7, np.int32)
    bases, off = b"".join(reads), np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
    with gpu_ctx.sketch_options(tag_table_bits=bits - 1):
        rc = capi.lib.dg_sketch_tag_reads(gpu_ctx.h, bases, off.ctypes.data, len(reads), k, w, a3.ctypes.data, a3.size, b2.ctypes.data, b2.size, out.ctypes.data)
    assert rc == DG_ERR_ARG and (out == -7).all()
    assert np.array_equal(gpu_ctx.sketch_tag_reads(reads, k, w, a3, b2), want3)   # automatic again


def test_many_short_reads_keep_their_ids(gpu_ctx):
    """3,000 reads of ~150 bases in one call: many workgroups, every record at its own read"""
    k, w = 31, 25
    rng = np.random.default_rng(9)
    h1, h2 = _two_haplotypes(rng, 6000)
    reads = []
    for i in range(3000):
        n = int(rng.integers(100, 200))
        src = (h1, h2, None)[i % 3]
        s = int(rng.integers(0, 6000 - n))
        reads.append(src[s:s + n] if src else _rnd(rng, n))
    reads[17] = b"ACGT"                                                # no window in the middle of the set
    a, b = orc.minimizers(h1, k, w)[0], orc.minimizers(h2, k, w)[0]
    want = tm.tag_reads(reads, k, w, a, b)
    assert len({tuple(r) for r in want}) > 30 and (want[17] == 0).all()
    got = gpu_ctx.sketch_tag_reads(reads, k, w, a, b)
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:10]
    with gpu_ctx.sketch_options(tag_lds_entries=6):
        got = gpu_ctx.sketch_tag_reads(reads, k, w, a, b)
        assert 0 < gpu_ctx.sketch_stat("tag_long_reads") < 3000
    assert np.array_equal(got, want)


def test_argument_errors_leave_out_untouched(gpu_ctx):
    k, w = 11, 5
    rng = np.random.default_rng(10)
    reads = [_rnd(rng, 120) for _ in range(6)]
    bases, off = b"".join(reads), np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
    a = orc.minimizers(reads[0], k, w)[0]
    out = np.full((len(reads), 4), -7, np.int32)
    n, A, O, OUT = len(reads), a.ctypes.data, off.ctypes.data, out.ctypes.data
    call = lambda *args: capi.lib.dg_sketch_tag_reads(gpu_ctx.h, *args)
    bad = [(bases, O, n, 0, w, A, a.size, A, a.size, OUT), (bases, O, n, 256, w, A, a.size, A, a.size, OUT), (bases, O, n, k, 0, A, a.size, A, a.size, OUT),
           (bases, O, n, k, 256, A, a.size, A, a.size, OUT), (bases, O, -1, k, w, A, a.size, A, a.size, OUT), (bases, None, n, k, w, A, a.size, A, a.size, OUT),
           (bases, O, n, k, w, A, -1, A, a.size, OUT), (bases, O, n, k, w, A, a.size, A, -1, OUT), (bases, O, n, k, w, None, a.size, A, a.size, OUT),
           (bases, O, n, k, w, A, a.size, None, 3, OUT)]
    for args in bad:
        assert call(*args) == DG_ERR_ARG, args[2:9]
        assert (out == -7).all()
    assert call(bases, O, n, k, w, A, a.size, A, a.size, None) == DG_ERR_ARG   # null out
    assert call(bases, O, 0, k, w, A, a.size, None, 0, OUT) == 0 and (out == -7).all()   # n_reads = 0 is DG_OK
    assert call(None, None, 0, k, w, None, 0, None, 0, None) == 0
    assert call(bases, O, n, k, w, A, a.size, None, 0, OUT) == 0
    assert np.array_equal(out, tm.tag_reads(reads, k, w, a, None))


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_sketch_reads_is_unchanged_by_a_tag_call(gpu_ctx, mode):
    k, w = 31, 25
    reads, a, b, want, _ = _case(k, w)
    with gpu_ctx.sketch_options(spectrum_mode=mode):
        h0, c0 = gpu_ctx.sketch_reads(reads, k, w)
        path0 = gpu_ctx.sketch_stat("spectrum_path")
        stats0 = [gpu_ctx.sketch_stat(s) for s in ("buckets", "overflow_buckets", "spilled_pairs")]
        assert np.array_equal(gpu_ctx.sketch_tag_reads(reads, k, w, a, b), want)
        assert gpu_ctx.sketch_stat("spectrum_path") == path0 and gpu_ctx.sketch_get_option("spectrum_mode") == mode
        assert [gpu_ctx.sketch_stat(s) for s in ("buckets", "overflow_buckets", "spilled_pairs")] == stats0
        h1, c1 = gpu_ctx.sketch_reads(reads, k, w)
        assert gpu_ctx.sketch_stat("spectrum_path") == path0
    assert np.array_equal(h1, h0) and np.array_equal(c1, c0)
    ho, co = orc.sketch_reads(reads, k, w)
    assert np.array_equal(h0, ho) and np.array_equal(c0, co)

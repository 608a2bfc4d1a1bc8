"""GPU (-m gpu): the sketch kernels over the whole k, w domain (1..255) against the oracle, compared exactly.

sketch_tile_kernel (dipgenie_amd/csrc/dg_sketch.hip) picks its code path from k, w and the tile; the API cannot observe
which one ran, so the read sets below are sized from the tile arithmetic to reach each of them.  A read of n bases has
nwin = n - k - w + 2 windows, cut into tiles of TW = 128 windows; tile t holds nkm = nwin_t + w - 1 k-mers, plus one
context k-mer (the previous tile's last window) for t >= 1.  Then:
  * register doubling: every k-mer of the tile pure ACGT, k <= 32 and nkm <= 128;
  * LDS doubling:      pure ACGT, k <= 32 and nkm > 128 (every haplotype tile but a short last one);
  * plain scan:        the tile holds a byte other than ACGT (after upper-casing), or k > 32;
  * byte path:         k > 32, or a k-mer holding a non-ACGT byte: bytewise canonical order and the byte-wise MurmurHash3;
                       pure ACGT k-mers of k <= 32 are hashed from their 2-bit code (murmur3_code: k >> 4 blocks, k & 15 tail).
The doubling runs one round of partner distance h = L / 2 per power of two L <= w: w >= 64 runs h = 32, w >= 128 runs h = 64.
Nothing here reads the reference; the oracle (oracle/liboracle.so) is pinned to it by tests/golden/kat_sketch_kw.json."""
import numpy as np
import pytest

import oracle_py as orc
from dipgenie_amd import capi, synth

pytestmark = pytest.mark.gpu
TW = 128

# the (k, w) pairs of tests/golden/kat_sketch_kw.json (make_golden.KW_RANGE): every k meets a w < 64, one in
# 64..127 and one >= 128; every w meets a k <= 32 and a k > 32
KW_RANGE = [(1, 1), (1, 64), (1, 255), (2, 2), (2, 127), (2, 128), (8, 33), (8, 65), (8, 129), (16, 63), (16, 64), (16, 200),
            (17, 1), (17, 127), (17, 128), (24, 2), (24, 65), (24, 255), (32, 33), (32, 127), (32, 129), (33, 1), (33, 64), (33, 128),
            (64, 2), (64, 65), (64, 200), (100, 33), (100, 127), (100, 129), (255, 63), (255, 64), (255, 255)]
IDS = [f"k{k}_w{w}" for k, w in KW_RANGE]
SPECTRUM_MODES = {"generic": {"spectrum_mode": 1}, "exact_placement": {"spectrum_mode": 2}}   # (test_gpu_parity.SPECTRUM_MODES)


def _rnd(rng, n, alpha=b"ACGT"):
    return bytes(rng.choice(np.frombuffer(alpha, np.uint8), max(n, 0)).tobytes())


def _put(s, i, c=b"N"):
    return s[:i] + c + s[i + 1:]


def _len_for(k, w, nwin):
    """read length with nwin windows"""
    return nwin + k + w - 2


def _reads_tiles(rng, k, w):
    """lengths from the tile arithmetic: no window (n = k + w - 2), one window; nkm = 128 and 129 in the first tile (n = k + 127 /
    k + 128: the register doubling vs the LDS doubling, for w <= 128); nwin = 128 / 129 / 256 / 257 (a second and third tile,
    whose context k-mer is the previous tile's last window); at least four tiles; and random lengths around all of these"""
    lens = [k + w - 2, _len_for(k, w, 1), k + 127, k + 128] + [_len_for(k, w, x) for x in (2, 127, 128, 129, 256, 257, 4 * TW + 37)]
    reads = [_rnd(rng, n) for n in lens for _ in range(3)]
    reads += [_rnd(rng, int(n)) for n in rng.integers(k + w - 2, _len_for(k, w, 300), 150)]
    return reads


def _reads_bytes(rng, k, w):
    """the plain scan and the byte path: N at base 0, at the last base and inside tile 2's context k-mer (k-mer 127: bases
    127 .. 127 + k - 1), N runs, lower case, IUPAC codes and '*'"""
    n = _len_for(k, w, 300)
    r = [_put(_rnd(rng, n), 0), _put(_rnd(rng, n), n - 1), _put(_rnd(rng, n), 127), _put(_rnd(rng, n), 127 + k - 1),
         _put(_rnd(rng, n), 127 + (k - 1) // 2), _put(_rnd(rng, n), TW + 127 + k // 3)]
    x = _rnd(rng, n)
    r += [x[:n // 2] + b"N" * (k + 3) + x[n // 2 + k + 3:], _rnd(rng, n, b"ACGTN"), _rnd(rng, n, b"acgt"), _rnd(rng, n, b"acgtACGT"),
          _rnd(rng, n, b"ACGTRYKM*"), b"N" * n, _rnd(rng, n).lower()[: n // 3] + _rnd(rng, n - n // 3)]
    return r


def _reads_ties(rng, k, w):
    """equal canonical k-mers in one window (ties: the newest wins): homopolymers, short-period repeats and, for even k,
    reverse-complement palindromes (forward == reverse complement: the orientation ties too)"""
    n = _len_for(k, w, 300)
    r = [c * n for c in (b"A", b"C", b"G", b"T")]
    r += [(u * n)[:n] for u in (b"AC", b"AT", b"GC", b"ACG", b"ACGT", b"AACCGGTT")]
    r += [(_rnd(rng, 7) * n)[:n], (_rnd(rng, 40) * n)[:n], b"A" * (n // 2) + _rnd(rng, n - n // 2)]
    if k % 2 == 0:
        half = _rnd(rng, k // 2)
        unit = half + synth.revcomp(half)
        r += [(unit * (n // k + 1))[:n], ((unit + _rnd(rng, 3)) * (n // k + 1))[:n]]
    return r


def _read_set(k, w):
    rng = np.random.default_rng(1000 * k + w)
    reads = _reads_tiles(rng, k, w) + _reads_bytes(rng, k, w) + _reads_ties(rng, k, w)
    return reads + reads[:25]                                          # (counts above 1)


@pytest.mark.parametrize("k,w", KW_RANGE, ids=IDS)
def test_sketch_reads_kw_domain(gpu_ctx, k, w):
    """Sp_R of the read set above == the oracle's, exactly.  Pairs with w >= 128 (every tile of more than one window takes
    the LDS path) or k > 32 (the byte path) also run the generic sort and the exact placement of the spectrum: the three
    routes must agree (bucket_plan sizes its buckets from w)."""
    reads = _read_set(k, w)
    ho, co = orc.sketch_reads(reads, k, w)
    hg, cg = gpu_ctx.sketch_reads(reads, k, w)
    assert np.array_equal(hg, ho) and np.array_equal(cg, co)
    assert ho.size > 0
    if w >= 128 or k > 32:
        for mode, opts in SPECTRUM_MODES.items():
            with gpu_ctx.sketch_options(**opts):
                hm, cm = gpu_ctx.sketch_reads(reads, k, w)
            assert np.array_equal(hm, hg) and np.array_equal(cm, cg), mode


@pytest.mark.parametrize("k,w", KW_RANGE, ids=IDS)
def test_sketch_reads_register_vs_lds_boundary(gpu_ctx, k, w):
    """one read per call around the register / LDS boundary and the tile boundaries (every call starts from fresh buckets):
    nkm = 127, 128, 129, 130 in the first tile, nwin = 128, 129, 256, 257"""
    rng = np.random.default_rng(7 * k + w)
    for n in sorted({k + 126, k + 127, k + 128, k + 129} | {_len_for(k, w, x) for x in (1, 128, 129, 256, 257)}):
        r = _rnd(rng, n)
        ho, co = orc.sketch_reads([r], k, w)
        hg, cg = gpu_ctx.sketch_reads([r], k, w)
        assert np.array_equal(hg, ho) and np.array_equal(cg, co), n


def _haplotype(rng):
    """~60 kbp: random stretches, N runs, lower case and repeats, several of them across tile boundaries (a tile is 128 windows)"""
    parts = [_rnd(rng, 9000), b"N" * 40, _rnd(rng, 4000, b"acgt"), b"A" * 700, _rnd(rng, 6000), b"AC" * 400, _rnd(rng, 3000, b"ACGTN"),
             _rnd(rng, 5000), b"AT" * 300, _rnd(rng, 2000, b"acgtACGT"), (_rnd(rng, 37) * 30), _rnd(rng, 8000), b"ACGT" * 200,
             _rnd(rng, 4000), b"N" * 300, _rnd(rng, 5000), b"GGGCCC" * 150, _rnd(rng, 4000), b"T" * 257, _rnd(rng, 3000, b"ACGTRY*")]
    return b"".join(parts)


@pytest.mark.parametrize("k,w", KW_RANGE, ids=IDS)
def test_sketch_haplotype_kw_domain(gpu_ctx, k, w):
    """the haplotype route (sparse output, position as aux, one minimizer run emitted once across two tiles): hashes AND the
    positions of the winning k-mers == the oracle's; the positions pin the newest-wins tie rule in every doubling round"""
    rng = np.random.default_rng(50_000 + 1000 * k + w)
    hap = _haplotype(rng)
    ho, po = orc.minimizers(hap, k, w)
    hg, pg = gpu_ctx.sketch_haplotype(hap, k, w)
    assert np.array_equal(hg, ho) and np.array_equal(pg, po)
    for n in (k + w - 2, k + w - 1, k + 127, k + 128, _len_for(k, w, TW), _len_for(k, w, TW + 1)):   # short haplotypes: one or two tiles
        s = hap[:n]
        ho, po = orc.minimizers(s, k, w)
        hg, pg = gpu_ctx.sketch_haplotype(s, k, w)
        assert np.array_equal(hg, ho) and np.array_equal(pg, po), n


def test_hash_kmers_long_k(gpu_ctx):
    """the byte-wise MurmurHash3 of hash_kmers_kernel at k = 101..255: 16-byte blocks and every tail length"""
    rng = np.random.default_rng(3)
    for k in (101, 104, 111, 112, 113, 120, 127, 128, 129, 143, 159, 160, 200, 239, 240, 241, 253, 254, 255):
        blob = _rnd(rng, 64 * k, b"ACGTNacgt")
        got = gpu_ctx.hash_kmers(blob, k)
        assert [int(x) for x in got] == [orc.hash_kmer(blob[i * k:(i + 1) * k]) for i in range(64)], k


BAD_KW = [(0, 25), (256, 25), (31, 0), (31, 256), (0, 0), (256, 256), (-1, 5)]


def test_k_w_outside_the_domain_are_errors(gpu_ctx):
    """k or w outside 1..255: DgError from every entry point, no launch; the context keeps working afterwards"""
    rng = np.random.default_rng(11)
    reads = [_rnd(rng, 600) for _ in range(20)]
    for k, w in BAD_KW:
        with pytest.raises(capi.DgError):
            gpu_ctx.sketch_reads(reads, k, w)
        with pytest.raises(capi.DgError):
            gpu_ctx.sketch_haplotype(reads[0], k, w)
    for k in (0, 256, -3):
        with pytest.raises(capi.DgError):
            gpu_ctx.hash_kmers(b"A" * 512, k)
    ho, co = orc.sketch_reads(reads, 31, 25)
    hg, cg = gpu_ctx.sketch_reads(reads, 31, 25)
    assert np.array_equal(hg, ho) and np.array_equal(cg, co)
    hm, pm = gpu_ctx.sketch_haplotype(reads[0], 31, 25)
    hx, px = orc.minimizers(reads[0], 31, 25)
    assert np.array_equal(hm, hx) and np.array_equal(pm, px)
    assert int(gpu_ctx.hash_kmers(reads[1][:31], 31)[0]) == orc.hash_kmer(reads[1][:31])


def test_k255_w255(gpu_ctx):
    """the domain's far corner: 509-base windows, 383 k-mers per tile"""
    rng = np.random.default_rng(255)
    reads = [_rnd(rng, n) for n in (508, 509, 510, 637, 638, 1000, 3000)] + [_rnd(rng, 1200, b"ACGTacgtN")]
    ho, co = orc.sketch_reads(reads, 255, 255)
    hg, cg = gpu_ctx.sketch_reads(reads, 255, 255)
    assert ho.size > 0 and np.array_equal(hg, ho) and np.array_equal(cg, co)
    hm, pm = gpu_ctx.sketch_haplotype(reads[5], 255, 255)
    hx, px = orc.minimizers(reads[5], 255, 255)
    assert np.array_equal(hm, hx) and np.array_equal(pm, px)

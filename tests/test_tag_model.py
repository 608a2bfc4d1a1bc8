"""CPU: the model of dg_sketch_tag_reads (tests/tag_model.py) on hand-made cases, and the exact substring property."""
import numpy as np

import oracle_py as orc
import tag_model as tm


def _rnd(rng, n, alpha=b"ACGT"):
    return bytes(rng.choice(np.frombuffer(alpha, np.uint8), n).tobytes())


def _hashes(seq, k, w):
    return orc.minimizers(seq, k, w)[0]


def test_repeat_counts_a_hash_once():
    """X + Y + X: the second copy of X re-emits the hashes of the first (not adjacent: Y lies between); every hash counts once"""
    rng = np.random.default_rng(1)
    k, w = 11, 5
    x, y = _rnd(rng, 120), _rnd(rng, 90)
    read = x + y + x
    emitted = _hashes(read, k, w)
    assert len(set(emitted.tolist())) < emitted.size                   # the repeat re-emits
    a = _hashes(x, k, w)
    n_min, only_a, only_b, both = tm.tag_read(read, k, w, tm.as_set(a), set())
    assert n_min == len(set(emitted.tolist()))
    assert only_a == len(set(a.tolist())) and only_b == 0 and both == 0   # every window of x is a window of the read
    # and with both lists: X's hashes in A and B -> both; Y's private hashes only in B
    b = np.concatenate([a, _hashes(y, k, w)])
    rec = tm.tag_read(read, k, w, tm.as_set(a), tm.as_set(b))
    assert rec[1] == 0 and rec[3] == len(set(a.tolist())) and rec[2] == len(set(_hashes(y, k, w).tolist()) - set(a.tolist()))
    assert rec[0] >= rec[1] + rec[2] + rec[3]


def test_homopolymer_has_one_hash():
    k, w = 7, 4
    read = b"A" * 200
    h = orc.hash_kmer(b"A" * k)
    assert tm.tag_read(read, k, w, {h}, set()) == (1, 1, 0, 0)
    assert tm.tag_read(read, k, w, set(), {h}) == (1, 0, 1, 0)
    assert tm.tag_read(read, k, w, {h}, {h}) == (1, 0, 0, 1)
    assert tm.tag_read(read, k, w, {h + 1}, {h - 1}) == (1, 0, 0, 0)


def test_k1_w1_has_two_hashes_in_all():
    """k = w = 1: the canonical 1-mers of ACGT are A and C, so a long random read has exactly two distinct hashes"""
    rng = np.random.default_rng(2)
    read = _rnd(rng, 500)
    ha, hc = orc.hash_kmer(b"A"), orc.hash_kmer(b"C")
    assert tm.tag_read(read, 1, 1, {ha}, {hc}) == (2, 1, 1, 0)
    assert tm.tag_read(read, 1, 1, {ha, hc}, {hc}) == (2, 1, 0, 1)
    assert tm.tag_read(b"AAAATTTT", 1, 1, {ha}, {hc}) == (1, 1, 0, 0)


def test_lists_with_duplicates_and_any_order_are_sets():
    rng = np.random.default_rng(3)
    k, w = 9, 6
    h1, h2 = _rnd(rng, 400), _rnd(rng, 400)
    reads = [h1[50:250], h2[100:300], h1[:150] + h2[150:320]]
    a, b = _hashes(h1, k, w), _hashes(h2, k, w)
    plain = tm.tag_reads(reads, k, w, a, b)
    a2 = np.concatenate([a, a[::3], a[:5]]); b2 = np.concatenate([b[::-1], b])
    rng.shuffle(a2); rng.shuffle(b2)
    assert np.array_equal(tm.tag_reads(reads, k, w, a2, b2), plain)
    assert plain[0, 1] > 0 and plain[1, 2] > 0 and plain[2, 1] > 0 and plain[2, 2] > 0


def test_empty_lists():
    rng = np.random.default_rng(4)
    k, w = 9, 6
    reads = [_rnd(rng, 200), _rnd(rng, 90)]
    a = _hashes(reads[0], k, w)
    for ea, eb in ((None, None), (np.zeros(0, np.uint64), None), ([], [])):
        rec = tm.tag_reads(reads, k, w, ea, eb)
        assert (rec[:, 0] > 0).all() and (rec[:, 1:] == 0).all()
    rec = tm.tag_reads(reads, k, w, a, None)
    assert rec[0, 1] == rec[0, 0] and rec[0, 2] == 0 and rec[0, 3] == 0
    rec = tm.tag_reads(reads, k, w, None, a)
    assert rec[0, 2] == rec[0, 0] and rec[0, 1] == 0 and rec[0, 3] == 0


def test_read_without_a_window_answers_zeros():
    k, w = 11, 5
    rng = np.random.default_rng(5)
    any_hash = tm.as_set(_hashes(_rnd(rng, 300), k, w))
    for n in (0, 1, k - 1, k, k + w - 2):
        assert tm.tag_read(_rnd(rng, n), k, w, any_hash, any_hash) == (0, 0, 0, 0), n
    assert tm.tag_read(_rnd(rng, k + w - 1), k, w, set(), set())[0] == 1   # one window


def test_tag_rule():
    assert [tm.tag_of(*p) for p in ((3, 1), (1, 3), (2, 2), (0, 0), (1, 0), (0, 1))] == [1, 2, 0, 0, 1, 2]


def test_substring_of_a_haplotype_has_nothing_private_to_the_other():
    """For a pure-ACGT sequence H and a substring r of it with at least one window, every window of r is a window of H, and a window's
    minimizer depends on the window alone: S(r) is a subset of A = minimizers(H).  So against (A, B): only_b == 0 and
    n_min == only_a + both.  Checked for EVERY substring sampled -- none is left out."""
    rng = np.random.default_rng(6)
    checked = 0
    for k, w in ((5, 3), (11, 5), (1, 1), (2, 2), (8, 33), (31, 25), (33, 1)):
        H = _rnd(rng, 1500)
        other = bytearray(H)
        for p in rng.integers(0, len(H), 40):                          # a second haplotype: H with substitutions, so B overlaps A
            other[p] = b"ACGT"[(b"ACGT".index(other[p]) + 1) % 4]
        a, b = tm.as_set(_hashes(H, k, w)), tm.as_set(_hashes(bytes(other), k, w))
        assert a & b
        for _ in range(60):
            n = int(rng.integers(k + w - 1, 400))
            s = int(rng.integers(0, len(H) - n + 1))
            n_min, only_a, only_b, both = tm.tag_read(H[s:s + n], k, w, a, b)
            assert n_min >= 1 and only_b == 0 and n_min == only_a + both, (k, w, s, n)
            checked += 1
    assert checked == 7 * 60

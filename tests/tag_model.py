"""The record of dg_sketch_tag_reads, stated with the oracle's per-read hash set and Python sets -- TEST INFRASTRUCTURE.

S = oracle_py.compute_hashes(read, k, w) (Solver::compute_hashes' std::set); A, B = the sets of the values of the two lists.
Record: (|S|, |S n (A \\ B)|, |S n (B \\ A)|, |S n A n B|)."""
import numpy as np

import oracle_py as orc


def as_set(hashes):
    return {int(x) for x in np.asarray(hashes, np.uint64).ravel()} if hashes is not None else set()


def tag_read(read, k, w, set_a, set_b):
    s = {int(x) for x in orc.compute_hashes(read, k, w)}
    return len(s), len((s & set_a) - set_b), len((s & set_b) - set_a), len(s & set_a & set_b)


def tag_reads(reads, k, w, hash_a, hash_b):
    """int32[n_reads, 4]: n_min, only_a, only_b, both"""
    a, b = as_set(hash_a), as_set(hash_b)
    out = np.zeros((len(reads), 4), np.int32)
    for i, r in enumerate(reads):
        out[i] = tag_read(r, k, w, a, b)
    return out


def tag_of(only_1, only_2):
    """the command line's rule: 1 / 2 = the haplotype with more private minimizers of the read, 0 = neither"""
    return 1 if only_1 > only_2 else (2 if only_2 > only_1 else 0)

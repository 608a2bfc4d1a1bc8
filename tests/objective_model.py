"""What a pair of source -> sink paths is worth in the distinct-colour objective -- plain Python / numpy, TEST INFRASTRUCTURE.

Written from the definition, twice, on top of paths_model.PathModel: Hom(p) is the union of the hom colour lists of p's vertices,
Het(p) that of its het lists; hom ids and het ids are two separate id spaces.  For a pair (p, q)

    hom_shared = |Hom(p) n Hom(q)|      hom_single = |Hom(p) /\\ Hom(q)|
    het_single = |Het(p) /\\ Het(q)|      het_both   = |Het(p) n Het(q)|

and the objective is hom_shared + het_single: every colour counts once, however many vertices of a path carry it.  Both forms
return the four counts in that order (the field order of capi.PAIR_OBJECTIVE).

  * objective_sets / objective_sets_many: Python sets over PathModel.hom / .het;
  * ObjectiveRanks.many: np.unique ranks of the colour pools plus boolean masks [pair, path, distinct colour], batched over pairs.
    It shares nothing with the first form but the graph's arrays."""
import numpy as np

FIELDS = ("hom_shared", "hom_single", "het_single", "het_both")


def path_colours(m, p):
    """(Hom(p), Het(p)) as Python sets; m = PathModel"""
    hom, het = set(), set()
    for v in p:
        hom |= m.hom[int(v)]
        het |= m.het[int(v)]
    return hom, het


def objective_sets(m, p, q):
    """(hom_shared, hom_single, het_single, het_both) of the pair (p, q)"""
    hp, tp = path_colours(m, p)
    hq, tq = path_colours(m, q)
    return len(hp & hq), len(hp ^ hq), len(tp ^ tq), len(tp & tq)


def objective_sets_many(m, paths):
    """paths [n, 2, L] -> int32 [n, 4]"""
    return np.array([objective_sets(m, p, q) for p, q in np.asarray(paths)], np.int32).reshape(-1, 4)


def as_rows(res):
    """a capi.PAIR_OBJECTIVE record array -> int32 [n, 4] in the order of FIELDS"""
    return np.stack([res[f] for f in FIELDS], axis=-1).astype(np.int32)


class ObjectiveRanks:
    """the numpy form: per kind the sorted distinct ids of the colour pool (np.unique) and the rank of every list entry"""

    def __init__(self, g):
        get = (lambda n: g[n]) if isinstance(g, dict) else (lambda n: getattr(g, n))
        self.kinds = []
        for kind in ("hom", "het"):
            off = np.asarray(get(kind + "_off"), np.int64)
            ids, rank = np.unique(np.asarray(get(kind + "_col"), np.int64), return_inverse=True)
            self.kinds.append((off, rank.reshape(-1).astype(np.int64), int(ids.size)))
        self.n_hom, self.n_het = self.kinds[0][2], self.kinds[1][2]

    def bitmap_bytes(self):
        """the four bitmaps of one pair, 32-bit words: 8 * (ceil(Ch / 32) + ceil(Ct / 32))"""
        return 8 * ((self.n_hom + 31) // 32 + (self.n_het + 31) // 32)

    def _masks(self, paths, off, rank, n_ids):
        n, _, L = paths.shape
        v = paths.reshape(-1).astype(np.int64)                           # [n * 2 * L], owner row = (pair, path)
        owner = np.repeat(np.arange(n * 2), L)
        cnt = off[v + 1] - off[v]
        first = np.cumsum(cnt) - cnt                                     # where every vertex's entries start in the flat list
        entry = np.repeat(off[v] - first, cnt) + np.arange(int(cnt.sum()))
        mask = np.zeros((n * 2, n_ids), bool)
        mask[np.repeat(owner, cnt), rank[entry]] = True
        return mask.reshape(n, 2, n_ids)

    def many(self, paths):
        """paths [n, 2, L] of vertex ids -> int32 [n, 4]"""
        paths = np.asarray(paths, np.int64)
        out = np.zeros((paths.shape[0], 4), np.int32)
        if paths.shape[0] == 0:
            return out
        hom = self._masks(paths, *self.kinds[0])
        het = self._masks(paths, *self.kinds[1])
        out[:, 0] = (hom[:, 0] & hom[:, 1]).sum(axis=1)
        out[:, 1] = (hom[:, 0] ^ hom[:, 1]).sum(axis=1)
        out[:, 2] = (het[:, 0] ^ het[:, 1]).sum(axis=1)
        out[:, 3] = (het[:, 0] & het[:, 1]).sum(axis=1)
        return out

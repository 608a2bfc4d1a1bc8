"""What a pair of source -> sink paths is worth on a levelized DP graph -- plain Python / numpy, TEST INFRASTRUCTURE.

Written from the definition the sweep implements, not from any implementation of it: for the transition l -> l + 1 the ordered
pair of paths (p, q) adds |(Hom(p[l]) u Hom(q[l])) n (Hom(p[l+1]) u Hom(q[l+1]))| + |(Het(p[l]) u Het(q[l])) /\\ (Het(p[l+1]) u
Het(q[l+1]))| to its value (approximator.cpp:269-311 are the two set sizes, :604-624 their sum per edge pair), the second term
alone to its s_het (:618, :662); r1 / r2 count the weight-1 edges of p / q (:646).  Parallel edges between two vertices carry equal
weights (the library rejects anything else at load) and are one edge here.

A graph is anything with the dg_dp_graph arrays as attributes or keys (capi.DpGraphArrays, a dict)."""
import numpy as np

NEG_INF = -(2 ** 31) // 4


def _get(g, name):
    return g[name] if isinstance(g, dict) else getattr(g, name)


def strip_colours(g, levels):
    """a copy of g (capi.DpGraphArrays) whose vertices of the listed levels carry no colour: colourless levels"""
    from dipgenie_amd.capi import DpGraphArrays
    drop = np.zeros(g.n_vertices, bool)
    for l in levels:
        drop[g.level_off[l]:g.level_off[l + 1]] = True
    arrs = {n: getattr(g, n) for n in DpGraphArrays.NAMES}
    for kind in ("hom", "het"):
        off, col = getattr(g, kind + "_off"), getattr(g, kind + "_col")
        keep = [[] if drop[v] else list(col[off[v]:off[v + 1]]) for v in range(g.n_vertices)]
        new_off = np.zeros(g.n_vertices + 1, np.int64)
        new_off[1:] = np.cumsum([len(x) for x in keep])
        arrs[kind + "_off"], arrs[kind + "_col"] = new_off, np.array([c for x in keep for c in x], np.int32)
    return DpGraphArrays(g.R, **arrs)


def repeat_edge(g, edge, copies):
    """a copy of g with out-edge number `edge` listed `copies` more times (parallel edges of equal weight, in-degree + copies)"""
    from dipgenie_amd.capi import DpGraphArrays
    src = int(np.searchsorted(g.out_off, edge, side="right") - 1)
    arrs = {n: getattr(g, n) for n in DpGraphArrays.NAMES}
    arrs["out_dst"] = np.insert(g.out_dst, [edge] * copies, g.out_dst[edge])
    arrs["out_w"] = np.insert(g.out_w, [edge] * copies, g.out_w[edge])
    off = g.out_off.copy()
    off[src + 1:] += copies
    arrs["out_off"] = off
    return DpGraphArrays(g.R, **arrs)


def edge_list(m, path):
    """the weight-1 hops of a path of the PathModel m and its last hop once more (approximator.cpp:673-692), sorted"""
    hops = [(int(path[l - 1]), int(path[l])) for l in range(1, m.L) if m.succ[int(path[l - 1])][int(path[l])] == 1]
    return sorted(hops + [(int(path[m.L - 2]), int(path[m.L - 1]))])


class PathModel:
    def __init__(self, g):
        self.level_off = np.asarray(_get(g, "level_off"), np.int64)
        self.out_off = np.asarray(_get(g, "out_off"), np.int64)
        self.out_dst = np.asarray(_get(g, "out_dst"), np.int64)
        self.out_w = np.asarray(_get(g, "out_w"), np.int64)
        self.L = self.level_off.size - 1
        self.nV = int(self.level_off[-1])
        self.level_of = np.repeat(np.arange(self.L), np.diff(self.level_off))
        hom_off, het_off = _get(g, "hom_off"), _get(g, "het_off")
        hom_col, het_col = _get(g, "hom_col"), _get(g, "het_col")
        self.hom = [frozenset(int(c) for c in hom_col[hom_off[v]:hom_off[v + 1]]) for v in range(self.nV)]
        self.het = [frozenset(int(c) for c in het_col[het_off[v]:het_off[v + 1]]) for v in range(self.nV)]
        self.succ = []                                   # per vertex: {destination: weight}, parallel edges merged
        for v in range(self.nV):
            d = {}
            for e in range(int(self.out_off[v]), int(self.out_off[v + 1])):
                t, w = int(self.out_dst[e]), int(self.out_w[e])
                assert d.setdefault(t, w) == w, "parallel edges with different weights"
                d[t] = w
            self.succ.append(d)
        self._delta = {}
        # out-edges of weight 0 as a CSR of their own (the biased sampler)
        w0 = np.flatnonzero(self.out_w == 0)
        src = np.repeat(np.arange(self.nV), np.diff(self.out_off))
        self.w0_edge = w0
        self.w0_off = np.zeros(self.nV + 1, np.int64)
        np.cumsum(np.bincount(src[w0], minlength=self.nV), out=self.w0_off[1:])

    # ---- the score ----
    def delta(self, u1, v1, u2, v2):
        """(inter, symd) of the transition (u1 -> u2, v1 -> v2)"""
        key = (u1, v1, u2, v2)
        d = self._delta.get(key)
        if d is None:
            inter = len((self.hom[u1] | self.hom[v1]) & (self.hom[u2] | self.hom[v2]))
            symd = len((self.het[u1] | self.het[v1]) ^ (self.het[u2] | self.het[v2]))
            d = self._delta[key] = (inter, symd)
        return d

    def check_path(self, p):
        """None if p is a source -> sink path of the graph, else (level, what)"""
        if len(p) != self.L:
            return (0, "length")
        for l, v in enumerate(p):
            if not (self.level_off[l] <= v < self.level_off[l + 1]):
                return (l, "level")
        for l in range(1, self.L):
            if int(p[l]) not in self.succ[int(p[l - 1])]:
                return (l, "edge")
        return None

    def recombinations(self, p):
        return sum(self.succ[int(p[l - 1])][int(p[l])] for l in range(1, self.L))

    def score(self, p, q):
        """(value, s_het, r1, r2) of the ordered pair (p, q)"""
        assert self.check_path(p) is None and self.check_path(q) is None
        value = s_het = 0
        for l in range(1, self.L):
            inter, symd = self.delta(int(p[l - 1]), int(q[l - 1]), int(p[l]), int(q[l]))
            value += inter + symd
            s_het += symd
        return value, s_het, self.recombinations(p), self.recombinations(q)

    def score_many(self, paths):
        """paths [n, 2, L] of valid paths -> int32 [n, 4] (a hop without an edge is a KeyError)"""
        out = np.zeros((len(paths), 4), np.int32)
        for n, (p, q) in enumerate(np.asarray(paths).tolist()):
            assert p[0] == 0 and q[0] == 0 and len(p) == len(q) == self.L
            value = s_het = r1 = r2 = 0
            for l in range(1, self.L):
                inter, symd = self.delta(p[l - 1], q[l - 1], p[l], q[l])
                value += inter + symd
                s_het += symd
                r1 += self.succ[p[l - 1]][p[l]]
                r2 += self.succ[q[l - 1]][q[l]]
            out[n] = (value, s_het, r1, r2)
        return out

    # ---- paths ----
    def count_paths(self):
        n = np.zeros(self.nV, object)
        n[self.nV - 1] = 1
        for v in range(self.nV - 2, -1, -1):
            n[v] = sum(n[t] for t in self.succ[v])
        return int(n[0])

    def all_paths(self):
        """every source -> sink path (distinct vertex sequences), as tuples"""
        out = []

        def walk(prefix):
            v = prefix[-1]
            if len(prefix) == self.L:
                out.append(tuple(prefix))
                return
            for t in sorted(self.succ[v]):
                walk(prefix + [t])
        walk([0])
        return out

    def sample_paths(self, rng, n, p_w0=None):
        """n random source -> sink paths [n, L] and their recombination counts [n]: at every step a uniformly random out-edge
        (parallel edges count as often as they are listed); with p_w0, a vertex that has weight-0 out-edges takes a uniformly
        random one of those with that probability instead.  Every non-sink vertex needs an out-edge."""
        paths = np.zeros((n, self.L), np.int32)
        rec = np.zeros(n, np.int64)
        cur = np.zeros(n, np.int64)
        for l in range(1, self.L):
            deg = self.out_off[cur + 1] - self.out_off[cur]
            assert (deg > 0).all(), "dead end"
            e = self.out_off[cur] + np.minimum((rng.random(n) * deg).astype(np.int64), deg - 1)
            if p_w0 is not None and self.w0_edge.size:
                d0 = self.w0_off[cur + 1] - self.w0_off[cur]
                take = (d0 > 0) & (rng.random(n) < p_w0)
                pick = self.w0_off[cur] + np.minimum((rng.random(n) * d0).astype(np.int64), np.maximum(d0 - 1, 0))
                e = np.where(take, self.w0_edge[np.minimum(pick, self.w0_edge.size - 1)], e)
            rec += self.out_w[e]
            cur = self.out_dst[e]
            paths[:, l] = cur
        return paths, rec

    def sample_pairs(self, rng, n, p_w0=None):
        """[n, 2, L] pairs of independent samples and their (r1, r2) [n, 2]"""
        p, rp = self.sample_paths(rng, n, p_w0)
        q, rq = self.sample_paths(rng, n, p_w0)
        return np.ascontiguousarray(np.stack([p, q], axis=1)), np.stack([rp, rq], axis=1)

    # ---- exhaustive optimum ----
    def best_per_budget(self, R, paths=None):
        """max over all ordered pairs with r1 + r2 <= b of the value, for b = 0..R; None where no pair fits.  Also the pair count.
        (Both unions of a transition's score are symmetric in the two paths, so (q, p) is worth what (p, q) is and spends the
        same r1 + r2: one of the two is evaluated.)"""
        paths = self.all_paths() if paths is None else paths
        rec = [self.recombinations(p) for p in paths]
        best_at = {}                                     # exact r1 + r2 -> best value
        for a, p in enumerate(paths):
            for b in range(a, len(paths)):
                q = paths[b]
                r = rec[a] + rec[b]
                if r > R:
                    continue
                v = 0
                for l in range(1, self.L):
                    d = self.delta(p[l - 1], q[l - 1], p[l], q[l])
                    v += d[0] + d[1]
                if v > best_at.get(r, -1):
                    best_at[r] = v
        out, run = [], None
        for b in range(R + 1):
            if b in best_at:
                run = best_at[b] if run is None else max(run, best_at[b])
            out.append(run)
        return out, len(paths) ** 2

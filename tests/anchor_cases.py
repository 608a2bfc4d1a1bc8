"""TEST INFRASTRUCTURE: seeded inputs for dg_anchor_* at its entry points (tests/test_gpu_anchor_kernels.py), built without a
GPU so that tests/test_anchor_model.py can check on the CPU that every input has the property it was made for.

A case is a dict: n_haps, n_vertices, top (a random permutation, never the identity), k, w, haps = [(hash uint64[n],
pos int64[n], step_vtx int32[s], step_start int64[s + 1])], sp_hash (sorted distinct uint64), min_shared (float32)."""
import numpy as np

INF = np.float32(np.inf)
# the largest top_order_map kept under about 64 MB (int32 entries); 999999999 and 1000000000 of the decimal-length ladder
# would need a 4 GB map, so the ladder stops at 10^7 and the int32 end of it is pinned on the model alone
BIG_N = 16_000_000
LADDER = [0, 1, 9, 10, 11, 15, 99, 100, 101, 159, 999, 1000, 1599, 9999, 10000, 15999, 99999, 100000, 159999, 999999, 1000000,
          1599999, 9999999, 10000000, 15999998, BIG_N - 1]


def random_top(rng, n):
    top = rng.permutation(n).astype(np.int32)
    assert n < 2 or not np.array_equal(top, np.arange(n))
    return top


def place_ranks(top, vertices, ranks):
    """swap entries of the permutation so that top[vertices[i]] == ranks[i]"""
    inv = np.empty(top.size, np.int64)
    inv[top] = np.arange(top.size)
    for v, r in zip(vertices, ranks):
        u = int(inv[r])                     # the vertex that holds rank r now
        rv = int(top[v])
        top[v], top[u] = r, rv
        inv[r], inv[rv] = v, u
    return top


def spectrum(rng, n, forbid=()):
    out = set()
    while len(out) < n:
        out.update(int(x) for x in rng.integers(0, 1 << 64, n - len(out), dtype=np.uint64))
        out.difference_update(forbid)
    return np.array(sorted(out), np.uint64)


class HapBuilder:
    """a haplotype put together from explicit occurrences: each one is a block of k bases whose steps carry a chosen vertex set"""

    def __init__(self, rng, k):
        self.rng, self.k = rng, k
        self.hash, self.pos, self.vtx, self.start = [], [], [], [0]

    def add(self, hash_, vertices):
        vs = list(vertices)
        assert 1 <= len(vs) <= self.k and len(set(vs)) == len(vs)
        self.rng.shuffle(vs)                                # any walk order: the list is sorted by top_order_map
        lens = [1] * len(vs)
        lens[int(self.rng.integers(0, len(vs)))] += self.k - len(vs)
        self.hash.append(int(hash_))
        self.pos.append(self.start[-1])
        for v, l in zip(vs, lens):
            self.vtx.append(v)
            self.start.append(self.start[-1] + l)

    def done(self):
        if not self.vtx:                                    # no occurrence: one vertex, k bases, no minimizer
            self.vtx.append(0)
            self.start.append(self.k)
        return (np.array(self.hash, np.uint64), np.array(self.pos, np.int64), np.array(self.vtx, np.int32), np.array(self.start, np.int64))


def from_occurrences(rng, n_haps, n_vertices, top, k, occs, n_sp, min_shared, sp=None):
    """occs = [(id, hap, vertex set)] in any order per haplotype (kept as push order)"""
    sp = spectrum(rng, n_sp) if sp is None else sp
    hb = [HapBuilder(rng, k) for _ in range(n_haps)]
    for r, h, vs in occs:
        hb[h].add(sp[r], vs)
    return dict(n_haps=n_haps, n_vertices=n_vertices, top=top, k=k, w=3, haps=[b.done() for b in hb], sp_hash=sp, min_shared=np.float32(min_shared))


# ---------------------------------------------------------------------------------------------------------------- spans
SPAN_VARIANTS = ["plain", "empty", "revisit_early", "revisit_late"]


def span_case(k, variant, seed=0):
    """every base position of three haplotypes is a minimizer with a hash of its own: every span comes back"""
    rng = np.random.default_rng([7, k, SPAN_VARIANTS.index(variant), seed])
    n_vertices = 1500
    top = random_top(rng, n_vertices)
    fresh = iter(rng.permutation(n_vertices).tolist())

    def walk():
        vtx, lens = [], []
        def step(v, l):
            vtx.append(v); lens.append(l)
        step(next(fresh), k + 2); step(next(fresh), k + 1)                       # k-mers over 1 and 2 vertices
        for _ in range(k + 20):                                                   # k distinct vertices
            step(next(fresh), 1)
        for l in rng.integers(1, 4, 150):                                         # 1..3 bases: everything between
            step(next(fresh), int(l))
        if variant == "revisit_early":
            pool = [next(fresh) for _ in range(6)]
            for l in rng.integers(1, 4, 80):
                step(pool[int(rng.integers(0, 6))], int(l))
            for q in range(40):                                                   # a b a c a d ...: revisits among the first eight
                step(pool[0] if q % 2 == 0 else next(fresh), 1)
        if variant == "revisit_late":
            for period in (9, 10, 12, 17):                                        # a cycle of `period` vertices: the first repeat is
                pool = [next(fresh) for _ in range(period)]                       # the (period + 1)-th vertex under the k-mer
                for q in range(3 * period):
                    step(pool[q % period], 1)
            pool = [next(fresh) for _ in range(13)]
            for q, l in enumerate(rng.integers(1, 3, 60)):
                step(pool[q % 13], int(l))
        for l in rng.integers(1, 4, 30):
            step(next(fresh), int(l))
        if variant == "empty":
            v2, l2 = [], []
            for q, (v, l) in enumerate(zip(vtx, lens)):
                if rng.random() < 0.25:
                    for _ in range(int(rng.integers(1, 4))):
                        v2.append(int(rng.integers(0, n_vertices))); l2.append(0)
                v2.append(v); l2.append(l)
            vtx[:] = [int(rng.integers(0, n_vertices)) for _ in range(3)] + v2[:-1] + [v2[0], v2[1]] + v2[-1:] + [v2[2], v2[0]]
            lens[:] = [0, 0, 0] + l2[:-1] + [0, 0] + l2[-1:] + [0, 0]      # runs at position 0, before the last base-carrying step, at the end
        start = np.zeros(len(lens) + 1, np.int64)
        np.cumsum(lens, out=start[1:])
        return np.array(vtx, np.int32), start

    steps = [walk(), (np.array([next(fresh)], np.int32), np.array([0, k + 3], np.int64)), walk()]    # the middle one: a single step
    poss = []
    for _, ss in steps:
        pos = np.arange(int(ss[-1]) - k + 1, dtype=np.int64)                      # the last one has pos + k == len
        poss.append(np.sort(np.concatenate([pos, pos[::5]])) if pos.size > 20 else pos)   # (some twice: pos is non-decreasing, not increasing)
    hashes = rng.permutation(spectrum(rng, sum(p.size for p in poss)))
    haps, used = [], 0
    for (sv, ss), pos in zip(steps, poss):
        haps.append((hashes[used:used + pos.size], pos, sv, ss))
        used += pos.size
    sp = np.sort(hashes)
    return dict(n_haps=3, n_vertices=n_vertices, top=top, k=k, w=3, haps=haps, sp_hash=sp, min_shared=INF)


# ---------------------------------------------------------------------------------------------- key order and stability
NC = 80


def big_top(seed=1):
    """the BIG_N permutation with NC front candidates on ranks 0..NC-1 and NC back candidates on the last NC ranks; a list
    {front, middles..., back} then starts and ends where the test wants it"""
    rng = np.random.default_rng([11, seed])
    top = random_top(rng, BIG_N)
    cand = [int(x) for x in rng.choice(BIG_N, 2 * NC + len(LADDER), replace=False) if x not in LADDER]
    fronts, backs = sorted(cand[:NC]), sorted(cand[NC:2 * NC])
    place_ranks(top, fronts + backs, [int(x) for x in rng.permutation(NC)] + [BIG_N - 1 - int(x) for x in rng.permutation(NC)])
    return top, fronts, backs


def key_order_case(big, seed=0):
    """groups of 2..16 occurrences of one (id, haplotype) that share front and back and differ in the middle, the middles
    taken from the decimal-length ladder: only the string order of the keys separates them"""
    top, fronts, backs = big
    rng = np.random.default_rng([13, seed])
    k, occs, r = 8, [], 0
    pairs = [(9, 10), (1, 10), (99, 100), (0, 10), (1, 15), (15, 159), (159, 1599), (1599999, 15999998), (15999998, BIG_N - 1), (999, 1000),
             (9999999, 10000000), (10, 11), (100, 101), (1, BIG_N - 1)]
    for a, b in pairs:                                                            # explicit pairs, both push orders, two haplotypes
        for h, order in ((0, (a, b)), (1, (b, a))):
            f, bk = fronts[r % NC], backs[(3 * r) % NC]
            for m in order:
                occs.append((r, h, [f, m, bk]))
        r += 1
    for size in list(range(2, 17)) * 3:                                           # random groups, lists of 3..8 vertices, some repeated
        f, bk = fronts[int(rng.integers(0, NC))], backs[int(rng.integers(0, NC))]
        h = int(rng.integers(0, 2))
        group = []
        while len(group) < size:
            mids = rng.choice(LADDER, int(rng.integers(1, 7)), replace=False).tolist()
            group.append([f] + mids + [bk])
            if len(group) < size and rng.random() < 0.2:
                group.append(list(group[int(rng.integers(0, len(group)))]))
        occs += [(r, h, g) for g in group]
        occs += [(r, 1 - h, [fronts[int(rng.integers(0, NC))], int(rng.choice(LADDER)), bk]) for _ in range(int(rng.integers(0, 4)))]
        r += 1
    return from_occurrences(rng, 2, BIG_N, top, k, occs, r, INF)


def boundary_case(big, size, where, tie, seed=0):
    """one (id, haplotype) group of `size` occurrences with distinct fronts, except that two of them -- at the start, in the
    middle or at the end of the sorted group -- share front and back: with tie = "different" their middles differ, with
    "identical" they are the same list, with "none" there is no tie at all.  A second id carries an ordinary small group."""
    top, fronts, backs = big
    rng = np.random.default_rng([17, size, ["start", "middle", "end"].index(where), seed])
    pairs = [(f, b) for f in fronts for b in backs]
    pick = sorted(pairs[int(i)] for i in rng.choice(len(pairs), size - 1 if tie != "none" else size, replace=False))
    at = {"start": 0, "middle": len(pick) // 2, "end": len(pick) - 1}[where]
    occs = [(1, 0, [f, int(rng.choice(LADDER)), b]) for f, b in pick]
    if tie != "none":
        f, m, b = occs[at][2]
        occs.append((1, 0, [f, m if tie == "identical" else int(rng.choice([x for x in LADDER if x != m])), b]))
    order = rng.permutation(len(occs))
    occs = [occs[int(i)] for i in order] + [(0, 0, [fronts[0], 9, backs[0]]), (0, 0, [fronts[0], 10, backs[0]]), (2, 1, [fronts[1], 5, backs[1]])]
    return from_occurrences(rng, 2, BIG_N, top, 4, occs, 3, INF)


# --------------------------------------------------------------------------------------------------------------- filter
FILTER_SETTINGS = [(4, np.float32(0.5) * np.float32(4)), (4, np.float32(0.75) * np.float32(4)), (3, np.float32(0.34) * np.float32(3)),
                   (7, np.float32(1.0) * np.float32(7)), (7, np.float32(0.999) * np.float32(7)), (1, np.float32(0.999) * np.float32(1))]


def filter_case(n_haps, min_shared, seed=0):
    """ids whose most frequent list occurs thr - 1, ceil(thr) and thr + 1 times, spread over the haplotypes or all in one; ids
    where only the second key in map order gets there.  Returns the case and the ids that must be dropped."""
    rng = np.random.default_rng([19, n_haps, int(float(min_shared) * 1000), seed])
    n_vertices = 3000
    top = random_top(rng, n_vertices)
    k, need = 6, int(np.ceil(float(min_shared)))
    occs, must_drop, r = [], set(), 0

    def some_list():
        return sorted(rng.choice(n_vertices, int(rng.integers(1, k + 1)), replace=False).tolist(), key=lambda v: top[v])

    for rep in range(6):
        for run in (need - 1, need, need + 1):
            for one_hap in (False, True):
                for second_key in (False, True):
                    main = some_list()
                    other = some_list()
                    while (("".join(f"{v}_" for v in other) < "".join(f"{v}_" for v in main)) != second_key) or other == main:
                        other = some_list()                                       # second_key: the frequent list is NOT the first key
                    h0 = int(rng.integers(0, n_haps))
                    for q in range(run):
                        occs.append((r, h0 if one_hap else int(rng.integers(0, n_haps)), main))
                    occs.append((r, int(rng.integers(0, n_haps)), other))          # (once: below every threshold here but 0.999 * 1)
                    for _ in range(int(rng.integers(0, 3))):
                        occs.append((r, int(rng.integers(0, n_haps)), some_list()))
                    if run >= need or np.float32(1) >= min_shared:
                        must_drop.add(r)
                    r += 1
    occs = [occs[int(i)] for i in rng.permutation(len(occs))]
    return from_occurrences(rng, n_haps, n_vertices, top, k, occs, r, min_shared), must_drop


# ----------------------------------------------------------------------------------------------------------- join sizes
def join_case(n_sp, seed=0):
    """three haplotypes, the middle one without a minimizer; hashes at ids 0 and n_sp - 1, in between, and absent ones"""
    rng = np.random.default_rng([23, n_sp, seed])
    n_vertices, k = 500, 7
    top = random_top(rng, n_vertices)
    sp = spectrum(rng, n_sp)
    absent = spectrum(rng, 40, forbid=set(int(x) for x in sp))
    haps = []
    for h in range(3):
        lens = rng.integers(1, 4, 120)
        ss = np.zeros(lens.size + 1, np.int64)
        np.cumsum(lens, out=ss[1:])
        sv = rng.integers(0, n_vertices, lens.size).astype(np.int32)
        if h == 1:
            haps.append((np.zeros(0, np.uint64), np.zeros(0, np.int64), sv, ss))
            continue
        pos = np.sort(rng.integers(0, int(ss[-1]) - k + 1, 90)).astype(np.int64)
        hs = rng.choice(np.concatenate([sp, absent]), pos.size)
        hs[[10, 20, 30]] = absent[:3]
        if n_sp:
            hs[[3, 50]] = sp[0], sp[-1]
        haps.append((hs.astype(np.uint64), pos, sv, ss))
    return dict(n_haps=3, n_vertices=n_vertices, top=top, k=k, w=3, haps=haps, sp_hash=sp, min_shared=np.float32(3.0))


def large_case(seed=0):
    """about 30,000 occurrences over 2,000 ids, four haplotypes walking one bubble chain: an id sits at the same few places of
    every walk, so its lists repeat across haplotypes (the filter has work) and share fronts inside one (no group above 16)"""
    rng = np.random.default_rng([29, seed])
    n_vertices, k, n_ids = 20000, 12, 2000
    top = random_top(rng, n_vertices)
    n_steps = 4000
    names = rng.permutation(n_vertices)[:2 * n_steps].reshape(2, n_steps)         # two alleles per step
    lens = rng.integers(1, 4, n_steps)
    ss = np.zeros(n_steps + 1, np.int64)
    np.cumsum(lens, out=ss[1:])
    L = int(ss[-1])
    sp = spectrum(rng, n_ids)
    absent = spectrum(rng, 16, forbid=set(int(x) for x in sp))
    haps = []
    for h in range(4):
        allele = (rng.random(n_steps) < 0.15).astype(np.int64)
        sv = names[allele, np.arange(n_steps)].astype(np.int32)
        pos = np.sort(rng.choice(L - k + 1, 7600, replace=False)).astype(np.int64)
        hs = sp[np.minimum(pos * n_ids // (L - k + 1), n_ids - 1)].copy()
        hs[rng.choice(pos.size, 100, replace=False)] = rng.choice(absent, 100)
        haps.append((hs, pos, sv, ss))
    return dict(n_haps=4, n_vertices=n_vertices, top=top, k=k, w=3, haps=haps, sp_hash=sp, min_shared=np.float32(3.0))

"""TEST INFRASTRUCTURE: the anchor stage of the reference (solver.cpp:343-357, 415-446, 590-663) restated literally in plain
Python -- per-base vertex map, dict join, std::map<std::string, ...> as a dict iterated in sorted() key order (Python compares
ASCII strings as std::string does), a stable sort by (front, back).  It shares nothing with dipgenie_amd/host or the oracle;
tests/test_anchor_model.py pins it to the reference's own dumps, tests/test_gpu_anchor_kernels.py holds dg_anchor_* to it."""
import numpy as np

STABLE_MAX = 16     # libstdc++'s std::sort is one insertion sort -- stable -- up to 16 elements


def key_of(lst):
    """the map key of solver.cpp:600-603"""
    return "".join(f"{v}_" for v in lst)


def spans(k, pos, step_vtx, step_start, top_order_map):
    """vertex list of every minimizer (:343-357): the distinct vertices under bases pos .. pos + k - 1 in order of first
    appearance, then sorted by top_order_map"""
    step_vtx = np.asarray(step_vtx, np.int64)
    step_start = np.asarray(step_start, np.int64)
    idx_vtx_map = np.repeat(step_vtx, np.diff(step_start)).tolist()         # base -> vertex; empty steps own no base
    out = []
    for p in pos:
        seen, lst = set(), []
        for j in range(int(p), int(p) + k):
            v = idx_vtx_map[j]
            if v not in seen:
                seen.add(v)
                lst.append(v)
        lst.sort(key=lambda v: int(top_order_map[v]))
        out.append(lst)
    return out


def join(sp_hash, haps):
    """occurrences (id, haplotype, list) in (haplotype, minimizer) order (:415-446, 560-575); haps[h] = (hashes, lists),
    id = rank of the hash in the sorted distinct sp_hash"""
    rank = {int(x): i for i, x in enumerate(sp_hash)}
    assert len(rank) == len(sp_hash) and list(sp_hash) == sorted(sp_hash)
    occs = []
    for h, (hashes, lists) in enumerate(haps):
        assert len(hashes) == len(lists)
        for x, lst in zip(hashes, lists):
            if int(x) in rank and len(lst):
                occs.append((rank[int(x)], h, list(lst)))
    return occs


class Result:
    def __init__(self, occs, n_candidates, dropped, unstable):
        self.occs = occs                    # [(id, hap, list)] in Anchor_hits order
        self.n_candidates = n_candidates
        self.dropped = dropped              # ids the filter removed
        self.unstable = unstable            # (id, hap) groups whose order std::sort does not define; their entries in occs mean nothing

    def arrays(self):
        occ_len = np.array([len(l) for _, _, l in self.occs], np.uint32)
        occ_off = np.zeros(len(self.occs), np.uint32)
        if len(self.occs):
            occ_off[1:] = np.cumsum(occ_len[:-1], dtype=np.uint64).astype(np.uint32)
        return dict(occ_id=np.array([i for i, _, _ in self.occs], np.int32), occ_hap=np.array([h for _, h, _ in self.occs], np.int32),
                    occ_off=occ_off, occ_len=occ_len, vpool=np.array([v for _, _, l in self.occs for v in l], np.int32))


def filter_and_sort(occs, n_haps, min_shared=None):
    """the shared-anchor filter (:590-638; min_shared = threshold * num_walks, None switches it off) and the occurrence sort
    (:641-663) on occurrences in push order (haplotype ascending)"""
    assert all(a[1] <= b[1] for a, b in zip(occs, occs[1:]) if a[0] == b[0]), "push order is by haplotype"
    by_id = {}
    for r, h, lst in occs:
        by_id.setdefault(r, []).append((h, lst))
    out, dropped, unstable = [], set(), []
    for r in sorted(by_id):
        hits_map = {}                                                       # key -> [count, [(hap, list)]]
        for h, lst in by_id[r]:
            e = hits_map.setdefault(key_of(lst), [0, []])
            e[0] += 1
            e[1].append((h, lst))
        if min_shared is not None and any(np.float32(hits_map[key][0]) >= np.float32(min_shared) for key in sorted(hits_map)):
            dropped.add(r)
            continue
        per_hap = [[] for _ in range(n_haps)]
        for key in sorted(hits_map):                                        # std::map iteration order, push order inside a key
            for h, lst in hits_map[key][1]:
                per_hap[h].append(lst)
        for h, group in enumerate(per_hap):
            if len(group) > STABLE_MAX:                                     # introsort: defined only up to ties
                ties = {}
                for lst in group:
                    ties.setdefault((lst[0], lst[-1]), set()).add(tuple(lst))
                if any(len(s) > 1 for s in ties.values()):
                    unstable.append((r, h))
            group = sorted(group, key=lambda lst: (lst[0], lst[-1]))        # (Python's sort is stable)
            out.extend((r, h, lst) for lst in group)
    return Result(out, len(occs), dropped, unstable)


def run(k, top_order_map, haps, sp_hash, min_shared):
    """the whole stage: haps[h] = (hashes, pos, step_vtx, step_start)"""
    joined = join(sp_hash, [(hs, spans(k, ps, sv, ss, top_order_map)) for hs, ps, sv, ss in haps])
    return filter_and_sort(joined, len(haps), min_shared)

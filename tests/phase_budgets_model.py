"""The slot plan of dg_dp_phase_margins_budgets in plain Python -- TEST INFRASTRUCTURE.

Written from the contract in include/dipgenie_hip.h, not from the library's code.  A query is a called pair [2, L]; its het levels are
those where the classes of its two vertices differ, h_0 < ... < h_last.  Going down the levels a query carries on h_0 <= l < h_last, and
its key there is (e, c_0[e], c_1[e]) with e its nearest het level above l.  Fewer than two het levels: the query never carries.

    plan(...)        the plan the device call must follow: per level the live keys (the distinct keys of the carrying queries), the keys
                     created (seeded at level e, live from e - 1 down), slots handed out by the rule of the header -- a slot is freed
                     when no query carries its key any more and may be taken by a key seeded at that same level
    naive_live(...)  the same live sets from a per-query simulation that shares nothing: every query walks its own intervals, and the
                     union is grouped by key afterwards

tests/test_phase_budgets_model.py pins the two to each other."""
import numpy as np

STATS = ("queries", "records", "seed_keys", "slot_levels", "backward_launches", "readout_launches", "max_live_slots", "slots_allocated")


def classes_of(called, vertex_class=None):
    """called int [n, 2, L] -> the ordered classes int64 [n, 2, L]"""
    called = np.asarray(called, np.int64)
    return called if vertex_class is None else np.asarray(vertex_class, np.int64)[called]


def query_keys(c):
    """c int [2, L], the classes of one query -> {l: key} on the levels it carries on"""
    L = c.shape[1]
    het = [l for l in range(L) if c[0, l] != c[1, l]]
    keys = {}
    for a, e in zip(het[:-1], het[1:]):
        for l in range(a, e):
            keys[l] = (e, int(c[0, e]), int(c[1, e]))
    return keys


def naive_live(called, vertex_class=None):
    """-> per level the set of keys, from the queries one at a time"""
    cl = classes_of(called, vertex_class)
    L = cl.shape[2]
    live = [set() for _ in range(L)]
    for c in cl:
        for l, key in query_keys(c).items():
            live[l].add(key)
    return live


def plan(called, vertex_class=None):
    """-> dict: live[l] = {key: slot} of the keys live on l; created[l] = the keys seeded at l, sorted; reads[l] = [(query, record index
    within the query, slot)] of the read-outs at l in query order; on_slot[l] = {query: slot} of the carrying queries; stats = the first
    eight words of dg_dp_get_phase_budget_stats"""
    cl = classes_of(called, vertex_class)
    n, _, L = cl.shape
    keys = [query_keys(c) for c in cl]
    het = [[l for l in range(L) if c[0, l] != c[1, l]] for c in cl]
    live = [dict() for _ in range(L)]
    created = [[] for _ in range(L)]
    reads = [[] for _ in range(L)]
    on_slot = [dict() for _ in range(L)]
    cur, free, n_slots = {}, [], 0
    for l in range(L - 1, -1, -1):
        live[l] = dict(cur)
        for q in range(n):
            if l in keys[q]:
                on_slot[l][q] = cur[keys[q][l]]
                if l in het[q]:
                    reads[l].append((q, het[q].index(l), cur[keys[q][l]]))
        below = sorted({keys[q][l - 1] for q in range(n) if l - 1 in keys[q]}) if l else []
        free += [slot for key, slot in cur.items() if key not in below]
        nxt = {}
        for key in below:
            if key in cur:
                nxt[key] = cur[key]
                continue
            if free:
                free.sort()
                nxt[key] = free.pop(0)
            else:
                nxt[key] = n_slots
                n_slots += 1
            created[l].append(key)
        cur = nxt
    counts = [len(x) for x in live]
    stats = dict(queries=n, records=sum(max(len(h) - 1, 0) for h in het), seed_keys=sum(len(x) for x in created), slot_levels=sum(counts),
                 backward_launches=sum(1 for x in counts if x), readout_launches=sum(1 for x in reads if x), max_live_slots=max(counts),
                 slots_allocated=n_slots)
    return dict(live=live, created=created, reads=reads, on_slot=on_slot, stats=stats)

// ======================================================================================
// Solver::compute_and_classify_anchors  (solver.cpp:449-887)
// ======================================================================================
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <future>
#include <iostream>
#include <map>
#include <numeric>
#include <string_view>

#include "stage_util.hpp"

namespace dg {

namespace {

// one haplotype's minimizers: hash[m], and the vertex span v[voff[m], voff[m + 1]) of minimizer m
struct HapIndex { std::vector<uint64_t> hash; std::vector<uint32_t> voff; std::vector<int32_t> v; };
struct Raw { int32_t h; uint32_t m; };   // minimizer m of haplotype h

bool injected(const Pipeline &p, uint32_t h) { return h < p.inj_hap.size() && p.inj_hap[h].set; }

// ---- read sketches: Read_hashes / Sp_R / kmer_count (solver.cpp:526-555, 711-732) ----
// sp_hash: sorted distinct read-minimizer hashes, id = rank (:541-546); sp_count: number of reads containing it (== kmer_count)
std::string read_spectrum(Pipeline &p, std::vector<uint64_t> &sp_hash, std::vector<int32_t> &sp_count) {
    if (p.spectrum_injected) {                                         // the read-sharded ranks' merged spectrum (dist_sketch.py)
        for (size_t q = 1; q < p.inj_sp_hash.size(); ++q)
            if (p.inj_sp_hash[q] <= p.inj_sp_hash[q - 1]) return "injected spectrum: hashes must be strictly ascending";
        if (p.inj_sp_count.size() != p.inj_sp_hash.size()) return "injected spectrum: one count per hash";
        sp_hash = p.inj_sp_hash; sp_count = p.inj_sp_count;
        return "";
    }
    std::vector<int64_t> off(p.reads.size() + 1, 0);
    for (size_t r = 0; r < p.reads.size(); ++r) off[r + 1] = off[r] + (int64_t)p.reads[r].second.size();
    std::string bases;
    bases.reserve((size_t)off.back());
    for (auto &rd : p.reads) bases += rd.second;
    uint64_t *hh = nullptr; int32_t *cc = nullptr; int64_t n = 0;
    int rc = p.be.sketch_reads(p.be.ctx, bases.data(), off.data(), (int64_t)p.reads.size(), p.opt.k, p.opt.w, &hh, &cc, &n);
    if (rc != 0) return backend_error(p.be, "sketch_reads");
    sp_hash.assign(hh, hh + n);
    sp_count.assign(cc, cc + n);
    p.be.free_buf(hh); p.be.free_buf(cc);
    if (!p.opt.tag_reads.empty()) { p.tag_bases = std::move(bases); p.tag_off = std::move(off); }   // --tag-reads: the same bytes are tagged after the DP
    return "";
}

// ---- haplotype sketches (index_kmers, solver.cpp:277-363) ----
// Device path: the backend keeps every haplotype's minimizers and vertex lists on the device
// (dg_anchor_*) and later returns the finished occurrence list; the host path does the same with the
// position lists of be.sketch_haplotype.  Both end in the same `occs` / `vpool` (tests/golden/anchors.json).
bool device_anchors_offered(const Pipeline &p) {
    bool dev = p.be.anchor_begin && p.be.anchor_add_haplotype && p.be.anchor_finish && !p.opt.host_anchors;
    for (const Pipeline::HapSketch &hs : p.inj_hap) if (hs.set && !p.be.anchor_add_haplotype_sketched) dev = false;   // (a backend without the import: host index)
    return dev;
}

// position -> vertex span of every minimizer of haplotype h (:343-357)
void index_vertex_spans(const Pipeline &p, uint32_t h, const uint64_t *hh, const int64_t *pp, int64_t n, const std::vector<int64_t> &seg_start, HapIndex &ix) {
    const int k = p.opt.k;
    ix.hash.assign(hh, hh + n);
    ix.voff.reserve(n + 1);
    ix.voff.push_back(0);
    std::vector<int32_t> uniq;
    size_t seg = 0;
    for (int64_t m = 0; m < n; ++m) {
        int64_t pos = pp[m];
        // positions are non-decreasing; seg = index of the path step containing base pos
        if (seg_start[seg] > pos) seg = 0;
        while (seg + 1 < seg_start.size() - 1 && seg_start[seg + 1] <= pos) ++seg;
        uniq.clear();
        size_t s2 = seg;
        for (;;) {
            int32_t vtx = (int32_t)p.paths[h][s2];
            if (seg_start[s2 + 1] > seg_start[s2] &&                   // empty segments contribute no base
                std::find(uniq.begin(), uniq.end(), vtx) == uniq.end()) uniq.push_back(vtx);
            if (seg_start[s2 + 1] >= pos + k) break;
            ++s2;
        }
        std::sort(uniq.begin(), uniq.end(), [&](int32_t a, int32_t b) { return p.top_order_map[a] < p.top_order_map[b]; });
        ix.v.insert(ix.v.end(), uniq.begin(), uniq.end());
        ix.voff.push_back((uint32_t)ix.v.size());
    }
}

// The backend calls are issued by one thread, back to back (a ctx is not thread-safe); the position -> vertex-span
// mapping of a finished haplotype runs as a task on the other threads meanwhile.
std::string host_haplotype_index(Pipeline &p, std::vector<HapIndex> &kmer_index, double &t_sketch) {
    kmer_index.assign(p.num_walks, HapIndex());
    std::string failure;
#pragma omp parallel num_threads(p.opt.threads)
#pragma omp single
    for (uint32_t h = 0; h < p.num_walks && failure.empty(); ++h) {
        HapAssembly a = p.assemble_haplotype(h, true);                 // :283-285
        auto *seg_start_p = new std::vector<int64_t>(std::move(a.step_start));   // (the task gets the pointer, not a copy of the vector)
        uint64_t *hh = nullptr; int64_t *pp = nullptr; int64_t n = 0;
        const double ts0 = now_s();
        int rc = 0;
        if (injected(p, h)) {                                          // sketched by another rank: same (malloc'ed) hand-off as the backend's
            n = (int64_t)p.inj_hap[h].hash.size();
            hh = (uint64_t *)malloc(8 * (size_t)(n + 1)); pp = (int64_t *)malloc(8 * (size_t)(n + 1));
            std::copy(p.inj_hap[h].hash.begin(), p.inj_hap[h].hash.end(), hh);
            std::copy(p.inj_hap[h].pos.begin(), p.inj_hap[h].pos.end(), pp);
        } else {
            rc = p.be.sketch_haplotype(p.be.ctx, a.seq.data(), (int64_t)a.seq.size(), p.opt.k, p.opt.w, &hh, &pp, &n);
        }
        t_sketch += now_s() - ts0;
        if (rc != 0) {
            failure = backend_error(p.be, "sketch_haplotype");
            delete seg_start_p;
            break;
        }
        p.sum.minimizers_per_hap[h] = n;
#pragma omp task firstprivate(h, hh, pp, n, seg_start_p)
        {
            index_vertex_spans(p, h, hh, pp, n, *seg_start_p, kmer_index[h]);
            if (injected(p, h)) { free(hh); free(pp); } else { p.be.free_buf(hh); p.be.free_buf(pp); }
            delete seg_start_p;
        }
    }
    return failure;
}

struct HapInput { HapAssembly a; std::vector<int32_t> step_vtx; };
HapInput device_hap_input(const Pipeline *p, uint32_t h) {
    HapInput in;
    in.a = p->assemble_haplotype(h, !injected(*p, h));                 // (an injected haplotype needs no string)
    in.step_vtx.assign(p->paths[h].begin(), p->paths[h].end());
    return in;
}

std::string device_haplotype_index(Pipeline &p, double &t_sketch) {
    const Backend &be = p.be;
    if (be.anchor_begin(be.ctx, (int32_t)p.num_walks, (int32_t)p.n_vtx, p.top_order_map.data(), p.opt.k, p.opt.w) != 0) return backend_error(be, "anchor_begin");
    // the next haplotypes' strings and step arrays are assembled on helper threads while the device works on this one
    // (several helpers: one assembly takes longer than the device needs for a haplotype -- 6 ms against 2 on MHC-24)
    const uint32_t depth = (uint32_t)std::max(1, std::min(p.opt.threads - 1, 6));
    std::vector<std::future<HapInput>> ahead(depth);
    for (uint32_t q = 0; q < depth && q < p.num_walks; ++q) ahead[q] = std::async(std::launch::async, device_hap_input, &p, q);
    for (uint32_t h = 0; h < p.num_walks; ++h) {
        HapInput cur = ahead[h % depth].get();
        if (h + depth < p.num_walks) ahead[h % depth] = std::async(std::launch::async, device_hap_input, &p, h + depth);
        const int64_t ns = (int64_t)p.paths[h].size();
        int64_t n = 0;
        const double ts0 = now_s();
        if (injected(p, h)) {                                          // sketched by another rank
            const Pipeline::HapSketch &sk = p.inj_hap[h];
            n = (int64_t)sk.hash.size();
            if (be.anchor_add_haplotype_sketched(be.ctx, (int32_t)h, (int64_t)cur.a.total, sk.hash.data(), sk.pos.data(), n, cur.step_vtx.data(),
                                                 cur.a.step_start.data(), ns) != 0)
                return backend_error(be, "anchor_add_haplotype_sketched");
        } else if (be.anchor_add_haplotype(be.ctx, (int32_t)h, cur.a.seq.data(), (int64_t)cur.a.seq.size(), cur.step_vtx.data(), cur.a.step_start.data(), ns, &n) != 0) {
            return backend_error(be, "anchor_add_haplotype");
        }
        t_sketch += now_s() - ts0;
        p.sum.minimizers_per_hap[h] = n;
    }
    return "";
}

// Once the device work of this stage is done the device side may reserve the DP lattice: mapping 100+ GB takes
// seconds during which every other HIP call of the process queues behind the allocation, so it must start where
// only host work follows -- before the host join, after the device join.
void hint_lattice(const Pipeline &p) {
    if (!(p.opt.ploidy == 2 && p.be.hint_dp_soon)) return;
    size_t max_path = 0;
    for (auto &pw : p.paths) max_path = std::max(max_path, pw.size());
    // Generous on purpose (levels ~ 2.5 x path steps, width ~ 5 x walks: chain + recombination + dummy vertices):
    // reserving too much costs nothing once the exact figure (diploid()) stops it, too little stalls the DP.
    const double kk = 5.0 * (double)p.num_walks;
    p.be.hint_dp_soon(p.be.ctx, (int64_t)std::min(9.0e18, 2.5 * (double)max_path * kk * kk * (p.opt.R + 1)));
}

// ---- compute_anchors (solver.cpp:415-446, 560-575): hap minimizers whose hash is in Sp_R ----
// ids[h][m] = rank of minimizer m of haplotype h in sp_hash, -1 if absent
std::vector<std::vector<int32_t>> lookup_ids(const Pipeline &p, const std::vector<uint64_t> &sp_hash, const std::vector<HapIndex> &kmer_index) {
    const uint32_t num_walks = p.num_walks;
    std::vector<std::vector<int32_t>> ids(num_walks);
    for (uint32_t h = 0; h < num_walks; ++h) ids[h].resize(kmer_index[h].hash.size());
    // (haplotype, block of minimizers) work items: 24 whole haplotypes do not balance over 16+ threads
    const size_t BLK = 1 << 15;
    // Sp_R is sorted: a table over the top bits of the hash (about two keys per slot) replaces most of the binary search
    // (19 dependent cache misses per probe at 5 x 10^5 keys) by one table read and a search over a handful of keys
    int tb = 1;
    while (tb < 28 && ((size_t)1 << tb) < sp_hash.size() / 2) ++tb;
    std::vector<uint32_t> top(((size_t)1 << tb) + 1);
    const int64_t nt = (int64_t)1 << tb;
#pragma omp parallel for num_threads(p.opt.threads) schedule(static)
    for (int64_t q = 0; q <= nt; ++q) {
        const uint64_t lo_key = q == nt ? ~(uint64_t)0 : (uint64_t)q << (64 - tb);
        top[q] = q == nt ? (uint32_t)sp_hash.size() : (uint32_t)(std::lower_bound(sp_hash.begin(), sp_hash.end(), lo_key) - sp_hash.begin());
    }
    std::vector<std::pair<uint32_t, size_t>> items;
    for (uint32_t h = 0; h < num_walks; ++h)
        for (size_t m0 = 0; m0 < kmer_index[h].hash.size(); m0 += BLK) items.emplace_back(h, m0);
#pragma omp parallel for num_threads(p.opt.threads) schedule(dynamic, 1)
    for (int64_t it = 0; it < (int64_t)items.size(); ++it) {
        const uint32_t h = items[it].first;
        const auto &ix = kmer_index[h];
        const size_t m1 = std::min(ix.hash.size(), items[it].second + BLK);
        for (size_t m = items[it].second; m < m1; ++m) {
            const uint64_t key = ix.hash[m];
            const size_t slot = (size_t)(key >> (64 - tb));
            auto itp = std::lower_bound(sp_hash.begin() + top[slot], sp_hash.begin() + top[slot + 1], key);
            ids[h][m] = (itp != sp_hash.begin() + top[slot + 1] && *itp == key) ? (int32_t)(itp - sp_hash.begin()) : -1;
        }
    }
    return ids;
}

// stable counting sort of the (h, m) sequence by id: one histogram per haplotype, offsets in (id, h) order,
// every haplotype then scatters its own minimizers -- (h asc, minimizer order asc) inside every id.
// bucket_off[id] .. bucket_off[id + 1] = the occurrences of id in the returned list
std::vector<Raw> bucket_by_id(const Pipeline &p, const std::vector<std::vector<int32_t>> &ids, std::vector<int64_t> &bucket_off) {
    const uint32_t num_walks = p.num_walks;
    const int32_t count_sp_r = p.count_sp_r;
    bucket_off.assign((size_t)count_sp_r + 1, 0);
    std::vector<Raw> raw;
    if ((size_t)num_walks * (size_t)count_sp_r > ((size_t)1 << 29)) {   // histograms would not fit comfortably: serial sort
        for (uint32_t h = 0; h < num_walks; ++h)
            for (int32_t id : ids[h]) if (id >= 0) bucket_off[id + 1]++;
        for (int32_t r = 0; r < count_sp_r; ++r) bucket_off[r + 1] += bucket_off[r];
        raw.resize((size_t)bucket_off[count_sp_r]);
        std::vector<int64_t> fill(bucket_off.begin(), bucket_off.end() - 1);
        for (uint32_t h = 0; h < num_walks; ++h)
            for (size_t m = 0; m < ids[h].size(); ++m)
                if (ids[h][m] >= 0) raw[fill[ids[h][m]]++] = Raw{(int32_t)h, (uint32_t)m};
        return raw;
    }
    const size_t NS = (size_t)count_sp_r;
    std::vector<int32_t> cnt((size_t)num_walks * NS, 0);               // cnt[h][id]
#pragma omp parallel for num_threads(p.opt.threads) schedule(dynamic, 1)
    for (int32_t h = 0; h < (int32_t)num_walks; ++h) {
        int32_t *c = cnt.data() + (size_t)h * NS;
        for (int32_t id : ids[h]) if (id >= 0) c[id]++;
    }
    int64_t run = 0;
    for (size_t r = 0; r < NS; ++r) {                                  // exclusive prefix in (id, h) order
        bucket_off[r] = run;
        for (uint32_t h = 0; h < num_walks; ++h) { int32_t &c = cnt[(size_t)h * NS + r]; const int32_t n = c; c = (int32_t)(run - bucket_off[r]); run += n; }
    }
    bucket_off[NS] = run;
    raw.resize((size_t)run);
#pragma omp parallel for num_threads(p.opt.threads) schedule(dynamic, 1)
    for (int32_t h = 0; h < (int32_t)num_walks; ++h) {
        int32_t *c = cnt.data() + (size_t)h * NS;                      // now: offset of (id, h) inside bucket id
        for (size_t m = 0; m < ids[h].size(); ++m) {
            const int32_t id = ids[h][m];
            if (id >= 0) raw[(size_t)(bucket_off[id] + c[id]++)] = Raw{h, (uint32_t)m};
        }
    }
    return raw;
}

// the n occurrences raw[0 .. n) of one id, with the scratch buffers a chunk of ids re-uses
struct IdGroup {
    const std::vector<HapIndex> &kmer_index;
    const Raw *raw = nullptr;
    int32_t n = 0;
    std::string arena;                                                 // keys "v0_v1_..._" back to back (:600-603)
    std::vector<uint32_t> koff;
    std::vector<int32_t> order, grp, byhap;
    explicit IdGroup(const std::vector<HapIndex> &ix) : kmer_index(ix) {}
    std::pair<const int32_t *, uint32_t> list(int32_t t) const {       // vertex list of occurrence t
        const HapIndex &ix = kmer_index[raw[t].h];
        return {ix.v.data() + ix.voff[raw[t].m], ix.voff[raw[t].m + 1] - ix.voff[raw[t].m]};
    }
    bool same_list(int32_t x, int32_t y) const {
        const auto a = list(x), b = list(y);
        return a.second == b.second && std::equal(a.first, a.first + a.second, b.first);
    }
    std::string_view key(int32_t t) const { return std::string_view(arena.data() + koff[t], koff[t + 1] - koff[t]); }
};

// The filter (:615-622) only asks whether some vertex path occurs >= thr times; equal keys <=> equal vertex
// lists, so the lists themselves are grouped first (any order consistent with equality serves for counting).
// Most ids are dropped here -- every haplotype carries the k-mer on the same path -- without a key being built.
bool shared_by_too_many(IdGroup &g, float thr) {
    const int32_t n = g.n;
    if (!((float)n >= thr)) return false;
    int32_t same = 1;
    while (same < n && g.same_list(same, 0)) ++same;
    if (same == n) return true;                                        // the common case: one path, n >= thr occurrences
    g.order.resize(n);
    std::iota(g.order.begin(), g.order.end(), 0);
    std::sort(g.order.begin(), g.order.end(), [&](int32_t x, int32_t y) {
        const auto a = g.list(x), c2 = g.list(y);
        if (a.second != c2.second) return a.second < c2.second;
        return std::lexicographical_compare(a.first, a.first + a.second, c2.first, c2.first + c2.second);
    });
    for (int32_t i = 0; i < n;) {
        int32_t j = i + 1;
        while (j < n && g.same_list(g.order[j], g.order[i])) ++j;
        if ((float)(j - i) >= thr) return true;
        i = j;
    }
    return false;
}

void build_keys(IdGroup &g) {
    g.arena.clear();
    g.koff.assign(1, 0);
    for (int32_t t = 0; t < g.n; ++t) {
        const auto lst = g.list(t);
        for (uint32_t q = 0; q < lst.second; ++q) {
            char buf[12];
            int len = 0;
            uint32_t x = (uint32_t)lst.first[q];                       // vertex ids are non-negative
            do { buf[len++] = (char)('0' + x % 10); x /= 10; } while (x);
            while (len) g.arena += buf[--len];
            g.arena += '_';
        }
        g.koff.push_back((uint32_t)g.arena.size());
    }
}

// occurrence sort (:641-663) of id r: appends its occurrences to occs_l / vpool_l
void emit_sorted_occurrences(IdGroup &g, int32_t r, std::vector<Occ> &occs_l, std::vector<int32_t> &vpool_l) {
    const int32_t n = g.n;
    const Raw *raw = g.raw;
    build_keys(g);
    g.order.resize(n);
    std::iota(g.order.begin(), g.order.end(), 0);
    // std::map<std::string,...> iteration = lexicographic on the key; inside a key, push order
    std::stable_sort(g.order.begin(), g.order.end(), [&](int32_t x, int32_t y) { return g.key(x) < g.key(y); });
    // Anchor_hits_1[r][h] in map-iteration order, then std::sort per (r,h) (:641-663)
    g.byhap = g.order;                                                 // haplotype ascending, map-iteration order inside one
    std::stable_sort(g.byhap.begin(), g.byhap.end(), [&](int32_t x, int32_t y) { return raw[x].h < raw[y].h; });
    for (int32_t g0 = 0; g0 < n;) {
        const int32_t h = raw[g.byhap[g0]].h;
        int32_t g1 = g0;
        while (g1 < n && raw[g.byhap[g1]].h == h) ++g1;
        g.grp.assign(g.byhap.begin() + g0, g.byhap.begin() + g1);
        g0 = g1;
        const HapIndex &ix = g.kmer_index[h];
        std::sort(g.grp.begin(), g.grp.end(), [&](int32_t x, int32_t y) {
            const uint32_t mx = raw[x].m, my = raw[y].m;
            const int32_t ax0 = ix.v[ix.voff[mx]], ay0 = ix.v[ix.voff[my]];
            if (ax0 != ay0) return ax0 < ay0;
            return ix.v[ix.voff[mx + 1] - 1] < ix.v[ix.voff[my + 1] - 1];
        });
        for (int32_t x : g.grp) {
            const uint32_t m = raw[x].m;
            Occ o{r, (int32_t)h, (uint32_t)vpool_l.size(), ix.voff[m + 1] - ix.voff[m]};
            vpool_l.insert(vpool_l.end(), ix.v.begin() + ix.voff[m], ix.v.begin() + ix.voff[m + 1]);
            occs_l.push_back(o);
        }
    }
}

// ---- shared-anchor filter (:590-633) + occurrence sort (:641-663) ----
// ids are independent (the reference runs this loop under OpenMP too, :593): contiguous id chunks balanced by
// occurrence count, each with private output, to be concatenated in id order afterwards
void filter_and_sort(const Pipeline &p, const std::vector<HapIndex> &kmer_index, const std::vector<Raw> &raw, const std::vector<int64_t> &bucket_off,
                     std::vector<std::vector<Occ>> &occs_c, std::vector<std::vector<int32_t>> &vpool_c) {
    const int32_t count_sp_r = p.count_sp_r;
    const float thr = p.opt.threshold * p.num_walks;                   // float * uint32 -> float (:618)
    const int n_chunks = std::max(1, p.opt.threads * 4);
    std::vector<int32_t> chunk_lo(n_chunks + 1, count_sp_r);
    chunk_lo[0] = 0;
    for (int c = 1; c < n_chunks; ++c) {
        const int64_t want = (int64_t)raw.size() * c / n_chunks;
        chunk_lo[c] = (int32_t)(std::lower_bound(bucket_off.begin(), bucket_off.end(), want) - bucket_off.begin());
        chunk_lo[c] = std::min(std::max(chunk_lo[c], chunk_lo[c - 1]), count_sp_r);
    }
    occs_c.assign(n_chunks, {});
    vpool_c.assign(n_chunks, {});
#pragma omp parallel for num_threads(p.opt.threads) schedule(dynamic, 1)
    for (int c = 0; c < n_chunks; ++c) {
        IdGroup g(kmer_index);
        for (int32_t r = chunk_lo[c]; r < chunk_lo[c + 1]; ++r) {
            if (bucket_off[r] == bucket_off[r + 1]) continue;
            g.raw = raw.data() + bucket_off[r];
            g.n = (int32_t)(bucket_off[r + 1] - bucket_off[r]);
            if (shared_by_too_many(g, thr)) continue;                  // :624-632 id dropped entirely
            emit_sorted_occurrences(g, r, occs_c[c], vpool_c[c]);
        }
    }
}

void concatenate(Pipeline &p, const std::vector<std::vector<Occ>> &occs_c, const std::vector<std::vector<int32_t>> &vpool_c) {
    p.occs.clear(); p.vpool.clear();
    size_t no = 0, nv = 0;
    for (size_t c = 0; c < occs_c.size(); ++c) { no += occs_c[c].size(); nv += vpool_c[c].size(); }
    p.occs.reserve(no); p.vpool.reserve(nv);
    for (size_t c = 0; c < occs_c.size(); ++c) {
        const uint32_t base = (uint32_t)p.vpool.size();
        p.vpool.insert(p.vpool.end(), vpool_c[c].begin(), vpool_c[c].end());
        for (Occ o : occs_c[c]) { o.off += base; p.occs.push_back(o); }
    }
}

void host_join(Pipeline &p, const std::vector<uint64_t> &sp_hash, const std::vector<HapIndex> &kmer_index, Lap &lap) {
    std::vector<int64_t> bucket_off;
    std::vector<Raw> raw;
    {
        const std::vector<std::vector<int32_t>> ids = lookup_ids(p, sp_hash, kmer_index);
        lap("dictionary lookup");
        raw = bucket_by_id(p, ids, bucket_off);
    }
    lap("bucket by id");
    std::vector<std::vector<Occ>> occs_c;
    std::vector<std::vector<int32_t>> vpool_c;
    filter_and_sort(p, kmer_index, raw, bucket_off, occs_c, vpool_c);
    lap("filter + sort");
    concatenate(p, occs_c, vpool_c);
    lap("concatenate");
}

// The device's join / filter / sort.  needs_host: a group whose order would hinge on std::sort's unstable partitioning
// (dg_anchor.hip) -- the host algorithm decides, occs / vpool are left alone.
std::string device_join(Pipeline &p, const std::vector<uint64_t> &sp_hash, Lap &lap, bool &needs_host) {
    const Backend &be = p.be;
    dg_anchor_result ar;
    if (be.anchor_finish(be.ctx, sp_hash.data(), (int64_t)sp_hash.size(), p.opt.threshold * p.num_walks, &ar) != 0) return backend_error(be, "anchor_finish");
    lap("device join+filter");
    hint_lattice(p);
    needs_host = ar.n_unstable_groups > 0;
    if (needs_host) {
        if (!p.opt.quiet) fprintf(stderr, "[dg::anchors] %lld occurrence group(s) need the host sort; redoing the stage on the host\n", (long long)ar.n_unstable_groups);
    } else {
        p.occs.resize((size_t)ar.n_occ);
        for (int64_t i = 0; i < ar.n_occ; ++i) p.occs[i] = Occ{ar.occ_id[i], ar.occ_hap[i], ar.occ_off[i], ar.occ_len[i]};
        p.vpool.assign(ar.vpool, ar.vpool + ar.n_vtx);
    }
    for (void *q : {(void *)ar.occ_id, (void *)ar.occ_hap, (void *)ar.occ_off, (void *)ar.occ_len, (void *)ar.vpool}) if (q) be.free_buf(q);
    return "";
}

}  // namespace

// ---- multiplicity histogram, fit, classify (:745-879) ----
std::string Pipeline::start_fit(std::vector<int32_t> &sp_count) {
    std::map<int32_t, int32_t> kmer_freq;                              // :745-750
    for (int32_t c : sp_count) kmer_freq[c] += 1;
    if (spectrum_injected && !inj_hist.empty()) {                      // the ranks' all-reduced Hist_kmer must be the histogram of the counts they sent
        std::vector<int64_t> mine(inj_hist.size(), 0);
        for (auto &kv : kmer_freq) mine[std::min<size_t>((size_t)std::max(kv.first, 0), mine.size() - 1)] += kv.second;
        if (mine != inj_hist) return "injected multiplicity histogram does not match the injected counts";
    }
    std::vector<HistBin> hist;
    int max_mult = 0;
    for (auto &kv : kmer_freq) { hist.push_back({(int)kv.first, (double)kv.second}); max_mult = std::max(max_mult, (int)kv.first); }
    // The grid fit (serial in the reference, :785) needs nothing but the histogram, and nothing before the colour split of the
    // graph stage needs its result (homo_bv): it runs on a thread of its own beside the first phases of that stage
    // (wait_fit() joins it and prints its two lines).
    const int threads = std::max(1, opt.threads / 2);
    fit_sp_count.swap(sp_count);
    fit_pending = true;
    if (opt.threads > 1 && !getenv("DG_FIT_INLINE")) fit_thread = std::thread([this, hist, max_mult, threads] { fit_and_classify(hist, max_mult, threads); });
    else fit_and_classify(hist, max_mult, threads);
    return "";
}

void Pipeline::fit_and_classify(const std::vector<HistBin> &hist, int max_mult, int threads) {
    sum.fit = kg_fit(hist, /*max_copy=*/10, max_mult, threads);
    const KGParams &P = sum.fit.P;
    std::vector<int8_t> label(max_mult + 1, -1);
    homo_bv.assign(count_sp_r, 0);                                     // :830-879
    fit_n_hom = 0;
    for (int32_t id = 0; id < count_sp_r; ++id) {
        int m = fit_sp_count[id];
        if (m <= 0 || m > max_mult) continue;                          // (0: solver.cpp:845; the rest cannot come from the device path, and injected spectra are checked in dgr_inject_spectrum)
        if (label[m] < 0) label[m] = kg_is_hom(P, m) ? 1 : 0;
        homo_bv[id] = (uint8_t)label[m];
        fit_n_hom += label[m];
    }
}

// Order of the stages: the reference sketches the haplotypes first, then the reads, then joins, then fits (solver.cpp:449-887).
// Nothing in the haplotype index depends on the reads and the fit needs only the reads' multiplicity histogram, so the reads are
// sketched FIRST and the fit (0.15 s of host arithmetic on MHC-24) runs on its thread beside the haplotype index and the anchor
// join instead of in front of the graph stage.  The log lines keep the reference's order.
int Pipeline::compute_and_classify_anchors(std::string &err) {
    double t0 = now_s();
    std::vector<uint64_t> sp_hash;
    {
        std::vector<int32_t> sp_count;
        if (failed(read_spectrum(*this, sp_hash, sp_count), err)) return -1;
        count_sp_r = (int32_t)sp_hash.size();
        sum.spectrum = count_sp_r;
        stamp("compute_hashes+Sp_R", t0);
        if (failed(start_fit(sp_count), err)) return -1;
    }
    t0 = now_s();
    std::vector<HapIndex> kmer_index;
    sum.minimizers_per_hap.assign(num_walks, 0);
    double t_sketch = 0;
    const bool dev_anchors = device_anchors_offered(*this);
    if (failed(dev_anchors ? device_haplotype_index(*this, t_sketch) : host_haplotype_index(*this, kmer_index, t_sketch), err)) return -1;
    if (!opt.quiet) {
        std::cerr << "Number of Minimizers" << std::endl;              // :467-474
        for (uint32_t h = 0; h < num_walks; ++h) fprintf(stderr, "%s : %d\n", hap_id2name[h].c_str(), (int)sum.minimizers_per_hap[h]);
    }
    if (getenv("DG_DEBUG")) fprintf(stderr, "[dg::index] backend sketch calls %.3f s of %.3f s\n", t_sketch, now_s() - t0);
    stamp("index_kmers", t0);

    if (!opt.quiet) fprintf(stderr, "[M::%s] Indexed reads with spectrum size: %d\n", __func__, count_sp_r);   // :558

    t0 = now_s();
    if (!dev_anchors) hint_lattice(*this);
    Lap lap("anchors", 18);
    bool on_host = !dev_anchors;
    if (dev_anchors) {
        if (failed(device_join(*this, sp_hash, lap, on_host), err)) return -1;
        if (on_host && failed(host_haplotype_index(*this, kmer_index, t_sketch), err)) return -1;   // built now, for the first time
    }
    if (on_host) host_join(*this, sp_hash, kmer_index, lap);
    sum.anchors_per_hap.assign(num_walks, 0);
    for (auto &o : occs) sum.anchors_per_hap[o.h]++;
    if (!opt.quiet) {
        std::cerr << "Number of Anchors" << std::endl;                 // :674-685
        for (uint32_t h = 0; h < num_walks; ++h) fprintf(stderr, "%s : %d\n", hap_id2name[h].c_str(), (int)sum.anchors_per_hap[h]);
    }
    stamp("compute_anchors+filter+sort", t0);

    if (!opt.quiet) std::cout << "Classifying kmers..." << std::endl;  // :784
    return 0;
}

void Pipeline::wait_fit() {                                             // homo_bv is valid after this
    if (!fit_pending) return;
    fit_t0 = now_s();                                                  // the stage's time is what the caller waits here
    if (fit_thread.joinable()) fit_thread.join();
    fit_pending = false;
    const KGParams &P = sum.fit.P;
    if (!opt.quiet)
        fprintf(stderr, "[M::%s] Fitted model: best NLL=%.2f, u_v=%.2f (hom mean), sd_v=%.2f (hom SD), "
                "var_w=%.2f, p_d=%.2f, zp_copy=%.2f, zp_copy_het=%.2f, err_shape=%.2f, max_copy=%d\n",
                "compute_and_classify_anchors", sum.fit.nll, P.u_v, P.sd_v, P.var_w, P.p_d, P.zp_copy, P.zp_copy_het, P.err_shape, P.max_copy);
    if (!opt.quiet) {
        int64_t tot = std::max<int64_t>(1, count_sp_r);
        fprintf(stderr, "[M::%s] Phasing done. Homozygous: %.2f%%, Heterozygous: %.2f%%, Total kmers: %lld\n", "compute_and_classify_anchors",
                100.f * float(fit_n_hom) / tot, 100.f * float(count_sp_r - fit_n_hom) / tot, (long long)count_sp_r);
    }
    std::vector<int32_t>().swap(fit_sp_count);
    stamp("fit+classify (joined)", fit_t0);
}

}  // namespace dg

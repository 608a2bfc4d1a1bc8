#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <stdexcept>

#include "stage_util.hpp"

#ifdef _OPENMP
#include <omp.h>
#endif

namespace dg {

// ======================================================================================
// ExpandedGraph  (ExpandedGraph.hpp:29-102, 269-409), flat CSR restatement
// ======================================================================================
void ExpandedGraph::permute(const uvec<int32_t> &order) {
    // new vertex i = old vertex order[i]; adjacency keeps its per-vertex order (ExpandedGraph.hpp:93-101, 392-400)
    Lap lap("permute", 18);
    const int32_t nn = (int32_t)order.size();
    uvec<int32_t> new_idx(nn);
#pragma omp parallel for schedule(static)
    for (int32_t i = 0; i < nn; ++i) new_idx[order[i]] = i;
    uvec<int64_t> noff((size_t)nn + 1, 0);
#pragma omp parallel for schedule(static)
    for (int32_t i = 0; i < nn; ++i) noff[i + 1] = deg(order[i]);      // (random gathers in parallel, the running sum alone is cheap)
    for (int32_t i = 0; i < nn; ++i) noff[i + 1] += noff[i];
    lap("new_idx+noff");
    uvec<int32_t> ndst(adj_dst.size());
    uvec<uint8_t> nw(adj_w.size());
    lap("alloc");
    // the remap is a random gather (cache-miss bound): spread it over the host threads
#pragma omp parallel for schedule(static)
    for (int32_t i = 0; i < nn; ++i) {
        int64_t o = noff[i];
        for (int64_t e = adj_off[order[i]]; e < adj_off[order[i] + 1]; ++e, ++o) { ndst[o] = new_idx[adj_dst[e]]; nw[o] = adj_w[e]; }
    }
    lap("edges");
    adj_off.swap(noff); adj_dst.swap(ndst); adj_w.swap(nw);
    uvec<int32_t> nh(nn);
    uvec<uint32_t> noo(nn), nol(nn);
#pragma omp parallel for schedule(static)
    for (int32_t i = 0; i < nn; ++i) { nh[i] = haplotype[order[i]]; noo[i] = orig_off[order[i]]; nol[i] = orig_len[order[i]]; }
    haplotype.swap(nh); orig_off.swap(noo); orig_len.swap(nol);
    if ((int32_t)level.size() == nn) {
        uvec<int32_t> nl(nn);
#pragma omp parallel for schedule(static)
        for (int32_t i = 0; i < nn; ++i) nl[i] = level[order[i]];
        level.swap(nl);
    }
    lap("vertex arrays");
    uvec<int64_t> nco((size_t)nn + 1, 0);
#pragma omp parallel for schedule(static)
    for (int32_t i = 0; i < nn; ++i) nco[i + 1] = ncol(order[i]);
    for (int32_t i = 0; i < nn; ++i) nco[i + 1] += nco[i];
    uvec<int32_t> ncp(col_pool.size());
#pragma omp parallel for schedule(static)
    for (int32_t i = 0; i < nn; ++i)
        std::copy(col_pool.begin() + col_off[order[i]], col_pool.begin() + col_off[order[i] + 1], ncp.begin() + nco[i]);
    col_off.swap(nco); col_pool.swap(ncp);
    lap("colours");
}

void ExpandedGraph::topologically_reorder(int sink) {                  // ExpandedGraph.hpp:29-102
    std::vector<int32_t> indeg(n, 0);
    const int64_t n_edges = (int64_t)adj_dst.size();
    if (n_edges < ((int64_t)1 << 26)) {                                // (MHC-24: 0.105 s serial, 0.123 s with atomics; 5 Mbp x 100 walks: 1.07 -> 0.89 s)
        for (int32_t d : adj_dst) ++indeg[d];
    } else {
#pragma omp parallel for schedule(static)
        for (int64_t e = 0; e < n_edges; ++e) {
#pragma omp atomic
            ++indeg[adj_dst[e]];
        }
    }
    uvec<int32_t> order;                                               // doubles as the FIFO queue
    order.reserve(n);
    for (int32_t v = 0; v < n; ++v) if (indeg[v] == 0 && v != sink) order.push_back(v);   // never push the sink now
    bool sink_ready = (indeg[sink] == 0);
    size_t head = 0;
    while (head < order.size() || sink_ready) {
        int u;
        if (head < order.size()) u = order[head++];                    // process the queue first
        else { u = sink; sink_ready = false; order.push_back(sink); ++head; }   // queue empty -> only the sink is left
        for (int64_t e = adj_off[u]; e < adj_off[u + 1]; ++e) {
            const int v = adj_dst[e];
            if (--indeg[v] == 0) { if (v == sink) sink_ready = true; else order.push_back(v); }
        }
    }
    if ((int32_t)order.size() != n) throw std::runtime_error("Graph contains a cycle; topological order impossible");
    permute(order);
}

int ExpandedGraph::strict_bfs_levelize_and_reorder() {                 // ExpandedGraph.hpp:269-409
    Lap lap("levelize", 18);
    const int32_t n0 = n;
    if (n0 == 0) return 0;
    int source = -1;
    auto take_source = [&](int32_t v) {                                // ExpandedGraph.hpp:283-296: exactly one vertex without in-edges may have out-edges
        if (source == -1) source = v;
        else { std::cout << "Uh oh, multiple potential sources found while leveling\n"; std::exit(-1); }
    };
    // 1)-3) levels.  The reference seeds lvl with the BFS distance from the source, takes a Kahn order and relaxes
    // lvl[v] = max(lvl[v], lvl[u] + 1) along it (ExpandedGraph.hpp:300-352).  The fixed point is the longest-path distance
    // from the source whatever the seed (a vertex's BFS parent already forces lvl >= dist) and whichever topological order is
    // used; vertices without in-edges stay at 0.  After topologically_reorder every edge goes from a smaller to a larger id,
    // so the ids themselves are such an order: one pass, no queue, no BFS.  (Any other input takes the literal route.)
    std::vector<int32_t> lvl(n0, 0);
    bool sorted = true;
#pragma omp parallel for schedule(static) reduction(&& : sorted)
    for (int32_t u = 0; u < n0; ++u)
        for (int64_t e = adj_off[u]; e < adj_off[u + 1]; ++e) sorted = sorted && adj_dst[e] > u;
    if (getenv("DG_LEVELIZE_LITERAL")) sorted = false;                // (tests: the literal BFS + Kahn + relaxation route must give the same levels)
    if (sorted) {
        for (int32_t u = 0; u < n0; ++u) {
            const int32_t lu = lvl[u] + 1;
            for (int64_t e = adj_off[u]; e < adj_off[u + 1]; ++e) { int32_t &lv = lvl[adj_dst[e]]; if (lv < lu) lv = lu; }
        }
        for (int32_t v = 0; v < n0; ++v) if (lvl[v] == 0 && deg(v) > 0) take_source(v);      // level 0 <=> no in-edge
        if (source < 0) throw std::runtime_error("bad source index");
        lap("levels (one pass)");
    } else {
        std::vector<int32_t> indeg(n0, 0);
        for (int32_t d : adj_dst) ++indeg[d];
        for (int32_t v = 0; v < n0; ++v) if (indeg[v] == 0 && deg(v) > 0) take_source(v);
        if (source < 0 || source >= n0) throw std::runtime_error("bad source index");
        std::vector<int32_t> dist(n0, -1), q;                          // 1) BFS from the source
        q.reserve(n0);
        dist[source] = 0; q.push_back(source);
        for (size_t h = 0; h < q.size(); ++h) {
            const int u = q[h];
            for (int64_t e = adj_off[u]; e < adj_off[u + 1]; ++e) { const int v = adj_dst[e]; if (dist[v] == -1) { dist[v] = dist[u] + 1; q.push_back(v); } }
        }
        lap("indeg+bfs");
        std::vector<int32_t> topo;                                     // 2) Kahn over ALL indeg-0 vertices
        topo.reserve(n0);
        for (int32_t v = 0; v < n0; ++v) if (indeg[v] == 0) topo.push_back(v);
        for (size_t h = 0; h < topo.size(); ++h) {
            const int u = topo[h];
            for (int64_t e = adj_off[u]; e < adj_off[u + 1]; ++e) if (--indeg[adj_dst[e]] == 0) topo.push_back(adj_dst[e]);
        }
        if ((int32_t)topo.size() != n0) throw std::runtime_error("Graph contains a cycle; strict leveling requires a DAG");
        for (int32_t v = 0; v < n0; ++v) if (dist[v] >= 0) lvl[v] = dist[v];         // 3) seed / relax
        for (int u : topo) for (int64_t e = adj_off[u]; e < adj_off[u + 1]; ++e) { const int v = adj_dst[e]; if (lvl[v] <= lvl[u]) lvl[v] = lvl[u] + 1; }
    }

    lap("kahn+relax");
    // 4) dummies for skipped levels: edge (u,v,w) with gap g becomes u -w-> d1 -0-> ... -0-> dg -0-> v; dummy ids are
    //    handed out in (u ascending, edge order) sequence (prefix sum, so vertices can be processed in parallel), each
    //    inherits haplotype[u] and u's original-vertex list.
    std::vector<int64_t> dbase((size_t)n0 + 1, 0);                     // dummies created before vertex u's edges
#pragma omp parallel for schedule(static)
    for (int32_t u = 0; u < n0; ++u) {
        int64_t c = 0;
        for (int64_t e = adj_off[u]; e < adj_off[u + 1]; ++e) { const int gap = lvl[adj_dst[e]] - lvl[u] - 1; if (gap > 0) c += gap; }
        dbase[u + 1] = c;
    }
    for (int32_t u = 0; u < n0; ++u) dbase[u + 1] += dbase[u];
    const int64_t n_dummy = dbase[n0];
    const int64_t n1l = (int64_t)n0 + n_dummy;
    if (n1l >= INT32_MAX) throw std::runtime_error("expanded graph too large");
    const int32_t n1 = (int32_t)n1l;
    uvec<int32_t> lv(n1), hp2(n1);
    uvec<uint32_t> oo(n1), ol(n1);
    uvec<int64_t> noff((size_t)n1 + 1, 0);
    uvec<int32_t> ndst((size_t)adj_dst.size() + (size_t)n_dummy);
    uvec<uint8_t> nw(ndst.size());
    // old vertices keep their out-degree and edge slots; dummy d (id n0 + d) owns the single slot E + d
    const int64_t E0 = (int64_t)adj_dst.size();
#pragma omp parallel for schedule(static)
    for (int32_t u = 0; u <= n0; ++u) noff[u] = adj_off[u];
#pragma omp parallel for schedule(static)
    for (int32_t d = n0 + 1; d <= n1; ++d) noff[d] = E0 + (d - n0);
#pragma omp parallel for schedule(static)
    for (int32_t u = 0; u < n0; ++u) {
        lv[u] = lvl[u]; hp2[u] = haplotype[u]; oo[u] = orig_off[u]; ol[u] = orig_len[u];
        int32_t next_dummy = n0 + (int32_t)dbase[u];
        for (int64_t e = adj_off[u]; e < adj_off[u + 1]; ++e) {
            const int v = adj_dst[e], w = adj_w[e];
            const int gap = lvl[v] - lvl[u] - 1;
            if (gap <= 0) { ndst[e] = v; nw[e] = (uint8_t)w; continue; }
            int64_t slot = e;                                           // where the next hop is written
            for (int step = 1; step <= gap; ++step) {
                const int32_t dmy = next_dummy++;
                lv[dmy] = lvl[u] + step; hp2[dmy] = haplotype[u]; oo[dmy] = orig_off[u]; ol[dmy] = orig_len[u];
                ndst[slot] = dmy; nw[slot] = (uint8_t)(step == 1 ? w : 0);
                slot = E0 + (dmy - n0);
            }
            ndst[slot] = v; nw[slot] = 0;
        }
    }
    adj_off.swap(noff); adj_dst.swap(ndst); adj_w.swap(nw);
    haplotype.swap(hp2); orig_off.swap(oo); orig_len.swap(ol); level.swap(lv);
    {
        uvec<int64_t> nco((size_t)n1 + 1);                             // dummies have no colour
        for (int32_t v = 0; v <= n0; ++v) nco[v] = col_off[v];
        for (int32_t v = n0 + 1; v <= n1; ++v) nco[v] = col_off[n0];
        col_off.swap(nco);
    }
    n = n1;

    lap("dummies");
    // 5) order by (level, id): stable, so a counting sort by level -- in parallel: every thread owns a contiguous range of ids,
    //    counts its vertices per level, and scatters them behind the counts of the threads before it
    int max_level = 0;
#pragma omp parallel for schedule(static) reduction(max : max_level)
    for (int32_t v = 0; v < n1; ++v) if (level[v] > max_level) max_level = level[v];
    const int NT = std::max(1, std::min(omp_get_max_threads(), 32));
    const size_t NL = (size_t)max_level + 1;
    std::vector<int32_t> hist((size_t)NT * NL, 0);
    auto v_lo = [&](int t) { return (int32_t)((int64_t)n1 * t / NT); };
#pragma omp parallel for num_threads(NT) schedule(static, 1)
    for (int t = 0; t < NT; ++t) {
        int32_t *h = hist.data() + (size_t)t * NL;
        for (int32_t v = v_lo(t); v < v_lo(t + 1); ++v) ++h[level[v]];
    }
    level_off.assign(max_level + 2, 0);
    int max_width = 0;
    for (size_t l = 0; l < NL; ++l) {                                   // per level: width, and each thread's first slot
        int32_t run = level_off[l];
        for (int t = 0; t < NT; ++t) { const int32_t c = hist[(size_t)t * NL + l]; hist[(size_t)t * NL + l] = run; run += c; }
        level_off[l + 1] = run;
        max_width = std::max(max_width, run - level_off[l]);
    }
    uvec<int32_t> order(n1);
#pragma omp parallel for num_threads(NT) schedule(static, 1)
    for (int t = 0; t < NT; ++t) {
        int32_t *fill = hist.data() + (size_t)t * NL;
        for (int32_t v = v_lo(t); v < v_lo(t + 1); ++v) order[fill[level[v]]++] = v;
    }
    lap("sort");
    permute(order);
    lap("permute");
    return max_width;
}

// ======================================================================================
// DpGraphStorage
// ======================================================================================
dg_dp_graph DpGraphStorage::view(int R) const {
    dg_dp_graph g;
    g.n_vertices = (int32_t)(out_off.size() - 1);
    g.n_levels = (int32_t)(level_off.size() - 1);
    g.R = R;
    g.level_off = level_off.data();
    g.out_off = out_off.data(); g.out_dst = out_dst.data(); g.out_w = out_w.data();
    g.hom_off = hom_off.data(); g.het_off = het_off.data();
    g.hom_col = hom_col.data(); g.het_col = het_col.data();
    return g;
}

namespace {
template <class V> void wr(std::ofstream &f, const V &v) {
    using T = typename V::value_type;
    uint64_t n = v.size();
    f.write((const char *)&n, 8);
    f.write((const char *)v.data(), (std::streamsize)(n * sizeof(T)));
}
template <class V> bool rd(std::ifstream &f, V &v) {
    using T = typename V::value_type;
    uint64_t n = 0;
    if (!f.read((char *)&n, 8)) return false;
    v.resize(n);
    return (bool)f.read((char *)v.data(), (std::streamsize)(n * sizeof(T)));
}
}  // namespace

// file = "DGDP0001" | int32 R | 8 length-prefixed arrays (level_off,out_off,out_dst,out_w,hom_off,hom_col,het_off,het_col)
bool DpGraphStorage::save(const std::string &path, int R) const {
    std::ofstream f(path, std::ios::binary);
    if (!f) return false;
    f.write("DGDP0001", 8);
    int32_t r = R;
    f.write((const char *)&r, 4);
    wr(f, level_off); wr(f, out_off); wr(f, out_dst); wr(f, out_w);
    wr(f, hom_off); wr(f, hom_col); wr(f, het_off); wr(f, het_col);
    return (bool)f;
}
bool DpGraphStorage::load(const std::string &path, int &R) {
    std::ifstream f(path, std::ios::binary);
    char magic[8];
    if (!f || !f.read(magic, 8) || memcmp(magic, "DGDP0001", 8) != 0) return false;
    int32_t r;
    if (!f.read((char *)&r, 4)) return false;
    R = r;
    return rd(f, level_off) && rd(f, out_off) && rd(f, out_dst) && rd(f, out_w) &&
           rd(f, hom_off) && rd(f, hom_col) && rd(f, het_off) && rd(f, het_col);
}

}  // namespace dg

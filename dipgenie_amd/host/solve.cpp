// ======================================================================================
// Approximator::solve  (approximator.cpp:1014-1331)
// ======================================================================================
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <fstream>
#include <iostream>

#include "stage_util.hpp"

namespace dg {

namespace {

using AnchorsByHap = std::vector<std::vector<AnchorRec>>;
using ColourPairs = std::vector<std::pair<int32_t, int32_t>>;         // (nodeID, colour)

// The literal graph construction (:1017-1246), one method per phase.  Adjacency is recorded as one global push log;
// a stable counting sort by source gives the CSR with the reference's per-vertex push order (chain edge, weight-1
// edges, start->super edges, overlap edges).
struct LiteralBuild {
    struct ELog { int32_t src, dst; uint8_t w; };
    const Pipeline &p;
    ExpandedGraph &g;
    const int H;
    int32_t number_of_vertices = 0;                                    // chain vertices
    int32_t nvert = 0, sink = 0;
    std::vector<ELog> elog;
    std::vector<int32_t> v2e;                                          // vertex_to_expanded_map[v][h]  (:1023)

    LiteralBuild(const Pipeline &p_, ExpandedGraph &g_) : p(p_), g(g_), H((int)p_.paths.size()) {
        for (size_t h = 0; h < p.paths.size(); h++) number_of_vertices += (int32_t)p.paths[h].size();
        elog.reserve((size_t)number_of_vertices * 2 + 1024);
        nvert = 2 + number_of_vertices;                                // :1022
        sink = nvert - 1;
        g.haplotype.assign(nvert, 0);                                  // :1025 (source and sink keep 0)
        g.orig_off.assign(nvert, 0);
        g.orig_len.assign(nvert, 0);
        g.orig_pool.reserve((size_t)number_of_vertices + p.vpool.size());
        v2e.assign((size_t)p.n_vtx * H, -1);
    }

    void chains() {                                                    // :1029-1049
        const auto &paths = p.paths;
        int32_t current_vertex = 1;
        for (int h = 0; h < H; h++) {
            elog.push_back({0, current_vertex, 0});
            for (size_t i = 0; i < paths[h].size(); i++) {
                v2e[(size_t)paths[h][i] * H + h] = current_vertex;     // last occurrence wins (:1035)
                g.orig_off[current_vertex] = (uint32_t)g.orig_pool.size();
                g.orig_len[current_vertex] = 1;
                g.orig_pool.push_back((int32_t)paths[h][i]);
                g.haplotype[current_vertex] = h;
                if (i < paths[h].size() - 1) elog.push_back({current_vertex, current_vertex + 1, 0});
                else elog.push_back({current_vertex, sink, 0});
                current_vertex++;
            }
        }
    }

    void recombination_edges() {                                       // :1051-1095
        const auto &paths = p.paths;
        const auto &adj_list = p.adj_list;
        std::vector<int64_t> wslot_off((size_t)p.n_vtx + 1, 0);        // vertex_w_uv[u][j] flattened
        for (size_t u = 0; u < adj_list.size(); u++) wslot_off[u + 1] = wslot_off[u] + (int64_t)adj_list[u].size();
        std::vector<int32_t> vertex_w_uv((size_t)wslot_off[p.n_vtx], -1);
        std::vector<uint8_t> w_filled;                                 // "adjacency of w_uv is non-empty" (:1082)
        for (int h = 0; h < H; h++) {
            for (size_t i = 0; i < paths[h].size(); i++) {
                const int u = (int)paths[h][i];
                for (size_t j = 0; j < adj_list[u].size(); j++) {
                    const int v = (int)adj_list[u][j];
                    if (!(i == paths[h].size() - 1 || v != (int)paths[h][i + 1])) continue;
                    int32_t &wv = vertex_w_uv[wslot_off[u] + (int64_t)j];
                    if (wv == -1) {
                        wv = nvert++;
                        g.haplotype.push_back(-1);
                        g.orig_off.push_back(0);
                        g.orig_len.push_back(0);
                        w_filled.push_back(0);
                    }
                    elog.push_back({v2e[(size_t)u * H + h], wv, 1});
                    uint8_t &filled = w_filled[wv - (number_of_vertices + 2)];
                    if (!filled)
                        for (int hh = 0; hh < H; ++hh) {
                            const int32_t v_e = v2e[(size_t)v * H + hh];
                            if (v_e >= 0) { elog.push_back({wv, v_e, 0}); filled = 1; }
                        }
                }
            }
        }
    }

    // anchors -> AnchorRec per haplotype (:1114-1176); returns the number of colours
    int anchor_records(AnchorsByHap &anchorsByHap, std::vector<int32_t> &color_to_anchor) {
        const auto &occs = p.occs;
        const auto &vpool = p.vpool;
        int nextID = nvert;
        int colourID = 0;
        std::vector<size_t> cnt(H, 0);
        for (const Occ &o : occs) cnt[o.h]++;
        for (int h = 0; h < H; ++h) anchorsByHap[h].reserve(cnt[h]);
        size_t q = 0;
        while (q < occs.size()) {                                      // ids without occurrences use no colour
            const int32_t a = occs[q].a;
            for (; q < occs.size() && occs[q].a == a; ++q) {           // occs sorted by (a, h, occurrence order)
                const Occ &o = occs[q];
                const int h = o.h;
                const int startOrig = vpool[o.off], endOrig = vpool[o.off + o.len - 1];
                const int startExp = v2e[(size_t)startOrig * H + h], endExp = v2e[(size_t)endOrig * H + h];
                int nodeID;
                if (startExp == endExp) {
                    nodeID = startExp;
                } else {
                    elog.push_back({startExp, nextID, 0});             // :1148
                    elog.push_back({nextID, endExp, 0});               // :1149
                    g.orig_off.push_back((uint32_t)g.orig_pool.size());
                    g.orig_len.push_back(o.len);
                    g.orig_pool.insert(g.orig_pool.end(), vpool.begin() + o.off, vpool.begin() + o.off + o.len);
                    g.haplotype.push_back(-1);
                    nodeID = nextID++;
                }
                anchorsByHap[h].push_back({startOrig, endOrig, startExp, endExp, {colourID}, nodeID});
            }
            color_to_anchor.push_back(a);
            colourID++;
        }
        nvert = nextID;
        { std::vector<int32_t>().swap(v2e); }
        return colourID;
    }

    // per-haplotype sweep: overlap edges + containment colour propagation (:1193-1246)
    // Haplotypes are independent here (anchor records, node ids and stacks are per haplotype); the overlap edges
    // each one produces are appended to the push log afterwards in haplotype order, as the serial loop would.
    static void sweep_haplotype(std::vector<AnchorRec> &vec, std::vector<ELog> &overlap, ColourPairs &cp) {
        if (vec.empty()) return;
        std::sort(vec.begin(), vec.end(), [](const AnchorRec &a, const AnchorRec &b) {
            if (a.startExp != b.startExp) return a.startExp < b.startExp;
            else return a.endExp < b.endExp;
        });
        std::vector<AnchorRec *> stk;
        for (auto &anc : vec) {
            while (!stk.empty() && stk.back()->endExp < anc.startExp) stk.pop_back();
            if (!stk.empty() && anc.startExp <= stk.back()->endExp && stk.back()->nodeID != anc.nodeID)
                overlap.push_back({stk.back()->nodeID, anc.nodeID, 0});
            for (int i = (int)stk.size() - 1; i >= 0; --i) {
                if (anc.endExp <= stk[i]->endExp) {
                    for (int c : anc.colours)
                        if (std::find(stk[i]->colours.begin(), stk[i]->colours.end(), c) == stk[i]->colours.end())
                            stk[i]->colours.push_back(c);
                } else break;
            }
            stk.push_back(&anc);
        }
        for (const auto &anc : vec)                                    // :1240-1245: per node, sorted-unique union
            for (int c : anc.colours) cp.emplace_back(anc.nodeID, c);
        std::sort(cp.begin(), cp.end());
        cp.erase(std::unique(cp.begin(), cp.end()), cp.end());
    }

    ColourPairs sweep(AnchorsByHap &anchorsByHap, Lap &lap) {
        std::vector<std::vector<ELog>> ov_edges(anchorsByHap.size());
        std::vector<ColourPairs> colpairs_h(anchorsByHap.size());
#pragma omp parallel for schedule(dynamic, 1)
        for (int64_t h = 0; h < (int64_t)anchorsByHap.size(); ++h) sweep_haplotype(anchorsByHap[h], ov_edges[h], colpairs_h[h]);
        lap("sweep");
        for (auto &ve : ov_edges) elog.insert(elog.end(), ve.begin(), ve.end());
        { std::vector<std::vector<ELog>>().swap(ov_edges); }
        // node ids of different haplotypes are disjoint, so the per-haplotype sorted lists only need a count + scatter
        ColourPairs colpairs;
        size_t tot = 0;
        for (auto &cp : colpairs_h) tot += cp.size();
        colpairs.reserve(tot);
        for (auto &cp : colpairs_h) colpairs.insert(colpairs.end(), cp.begin(), cp.end());
        return colpairs;
    }

    void assemble(const ColourPairs &colpairs) {                       // the flat graph
        g.n = nvert;
        g.adj_off.assign((size_t)nvert + 1, 0);
        for (const ELog &e : elog) g.adj_off[e.src + 1]++;
        for (int32_t v = 0; v < nvert; ++v) g.adj_off[v + 1] += g.adj_off[v];
        g.adj_dst.resize(elog.size());
        g.adj_w.resize(elog.size());
        {
            // stable scatter by source, in parallel: every thread owns a contiguous range of sources (balanced by edge
            // count) and reads the whole push log in order, so a vertex keeps its push order as in the serial loop
            std::vector<int64_t> fill(g.adj_off.begin(), g.adj_off.end() - 1);
            const int T = std::max(1, std::min(p.opt.threads, 32));
            std::vector<int32_t> cut(T + 1, nvert);
            cut[0] = 0;
            for (int t = 1; t < T; ++t) {
                const int64_t want = (int64_t)elog.size() * t / T;
                cut[t] = (int32_t)(std::lower_bound(g.adj_off.begin(), g.adj_off.end(), want) - g.adj_off.begin());
                cut[t] = std::min(std::max(cut[t], cut[t - 1]), nvert);
            }
#pragma omp parallel for num_threads(T) schedule(static, 1)
            for (int t = 0; t < T; ++t) {
                const int32_t lo = cut[t], hi = cut[t + 1];
                if (lo >= hi) continue;
                for (const ELog &e : elog)
                    if (e.src >= lo && e.src < hi) { const int64_t o = fill[e.src]++; g.adj_dst[o] = e.dst; g.adj_w[o] = e.w; }
            }
        }
        { std::vector<ELog>().swap(elog); }
        g.col_off.assign((size_t)nvert + 1, 0);
        for (auto &pc : colpairs) g.col_off[pc.first + 1]++;
        for (int32_t v = 0; v < nvert; ++v) g.col_off[v + 1] += g.col_off[v];
        g.col_pool.resize(colpairs.size());
        std::vector<int64_t> fill(g.col_off.begin(), g.col_off.end() - 1);
        for (auto &pc : colpairs) g.col_pool[fill[pc.first]++] = pc.second;   // a node's colours arrive ascending
    }
};

// g, anchorsByHap and color_to_anchor (colour -> read-minimizer id) as the reference builds them; returns the sink
int build_literal_graph(Pipeline &p, ExpandedGraph &g, AnchorsByHap &anchorsByHap, std::vector<int32_t> &color_to_anchor) {
    Lap lap("build", 18);
    LiteralBuild b(p, g);
    b.chains();
    lap("chains");
    b.recombination_edges();
    lap("recomb edges");
    anchorsByHap.assign(p.paths.size(), {});
    p.sum.n_colours = b.anchor_records(anchorsByHap, color_to_anchor);
    lap("anchor recs");
    const ColourPairs colpairs = b.sweep(anchorsByHap, lap);
    b.assemble(colpairs);
    lap("assemble");
    return b.sink;
}

std::string write_haploid_fasta(Pipeline &p, const std::vector<int> &dp_path) {   // :1260-1278
    std::string out;
    for (auto u : dp_path) out += p.node_seq[u];
    std::ofstream f(p.opt.hap_file, std::ios::out);
    if (!f.is_open()) return "cannot open output file " + p.opt.hap_file;
    f << ">" << "dp_sol" << " LN:" << out.size() << std::endl;
    for (size_t i = 0; i < out.size(); i += 80) f << out.substr(i, 80) << std::endl;
    f.close();
    if (!f.good()) return "write to " + p.opt.hap_file + " failed";
    p.sum.len1 = (int64_t)out.size();
    return "";
}

}  // namespace

int Pipeline::solve(std::string &err) {
    double t0 = now_s();
    if (opt.ploidy == 2 && !getenv("DG_GRAPH_LITERAL")) {
        bool declined = false;
        const int rc = solve_fused(t0, declined, err);
        if (!declined) return rc;
        t0 = now_s();
    } else {
        wait_fit();
    }
    return solve_literal(t0, err);
}

// the fused route (fast_graph.cpp) covers everything up to the levelized graph; it declines inputs it does not model
// (empty walks, several sources, a vertex deeper than the sink ...), which then take the literal route
// (heap objects: a process that is about to exit -- the CLI -- skips their teardown, ~0.07 s of munmap and 2 x 10^6 small
// destructors on MHC-24; Options::leak_at_exit)
int Pipeline::solve_fused(double t0, bool &declined, std::string &err) {
    ExpandedGraph *gf = new ExpandedGraph();
    auto *anchorsByHapF = new std::vector<std::vector<AnchorRec>>();
    std::vector<uint8_t> color_homo_bv_f;
    declined = !build_levelized_fast(*gf, *anchorsByHapF, color_homo_bv_f);
    if (declined) {
        delete gf; delete anchorsByHapF;
        wait_fit();
        sum.n_colours = 0;
        return 0;
    }
    stamp("levelized_graph_build", t0);
    const int rc = diploid(*gf, color_homo_bv_f, *anchorsByHapF, err);
    if (!opt.leak_at_exit) { delete gf; delete anchorsByHapF; }
    if (rc != 0) return rc;
    if (!opt.quiet) std::cout << "Diploid sequences written to: " << opt.hap_file << std::endl;   // :1330
    return 0;
}

int Pipeline::solve_literal(double t0, std::string &err) {
    ExpandedGraph g;
    std::vector<std::vector<AnchorRec>> anchorsByHap;
    std::vector<int32_t> color_to_anchor;
    const int sink = build_literal_graph(*this, g, anchorsByHap, color_to_anchor);
    stamp("expanded_graph_build", t0);
    t0 = now_s();
    g.topologically_reorder(sink);                                     // :1256
    stamp("topologically_reorder", t0);

    if (opt.ploidy == 1) {                                             // :1260-1278
        t0 = now_s();
        std::vector<int> dp_path = haploid_dp(g, opt.R, err);
        if (!err.empty()) return -1;
        if (failed(write_haploid_fasta(*this, dp_path), err)) return -1;
        stamp("haploid_dp+write", t0);
    } else {
        const int n_colours = (int)sum.n_colours;
        std::vector<uint8_t> color_homo_bv(n_colours, 0);              // :1283-1290
        for (int c = 0; c < n_colours; ++c) if (homo_bv[color_to_anchor[c]]) color_homo_bv[c] = 1;
        t0 = now_s();
        g.strict_bfs_levelize_and_reorder();                           // :1302
        stamp("strict_levelize", t0);
        int rc = diploid(g, color_homo_bv, anchorsByHap, err);
        if (rc != 0) return rc;
    }
    if (!opt.quiet) std::cout << "Diploid sequences written to: " << opt.hap_file << std::endl;   // :1330
    return 0;
}

}  // namespace dg

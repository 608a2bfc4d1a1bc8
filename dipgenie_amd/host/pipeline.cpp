#include "pipeline.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <limits>
#include <mutex>
#include <numeric>

#include "seq_reader.hpp"

#ifdef _OPENMP
#include <omp.h>
#endif

namespace dg {

double now_s() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

void Pipeline::stamp(const char *name, double t0) {
    double dt = now_s() - t0;
    static std::mutex mu;                                              // (the sharded CLI reads the GFA and the reads on two threads)
    std::lock_guard<std::mutex> lk(mu);
    sum.stage_s.emplace_back(name, dt);
    if (!opt.quiet) fprintf(stderr, "[dg::stage] %-28s %.3f s\n", name, dt);
}

// ======================================================================================
// Solver::read_gfa  (solver.cpp:27-227)
// ======================================================================================
void Pipeline::read_gfa_from(const GfaGraph &g) {
    // graph: one vertex per segment, forward-strand arcs only (:60-91); walks -> paths, named sample.hap (:108-125)
    n_vtx = g.n_seg();
    node_seq.assign(g.seg_seq.begin(), g.seg_seq.end());
    if (!opt.site_margins.empty() || !opt.genotype_margins.empty() || !opt.genotype_table.empty() || !opt.budget_genotype_margins.empty() || !opt.phase_margins.empty() || !opt.budget_phase_margins.empty() || !opt.recombination_margins.empty() || !opt.budget_recombination_margins.empty()) node_name.assign(g.seg_name.begin(), g.seg_name.end());
    adj_list.assign(n_vtx, {});
    for (uint32_t seg = 0; seg < n_vtx; ++seg)
        for (uint32_t arc : g.arcs[(size_t)2 * seg]) adj_list[seg].push_back(arc >> 1);
    num_walks = (uint32_t)g.walks.size();
    paths.assign(num_walks, {});
    hap_id2name.assign(num_walks, std::string());
    for (uint32_t w = 0; w < num_walks; ++w) {
        hap_id2name[w] = g.walks[w].sample + "." + std::to_string(g.walks[w].hap);
        paths[w].reserve(g.walks[w].v.size());
        for (uint32_t oriented : g.walks[w].v) {
            if (oriented & 1) exit(1);                                 // a reverse-strand step ends the run silently (:116-119)
            paths[w].push_back(oriented >> 1);
        }
    }
    // MSA-like column of every vertex (:127-171): seeded with the earliest step index at which any walk visits it
    // (vertices on no walk are parked one column past the largest seed), then raised until column[next] > column[prev]
    // holds along every walk.  The least such assignment is a longest-path labelling of the walk-step graph: one pass
    // in topological order when that graph is acyclic; otherwise the reference's sweep-until-stable loop, cap included.
    const int32_t nv = (int32_t)n_vtx;
    constexpr int64_t UNSEEN = std::numeric_limits<int64_t>::max() / 4;
    std::vector<int64_t> column(nv, UNSEEN);
    for (const auto &walk : paths)
        for (size_t step = 0; step < walk.size(); ++step) column[walk[step]] = std::min(column[walk[step]], (int64_t)step);
    {
        int64_t last_seed = -1;
        for (int64_t c : column) if (c != UNSEEN) last_seed = std::max(last_seed, c);
        for (int64_t &c : column) if (c == UNSEEN) c = last_seed + 1;
    }
    bool labelled = false;
    {
        std::vector<int64_t> succ_off((size_t)nv + 1, 0);
        for (const auto &walk : paths) for (size_t t = 1; t < walk.size(); ++t) succ_off[walk[t - 1] + 1]++;
        for (int32_t v = 0; v < nv; ++v) succ_off[v + 1] += succ_off[v];
        std::vector<int32_t> succ((size_t)succ_off[nv]), pending(nv, 0), order;
        std::vector<int64_t> cursor(succ_off.begin(), succ_off.end() - 1);
        for (const auto &walk : paths)
            for (size_t t = 1; t < walk.size(); ++t) { succ[cursor[walk[t - 1]]++] = (int32_t)walk[t]; pending[walk[t]]++; }
        order.reserve(nv);
        for (int32_t v = 0; v < nv; ++v) if (!pending[v]) order.push_back(v);
        std::vector<int64_t> raised(column);
        for (size_t at = 0; at < order.size(); ++at) {
            const int32_t u = order[at];
            for (int64_t e = succ_off[u]; e < succ_off[u + 1]; ++e) {
                raised[succ[e]] = std::max(raised[succ[e]], raised[u] + 1);
                if (--pending[succ[e]] == 0) order.push_back(succ[e]);
            }
        }
        if ((int32_t)order.size() == nv) { column.swap(raised); labelled = true; }
    }
    for (int sweep = 0, cap = std::max(10, nv); !labelled && sweep < cap; ++sweep) {   // cyclic step graph (:158-171)
        labelled = true;
        for (const auto &walk : paths)
            for (size_t t = 1; t < walk.size(); ++t)
                if (column[walk[t]] <= column[walk[t - 1]]) { column[walk[t]] = column[walk[t - 1]] + 1; labelled = false; }
    }
    // top_order_map (:174-199) = rank of the vertex in (column, id) order; adjacency lists (:216-223) sorted by (dense
    // column rank, id).  Both are total orders, so one 64-bit key per vertex serves either sort.
    std::vector<int32_t> by_column(nv);
    std::iota(by_column.begin(), by_column.end(), 0);
    std::stable_sort(by_column.begin(), by_column.end(), [&](int32_t x, int32_t y) { return column[x] < column[y]; });   // ids ascending inside a column
    top_order_map.assign(nv, -1);
    std::vector<uint64_t> sort_key(nv);
    int64_t n_columns = -1, last_column = std::numeric_limits<int64_t>::min();
    for (int32_t rank = 0; rank < nv; ++rank) {
        const int32_t v = by_column[rank];
        top_order_map[v] = rank;
        if (column[v] != last_column) { ++n_columns; last_column = column[v]; }
        sort_key[v] = ((uint64_t)n_columns << 32) | (uint32_t)v;
    }
    for (auto &targets : adj_list)
        std::sort(targets.begin(), targets.end(), [&](uint32_t x, uint32_t y) { return sort_key[x] < sort_key[y]; });
}

int Pipeline::load_graph(std::string &err) {
    double t0 = now_s();
    GfaGraph g;
    if (!read_gfa_file(opt.gfa_file, g, err)) return -1;
    const double t1 = now_s();
    read_gfa_from(g);
    if (getenv("DG_DEBUG")) fprintf(stderr, "[dg::gfa] file %.3f s, read_gfa (adjacency, paths, column order) %.3f s\n", t1 - t0, now_s() - t1);
    stamp("gfa_read+read_gfa", t0);
    return 0;
}

int Pipeline::load_reads(std::string &err) {                           // solver.cpp:230-245
    double t0 = now_s();
    reads.clear();
    if (!read_sequences(opt.reads_file, reads, err)) return -1;
    stamp("read_ip_reads", t0);
    return 0;
}


// "id hap v0,v1,..." per occurrence in Anchor_hits order (id asc, hap asc, occurrence order), then "homo id" per set bit of
// homo_bv: the format oracle/ref_harness.cpp dumps from the reference's own Solver object (tests/golden/anchors.json)
bool Pipeline::dump_anchors(const std::string &path) const {
    FILE *f = fopen(path.c_str(), "w");
    if (!f) return false;
    for (const Occ &o : occs) {
        fprintf(f, "%d %d ", o.a, o.h);
        for (uint32_t q = 0; q < o.len; ++q) fprintf(f, "%s%d", q ? "," : "", vpool[o.off + q]);
        fputc('\n', f);
    }
    for (size_t id = 0; id < homo_bv.size(); ++id) if (homo_bv[id]) fprintf(f, "homo %zu\n", id);
    return fclose(f) == 0;
}

void Pipeline::clamp_threads() {
    opt.threads = std::max(1, opt.threads);
#ifdef _OPENMP
    omp_set_num_threads(opt.threads);
#endif
}

int Pipeline::run(std::string &err) {                                  // main.cpp:117-165
    sum = Summary();
    clamp_threads();
    t_run0 = now_s();
    // the reads file is parsed on a thread of its own beside the GFA (neither needs the other)
    std::thread reads_thread;
    std::string reads_err;
    int reads_rc = 0;
    double reads_dt = 0;
    const bool want_reads = !spectrum_injected && (opt.ploidy == 1 || opt.ploidy == 2);
    if (want_reads) reads_thread = std::thread([&] { const double t = now_s(); reads.clear(); reads_rc = read_sequences(opt.reads_file, reads, reads_err) ? 0 : -1; reads_dt = now_s() - t; });
    const int grc = load_graph(err);
    if (reads_thread.joinable()) reads_thread.join();
    if (grc) return -1;
    if (want_reads) {
        if (reads_rc) { err = reads_err; return -1; }
        sum.stage_s.emplace_back("read_ip_reads (beside the GFA)", reads_dt);
        if (!opt.quiet) fprintf(stderr, "[dg::stage] %-28s %.3f s\n", "read_ip_reads (beside GFA)", reads_dt);
        reads_loaded = true;
    }
    return run_loaded(err);
}

HapAssembly Pipeline::assemble_haplotype(uint32_t h, bool with_sequence) const {
    const std::vector<uint32_t> &walk = paths.at(h);
    HapAssembly a;
    a.step_start.assign(walk.size() + 1, 0);
    for (size_t i = 0; i < walk.size(); ++i) { a.step_start[i] = (int64_t)a.total; a.total += node_seq[walk[i]].size(); }
    a.step_start[walk.size()] = (int64_t)a.total;
    if (with_sequence) {                                               // solver.cpp:283-288
        a.seq.reserve(a.total);
        for (uint32_t v : walk) a.seq += node_seq[v];
    }
    return a;
}

std::string Pipeline::haplotype_sequence(uint32_t h) const { return assemble_haplotype(h, true).seq; }

int Pipeline::run_loaded(std::string &err) {                           // main.cpp:163-165
    clamp_threads();
    const double t0 = t_run0 > 0 ? t_run0 : now_s();
    if (opt.ploidy != 1 && opt.ploidy != 2) {
        std::cout << "Current approximator support is only for ploidy = 1 or ploidy = 2" << std::endl;
        return 0;
    }
    if (!spectrum_injected && !reads_loaded && load_reads(err)) return -1;
    if (compute_and_classify_anchors(err)) return -1;
    if (!opt.anchor_dump.empty()) {
        wait_fit();
        if (!dump_anchors(opt.anchor_dump)) { err = "cannot write " + opt.anchor_dump; return -1; }
        if (opt.dump_only && opt.dump_prefix.empty()) { err = "dump_only"; return -1; }
    }
    if (solve(err)) return -1;
    sum.stage_s.emplace_back("total", now_s() - t0);
    return 0;
}

}  // namespace dg

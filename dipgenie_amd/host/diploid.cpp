// ======================================================================================
// diploid_dp_approximation_solver minus the level loop  (approximator.cpp:362-453, 720-1011)
// ======================================================================================
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <iterator>
#include <queue>
#include <stdexcept>
#include <unordered_map>
#include <unordered_set>

#include "stage_util.hpp"

namespace dg {

namespace {

using AnchorsByHap = std::vector<std::vector<AnchorRec>>;
using EdgeList = std::vector<std::pair<int, int>>;                     // the weight-1 edges of one path, source to sink

// One chain's answer: the dg_dp_result and the four edge arrays (cap entries each) it points into.
struct ChainAnswer {
    dg_dp_result res;
    std::vector<int32_t> p1_from, p1_to, p2_from, p2_to;
    explicit ChainAnswer(int cap) : p1_from(cap), p1_to(cap), p2_from(cap), p2_to(cap) {
        memset(&res, 0, sizeof(res));
        res.p1_from = p1_from.data(); res.p1_to = p1_to.data(); res.p2_from = p2_from.data(); res.p2_to = p2_to.data();
        res.cap = cap;
    }
    ChainAnswer(ChainAnswer &&) = default;                             // (a moved vector keeps its buffer, so res still points into it)
    ChainAnswer(const ChainAnswer &) = delete;
    bool reachable() const { return res.value != INT32_MIN / 4; }
    std::pair<EdgeList, EdgeList> edge_lists() const {
        EdgeList w1, w2;
        for (int i = 0; i < res.n_p1 && i < res.cap; ++i) w1.emplace_back(p1_from[i], p1_to[i]);
        for (int i = 0; i < res.n_p2 && i < res.cap; ++i) w2.emplace_back(p2_from[i], p2_to[i]);
        return {w1, w2};
    }
};

// what one pair of paths reads out of the graph: the two sequences and the colours met on the way
struct PathReadout {
    std::string seq[2];
    std::unordered_map<int, int> color_freq[2];
    std::vector<int> colors[2];
};

// The flat graph already is the dg_dp_graph layout (vertex ids are level-sorted: ExpandedGraph.hpp:360-407).
// Topology arrays are handed to the device library in place (no copies); only the HOM / HET colour CSR (:431-453,
// lists are sorted-unique already) is new: counts, prefix sums, fill -- in parallel over vertex blocks.
void split_colours(ExpandedGraph &g, const std::vector<uint8_t> &color_homo_bv, DpGraphStorage &dpg) {
    if (g.colours_split) {                                             // the fused route wrote the split lists directly
        dpg.hom_off.swap(g.hom_off); dpg.het_off.swap(g.het_off); dpg.hom_col.swap(g.hom_col); dpg.het_col.swap(g.het_col);
        return;
    }
    const int nV = g.n;
    dpg.hom_off.assign((size_t)nV + 1, 0);
    dpg.het_off.assign((size_t)nV + 1, 0);
    for (int c : g.col_pool) (void)color_homo_bv.at(c);                // same out_of_range behaviour as the reference's .at()
#pragma omp parallel for schedule(static)
    for (int v = 0; v < nV; ++v) {
        int64_t nh = 0;
        for (int64_t q = g.col_off[v]; q < g.col_off[v + 1]; ++q) nh += color_homo_bv[g.col_pool[q]] == 1;
        dpg.hom_off[v + 1] = nh;
        dpg.het_off[v + 1] = (g.col_off[v + 1] - g.col_off[v]) - nh;
    }
    for (int v = 0; v < nV; ++v) { dpg.hom_off[v + 1] += dpg.hom_off[v]; dpg.het_off[v + 1] += dpg.het_off[v]; }
    dpg.hom_col.resize((size_t)dpg.hom_off[nV]);
    dpg.het_col.resize((size_t)dpg.het_off[nV]);
#pragma omp parallel for schedule(static)
    for (int v = 0; v < nV; ++v) {
        int64_t ph = dpg.hom_off[v], pt = dpg.het_off[v];
        for (int64_t q = g.col_off[v]; q < g.col_off[v + 1]; ++q) {
            const int c = g.col_pool[q];
            if (color_homo_bv[c] == 1) dpg.hom_col[ph++] = c; else dpg.het_col[pt++] = c;
        }
    }
}

void dump_graph(DpGraphStorage &dpg, const ExpandedGraph &g, const std::string &path, int R) {   // the dump wants the topology too
    dpg.level_off = g.level_off; dpg.out_off = g.adj_off; dpg.out_dst = g.adj_dst; dpg.out_w = g.adj_w;
    dpg.save(path, R);
    uvec<int32_t>().swap(dpg.level_off); uvec<int64_t>().swap(dpg.out_off);
    uvec<int32_t>().swap(dpg.out_dst); uvec<uint8_t>().swap(dpg.out_w);
}

// ---- the level loop + sink read-out: DEVICE (approximator.cpp:532-716, 774-785) ----
// answers[q] is filled for budgets[q].  --budgets: the listed budgets and -R itself from ONE sweep of the graph loaded with R
// (plane r of the sink is the cell a run with -R r reads out; one chain walk per budget).  Without the option: the plain call, as ever.
std::string run_dp(const Pipeline &p, const ExpandedGraph &g, const std::vector<int32_t> &budgets, std::vector<ChainAnswer> &answers, const std::vector<dg_dp_pin> &pins) {
    const Backend &be = p.be;
    dg_dp_graph view = p.dpg.view(p.opt.R);
    view.n_vertices = g.n; view.n_levels = (int32_t)g.level_off.size() - 1;
    view.level_off = g.level_off.data(); view.out_off = g.adj_off.data(); view.out_dst = g.adj_dst.data(); view.out_w = g.adj_w.data();
    if (p.opt.budgets.empty() && p.opt.site_margins.empty() && p.opt.objective_table.empty() && p.opt.genotype_margins.empty() && p.opt.genotype_table.empty() && p.opt.pins_file.empty() && p.opt.phase_margins.empty() && p.opt.recombination_margins.empty()) {
        if (be.dp_solve_diploid(be.ctx, &view, &answers[0].res) != 0) return backend_error(be, "dp_solve_diploid");
        return "";
    }
    // --site-margins takes the same load-then-run route: the margins are read off the run that stays behind
    if (!p.opt.site_margins.empty() && (!be.dp_load_graph || !be.dp_run_budgets || !be.dp_call_margins)) return "--site-margins: this backend has no dp_call_margins";
    // and so does --objective-table: the answers' paths stay on the device
    if (!p.opt.objective_table.empty() && (!be.dp_load_graph || !be.dp_run_budgets || !be.dp_answer_objectives)) return "--objective-table: this backend has no dp_answer_objectives";
    // and --genotype-margins: the called genotype is the answer that stays behind
    if (!p.opt.genotype_margins.empty() && (!be.dp_load_graph || !be.dp_run_budgets || !be.dp_answer_paths || !be.dp_genotype_margins)) return "--genotype-margins: this backend has no dp_genotype_margins";
    // and --genotype-table: the same pass lists every genotype
    if (!p.opt.genotype_table.empty() && (!be.dp_load_graph || !be.dp_run_budgets || !be.dp_answer_paths || !be.dp_genotype_table || !be.free_buf)) return "--genotype-table: this backend has no dp_genotype_table";
    // and --budget-genotype-margins: the answers at the listed limits stay behind, one joint pass describes them all
    if (!p.opt.budget_genotype_margins.empty() && (!be.dp_answer_paths || !be.dp_genotype_margins_budgets)) return "--budget-genotype-margins: this backend has no dp_genotype_margins_budgets";
    // and --phase-margins: the called pair is the answer that stays behind
    if (!p.opt.phase_margins.empty() && (!be.dp_load_graph || !be.dp_run_budgets || !be.dp_answer_paths || !be.dp_phase_margins)) return "--phase-margins: this backend has no dp_phase_margins";
    // and --budget-phase-margins: the answers at the listed limits stay behind, one joint pass describes the phase of them all
    if (!p.opt.budget_phase_margins.empty() && (!be.dp_answer_paths || !be.dp_phase_margins_budgets)) return "--budget-phase-margins: this backend has no dp_phase_margins_budgets";
    // and --recombination-margins: the called hops are those of the answer that stays behind
    if (!p.opt.recombination_margins.empty() && (!be.dp_load_graph || !be.dp_run_budgets || !be.dp_answer_paths || !be.dp_recombination_margins || !be.dp_score_paths))
        return "--recombination-margins: this backend has no dp_recombination_margins";
    // and --budget-recombination-margins: the answers at the listed limits stay behind, one joint pass describes the crossovers of them all
    if (!p.opt.budget_recombination_margins.empty() && (!be.dp_answer_paths || !be.dp_recombination_margins_budgets || !be.dp_score_paths))
        return "--budget-recombination-margins: this backend has no dp_recombination_margins_budgets";
    // and --pins: the same run under the file's cell constraints
    if (!p.opt.pins_file.empty() && (!be.dp_load_graph || !be.dp_run_pinned || !be.dp_pin_stats || !be.dp_answer_paths)) return "--pins: this backend has no dp_run_pinned";
    // and --pinned-genotype-margins / --pinned-genotype-table: the joint pass under the same constraints
    if (!p.opt.pinned_genotype_margins.empty() && !be.dp_genotype_margins_pinned) return "--pinned-genotype-margins: this backend has no dp_genotype_margins_pinned";
    if (!p.opt.pinned_genotype_table.empty() && (!be.dp_genotype_table_pinned || !be.free_buf)) return "--pinned-genotype-table: this backend has no dp_genotype_table_pinned";
    if (!be.dp_load_graph || !be.dp_run_budgets) return "--budgets: this backend has no dp_run_budgets";
    std::vector<dg_dp_result> res;                                     // (the ABI takes the results as one array)
    for (const ChainAnswer &a : answers) res.push_back(a.res);
    int rc = be.dp_load_graph(be.ctx, &view);
    if (rc == 0 && !p.opt.pins_file.empty()) {
        rc = be.dp_run_pinned(be.ctx, pins.data(), (int64_t)pins.size(), budgets.data(), (int32_t)budgets.size(), res.data());
        if (rc != 0) return backend_error(be, "dp_run_pinned");
    } else if (rc == 0) rc = be.dp_run_budgets(be.ctx, budgets.data(), (int32_t)budgets.size(), res.data());
    if (rc != 0) return backend_error(be, "dp_run_budgets");
    for (size_t q = 0; q < answers.size(); ++q) answers[q].res = res[q];
    return "";
}

// --pins: the rows against the levels of the graph, as pins of the C ABI.  "" or what is wrong with the first bad row
std::string expand_pin_rows(const std::vector<PinRow> &rows, const ExpandedGraph &g, std::vector<dg_dp_pin> &pins) {
    const int L = (int)g.level_off.size() - 1;
    for (const PinRow &r : rows) {
        const std::string at = "--pins: line " + std::to_string(r.line) + ": ";
        if (r.level < 1 || r.level > L - 2) return at + "level " + std::to_string(r.level) + " outside 1.." + std::to_string(L - 2);
        for (int32_t v : {r.vertex1, r.vertex2})
            if (v != -1 && (v < g.level_off[(size_t)r.level] || v >= g.level_off[(size_t)r.level + 1]))
                return at + "vertex " + std::to_string(v) + " is not on level " + std::to_string(r.level) + " (" + std::to_string(g.level_off[(size_t)r.level]) + ".." +
                       std::to_string(g.level_off[(size_t)r.level + 1] - 1) + ")";
        pins.push_back(dg_dp_pin{r.level, r.vertex1, r.vertex2, r.forbid ? 1 : 0});
        if (!r.ordered && r.vertex1 != r.vertex2) pins.push_back(dg_dp_pin{r.level, r.vertex2, r.vertex1, r.forbid ? 1 : 0});
    }
    return "";
}

// --pins: the run's statistics, and whether the answer at -R passes only allowed cells (checked here, on the paths the run walked)
std::string summarize_pins(Pipeline &p, const ExpandedGraph &g, const std::vector<dg_dp_pin> &pins, bool reachable) {
    const Backend &be = p.be;
    const int L = (int)g.level_off.size() - 1;
    PinSummary &ps = p.sum.pins;
    ps.set = true;
    ps.rows = (int64_t)p.opt.pin_rows.size();
    int64_t st[5] = {0, 0, 0, 0, 0};
    if (!pins.empty() && be.dp_pin_stats(be.ctx, st, 5) != 0) return backend_error(be, "dp_pin_stats");
    ps.pins = (int64_t)pins.size(); ps.levels = st[1]; ps.pairs_as_singles = st[3];
    ps.satisfied = false;
    if (!reachable) return "";
    std::vector<int32_t> paths(2 * (size_t)L);
    if (be.dp_answer_paths(be.ctx, p.opt.R, paths.data()) != 0) return backend_error(be, "dp_answer_paths");
    std::vector<char> any_req((size_t)L, 0), req((size_t)L, 0), forbid((size_t)L, 0);
    for (const dg_dp_pin &q : pins) {
        const bool m = (q.vertex1 == -1 || q.vertex1 == paths[(size_t)q.level]) && (q.vertex2 == -1 || q.vertex2 == paths[(size_t)L + q.level]);
        if (q.kind == 0) { any_req[(size_t)q.level] = 1; req[(size_t)q.level] |= m; } else forbid[(size_t)q.level] |= m;
    }
    ps.satisfied = true;
    for (int l = 0; l < L; ++l) if ((any_req[(size_t)l] && !req[(size_t)l]) || forbid[(size_t)l]) ps.satisfied = false;
    return "";
}

int find_next_zero_hap(const ExpandedGraph &g, int src, int target_hap) {   // :732-755
    if (g.haplotype.at(src) == target_hap && g.orig_len.at(src) > 0) return src;
    std::queue<int> q;
    std::unordered_set<int> visited;
    q.push(src); visited.insert(src);
    while (!q.empty()) {
        int u = q.front(); q.pop();
        for (int64_t e = g.adj_off[u]; e < g.adj_off[u + 1]; ++e) {
            const int v = g.adj_dst[e];
            if (g.adj_w[e] != 0) continue;
            if (!visited.insert(v).second) continue;
            if (g.haplotype.at(v) == target_hap && g.orig_len.at(v) > 0) return v;
            q.push(v);
        }
    }
    return -1;
}

// weighted-edge list -> the sequence and the colours met on the way (:790-923), for path `which` (0: P1, 1: P2).  primary: the
// answer at -R, which speaks on stdout as the reference does; the other budgets of --budgets leave stdout alone
void path_sequence(const Pipeline &p, const ExpandedGraph &g, const AnchorsByHap &anchorsByHap, const EdgeList &wedges, int which, bool primary, PathReadout &out) {
    const auto &paths = p.paths;
    const int L = (int)g.level_off.size() - 1;
    const char *tag = which == 0 ? "P1" : "P2";
    std::string &hs = out.seq[which];
    auto &color_freq = out.color_freq[which];
    const int first_vertex = g.level_off.at(0);                        // vertices_in_level[0][0]
    int start_exp = first_vertex;
    for (int i = 0; i < (int)wedges.size(); i++) {
        const auto &edge = wedges.at(i);
        if (g.orig_len[edge.first] != 1) {
            std::cout << tag << ": Vertex " << edge.first << " in map back has " << g.orig_len[edge.first]
                      << " original vertices" << std::endl;
            exit(1);
        }
        int end_exp = edge.first;
        int h = g.haplotype.at(end_exp);
        if (start_exp == first_vertex)
            for (int v = g.level_off.at(1); v < g.level_off.at(2); ++v) if (g.haplotype.at(v) == h) start_exp = v;
        if (g.orig_len.at(start_exp) < 1 || g.orig_len.at(end_exp) < 1) throw std::out_of_range("original_vertex.at(0)");
        int start_org = g.orig_pool[g.orig_off[start_exp]];
        int end_org = g.orig_pool[g.orig_off[end_exp]];
        bool activated = false;
        for (int t = 0; t < (int)paths[h].size(); t++) {
            if ((int)paths[h][t] == start_org) activated = true;
            if (activated) hs += p.node_seq[paths[h][t]];
            if ((int)paths[h][t] == end_org) { activated = false; break; }
        }
        for (const auto &a : anchorsByHap[h])
            if (a.startOrg > start_org && a.endOrg < end_org)
                for (auto c : a.colours) {
                    if (color_freq.find(c) == color_freq.end()) { color_freq[c] = 1; out.colors[which].push_back(c); }
                    else color_freq[c] += 1;
                }
        if (g.haplotype.at(edge.second), edge.second >= g.level_off[L - 1]) break;   // level[edge.second] == L - 1 (ids are level-sorted)
        const auto &next_edge = wedges.at(i + 1);
        int next_hap = g.haplotype.at(next_edge.first);
        int next_start = find_next_zero_hap(g, edge.second, next_hap);
        if (next_start != -1) start_exp = next_start;
        else (primary ? std::cout : std::cerr) << tag << " (path recovery) Could not find next_hap=" << next_hap << " from " << edge.second << " via 0-weight edges\n";
    }
}

// :1314-1325 -- same bytes (80 columns, '\n' line ends), assembled in memory and written once instead of one flushed line at a time
std::string write_diploid_fasta(const std::string &path, const std::string *hs) {
    std::string text;
    text.reserve(hs[0].size() + hs[1].size() + (hs[0].size() + hs[1].size()) / 80 + 128);
    for (int q = 0; q < 2; ++q) {
        text += q == 0 ? ">sol_1 bp:" : ">sol_2 bp:";
        text += std::to_string(hs[q].size());
        text += '\n';
        for (size_t i = 0; i < hs[q].size(); i += 80) { text.append(hs[q], i, 80); text += '\n'; }
    }
    std::ofstream f(path, std::ios::out | std::ios::binary);
    if (!f.is_open()) return "cannot open output file " + path;
    f.write(text.data(), (std::streamsize)text.size());
    f.close();
    if (!f.good()) return "write to " + path + " failed";
    return "";
}

void split_sorted_unique(const std::vector<uint8_t> &color_homo_bv, const std::vector<int> &cs, std::vector<int> &hom, std::vector<int> &het) {
    for (auto c : cs) { if (color_homo_bv[c]) hom.push_back(c); else het.push_back(c); }
    std::sort(hom.begin(), hom.end()); hom.erase(std::unique(hom.begin(), hom.end()), hom.end());
    std::sort(het.begin(), het.end()); het.erase(std::unique(het.begin(), het.end()), het.end());
}

// score + approximation certificate (:933-1004) -- stdout only
void certificate(Pipeline &p, const std::vector<uint8_t> &color_homo_bv, const PathReadout &out, int s_het) {
    std::vector<int> h1, t1, h2, t2, inter, symd;
    split_sorted_unique(color_homo_bv, out.colors[0], h1, t1);
    split_sorted_unique(color_homo_bv, out.colors[1], h2, t2);
    std::set_intersection(h1.begin(), h1.end(), h2.begin(), h2.end(), std::back_inserter(inter));
    std::set_symmetric_difference(t1.begin(), t1.end(), t2.begin(), t2.end(), std::back_inserter(symd));
    int intersection_count = (int)inter.size(), symdiff_count = (int)symd.size();
    int m_G_hom = 0, m_G_het = 0;
    auto freq = [&](int which, int c) { auto it = out.color_freq[which].find(c); return it == out.color_freq[which].end() ? 0 : it->second; };
    for (auto c : inter) { int k1 = freq(0, c), k2 = freq(1, c); m_G_hom += (k1 >= k2 ? k1 : k2); }
    for (auto c : symd) m_G_het += freq(0, c) + freq(1, c);
    float m_G_hom_avg = m_G_hom / (float)intersection_count;
    float m_G_het_avg = m_G_het / (float)symdiff_count;
    float m_bar = std::max(m_G_hom_avg, m_G_het_avg);
    int loss_het = s_het - m_G_het;
    float additive_term = loss_het / (float)m_G_het_avg;
    int obj = intersection_count + symdiff_count;
    p.sum.obj = obj;
    if (!p.opt.quiet) {
        std::cout << "r: " << p.opt.R << " obj: " << obj << std::endl;
        float ub = m_bar * (obj + additive_term);
        std::cout << "Approximation certificate: multiplicative factor: " << ub / (float)obj << std::endl;
    }
}

// --budgets: every listed budget r other than -R gets <hap_file>.R<r>, the FASTA a run with -R r writes (an unreachable one: no
// file), and every listed budget its row (answers starts with the listed budgets, in order)
std::string write_budget_fastas(Pipeline &p, const ExpandedGraph &g, const AnchorsByHap &anchorsByHap, const std::vector<ChainAnswer> &answers) {
    for (size_t q = 0; q < p.opt.budgets.size(); ++q) {
        const ChainAnswer &b = answers[q];
        BudgetRow row;
        row.r = p.opt.budgets[q];
        row.reachable = b.reachable();
        if (row.r == p.opt.R) { row.dp_value = p.sum.dp_value; row.r1 = p.sum.r1; row.r2 = p.sum.r2; row.len1 = p.sum.len1; row.len2 = p.sum.len2; }
        else if (row.reachable) {
            const auto [w1, w2] = b.edge_lists();
            PathReadout out;
            path_sequence(p, g, anchorsByHap, w1, 0, false, out);
            path_sequence(p, g, anchorsByHap, w2, 1, false, out);
            const std::string e = write_diploid_fasta(p.opt.hap_file + ".R" + std::to_string(row.r), out.seq);
            if (!e.empty()) return e;
            row.dp_value = b.res.value; row.r1 = (int)w1.size() - 1; row.r2 = (int)w2.size() - 1;
            row.len1 = (int64_t)out.seq[0].size(); row.len2 = (int64_t)out.seq[1].size();
        }
        p.sum.budget_rows.push_back(row);
    }
    return "";
}

// r  dp_value  r1  r2  len1  len2, NA for an unreachable budget
std::string write_budget_table(const std::string &path, const std::vector<BudgetRow> &rows) {
    std::ofstream f(path, std::ios::out | std::ios::binary);
    if (!f.is_open()) return "cannot open budget table " + path;
    for (const BudgetRow &row : rows) {
        if (row.reachable) f << row.r << '\t' << row.dp_value << '\t' << row.r1 << '\t' << row.r2 << '\t' << row.len1 << '\t' << row.len2 << '\n';
        else f << row.r << "\tNA\tNA\tNA\tNA\tNA\n";
    }
    f.close();
    if (!f.good()) return "write to " + path + " failed";
    return "";
}

// --objective-table: what the answer at every listed budget (without --budgets: at -R) is worth in the surrogate the DP maximises and
// in the distinct-colour objective (dg_dp_answer_objectives).  budgets / answers: the run's, the listed budgets first.
// r  dp_value  objective  hom_shared  hom_single  het_single  het_both under one header line; "." for an unreachable budget
std::string write_objective_table(Pipeline &p, const std::vector<int32_t> &budgets, const std::vector<ChainAnswer> &answers) {
    const size_t n = p.opt.budgets.empty() ? 1 : p.opt.budgets.size();  // (without --budgets the run's only budget is -R)
    std::vector<dg_dp_pair_objective> rec(n);
    if (p.be.dp_answer_objectives(p.be.ctx, budgets.data(), (int32_t)n, rec.data()) != 0) return backend_error(p.be, "dp_answer_objectives");
    std::ofstream f(p.opt.objective_table, std::ios::out | std::ios::binary);
    if (!f.is_open()) return "cannot open objective table " + p.opt.objective_table;
    f << "r\tdp_value\tobjective\thom_shared\thom_single\thet_single\thet_both\n";
    for (size_t q = 0; q < n; ++q) {
        ObjectiveRow row;
        row.r = budgets[q]; row.reachable = answers[q].reachable(); row.dp_value = answers[q].res.value; row.rec = rec[q];
        if (row.reachable != (rec[q].hom_shared >= 0)) return "dp_answer_objectives and the run disagree on whether budget " + std::to_string(row.r) + " is reachable";
        if (row.reachable) f << row.r << '\t' << row.dp_value << '\t' << rec[q].hom_shared + rec[q].het_single << '\t' << rec[q].hom_shared << '\t' << rec[q].hom_single << '\t'
                             << rec[q].het_single << '\t' << rec[q].het_both << '\n';
        else f << row.r << "\t.\t.\t.\t.\t.\t.\n";
        p.sum.objective_rows.push_back(row);
    }
    f.close();
    if (!f.good()) return "write to " + p.opt.objective_table + " failed";
    return "";
}

// --site-margins: the allele class of every vertex.  Two vertices are the same class exactly when their original-vertex lists are
// equal (a dummy shares its source's list; source and sink have an empty one): copies of one segment on several panel haplotypes
// are one allele.
std::vector<int32_t> allele_classes(const ExpandedGraph &g) {
    std::vector<int32_t> cls((size_t)g.n);
    // an empty list is class 0, a list of one original vertex x is class 1 + x (nearly every vertex); longer lists are numbered from
    // `next` on, found by a hash of the list and compared in full with the lists that share it
    int32_t next = 1;
    for (int32_t x : g.orig_pool) next = std::max(next, x + 2);
    std::unordered_map<uint64_t, std::vector<std::pair<int32_t, int32_t>>> seen;   // hash -> (a vertex with that list, its class)
    for (int v = 0; v < g.n; ++v) {
        const uint32_t off = g.orig_off[v], len = g.orig_len[v];
        if (len == 0) { cls[v] = 0; continue; }
        if (len == 1) { cls[v] = 1 + g.orig_pool[off]; continue; }
        uint64_t h = 1469598103934665603ull;
        for (uint32_t q = 0; q < len; ++q) h = (h ^ (uint32_t)g.orig_pool[off + q]) * 1099511628211ull;
        auto &bucket = seen[h];
        int32_t c = -1;
        for (const auto &rep : bucket) {
            const uint32_t roff = g.orig_off[rep.first];
            if (g.orig_len[rep.first] == len && (roff == off || std::equal(g.orig_pool.begin() + off, g.orig_pool.begin() + off + len, g.orig_pool.begin() + roff))) { c = rep.second; break; }
        }
        if (c < 0) { c = next++; bucket.emplace_back(v, c); }
        cls[v] = c;
    }
    return cls;
}

std::string write_raw_int32(const std::string &path, const std::vector<int32_t> &a) {
    std::ofstream f(path, std::ios::out | std::ios::binary);
    if (!f.is_open()) return "cannot open " + path;
    f.write((const char *)a.data(), (std::streamsize)(a.size() * sizeof(int32_t)));
    f.close();
    return f.good() ? "" : "write to " + path + " failed";
}

// what the margin tables call a vertex: the panel haplotype it lies on and the GFA segment it copies; '.' for what does not exist
std::string panel_name(const Pipeline &p, const ExpandedGraph &g, int v) {
    const int h = v >= 0 ? g.haplotype.at(v) : -1;
    return h >= 0 && h < (int)p.hap_id2name.size() ? p.hap_id2name[h] : ".";
}
std::string segment_name(const Pipeline &p, const ExpandedGraph &g, int v) {
    if (v < 0 || g.orig_len.at(v) < 1) return ".";
    const int32_t seg = g.orig_pool[g.orig_off[v]];
    return seg >= 0 && seg < (int32_t)p.node_name.size() ? p.node_name[seg] : ".";
}

// level  hap  vertex  panel_hap  segment  value  alt_vertex  alt_panel_hap  alt_segment  margin: levels 1 .. L - 2, haplotype 1 before
// haplotype 2 within a level; '.' for what does not exist
std::string write_site_margins(Pipeline &p, const ExpandedGraph &g, const std::vector<int32_t> &cls) {
    const double t0 = now_s();
    const int L = (int)g.level_off.size() - 1;
    std::vector<dg_dp_call_margin> rec(2 * (size_t)L);
    if (p.be.dp_call_margins(p.be.ctx, p.opt.R, cls.data(), rec.data(), nullptr) != 0) return backend_error(p.be, "dp_call_margins");
    auto panel = [&](int v) { return panel_name(p, g, v); };
    auto segment = [&](int v) { return segment_name(p, g, v); };
    SiteMargins &sm = p.sum.site_margins;
    sm = SiteMargins();
    sm.set = true;
    std::string text = "level\thap\tvertex\tpanel_hap\tsegment\tvalue\talt_vertex\talt_panel_hap\talt_segment\tmargin\n";
    for (int l = 1; l < L - 1; ++l)
        for (int h = 0; h < 2; ++h) {
            const dg_dp_call_margin &r = rec[(size_t)h * L + l];
            text += std::to_string(l) + '\t' + std::to_string(h + 1) + '\t' + std::to_string(r.vertex) + '\t' + panel(r.vertex) + '\t' + segment(r.vertex) + '\t' +
                    std::to_string(r.value) + '\t' + std::to_string(r.alt_vertex) + '\t' + panel(r.alt_vertex) + '\t' + segment(r.alt_vertex) + '\t';
            if (r.alt_vertex >= 0) {
                const int32_t margin = r.value - r.alt_value;
                text += std::to_string(margin);
                sm.with_alternative[h]++;
                if (margin == 0) sm.margin0[h]++;
                else if (sm.min_positive_margin[h] < 0 || margin < sm.min_positive_margin[h]) sm.min_positive_margin[h] = margin;
            } else text += '.';
            text += '\n';
        }
    std::ofstream f(p.opt.site_margins, std::ios::out | std::ios::binary);
    if (!f.is_open()) return "cannot open site margins file " + p.opt.site_margins;
    f.write(text.data(), (std::streamsize)text.size());
    f.close();
    if (!f.good()) return "write to " + p.opt.site_margins + " failed";
    sm.wall_s = now_s() - t0;
    return "";
}

// level  vertex1  panel_hap1  segment1  vertex2  panel_hap2  segment2  value  alt_vertex1  alt_segment1  alt_vertex2  alt_segment2  alt_value  margin:
// levels 1 .. L - 2; the called cell is the answer at -R (its two paths), the alternative the best cell of another genotype with both
// haplotypes free; '.' for what does not exist (no other genotype reachable; every field if no pair of paths fits -R)
// What --genotype-margins and --genotype-table share: the answer at -R as the called cells, and ONE pass over the graph with both
// haplotypes free -- dp_genotype_table when the table is asked for (it answers the margin records too), dp_genotype_margins otherwise.
// --pinned-genotype-margins and --pinned-genotype-table share the same on the DP under --pins: the called cells are the pinned answer's
struct GenotypePass {
    const Backend *be = nullptr;
    bool fits = false;                                   // a pair of paths fits -R (none: no device call, both files say so)
    std::vector<int32_t> paths;                          // [2][L]
    std::vector<dg_dp_genotype_margin> rec;              // [L]
    std::vector<int64_t> level_off;                      // [L + 1], with the table
    dg_dp_genotype_entry *entries = nullptr;             // the backend's buffer
    int64_t n_entries = 0, segments = 0;
    int32_t best = 0;
    double wall_s = 0;
    GenotypePass() = default;
    GenotypePass(const GenotypePass &) = delete;
    GenotypePass &operator=(const GenotypePass &) = delete;
    ~GenotypePass() { if (entries && be) be->free_buf(entries); }
};

// pins = null: the unconstrained DP; else the DP under these pins (the *_pinned calls)
std::string genotype_pass(Pipeline &p, const ExpandedGraph &g, const std::vector<int32_t> &cls, GenotypePass &gp, bool want_table, const std::vector<dg_dp_pin> *pins = nullptr) {
    const double t0 = now_s();
    const Backend &be = p.be;
    gp.be = &be;
    const int L = (int)g.level_off.size() - 1;
    gp.paths.assign(2 * (size_t)L, 0);
    if (be.dp_answer_paths(be.ctx, p.opt.R, gp.paths.data()) != 0) return backend_error(be, "dp_answer_paths");
    gp.fits = gp.paths[0] >= 0;
    gp.rec.assign((size_t)L, dg_dp_genotype_margin());
    gp.level_off.assign((size_t)L + 1, 0);
    if (gp.fits) {
        if (pins) {
            if (want_table) {
                if (be.dp_genotype_table_pinned(be.ctx, pins->data(), (int64_t)pins->size(), p.opt.R, cls.data(), gp.paths.data(), 1, gp.rec.data(), gp.level_off.data(), &gp.entries,
                                                &gp.n_entries, &gp.best) != 0)
                    return backend_error(be, "dp_genotype_table_pinned");
            } else if (be.dp_genotype_margins_pinned(be.ctx, pins->data(), (int64_t)pins->size(), gp.paths.data(), 1, p.opt.R, cls.data(), gp.rec.data(), nullptr, &gp.best) != 0)
                return backend_error(be, "dp_genotype_margins_pinned");
        } else if (want_table) {
            if (be.dp_genotype_table(be.ctx, p.opt.R, cls.data(), gp.paths.data(), 1, gp.rec.data(), gp.level_off.data(), &gp.entries, &gp.n_entries, &gp.best) != 0)
                return backend_error(be, "dp_genotype_table");
        } else if (be.dp_genotype_margins(be.ctx, gp.paths.data(), 1, p.opt.R, cls.data(), gp.rec.data(), nullptr, &gp.best) != 0) return backend_error(be, "dp_genotype_margins");
        int64_t stats[4] = {0, 0, 0, 0};
        if (be.dp_genotype_stats && be.dp_genotype_stats(be.ctx, stats, 4) != 0) return backend_error(be, "dp_genotype_stats");
        gp.segments = stats[0];
    }
    gp.wall_s = now_s() - t0;
    return "";
}

// (pinned: the file of the DP under --pins; without a pair of paths that satisfies them within -R it holds the header alone)
std::string write_genotype_margins(Pipeline &p, const ExpandedGraph &g, const GenotypePass &gp, const std::string &path, GenotypeMargins &gm, bool pinned) {
    const double t0 = now_s();
    const int L = (int)g.level_off.size() - 1;
    const bool fits = gp.fits;
    const std::vector<dg_dp_genotype_margin> &rec = gp.rec;
    gm = GenotypeMargins();
    gm.set = true;
    gm.segments = gp.segments;
    std::string text = "level\tvertex1\tpanel_hap1\tsegment1\tvertex2\tpanel_hap2\tsegment2\tvalue\talt_vertex1\talt_segment1\talt_vertex2\talt_segment2\talt_value\tmargin\n";
    for (int l = 1; l < L - 1 && (fits || !pinned); ++l) {
        text += std::to_string(l);
        if (!fits) { text += "\t.\t.\t.\t.\t.\t.\t.\t.\t.\t.\t.\t.\t.\n"; continue; }
        const dg_dp_genotype_margin &r = rec[(size_t)l];
        text += '\t' + std::to_string(r.vertex1) + '\t' + panel_name(p, g, r.vertex1) + '\t' + segment_name(p, g, r.vertex1) + '\t' + std::to_string(r.vertex2) + '\t' +
                panel_name(p, g, r.vertex2) + '\t' + segment_name(p, g, r.vertex2) + '\t' + std::to_string(r.value) + '\t';
        if (r.alt_vertex1 >= 0) {
            const int32_t margin = r.value - r.alt_value;
            text += std::to_string(r.alt_vertex1) + '\t' + segment_name(p, g, r.alt_vertex1) + '\t' + std::to_string(r.alt_vertex2) + '\t' + segment_name(p, g, r.alt_vertex2) + '\t' +
                    std::to_string(r.alt_value) + '\t' + std::to_string(margin);
            gm.with_alternative++;
            if (margin == 0) gm.margin0++;
            else if (margin > 0 && (gm.min_positive_margin < 0 || margin < gm.min_positive_margin)) gm.min_positive_margin = margin;
        } else text += ".\t.\t.\t.\t.\t.";
        text += '\n';
    }
    std::ofstream f(path, std::ios::out | std::ios::binary);
    if (!f.is_open()) return "cannot open genotype margins file " + path;
    f.write(text.data(), (std::streamsize)text.size());
    f.close();
    if (!f.good()) return "write to " + path + " failed";
    gm.wall_s = gp.wall_s + (now_s() - t0);
    return "";
}

// level_a  level_b  vertex1_a  segment1_a  vertex2_a  segment2_a  vertex1_b  segment1_b  vertex2_b  segment2_b  cis_value  trans_value
// trans_vertex1  trans_vertex2  margin: one row per pair of neighbouring het levels (the alleles of the answer's two vertices differ) of
// the answer at -R, ascending.  cis: the best pair of paths within -R with the answer's ordered alleles at both levels -- the answer
// itself is one, so it must be the run's DP value; trans: the best with the alleles at level_a swapped, and its cell there; '.' where no
// such pair exists.  Without a pair of paths that fits -R, or with fewer than two het levels, the file holds the header alone.
std::string write_phase_margins(Pipeline &p, const ExpandedGraph &g, const std::vector<int32_t> &cls) {
    const double t0 = now_s();
    const Backend &be = p.be;
    const int L = (int)g.level_off.size() - 1;
    PhaseMargins &pm = p.sum.phase_margins;
    pm = PhaseMargins();
    pm.set = true;
    std::vector<int32_t> paths(2 * (size_t)L, 0);
    if (be.dp_answer_paths(be.ctx, p.opt.R, paths.data()) != 0) return backend_error(be, "dp_answer_paths");
    std::vector<dg_dp_phase_margin> rec((size_t)std::max(L - 1, 1));
    int64_t n = 0;
    if (paths[0] >= 0) {
        int32_t best = 0;
        if (be.dp_phase_margins(be.ctx, paths.data(), p.opt.R, cls.data(), rec.data(), &n, &best) != 0) return backend_error(be, "dp_phase_margins");
        int64_t stats[6] = {0, 0, 0, 0, 0, 0};
        if (be.dp_phase_stats && be.dp_phase_stats(be.ctx, stats, 6) != 0) return backend_error(be, "dp_phase_stats");
        pm.het_levels = stats[0];
        pm.segments = stats[4];
        if (best != p.sum.dp_value) return "--phase-margins: the joint pass finds " + std::to_string(best) + ", the run's DP value is " + std::to_string(p.sum.dp_value);
    }
    std::string text = "level_a\tlevel_b\tvertex1_a\tsegment1_a\tvertex2_a\tsegment2_a\tvertex1_b\tsegment1_b\tvertex2_b\tsegment2_b\tcis_value\ttrans_value\ttrans_vertex1\ttrans_vertex2\tmargin\n";
    for (int64_t q = 0; q < n; ++q) {
        const dg_dp_phase_margin &r = rec[(size_t)q];
        if (r.cis_value != p.sum.dp_value)
            return "--phase-margins: levels " + std::to_string(r.level_a) + ", " + std::to_string(r.level_b) + ": the answer's phase is worth " + std::to_string(r.cis_value) + ", the run's DP value is " +
                   std::to_string(p.sum.dp_value);
        text += std::to_string(r.level_a) + '\t' + std::to_string(r.level_b);
        for (const int l : {r.level_a, r.level_b})
            for (int h = 0; h < 2; ++h) {
                const int32_t v = paths[(size_t)h * L + l];
                text += '\t' + std::to_string(v) + '\t' + segment_name(p, g, v);
            }
        text += '\t' + std::to_string(r.cis_value) + '\t';
        if (r.trans_vertex1 >= 0) {
            const int32_t margin = r.cis_value - r.trans_value;
            text += std::to_string(r.trans_value) + '\t' + std::to_string(r.trans_vertex1) + '\t' + std::to_string(r.trans_vertex2) + '\t' + std::to_string(margin);
            pm.with_alternative++;
            if (margin == 0) pm.margin0++;
            else if (margin > 0 && (pm.min_positive_margin < 0 || margin < pm.min_positive_margin)) pm.min_positive_margin = margin;
        } else text += ".\t.\t.\t.";
        text += '\n';
    }
    pm.records = n;
    std::ofstream f(p.opt.phase_margins, std::ios::out | std::ios::binary);
    if (!f.is_open()) return "cannot open phase margins file " + p.opt.phase_margins;
    f.write(text.data(), (std::streamsize)text.size());
    f.close();
    if (!f.good()) return "write to " + p.opt.phase_margins + " failed";
    pm.wall_s = now_s() - t0;
    return "";
}

// one row of the --recombination-margins file (its comment is below), without the newline: transition l of the pair `paths` ([2][L]) against its record; counts what -J reports into rm
static void recombination_row(const Pipeline &p, const ExpandedGraph &g, const int32_t *paths, int64_t l, const dg_dp_recombination_margin &r, int32_t s_called, int32_t value,
                              int32_t dp_value, RecombinationMargins &rm, std::string &text) {
    const int L = (int)g.level_off.size() - 1;
    auto weight = [&](int32_t u, int32_t v) -> std::string {             // of the hop u -> v (parallel edges share it)
        for (int64_t e = g.adj_off[(size_t)u]; e < g.adj_off[(size_t)u + 1]; ++e)
            if (g.adj_dst[(size_t)e] == v) return std::to_string((int)g.adj_w[(size_t)e]);
        return ".";
    };
    text += std::to_string(l);
    for (int h = 0; h < 2; ++h) {
        const int32_t u = paths[(size_t)h * L + l], v = paths[(size_t)h * L + l + 1];
        text += '\t' + std::to_string(u) + '\t' + segment_name(p, g, u) + '\t' + std::to_string(v) + '\t' + segment_name(p, g, v) + '\t' + weight(u, v);
    }
    text += '\t' + std::to_string(s_called) + '\t' + std::to_string(value);
    int alt = -1;
    for (int s = 0; s < 3; ++s) {
        text += '\t' + (r.from1[s] >= 0 ? std::to_string(r.value[s]) : std::string("."));
        if (s != s_called && r.from1[s] >= 0 && (alt < 0 || r.value[s] > r.value[alt])) alt = s;      // ties: the smaller s
    }
    rm.called_recombinations += s_called;
    if (alt >= 0) {
        const int32_t margin = value - r.value[alt];
        text += '\t' + std::to_string(alt) + '\t' + std::to_string(r.value[alt]) + '\t' + std::to_string(margin) + '\t' + std::to_string(r.from1[alt]) + '\t' + std::to_string(r.to1[alt]) + '\t' +
                std::to_string(r.from2[alt]) + '\t' + std::to_string(r.to2[alt]);
        if (s_called > 0 && margin == 0) rm.breakpoints_margin0++;
        else if (s_called > 0 && margin > 0 && (rm.min_positive_breakpoint_margin < 0 || margin < rm.min_positive_breakpoint_margin)) rm.min_positive_breakpoint_margin = margin;
        if (s_called == 0 && r.value[alt] == dp_value) rm.co_optimal_elsewhere++;
    } else text += "\t.\t.\t.\t.\t.\t.\t.";
}

static const char *const RECOMBINATION_COLUMNS =
    "level\tvertex1_from\tsegment1_from\tvertex1_to\tsegment1_to\tw1\tvertex2_from\tsegment2_from\tvertex2_to\tsegment2_to\tw2\ts_called\tvalue\tvalue_s0\tvalue_s1\tvalue_s2\t"
    "alt_s\talt_value\tmargin\talt_from1\talt_to1\talt_from2\talt_to2\n";

// level  vertex1_from segment1_from vertex1_to segment1_to w1  vertex2_from segment2_from vertex2_to segment2_to w2  s_called value
// value_s0 value_s1 value_s2  alt_s alt_value margin  alt_from1 alt_to1 alt_from2 alt_to2: one row per transition level -> level + 1.  The
// two hops of the answer at -R with their weights, s_called = w1 + w2, value = the best pair of paths within -R that takes exactly these
// two hops -- the answer is one, so it must be the run's DP value; value_s = the best pair that spends s crossovers at this transition;
// alt_s = the best other s (among equals the smaller), its value and hop pair, margin = value - alt_value; '.' where there is none.
// A row with s_called > 0 is a breakpoint of the answer: margin 0 there says the crossover can be dropped or moved at no cost.  Without a
// pair of paths that fits -R the file holds the header alone.
std::string write_recombination_margins(Pipeline &p, const ExpandedGraph &g) {
    const double t0 = now_s();
    const Backend &be = p.be;
    const int L = (int)g.level_off.size() - 1;
    RecombinationMargins &rm = p.sum.recombination_margins;
    rm = RecombinationMargins();
    rm.set = true;
    std::vector<int32_t> paths(2 * (size_t)L, 0);
    if (be.dp_answer_paths(be.ctx, p.opt.R, paths.data()) != 0) return backend_error(be, "dp_answer_paths");
    const int64_t T = paths[0] >= 0 ? L - 1 : 0;
    std::vector<dg_dp_recombination_margin> rec((size_t)std::max(L - 1, 1));
    std::vector<int32_t> out(2 * (size_t)std::max(L - 1, 1), 0);
    dg_dp_pair_score score = {};
    if (T) {
        int32_t best = 0;
        if (be.dp_recombination_margins(be.ctx, p.opt.R, paths.data(), 1, rec.data(), out.data(), &best) != 0) return backend_error(be, "dp_recombination_margins");
        int64_t stats[7] = {0, 0, 0, 0, 0, 0, 0};
        if (be.dp_recombination_stats && be.dp_recombination_stats(be.ctx, stats, 7) != 0) return backend_error(be, "dp_recombination_stats");
        rm.segments = stats[3];
        if (best != p.sum.dp_value) return "--recombination-margins: the joint pass finds " + std::to_string(best) + ", the run's DP value is " + std::to_string(p.sum.dp_value);
        if (be.dp_score_paths(be.ctx, paths.data(), 1, &score) != 0) return backend_error(be, "dp_score_paths");
    }
    std::string text = RECOMBINATION_COLUMNS;
    for (int64_t l = 0; l < T; ++l) {
        const int32_t s_called = out[2 * (size_t)l], value = out[2 * (size_t)l + 1];
        if (s_called < 0 || value != p.sum.dp_value)
            return "--recombination-margins: level " + std::to_string(l) + ": the answer's hops are worth " + std::to_string(value) + " (s_called " + std::to_string(s_called) + "), the run's DP value is " +
                   std::to_string(p.sum.dp_value);
        recombination_row(p, g, paths.data(), l, rec[(size_t)l], s_called, value, p.sum.dp_value, rm, text);
        text += '\n';
    }
    rm.transitions = T;
    if (T && rm.called_recombinations != (int64_t)score.r1 + score.r2)
        return "--recombination-margins: the answer's hops spend " + std::to_string(rm.called_recombinations) + " crossovers, dp_score_paths counts " + std::to_string(score.r1) + " + " + std::to_string(score.r2);
    std::ofstream f(p.opt.recombination_margins, std::ios::out | std::ios::binary);
    if (!f.is_open()) return "cannot open recombination margins file " + p.opt.recombination_margins;
    f.write(text.data(), (std::streamsize)text.size());
    f.close();
    if (!f.good()) return "write to " + p.opt.recombination_margins + " failed";
    rm.wall_s = now_s() - t0;
    return "";
}

// r and the columns of --recombination-margins: per listed limit r with an answer, in the order of the list, one row per transition with the
// two hops of the answer at r against the best pairs of paths within r.  ONE device call serves every limit
// (dp_recombination_margins_budgets: the joint pass at the largest of them) and one dp_score_paths call scores all answers.  A limit nobody
// fits is left out: it has no paths to call.  At every transition the answer's hops must be worth the run's DP value at r, and its called
// crossovers must add up to the r1 + r2 of its score.
std::string write_budget_recombination_margins(Pipeline &p, const ExpandedGraph &g, const std::vector<int32_t> &budgets, const std::vector<ChainAnswer> &answers) {
    const double t0 = now_s();
    const Backend &be = p.be;
    const int L = (int)g.level_off.size() - 1;
    const std::string O = "--budget-recombination-margins: limit ";
    BudgetRecombinationMargins &br = p.sum.budget_recombination_margins;
    br = BudgetRecombinationMargins();
    br.set = true;
    std::vector<int32_t> called, limits, values;                     // [n][2][L], [n], the run's DP value at each
    std::vector<int32_t> paths(2 * (size_t)L);
    for (const int r : p.opt.budgets) {
        const size_t q = (size_t)(std::find(budgets.begin(), budgets.end(), (int32_t)r) - budgets.begin());
        if (q >= answers.size() || !answers[q].reachable()) continue;
        if (be.dp_answer_paths(be.ctx, r, paths.data()) != 0) return backend_error(be, "dp_answer_paths");
        if (paths[0] < 0) continue;
        called.insert(called.end(), paths.begin(), paths.end());
        limits.push_back(r);
        values.push_back(answers[q].res.value);
    }
    const int64_t n = (int64_t)limits.size(), T = L - 1;
    std::vector<dg_dp_recombination_margin> rec((size_t)std::max<int64_t>(n * T, 1));
    std::vector<int32_t> out(2 * (size_t)std::max<int64_t>(n * T, 1), 0), best((size_t)n);
    std::vector<dg_dp_pair_score> scores((size_t)n);
    if (n > 0) {
        if (be.dp_recombination_margins_budgets(be.ctx, limits.data(), n, called.data(), rec.data(), out.data(), best.data()) != 0) return backend_error(be, "dp_recombination_margins_budgets");
        int64_t stats[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (be.dp_recombination_budget_stats && be.dp_recombination_budget_stats(be.ctx, stats, 9) != 0) return backend_error(be, "dp_recombination_budget_stats");
        br.segments = stats[5];
        if (be.dp_score_paths(be.ctx, called.data(), n, scores.data()) != 0) return backend_error(be, "dp_score_paths");
    }
    std::string text = std::string("r\t") + RECOMBINATION_COLUMNS;
    for (int64_t q = 0; q < n; ++q) {
        BudgetRecombinationMargins::Row row;
        row.r = limits[(size_t)q];
        const int32_t dp_value = values[(size_t)q];
        if (best[(size_t)q] != dp_value) return O + std::to_string(row.r) + ": the joint pass finds " + std::to_string(best[(size_t)q]) + ", the run's DP value is " + std::to_string(dp_value);
        for (int64_t l = 0; l < T; ++l) {
            const size_t x = (size_t)(q * T + l);
            const int32_t s_called = out[2 * x], value = out[2 * x + 1];
            if (s_called < 0 || value != dp_value)
                return O + std::to_string(row.r) + " level " + std::to_string(l) + ": the answer's hops are worth " + std::to_string(value) + " (s_called " + std::to_string(s_called) +
                       "), the run's DP value is " + std::to_string(dp_value);
            text += std::to_string(row.r) + '\t';
            recombination_row(p, g, &called[(size_t)q * 2 * (size_t)L], l, rec[x], s_called, value, dp_value, row.counts, text);
            text += '\n';
        }
        row.counts.transitions = T;
        if (row.counts.called_recombinations != (int64_t)scores[(size_t)q].r1 + scores[(size_t)q].r2)
            return O + std::to_string(row.r) + ": the answer's hops spend " + std::to_string(row.counts.called_recombinations) + " crossovers, dp_score_paths counts " +
                   std::to_string(scores[(size_t)q].r1) + " + " + std::to_string(scores[(size_t)q].r2);
        br.rows.push_back(row);
    }
    const std::string &path = p.opt.budget_recombination_margins;
    std::ofstream f(path, std::ios::out | std::ios::binary);
    if (!f.is_open()) return "cannot open budget recombination margins file " + path;
    f.write(text.data(), (std::streamsize)text.size());
    f.close();
    if (!f.good()) return "write to " + path + " failed";
    br.wall_s = now_s() - t0;
    return "";
}

// r and the columns of --phase-margins: per listed limit r with an answer, in the order of the list, one row per pair of neighbouring het
// levels of the answer at r, cis and trans within r.  ONE device call serves every limit (dp_phase_margins_budgets: the joint pass at the
// largest of them; answers at neighbouring limits share most of their seeded states).  A limit nobody fits is left out: it has no paths
// to call.  In every record cis must be the run's DP value at r.
std::string write_budget_phase_margins(Pipeline &p, const ExpandedGraph &g, const std::vector<int32_t> &cls, const std::vector<int32_t> &budgets, const std::vector<ChainAnswer> &answers) {
    const double t0 = now_s();
    const Backend &be = p.be;
    const int L = (int)g.level_off.size() - 1;
    BudgetPhaseMargins &bp = p.sum.budget_phase_margins;
    bp = BudgetPhaseMargins();
    bp.set = true;
    std::vector<int32_t> called, limits, values;                     // [n][2][L], [n], the run's DP value at each
    std::vector<int32_t> paths(2 * (size_t)L);
    for (const int r : p.opt.budgets) {
        const size_t q = (size_t)(std::find(budgets.begin(), budgets.end(), (int32_t)r) - budgets.begin());
        if (q >= answers.size() || !answers[q].reachable()) continue;
        if (be.dp_answer_paths(be.ctx, r, paths.data()) != 0) return backend_error(be, "dp_answer_paths");
        if (paths[0] < 0) continue;
        called.insert(called.end(), paths.begin(), paths.end());
        limits.push_back(r);
        values.push_back(answers[q].res.value);
    }
    const int64_t n = (int64_t)limits.size();
    std::vector<dg_dp_phase_margin> rec((size_t)std::max<int64_t>(n * (L - 1), 1));
    std::vector<int64_t> off((size_t)n + 1, 0);
    std::vector<int32_t> best((size_t)n);
    if (n > 0) {
        if (be.dp_phase_margins_budgets(be.ctx, called.data(), limits.data(), n, cls.data(), rec.data(), off.data(), best.data()) != 0) return backend_error(be, "dp_phase_margins_budgets");
        int64_t stats[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (be.dp_phase_budget_stats && be.dp_phase_budget_stats(be.ctx, stats, 10) != 0) return backend_error(be, "dp_phase_budget_stats");
        bp.seed_keys = stats[2];
        bp.slot_levels = stats[3];
        bp.segments = stats[8];
    }
    std::string text = "r\tlevel_a\tlevel_b\tvertex1_a\tsegment1_a\tvertex2_a\tsegment2_a\tvertex1_b\tsegment1_b\tvertex2_b\tsegment2_b\tcis_value\ttrans_value\ttrans_vertex1\ttrans_vertex2\tmargin\n";
    for (int64_t q = 0; q < n; ++q) {
        BudgetPhaseMargins::Row row;
        row.r = limits[(size_t)q];
        const int32_t *qp = &called[(size_t)q * 2 * (size_t)L];
        if (best[(size_t)q] != values[(size_t)q])
            return "--budget-phase-margins: limit " + std::to_string(row.r) + ": the joint pass finds " + std::to_string(best[(size_t)q]) + ", the run's DP value is " + std::to_string(values[(size_t)q]);
        for (int l = 0; l < L; ++l) row.het_levels += cls[(size_t)qp[l]] != cls[(size_t)qp[(size_t)L + l]];
        for (int64_t x = off[(size_t)q]; x < off[(size_t)q + 1]; ++x) {
            const dg_dp_phase_margin &r = rec[(size_t)x];
            if (r.cis_value != values[(size_t)q])
                return "--budget-phase-margins: limit " + std::to_string(row.r) + " levels " + std::to_string(r.level_a) + ", " + std::to_string(r.level_b) + ": the answer's phase is worth " +
                       std::to_string(r.cis_value) + ", the run's DP value is " + std::to_string(values[(size_t)q]);
            text += std::to_string(row.r) + '\t' + std::to_string(r.level_a) + '\t' + std::to_string(r.level_b);
            for (const int l : {r.level_a, r.level_b})
                for (int h = 0; h < 2; ++h) {
                    const int32_t v = qp[(size_t)h * L + l];
                    text += '\t' + std::to_string(v) + '\t' + segment_name(p, g, v);
                }
            text += '\t' + std::to_string(r.cis_value) + '\t';
            if (r.trans_vertex1 >= 0) {
                const int32_t margin = r.cis_value - r.trans_value;
                text += std::to_string(r.trans_value) + '\t' + std::to_string(r.trans_vertex1) + '\t' + std::to_string(r.trans_vertex2) + '\t' + std::to_string(margin);
                row.with_alternative++;
                if (margin == 0) row.margin0++;
                else if (margin > 0 && (row.min_positive_margin < 0 || margin < row.min_positive_margin)) row.min_positive_margin = margin;
            } else text += ".\t.\t.\t.";
            text += '\n';
        }
        row.records = off[(size_t)q + 1] - off[(size_t)q];
        bp.rows.push_back(row);
    }
    const std::string &path = p.opt.budget_phase_margins;
    std::ofstream f(path, std::ios::out | std::ios::binary);
    if (!f.is_open()) return "cannot open budget phase margins file " + path;
    f.write(text.data(), (std::streamsize)text.size());
    f.close();
    if (!f.good()) return "write to " + path + " failed";
    bp.wall_s = now_s() - t0;
    return "";
}

// r and the columns of --genotype-margins: per listed limit r with an answer, in the order of the list, the levels 1 .. L - 2 with the
// answer at r as the called cells and the alternative within r.  ONE device call serves every limit (dp_genotype_margins_budgets: the
// joint pass at the largest of them).  A limit nobody fits is left out: it has no paths to call.  On every level the called cell must be
// worth the run's DP value at r.
std::string write_budget_genotype_margins(Pipeline &p, const ExpandedGraph &g, const std::vector<int32_t> &cls, const std::vector<int32_t> &budgets, const std::vector<ChainAnswer> &answers) {
    const double t0 = now_s();
    const Backend &be = p.be;
    const int L = (int)g.level_off.size() - 1;
    BudgetGenotypeMargins &bm = p.sum.budget_genotype_margins;
    bm = BudgetGenotypeMargins();
    bm.set = true;
    std::vector<int32_t> called, limits, values;                     // [n][2][L], [n], the run's DP value at each
    std::vector<int32_t> paths(2 * (size_t)L);
    for (const int r : p.opt.budgets) {
        const size_t q = (size_t)(std::find(budgets.begin(), budgets.end(), (int32_t)r) - budgets.begin());
        if (q >= answers.size() || !answers[q].reachable()) continue;
        if (be.dp_answer_paths(be.ctx, r, paths.data()) != 0) return backend_error(be, "dp_answer_paths");
        if (paths[0] < 0) continue;
        called.insert(called.end(), paths.begin(), paths.end());
        limits.push_back(r);
        values.push_back(answers[q].res.value);
    }
    const int64_t n = (int64_t)limits.size();
    std::vector<dg_dp_genotype_margin> rec((size_t)n * (size_t)L);
    std::vector<int32_t> best((size_t)n);
    if (n > 0) {
        if (be.dp_genotype_margins_budgets(be.ctx, nullptr, 0, called.data(), limits.data(), n, cls.data(), rec.data(), best.data()) != 0) return backend_error(be, "dp_genotype_margins_budgets");
        int64_t stats[4] = {0, 0, 0, 0};
        if (be.dp_genotype_stats && be.dp_genotype_stats(be.ctx, stats, 4) != 0) return backend_error(be, "dp_genotype_stats");
        bm.segments = stats[0];
    }
    std::string text = "r\tlevel\tvertex1\tpanel_hap1\tsegment1\tvertex2\tpanel_hap2\tsegment2\tvalue\talt_vertex1\talt_segment1\talt_vertex2\talt_segment2\talt_value\tmargin\n";
    for (int64_t q = 0; q < n; ++q) {
        BudgetGenotypeMargins::Row row;
        row.r = limits[(size_t)q];
        if (best[(size_t)q] != values[(size_t)q])
            return "--budget-genotype-margins: limit " + std::to_string(row.r) + ": the joint pass finds " + std::to_string(best[(size_t)q]) + ", the run's DP value is " + std::to_string(values[(size_t)q]);
        for (int l = 0; l < L; ++l) {
            const dg_dp_genotype_margin &r = rec[(size_t)q * (size_t)L + (size_t)l];
            if (r.value != values[(size_t)q])
                return "--budget-genotype-margins: limit " + std::to_string(row.r) + " level " + std::to_string(l) + ": the answer's cell is worth " + std::to_string(r.value) +
                       ", the run's DP value is " + std::to_string(values[(size_t)q]);
            if (l < 1 || l >= L - 1) continue;
            text += std::to_string(row.r) + '\t' + std::to_string(l) + '\t' + std::to_string(r.vertex1) + '\t' + panel_name(p, g, r.vertex1) + '\t' + segment_name(p, g, r.vertex1) + '\t' +
                    std::to_string(r.vertex2) + '\t' + panel_name(p, g, r.vertex2) + '\t' + segment_name(p, g, r.vertex2) + '\t' + std::to_string(r.value) + '\t';
            if (r.alt_vertex1 >= 0) {
                const int32_t margin = r.value - r.alt_value;
                text += std::to_string(r.alt_vertex1) + '\t' + segment_name(p, g, r.alt_vertex1) + '\t' + std::to_string(r.alt_vertex2) + '\t' + segment_name(p, g, r.alt_vertex2) + '\t' +
                        std::to_string(r.alt_value) + '\t' + std::to_string(margin);
                row.with_alternative++;
                if (margin == 0) row.margin0++;
                else if (margin > 0 && (row.min_positive_margin < 0 || margin < row.min_positive_margin)) row.min_positive_margin = margin;
            } else text += ".\t.\t.\t.\t.\t.";
            text += '\n';
        }
        bm.rows.push_back(row);
    }
    const std::string &path = p.opt.budget_genotype_margins;
    std::ofstream f(path, std::ios::out | std::ios::binary);
    if (!f.is_open()) return "cannot open budget genotype margins file " + path;
    f.write(text.data(), (std::streamsize)text.size());
    f.close();
    if (!f.good()) return "write to " + path + " failed";
    bm.wall_s = now_s() - t0;
    return "";
}

// level  vertex1  segment1  vertex2  segment2  value  delta  called: levels 1 .. L - 2, per level one row for every genotype that a pair
// of paths within -R passes through, in ascending (class1, class2) of the allele classes; (vertex1, vertex2) its best cell, delta = the
// DP value - value, called = 1 for the genotype of the answer's cell.  The header alone if no pair of paths fits -R
std::string write_genotype_table(Pipeline &p, const ExpandedGraph &g, const std::vector<int32_t> &cls, const GenotypePass &gp, const std::string &path, GenotypeTable &gt) {
    const double t0 = now_s();
    const int L = (int)g.level_off.size() - 1;
    gt = GenotypeTable();
    gt.set = true;
    std::string text = "level\tvertex1\tsegment1\tvertex2\tsegment2\tvalue\tdelta\tcalled\n";
    for (int l = 1; gp.fits && l < L - 1; ++l) {
        const int32_t c1 = cls.at((size_t)gp.paths[(size_t)l]), c2 = cls.at((size_t)gp.paths[(size_t)L + l]);
        const int64_t a = gp.level_off[(size_t)l], e = gp.level_off[(size_t)l + 1];
        int64_t at_best = 0;
        for (int64_t x = a; x < e; ++x) {
            const dg_dp_genotype_entry &r = gp.entries[x];
            const bool called = r.class1 == std::min(c1, c2) && r.class2 == std::max(c1, c2);
            text += std::to_string(l) + '\t' + std::to_string(r.vertex1) + '\t' + segment_name(p, g, r.vertex1) + '\t' + std::to_string(r.vertex2) + '\t' + segment_name(p, g, r.vertex2) +
                    '\t' + std::to_string(r.value) + '\t' + std::to_string(gp.best - r.value) + '\t' + (called ? '1' : '0') + '\n';
            at_best += r.value == gp.best;
        }
        gt.entries += e - a;
        gt.levels_with_choice += e - a >= 2;
        gt.co_optimal_levels += at_best >= 2;
        gt.max_per_level = std::max(gt.max_per_level, e - a);
    }
    std::ofstream f(path, std::ios::out | std::ios::binary);
    if (!f.is_open()) return "cannot open genotype table file " + path;
    f.write(text.data(), (std::streamsize)text.size());
    f.close();
    if (!f.good()) return "write to " + path + " failed";
    gt.wall_s = gp.wall_s + (now_s() - t0);
    return "";
}

// read  length  n_min  only_1  only_2  both  tag: one row per read in input order.  Both sequences of the answer are sketched with the
// backend's own (w,k) scheme, then every read's distinct minimizers are looked up in the two lists; tag = the haplotype with more
// private minimizers of the read, 0 where neither has more
std::string write_read_tags(Pipeline &p, const std::string *hs) {
    const Backend &be = p.be;
    if (!be.tag_reads) return "--tag-reads: this backend has no tag_reads";
    const int64_t n_reads = (int64_t)p.reads.size();
    if ((int64_t)p.tag_off.size() != n_reads + 1) return "--tag-reads: the reads were not kept (their spectrum came from elsewhere)";
    uint64_t *hh[2] = {nullptr, nullptr};
    int64_t nh[2] = {0, 0};
    for (int q = 0; q < 2; ++q) {
        int64_t *pos = nullptr;
        if (be.sketch_haplotype(be.ctx, hs[q].data(), (int64_t)hs[q].size(), p.opt.k, p.opt.w, &hh[q], &pos, &nh[q]) != 0) {
            if (q) be.free_buf(hh[0]);
            return backend_error(be, "sketch_haplotype");
        }
        be.free_buf(pos);
    }
    std::vector<dg_read_tag> rec((size_t)n_reads);
    const int rc = be.tag_reads(be.ctx, p.tag_bases.data(), p.tag_off.data(), n_reads, p.opt.k, p.opt.w, hh[0], nh[0], hh[1], nh[1], rec.data());
    be.free_buf(hh[0]); be.free_buf(hh[1]);
    if (rc != 0) return backend_error(be, "tag_reads");
    ReadTags &rt = p.sum.read_tags;
    rt = ReadTags();
    rt.set = true;
    rt.reads = n_reads;
    std::string text = "read\tlength\tn_min\tonly_1\tonly_2\tboth\ttag\n";
    for (int64_t r = 0; r < n_reads; ++r) {
        const dg_read_tag &t = rec[(size_t)r];
        const int tag = t.only_a > t.only_b ? 1 : (t.only_b > t.only_a ? 2 : 0);
        if (tag == 1) rt.hap1++; else if (tag == 2) rt.hap2++; else if (t.only_a > 0) rt.tie++; else rt.no_evidence++;
        text += p.reads[(size_t)r].first + '\t' + std::to_string(p.reads[(size_t)r].second.size()) + '\t' + std::to_string(t.n_min) + '\t' + std::to_string(t.only_a) + '\t' +
                std::to_string(t.only_b) + '\t' + std::to_string(t.both) + '\t' + std::to_string(tag) + '\n';
    }
    std::ofstream f(p.opt.tag_reads, std::ios::out | std::ios::binary);
    if (!f.is_open()) return "cannot open read tag file " + p.opt.tag_reads;
    f.write(text.data(), (std::streamsize)text.size());
    f.close();
    if (!f.good()) return "write to " + p.opt.tag_reads + " failed";
    return "";
}

}  // namespace

std::string read_pins_file(const std::string &path, std::vector<PinRow> &rows) {
    std::ifstream f(path, std::ios::in | std::ios::binary);
    if (!f.is_open()) return "--pins: cannot open " + path;
    std::string line;
    for (int n = 1; std::getline(f, line); ++n) {
        const std::string at = "--pins: line " + std::to_string(n) + ": ";
        line = line.substr(0, line.find('#'));
        while (!line.empty() && (line.back() == '\r' || line.back() == ' ' || line.back() == '\t')) line.pop_back();
        if (line.empty()) continue;
        std::vector<std::string> col;
        for (size_t a = 0; a <= line.size();) {
            size_t b = line.find('\t', a);
            if (b == std::string::npos) b = line.size();
            col.push_back(line.substr(a, b - a));
            a = b + 1;
        }
        if (col.size() < 3 || col.size() > 4) return at + "expected level, vertex1, vertex2 and an optional kind, separated by tabs; found " + std::to_string(col.size()) + " columns";
        PinRow r;
        r.line = n;
        int32_t *dst[3] = {&r.level, &r.vertex1, &r.vertex2};
        for (int q = 0; q < 3; ++q) {
            const std::string &s = col[(size_t)q];
            if (q > 0 && s == ".") { *dst[q] = -1; continue; }
            if (s.empty() || s.size() > 9 || s.find_first_not_of("0123456789") != std::string::npos)
                return at + "'" + s + "' is not a " + (q ? "vertex id (a non-negative integer, or . for any)" : "level (a non-negative integer)");
            *dst[q] = atoi(s.c_str());
        }
        const std::string kind = col.size() == 4 ? col[3] : "require";
        if (kind == "require") {}
        else if (kind == "forbid") r.forbid = true;
        else if (kind == "require-ordered") r.ordered = true;
        else if (kind == "forbid-ordered") r.forbid = r.ordered = true;
        else return at + "kind '" + kind + "' is not one of require, forbid, require-ordered, forbid-ordered";
        rows.push_back(r);
    }
    return "";
}

int Pipeline::diploid(ExpandedGraph &g, const std::vector<uint8_t> &color_homo_bv,
                      const std::vector<std::vector<AnchorRec>> &anchorsByHap, std::string &err) {
    double t0 = now_s();
    const int L = (int)g.level_off.size() - 1;
    const int R = opt.R;
    if (be.hint_dp_soon && !g.colours_split) {                         // level widths are final: the exact lattice size (the fused route has said so already)
        double cells = 0;
        for (int l = 1; l < L; ++l) { const double kw = (double)(g.level_off[l + 1] - g.level_off[l]); cells += kw * kw; }
        be.hint_dp_soon(be.ctx, (int64_t)std::min(9.0e18, cells * (R + 1)));
    }
    if (!opt.quiet && g.level_off[1] - g.level_off[0] > 1) std::cout << "There is more than one source on level zero!" << std::endl;
    dpg = DpGraphStorage();
    if (!opt.quiet) std::cout << "Creating hetro/hom-zygous colors per vertex lists" << std::endl;
    split_colours(g, color_homo_bv, dpg);
    sum.n_levels = L;
    sum.n_vertices = g.n;
    stamp("dp_prologue_flatten", t0);
    std::vector<int32_t> classes;
    if (!opt.site_margins.empty()) {                                   // what dg_dp_call_margins can hold, known before the DP: no output of any kind otherwise
        int64_t widest = 1;
        for (int l = 0; l < L; ++l) widest = std::max<int64_t>(widest, g.level_off[l + 1] - g.level_off[l]);
        if (opt.wide_levels) {                                          // the limits of the device-memory route of dg_dp_call_margins
            if (widest > 32767 || widest * ((int64_t)R + 1) > ((int64_t)1 << 24)) {
                err = "--site-margins --wide-levels: widest level " + std::to_string(widest) + " (at most 32767) x (R + 1) " + std::to_string(R + 1) + " exceeds 16777216 cells";
                return -1;
            }
        } else if (widest * ((int64_t)R + 1) > 16384) {
            err = "--site-margins: widest level " + std::to_string(widest) + " x (R + 1) " + std::to_string(R + 1) + " exceeds 16384 cells";
            return -1;
        }
    }
    const bool pinned_joint = !opt.pinned_genotype_margins.empty() || !opt.pinned_genotype_table.empty();
    if (!opt.genotype_margins.empty() || !opt.genotype_table.empty() || pinned_joint || !opt.budget_genotype_margins.empty() || !opt.phase_margins.empty() || !opt.budget_phase_margins.empty() || !opt.recombination_margins.empty() || !opt.budget_recombination_margins.empty()) {   // the limits of dg_dp_genotype_margins / dg_dp_genotype_table / dg_dp_phase_margins, known before the DP too
        int64_t widest = 1;
        for (int l = 0; l < L; ++l) widest = std::max<int64_t>(widest, g.level_off[l + 1] - g.level_off[l]);
        if (widest > 32767 || (int64_t)R + 1 > 4096) {
            err = std::string(pinned_joint ? (opt.pinned_genotype_margins.empty() ? "--pinned-genotype-table" : "--pinned-genotype-margins") : !opt.genotype_margins.empty() ? "--genotype-margins" : !opt.genotype_table.empty() ? "--genotype-table" : !opt.budget_genotype_margins.empty() ? "--budget-genotype-margins" : !opt.phase_margins.empty() ? "--phase-margins" : !opt.budget_phase_margins.empty() ? "--budget-phase-margins" : !opt.recombination_margins.empty() ? "--recombination-margins" : "--budget-recombination-margins") + ": widest level " + std::to_string(widest) + " (at most 32767), R + 1 = " + std::to_string(R + 1) + " (at most 4096)";
            return -1;
        }
    }
    if (!opt.site_margins.empty() || !opt.genotype_margins.empty() || !opt.genotype_table.empty() || pinned_joint || !opt.budget_genotype_margins.empty() || !opt.phase_margins.empty() || !opt.budget_phase_margins.empty()) {  // all these tables speak of alleles
        classes = allele_classes(g);
        if (!opt.dump_prefix.empty() && failed(write_raw_int32(opt.dump_prefix + ".cls", classes), err)) return -1;
    }
    std::vector<dg_dp_pin> pins;                                       // --pins: a row outside the graph ends the run before the DP
    if (!opt.pins_file.empty() && failed(expand_pin_rows(opt.pin_rows, g, pins), err)) { sum.pins.bad_rows = true; return -1; }
    if (!opt.dump_prefix.empty()) dump_graph(dpg, g, opt.dump_prefix + ".dpg", R);
    if (opt.dump_only) { err = "dump_only"; return 1; }

    t0 = now_s();
    if (!opt.quiet) std::cout << "Running DP" << std::endl;
    // one answer per budget: the listed ones in order, then -R itself unless it is listed (without --budgets: -R alone)
    std::vector<int32_t> budgets(opt.budgets.begin(), opt.budgets.end());
    if (std::find(budgets.begin(), budgets.end(), (int32_t)R) == budgets.end()) budgets.push_back(R);
    std::vector<ChainAnswer> answers;
    answers.reserve(budgets.size());
    for (size_t q = 0; q < budgets.size(); ++q) answers.emplace_back(R + 8);
    if (failed(run_dp(*this, g, budgets, answers, pins), err)) return -1;
    stamp("dp_level_loop", t0);

    t0 = now_s();
    const ChainAnswer &top = answers[(size_t)(std::find(budgets.begin(), budgets.end(), (int32_t)R) - budgets.begin())];
    sum.dp_value = top.res.value; sum.s_het = top.res.s_het; sum.cells = top.res.cells; sum.relaxations = top.res.relaxations;
    if (!opt.pins_file.empty() && failed(summarize_pins(*this, g, pins, top.reachable()), err)) return -1;
    if (!opt.quiet) std::cout << "DP value: " << top.res.value << std::endl;   // :776
    const auto [wp1, wp2] = top.edge_lists();
    PathReadout out;
    path_sequence(*this, g, anchorsByHap, wp1, 0, true, out);
    path_sequence(*this, g, anchorsByHap, wp2, 1, true, out);
    sum.r1 = (int)wp1.size() - 1; sum.r2 = (int)wp2.size() - 1;        // :784-785
    sum.len1 = (int64_t)out.seq[0].size(); sum.len2 = (int64_t)out.seq[1].size();
    certificate(*this, color_homo_bv, out, top.res.s_het);
    if (!opt.quiet)
        std::cout << "recombinations in P1: " << sum.r1 << ", recombinations in P2: " << sum.r2 << ", bp of P1: " << out.seq[0].length()
                  << ", bp of P2: " << out.seq[1].length() << std::endl;                 // :1307-1308
    if (failed(write_diploid_fasta(opt.hap_file, out.seq), err)) return -1;
    if (failed(write_budget_fastas(*this, g, anchorsByHap, answers), err)) return -1;
    if (!opt.budget_table.empty() && failed(write_budget_table(opt.budget_table, sum.budget_rows), err)) return -1;
    stamp("traceback+write", t0);
    if (!opt.objective_table.empty()) {
        t0 = now_s();
        if (failed(write_objective_table(*this, budgets, answers), err)) return -1;
        stamp("objective_table", t0);
    }
    if (!opt.site_margins.empty()) {
        t0 = now_s();
        if (failed(write_site_margins(*this, g, classes), err)) return -1;
        stamp("site_margins", t0);
    }
    if (!opt.genotype_margins.empty() || !opt.genotype_table.empty()) {   // one pass serves both files
        t0 = now_s();
        GenotypePass gp;
        if (failed(genotype_pass(*this, g, classes, gp, !opt.genotype_table.empty()), err)) return -1;
        if (!opt.genotype_margins.empty()) {
            if (failed(write_genotype_margins(*this, g, gp, opt.genotype_margins, sum.genotype_margins, false), err)) return -1;
            stamp("genotype_margins", t0);
        }
        if (!opt.genotype_table.empty()) {
            const double t1 = opt.genotype_margins.empty() ? t0 : now_s();
            if (failed(write_genotype_table(*this, g, classes, gp, opt.genotype_table, sum.genotype_table), err)) return -1;
            stamp("genotype_table", t1);
        }
    }
    if (!opt.budget_genotype_margins.empty()) {                           // after --genotype-margins: that option alone is exactly what it was
        t0 = now_s();
        if (failed(write_budget_genotype_margins(*this, g, classes, budgets, answers), err)) return -1;
        stamp("budget_genotype_margins", t0);
    }
    if (!opt.phase_margins.empty()) {                                     // after the genotype options: each of them alone is exactly what it was
        t0 = now_s();
        if (failed(write_phase_margins(*this, g, classes), err)) return -1;
        stamp("phase_margins", t0);
    }
    if (!opt.budget_phase_margins.empty()) {                              // after --phase-margins: that option alone is exactly what it was
        t0 = now_s();
        if (failed(write_budget_phase_margins(*this, g, classes, budgets, answers), err)) return -1;
        stamp("budget_phase_margins", t0);
    }
    if (!opt.recombination_margins.empty()) {                             // after the phase options: each of them alone is exactly what it was
        t0 = now_s();
        if (failed(write_recombination_margins(*this, g), err)) return -1;
        stamp("recombination_margins", t0);
    }
    if (!opt.budget_recombination_margins.empty()) {                      // after --recombination-margins: that option alone is exactly what it was
        t0 = now_s();
        if (failed(write_budget_recombination_margins(*this, g, budgets, answers), err)) return -1;
        stamp("budget_recombination_margins", t0);
    }
    if (pinned_joint) {                                                   // the same under --pins: one pass serves both files
        t0 = now_s();
        GenotypePass gp;
        if (failed(genotype_pass(*this, g, classes, gp, !opt.pinned_genotype_table.empty(), &pins), err)) return -1;
        if (!opt.pinned_genotype_margins.empty()) {
            if (failed(write_genotype_margins(*this, g, gp, opt.pinned_genotype_margins, sum.pinned_genotype_margins, true), err)) return -1;
            stamp("pinned_genotype_margins", t0);
        }
        if (!opt.pinned_genotype_table.empty()) {
            const double t1 = opt.pinned_genotype_margins.empty() ? t0 : now_s();
            if (failed(write_genotype_table(*this, g, classes, gp, opt.pinned_genotype_table, sum.pinned_genotype_table), err)) return -1;
            stamp("pinned_genotype_table", t1);
        }
    }
    if (!opt.tag_reads.empty()) {
        t0 = now_s();
        if (failed(write_read_tags(*this, out.seq), err)) return -1;
        stamp("tag_reads", t0);
    }
    return 0;
}

}  // namespace dg

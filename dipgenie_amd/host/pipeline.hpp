// Host-side mirror of the reference's Solver / Approximator objects for the diploid hot path.
//
// Everything that is NOT one of the two device loops stays here, restated so that vertex numbering,
// adjacency order and every tie-break match the reference exactly.  One translation unit per stage:
//   pipeline.cpp        driver (main.cpp:117-165) and
//                       Solver::read_gfa                       /root/reference/src/solver.cpp:27-227
//   anchors.cpp         Solver::compute_and_classify_anchors   /root/reference/src/solver.cpp:449-887
//   expanded_graph.cpp  ExpandedGraph::topologically_reorder   /root/reference/src/ExpandedGraph.hpp:29-102
//                       ExpandedGraph::strict_bfs_levelize_and_reorder   /root/reference/src/ExpandedGraph.hpp:269-409
//                       (and DpGraphStorage, the .dpg file)
//   haploid_dp.cpp      haploid dp_approximation_solver        /root/reference/src/approximator.cpp:44-168 (host twin of the device loop)
//   solve.cpp           Approximator::solve                    /root/reference/src/approximator.cpp:1014-1331 (literal graph construction)
//   fast_graph.cpp      the fused route to the same levelized graph
//   diploid.cpp         DP prologue; traceback -> sequences, certificate   /root/reference/src/approximator.cpp:362-453, 720-1011
// The two device loops are reached only through the Backend table (= include/dipgenie_hip.h).
#pragma once
#include <cstdint>
#include <map>
#include <memory>
#include <string>
#include <thread>
#include <initializer_list>
#include <utility>
#include <vector>

#include "../../include/dipgenie_hip.h"
#include "fitter.hpp"
#include "gfa_reader.hpp"

namespace dg {

// std::vector that leaves trivially-constructible elements uninitialised on resize: the graph arrays hold tens of millions of
// entries that are all written (in parallel) right after the allocation -- a serial zero fill first costs as much as the fill
template <class T> struct NoInitAlloc : std::allocator<T> {
    template <class U> struct rebind { using other = NoInitAlloc<U>; };
    NoInitAlloc() = default;
    template <class U> NoInitAlloc(const NoInitAlloc<U> &) {}
    template <class U, class... A> void construct(U *p, A &&...a) {
        if constexpr (sizeof...(A) == 0) ::new ((void *)p) U; else ::new ((void *)p) U(std::forward<A>(a)...);
    }
};
template <class T> using uvec = std::vector<T, NoInitAlloc<T>>;

struct Backend {     // same signatures as the C ABI, plus an opaque ctx
    void *ctx = nullptr;
    int (*sketch_reads)(void *, const char *, const int64_t *, int64_t, int, int, uint64_t **, int32_t **, int64_t *) = nullptr;
    int (*sketch_haplotype)(void *, const char *, int64_t, int, int, uint64_t **, int64_t **, int64_t *) = nullptr;
    int (*dp_solve_diploid)(void *, const dg_dp_graph *, dg_dp_result *) = nullptr;
    int (*dp_solve_haploid)(void *, const dg_hap_graph *, int32_t *dp, int32_t *back_vtx, int32_t *back_r) = nullptr;   // optional
    void (*free_buf)(void *) = nullptr;
    // optional: haplotype index with vertex spans + anchor join / filter / sort behind the boundary
    int (*anchor_begin)(void *, int32_t n_haps, int32_t n_vertices, const int32_t *top_order_map, int k, int w) = nullptr;
    int (*anchor_add_haplotype)(void *, int32_t h, const char *seq, int64_t len, const int32_t *step_vtx, const int64_t *step_start, int64_t n_steps,
                                int64_t *n_minimizers) = nullptr;
    int (*anchor_finish)(void *, const uint64_t *sp_hash, int64_t n_sp, float min_shared, dg_anchor_result *out) = nullptr;
    // optional (sharded runs): a haplotype whose minimizer list was sketched by another rank
    int (*anchor_add_haplotype_sketched)(void *, int32_t h, int64_t len, const uint64_t *hash, const int64_t *pos, int64_t n, const int32_t *step_vtx,
                                         const int64_t *step_start, int64_t n_steps) = nullptr;
    // optional (--budgets): the diploid graph loaded once, then the read-out of several recombination budgets from one sweep
    // (dg_dp_load_graph + dg_dp_run_budgets); nothing in a run without --budgets needs them
    int (*dp_load_graph)(void *, const dg_dp_graph *) = nullptr;
    int (*dp_run_budgets)(void *, const int32_t *budgets, int32_t n_budgets, dg_dp_result *results) = nullptr;
    void (*hint_dp_soon)(void *, int64_t est_cells) = nullptr;   // optional, may be called repeatedly (latest wins): the DP will run later with about est_cells cells
    const char *(*last_error)() = nullptr;
    // optional (--site-margins): after dp_run_budgets, both haplotypes of the answer at a budget against the best vertex of another
    // class per level (dg_dp_call_margins)
    int (*dp_call_margins)(void *, int32_t budget, const int32_t *vertex_class, dg_dp_call_margin *levels, int32_t *paths) = nullptr;
    // optional (--objective-table): after dp_run_budgets, the distinct-colour objective of the answers at the listed budgets
    // (dg_dp_answer_objectives)
    int (*dp_answer_objectives)(void *, const int32_t *budgets, int32_t n_budgets, dg_dp_pair_objective *out) = nullptr;
    // optional (--tag-reads): every read's distinct minimizers against the minimizer lists of the two answer sequences (dg_sketch_tag_reads)
    int (*tag_reads)(void *, const char *bases, const int64_t *read_off, int64_t n_reads, int k, int w, const uint64_t *hash_a, int64_t n_a,
                     const uint64_t *hash_b, int64_t n_b, dg_read_tag *out) = nullptr;
    // optional (--genotype-margins): after dp_run_budgets, the answer at a budget as two rows of vertex ids (dg_dp_get_answer_paths), the
    // margin of its genotype against the best other genotype per level with both haplotypes free (dg_dp_genotype_margins), and that
    // call's statistics (dg_dp_get_genotype_stats)
    int (*dp_answer_paths)(void *, int32_t budget, int32_t *paths) = nullptr;
    int (*dp_genotype_margins)(void *, const int32_t *called, int64_t n_called, int32_t budget, const int32_t *vertex_class, dg_dp_genotype_margin *levels,
                               int32_t *vertex_values, int32_t *best_value) = nullptr;
    int (*dp_genotype_stats)(void *, int64_t *out, int n) = nullptr;
    // optional (--genotype-table): every genotype of every level with its best pair of paths, and the margin records of the call above
    // from the same pass (dg_dp_genotype_table); *entries is released with free_buf
    int (*dp_genotype_table)(void *, int32_t budget, const int32_t *vertex_class, const int32_t *called, int64_t n_called, dg_dp_genotype_margin *levels, int64_t *level_off,
                             dg_dp_genotype_entry **entries, int64_t *n_entries, int32_t *best_value) = nullptr;
    // optional (--pins): the run of dp_run_budgets with per-level cell constraints (dg_dp_run_pinned), and that run's statistics
    // (dg_dp_get_pin_stats)
    int (*dp_run_pinned)(void *, const dg_dp_pin *pins, int64_t n_pins, const int32_t *budgets, int32_t n_budgets, dg_dp_result *results) = nullptr;
    int (*dp_pin_stats)(void *, int64_t *out, int n) = nullptr;
    // optional (--pinned-genotype-margins / --pinned-genotype-table): the two genotype calls above on the DP that the pins constrain
    // (dg_dp_genotype_margins_pinned, dg_dp_genotype_table_pinned)
    int (*dp_genotype_margins_pinned)(void *, const dg_dp_pin *pins, int64_t n_pins, const int32_t *called, int64_t n_called, int32_t budget, const int32_t *vertex_class,
                                      dg_dp_genotype_margin *levels, int32_t *vertex_values, int32_t *best_value) = nullptr;
    int (*dp_genotype_table_pinned)(void *, const dg_dp_pin *pins, int64_t n_pins, int32_t budget, const int32_t *vertex_class, const int32_t *called, int64_t n_called,
                                    dg_dp_genotype_margin *levels, int64_t *level_off, dg_dp_genotype_entry **entries, int64_t *n_entries, int32_t *best_value) = nullptr;
    // optional (--budget-genotype-margins): the margin records of dp_genotype_margins for one called genotype per listed limit, each at
    // its own budget, from one joint pass (dg_dp_genotype_margins_budgets)
    int (*dp_genotype_margins_budgets)(void *, const dg_dp_pin *pins, int64_t n_pins, const int32_t *called, const int32_t *budgets, int64_t n_called, const int32_t *vertex_class,
                                       dg_dp_genotype_margin *levels, int32_t *best_values) = nullptr;
    // optional (--phase-margins): cis against trans for every pair of neighbouring het levels of one called pair (dg_dp_phase_margins),
    // and that call's statistics (dg_dp_get_phase_stats)
    int (*dp_phase_margins)(void *, const int32_t *called, int32_t budget, const int32_t *vertex_class, dg_dp_phase_margin *records, int64_t *n_records, int32_t *best_value) = nullptr;
    int (*dp_phase_stats)(void *, int64_t *out, int n) = nullptr;
    // optional (--budget-phase-margins): the records of dp_phase_margins for one called pair per listed limit, each at its own budget, from
    // one joint pass (dg_dp_phase_margins_budgets), and that call's statistics (dg_dp_get_phase_budget_stats)
    int (*dp_phase_margins_budgets)(void *, const int32_t *called, const int32_t *budgets, int64_t n_called, const int32_t *vertex_class, dg_dp_phase_margin *records,
                                    int64_t *record_off, int32_t *best_values) = nullptr;
    int (*dp_phase_budget_stats)(void *, int64_t *out, int n) = nullptr;
    // optional (--recombination-margins): per transition the best pair of paths with 0, 1 or 2 crossovers there and what the called hops are
    // worth (dg_dp_recombination_margins), that call's statistics (dg_dp_get_recombination_stats), and the score of a pair of paths
    // (dg_dp_score_paths: r1 + r2 of the answer, against the called crossovers)
    int (*dp_recombination_margins)(void *, int32_t budget, const int32_t *called, int64_t n_called, dg_dp_recombination_margin *records, int32_t *called_out, int32_t *best_value) = nullptr;
    int (*dp_recombination_stats)(void *, int64_t *out, int n) = nullptr;
    int (*dp_score_paths)(void *, const int32_t *paths, int64_t n_pairs, dg_dp_pair_score *out) = nullptr;
    // optional (--budget-recombination-margins): the records of dp_recombination_margins for one called pair per listed limit, each at its
    // own budget, from one joint pass (dg_dp_recombination_margins_budgets), and that call's statistics
    int (*dp_recombination_margins_budgets)(void *, const int32_t *budgets, int64_t n, const int32_t *called, dg_dp_recombination_margin *records, int32_t *called_out,
                                            int32_t *best_values) = nullptr;
    int (*dp_recombination_budget_stats)(void *, int64_t *out, int n) = nullptr;
};

// one row of a --pins file: level, vertex ids as --genotype-table prints them (-1: any), require / forbid, the unordered genotype (two
// pins of the C ABI where the vertices differ) or the ordered cell (one)
struct PinRow { int32_t level = 0, vertex1 = -1, vertex2 = -1; bool forbid = false, ordered = false; int line = 0; };
// parses FILE (rows "level <tab> vertex1 <tab> vertex2 [<tab> kind]", '.' = any, '#' starts a comment); "" or what is wrong with the first bad row
std::string read_pins_file(const std::string &path, std::vector<PinRow> &rows);

struct Options {
    int threads = 4;          // -t
    int ploidy = 2;           // -p
    int R = 18;               // -R
    int k = 31, w = 25;       // -k -w
    float threshold = 1.0f;   // -T
    bool debug = false;       // -d
    bool quiet = false;       // (ours) suppress progress chatter
    std::string gfa_file, reads_file, hap_file;   // -g -r -o
    std::string dump_prefix;  // (ours) if set, dump the levelized DP graph to <prefix>.dpg
    bool dump_only = false;   // (ours, tests) stop after the dump
    std::string anchor_dump;  // (ours, tests) if set, write Anchor_hits + homo_bv as text (format of oracle/ref_harness.cpp `anchors`)
    int haploid_mode = 0;        // (ours) haploid (vertex, r) tables: 0 = by graph shape, 1 = host gather loop, 2 = device (if the backend offers it)
    bool leak_at_exit = false;   // (ours) the process exits right after run(): skip the teardown of the big graph objects
    std::vector<int> budgets;    // (ours) --budgets: recombination budgets below -R answered from the same DP pass (diploid); -R itself is always solved
    std::string budget_table;    // (ours) --budget-table: TSV of the listed budgets
    bool host_anchors = false;   // (ours, tests) keep the anchor join / filter / sort on the host even if the backend offers it
    std::string site_margins;    // (ours) --site-margins: TSV of the call margins of both haplotypes of the answer at -R, per level (diploid)
    bool wide_levels = false;    // (ours) --wide-levels, with --site-margins: the backend keeps the level state of dp_call_margins in device memory where LDS cannot hold it
    std::string objective_table; // (ours) --objective-table: TSV of the surrogate and the distinct-colour objective of the answer at every listed budget (diploid)
    std::string genotype_margins; // (ours) --genotype-margins: TSV of the margin of the answer's genotype at -R against the best other genotype, per level, both haplotypes free (diploid)
    std::string budget_genotype_margins; // (ours) --budget-genotype-margins, with --budgets: the rows of --genotype-margins for the answer at every listed limit that has one, behind a column r, from one joint pass (diploid)
    std::string genotype_table;  // (ours) --genotype-table: TSV with one row per genotype of every level: its best pair of paths against the answer at -R, both haplotypes free (diploid)
    std::string pins_file;       // (ours) --pins: the DP runs under the cell constraints of this file's rows (diploid); parsed into pin_rows before anything else runs
    std::vector<PinRow> pin_rows;
    std::string pinned_genotype_margins; // (ours) --pinned-genotype-margins, with --pins: the file of --genotype-margins for the DP under the pins, the called cells those of the pinned answer at -R
    std::string pinned_genotype_table;   // (ours) --pinned-genotype-table, with --pins: the file of --genotype-table for the DP under the pins
    std::string phase_margins;   // (ours) --phase-margins: TSV with one row per pair of neighbouring het levels of the answer at -R: the best pair of paths that keeps its phase against the best that switches it (diploid)
    std::string budget_phase_margins; // (ours) --budget-phase-margins, with --budgets: the rows of --phase-margins for the answer at every listed limit that has one, behind a column r, from one joint pass (diploid)
    std::string recombination_margins; // (ours) --recombination-margins: TSV with one row per transition: the crossovers the answer at -R spends there against the best pair of paths that spends another number there (diploid)
    std::string budget_recombination_margins; // (ours) --budget-recombination-margins, with --budgets: the rows of --recombination-margins for the answer at every listed limit that has one, behind a column r, from one joint pass (diploid)
    std::string tag_reads;       // (ours) --tag-reads: TSV with one row per read: which haplotype of the answer at -R its minimizers support (diploid)
};

// ExpandedGraph.hpp:16-26, flattened: CSR adjacency (per-vertex order = the reference's push order),
// CSR colours, and original-vertex lists as (offset, length) into one pool (dummies share their
// parent's list instead of copying it, ExpandedGraph.hpp:330).
struct ExpandedGraph {
    int32_t n = 0;
    uvec<int64_t> adj_off;                      // [n+1]
    uvec<int32_t> adj_dst;
    uvec<uint8_t> adj_w;
    uvec<int32_t> haplotype, level;             // (level: literal route only; the vertex ids are level-sorted, see level_of)
    uvec<uint32_t> orig_off, orig_len;
    uvec<int32_t> orig_pool;
    uvec<int64_t> col_off;                      // [n+1]  (literal route; the fused route writes the HOM / HET split directly)
    uvec<int32_t> col_pool;
    uvec<int32_t> level_off;                    // [L+1] after levelize (vertex ids are level-sorted)
    bool colours_split = false;                 // hom_* / het_* below are filled (Pipeline::build_levelized_fast)
    uvec<int64_t> hom_off, het_off;             // [n+1] sorted-unique HOM / HET colour CSR (approximator.cpp:431-453)
    uvec<int32_t> hom_col, het_col;
    int64_t deg(int v) const { return adj_off[v + 1] - adj_off[v]; }
    int64_t ncol(int v) const { return col_off[v + 1] - col_off[v]; }
    void topologically_reorder(int sink);
    int strict_bfs_levelize_and_reorder();
  private:
    void permute(const uvec<int32_t> &order);   // new vertex i = old vertex order[i]
};

// colour list of an anchor record: nearly always one entry (its own colour), a few more after containment
// propagation -- two inline slots, heap only beyond (millions of records at MHC scale)
class ColourList {
    int inl_[2] = {0, 0};
    uint32_t n_ = 0;
    std::vector<int> *more_ = nullptr;
    void spill() { more_ = new std::vector<int>(inl_, inl_ + n_); }
public:
    ColourList() = default;
    ColourList(std::initializer_list<int> il) { for (int c : il) push_back(c); }
    ColourList(const ColourList &o) : n_(o.n_), more_(o.more_ ? new std::vector<int>(*o.more_) : nullptr) { inl_[0] = o.inl_[0]; inl_[1] = o.inl_[1]; }
    ColourList(ColourList &&o) noexcept : n_(o.n_), more_(o.more_) { inl_[0] = o.inl_[0]; inl_[1] = o.inl_[1]; o.more_ = nullptr; o.n_ = 0; }
    ColourList &operator=(ColourList o) noexcept { std::swap(inl_[0], o.inl_[0]); std::swap(inl_[1], o.inl_[1]); std::swap(n_, o.n_); std::swap(more_, o.more_); return *this; }
    ~ColourList() { delete more_; }
    void push_back(int c) {
        if (!more_ && n_ < 2) { inl_[n_++] = c; return; }
        if (!more_) spill();
        more_->push_back(c); ++n_;
    }
    const int *begin() const { return more_ ? more_->data() : inl_; }
    const int *end() const { return begin() + n_; }
    size_t size() const { return n_; }
};

struct AnchorRec {            // approximator.h:11-18
    int startOrg, endOrg, startExp, endExp;
    ColourList colours;
    int nodeID;
};

// Flattened levelized graph in dg_dp_graph layout (owning storage).
struct DpGraphStorage {
    uvec<int32_t> level_off, out_dst, hom_col, het_col;
    uvec<int64_t> out_off, hom_off, het_off;
    uvec<uint8_t> out_w;
    dg_dp_graph view(int R) const;
    bool save(const std::string &path, int R) const;   // little-endian binary, see expanded_graph.cpp
    bool load(const std::string &path, int &R);
};

struct BudgetRow {            // --budgets: one listed budget (reachable = the sink's plane r holds a path)
    int32_t r = 0;
    bool reachable = false;
    int32_t dp_value = 0, r1 = -1, r2 = -1;
    int64_t len1 = 0, len2 = 0;
};

struct ObjectiveRow {         // --objective-table: one listed budget (reachable as in BudgetRow)
    int32_t r = 0;
    bool reachable = false;
    int32_t dp_value = 0;
    dg_dp_pair_objective rec = {-1, -1, -1, -1};
};

struct SiteMargins {          // --site-margins: per haplotype, over the levels 1 .. L - 2
    bool set = false;
    int64_t with_alternative[2] = {0, 0}, margin0[2] = {0, 0};
    int32_t min_positive_margin[2] = {-1, -1};   // -1: no level with a positive margin
    double wall_s = 0;
};

struct GenotypeTable {        // --genotype-table: over the levels 1 .. L - 2
    bool set = false;
    int64_t entries = 0, levels_with_choice = 0, co_optimal_levels = 0, max_per_level = 0;   // rows; levels with >= 2 genotypes; with >= 2 at the DP value; most rows of a level
    double wall_s = 0;
};

struct GenotypeMargins {      // --genotype-margins: over the levels 1 .. L - 2
    bool set = false;
    int64_t with_alternative = 0, margin0 = 0, segments = 0;
    int32_t min_positive_margin = -1;            // -1: no level with a positive margin
    double wall_s = 0;
};

struct BudgetGenotypeMargins { // --budget-genotype-margins: per listed limit with an answer the fields of GenotypeMargins; one device call for all
    bool set = false;
    struct Row { int32_t r = 0; int64_t with_alternative = 0, margin0 = 0; int32_t min_positive_margin = -1; };
    std::vector<Row> rows;
    int64_t segments = 0;
    double wall_s = 0;
};

struct PhaseMargins {         // --phase-margins: over the pairs of neighbouring het levels of the answer at -R
    bool set = false;
    int64_t het_levels = 0, records = 0, with_alternative = 0, margin0 = 0, segments = 0;   // with_alternative: records whose trans is reachable
    int32_t min_positive_margin = -1;            // -1: no record with a positive margin
    double wall_s = 0;
};

struct BudgetPhaseMargins {   // --budget-phase-margins: per listed limit with an answer the fields of PhaseMargins; one device call for all
    bool set = false;
    struct Row { int32_t r = 0; int64_t het_levels = 0, records = 0, with_alternative = 0, margin0 = 0; int32_t min_positive_margin = -1; };
    std::vector<Row> rows;
    int64_t seed_keys = 0, slot_levels = 0, segments = 0;   // of the call: distinct seeded states, the sum over the levels of the live ones
    double wall_s = 0;
};

struct RecombinationMargins { // --recombination-margins: over the transitions of the answer at -R
    bool set = false;
    int64_t transitions = 0, called_recombinations = 0, breakpoints_margin0 = 0, co_optimal_elsewhere = 0, segments = 0;   // breakpoints: rows with s_called > 0
    int32_t min_positive_breakpoint_margin = -1; // -1: no breakpoint with a positive margin
    double wall_s = 0;
};

struct BudgetRecombinationMargins {   // --budget-recombination-margins: per listed limit with an answer the counts of RecombinationMargins; one device call for all
    bool set = false;
    struct Row { int32_t r = 0; RecombinationMargins counts; };
    std::vector<Row> rows;
    int64_t segments = 0;
    double wall_s = 0;
};

struct ReadTags {             // --tag-reads: hap1 / hap2 = reads with more private minimizers of that haplotype; tie: as many of both (> 0); no_evidence: none of either
    bool set = false;
    int64_t reads = 0, hap1 = 0, hap2 = 0, tie = 0, no_evidence = 0;
};

struct PinSummary {           // --pins: rows of the file, pins and pinned levels of the run, level pairs it ran as two launches, whether the answer at -R passes only allowed cells
    bool set = false, bad_rows = false;          // bad_rows: a row names a level or a vertex the graph does not have (the run ended before the DP)
    int64_t rows = 0, pins = 0, levels = 0, pairs_as_singles = 0;
    bool satisfied = false;
};

struct Summary {              // what tests and the CLI report
    int32_t dp_value = 0, s_het = 0, r1 = -1, r2 = -1, obj = 0, best_r_haploid = -1;
    int64_t len1 = 0, len2 = 0;
    int64_t spectrum = 0, n_levels = 0, n_vertices = 0, n_colours = 0;
    uint64_t cells = 0, relaxations = 0;
    std::vector<int64_t> minimizers_per_hap, anchors_per_hap;
    KGFitResult fit;
    std::vector<std::pair<std::string, double>> stage_s;
    std::vector<BudgetRow> budget_rows;   // --budgets: in the order listed
    SiteMargins site_margins;
    GenotypeMargins genotype_margins;
    GenotypeTable genotype_table;
    BudgetGenotypeMargins budget_genotype_margins;
    GenotypeMargins pinned_genotype_margins;   // --pinned-genotype-margins: the same fields, of the DP under --pins
    GenotypeTable pinned_genotype_table;       // --pinned-genotype-table
    PhaseMargins phase_margins;
    BudgetPhaseMargins budget_phase_margins;
    RecombinationMargins recombination_margins;
    BudgetRecombinationMargins budget_recombination_margins;
    std::vector<ObjectiveRow> objective_rows;   // --objective-table: the listed budgets in order (without --budgets: -R)
    ReadTags read_tags;
    PinSummary pins;
};

// One anchor occurrence: vertex list vpool[off, off+len) of read-minimizer id `a` on haplotype `h`.
struct Occ { int32_t a, h; uint32_t off, len; };

// One haplotype laid out along its walk: start offset of every step (one more entry: the total length) and, on request,
// node_seq concatenated along paths[h] (solver.cpp:283-288).
struct HapAssembly {
    std::vector<int64_t> step_start;
    size_t total = 0;
    std::string seq;
};

class Pipeline {
  public:
    ~Pipeline() { if (fit_thread.joinable()) fit_thread.join(); }
    Options opt;
    Backend be;
    Summary sum;

    // ---- Solver state (solver.h:73-85) ----
    uint32_t n_vtx = 0, num_walks = 0;
    std::vector<std::vector<uint32_t>> adj_list;
    std::vector<std::string> node_seq;
    std::vector<std::string> node_name;    // GFA segment names (kept with --site-margins / --genotype-margins / --genotype-table only)
    std::vector<std::vector<uint32_t>> paths;
    std::vector<int32_t> top_order_map;
    std::vector<std::string> hap_id2name;
    std::vector<std::pair<std::string, std::string>> reads;
    // --tag-reads only: the concatenated bases and the offsets the spectrum was computed from, kept for the tagging after the DP
    std::string tag_bases;
    std::vector<int64_t> tag_off;
    int32_t count_sp_r = 0;
    // Anchor_hits[a][h] flattened: occs sorted by (a, h, final occurrence order)
    std::vector<Occ> occs;
    std::vector<int32_t> vpool;
    std::vector<uint8_t> homo_bv;          // per read-minimizer id

    // ---- sharded runs (dipgenie_amd/run_sharded.py, BASELINE configs[3]): what other ranks computed, handed in before run_loaded() ----
    // Sp_R keys in ascending order with kmer_count (solver.cpp:533-555, 711-732) = ShardedSketch.gather_spectrum; optionally the
    // multiplicity histogram Hist_kmer (:745-755) the ranks all-reduced, checked against the one derived from the counts
    bool spectrum_injected = false;
    std::vector<uint64_t> inj_sp_hash;
    std::vector<int32_t> inj_sp_count;
    std::vector<int64_t> inj_hist;
    // index_kmers' window loop per haplotype (hash, position of the winning k-mer: dg_sketch_haplotype), sketched by the owner rank
    struct HapSketch { std::vector<uint64_t> hash; std::vector<int64_t> pos; bool set = false; };
    std::vector<HapSketch> inj_hap;
    std::string haplotype_sequence(uint32_t h) const;   // node_seq concatenated along paths[h] (solver.cpp:283-288)
    HapAssembly assemble_haplotype(uint32_t h, bool with_sequence) const;

    int load_graph(std::string &err);      // gfa_read + Solver::read_gfa
    int run_loaded(std::string &err);      // everything after load_graph (main.cpp:163-165)
    int load_reads(std::string &err);      // Solver::read_ip_reads
    int compute_and_classify_anchors(std::string &err);
    int solve(std::string &err);           // Approximator::solve (writes the FASTA)
    int run(std::string &err);             // main.cpp:117-165
    bool dump_anchors(const std::string &path) const;

    // exposed for tests
    DpGraphStorage dpg;

  private:
    void read_gfa_from(const GfaGraph &g);
    std::vector<int> haploid_dp(const ExpandedGraph &g, int R, std::string &err);
    int diploid(ExpandedGraph &g, const std::vector<uint8_t> &color_homo_bv,
                const std::vector<std::vector<AnchorRec>> &anchorsByHap, std::string &err);
    // fused + threaded route from Anchor_hits to the levelized graph (fast_graph.cpp); false: take the literal route
    bool build_levelized_fast(ExpandedGraph &g, std::vector<std::vector<AnchorRec>> &anchorsByHap, std::vector<uint8_t> &color_homo_bv);
    void stamp(const char *name, double t0);
    void clamp_threads();                  // -t0 / negative: every num_threads clause sees a valid count
    double t_run0 = 0;
    bool reads_loaded = false;
    // fit + classify on its own thread (compute_and_classify_anchors starts it, wait_fit joins it)
    std::thread fit_thread;
    bool fit_pending = false;
    double fit_t0 = 0;
    int64_t fit_n_hom = 0;
    std::vector<int32_t> fit_sp_count;
    std::string start_fit(std::vector<int32_t> &sp_count);   // "" or the error; takes the counts
    void fit_and_classify(const std::vector<HistBin> &hist, int max_mult, int threads);
    void wait_fit();
    int solve_fused(double t0, bool &declined, std::string &err);   // fast_graph.cpp's route; declined: take the literal one
    int solve_literal(double t0, std::string &err);
};

double now_s();

}  // namespace dg

/* include/dipgenie_hip.h -- C ABI of libdipgenie_hip.so (MI355X / gfx950).
 *
 * The drop-in boundary for DipGenie's diploid hot path.  The reference has no FFI/plugin layer; the
 * seams these entry points replace are C++ member calls (all citations relative to the reference):
 *
 *   dg_dp_solve_diploid     replaces the level loop + sink read-out of
 *                           Approximator::diploid_dp_approximation_solver
 *                           (src/approximator.h:26, src/approximator.cpp:532-716 and :757-785)
 *   dg_dp_solve_haploid     replaces the scatter loop of Approximator::dp_approximation_solver
 *                           (src/approximator.h:25, src/approximator.cpp:44-72)
 *   dg_anchor_*             replace the vertex-span mapping of Solver::index_kmers, Solver::compute_anchors, the
 *                           shared-anchor filter and the occurrence sort (src/solver.cpp:343-357, 415-446, 560-663)
 *   dg_sketch_reads         replaces the per-read Solver::compute_hashes loop and the Sp_R /
 *                           kmer_count maps (src/solver.h:101, src/solver.cpp:526-546, 711-732)
 *   dg_sketch_haplotype     replaces the window loop of Solver::index_kmers
 *                           (src/solver.h:100, src/solver.cpp:302-361); the position -> vertex-span
 *                           mapping (:343-357) stays in the host code
 *   dg_hash_kmers           exposes hash128_to_64_ (src/solver.cpp:16-24) for known-answer tests
 *
 * Conventions: plain pointers and sizes only; `int` return (0 = ok, <0 = error, message from
 * dg_last_error()); no exceptions cross the boundary; one dg_ctx <-> one HIP device + stream; a ctx
 * is not thread-safe, different ctxs are independent.  "host" pointers are ordinary process memory;
 * "_dev" entry points take device pointers (e.g. torch tensors' data_ptr()) and run on the ctx
 * stream without synchronising unless stated.  There is NO CPU fallback: every entry point fails
 * with DG_ERR_NO_DEVICE when no gfx950 device is usable.
 */
#ifndef DIPGENIE_HIP_H
#define DIPGENIE_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define DG_OK              0
#define DG_ERR_ARG        -1
#define DG_ERR_NO_DEVICE  -2
#define DG_ERR_HIP        -3
#define DG_ERR_OOM        -4
#define DG_ERR_UNSUPPORTED -5
#define DG_ERR_STATE      -6

typedef struct dg_ctx dg_ctx;

/* ---- context ---- */
dg_ctx     *dg_create(int device);                 /* NULL on failure (see dg_last_error) */
void        dg_destroy(dg_ctx *);
const char *dg_last_error(void);                   /* thread-local message of the last failure */
int         dg_set_stream(dg_ctx *, void *hip_stream);   /* adopt an external hipStream_t (e.g. torch's) */
int         dg_synchronize(dg_ctx *);
int         dg_device_info(dg_ctx *, char *name, int name_cap, int *n_cu, int64_t *hbm_bytes);
int         dg_hip_versions(int *compiled, int *runtime);   /* HIP_VERSION of the build / of the runtime bound in this process (major * 10^7 + minor * 10^5 + patch) */

/* ---- diploid pair-of-paths DP ---- */
typedef struct dg_dp_graph {          /* levelized expanded graph, vertex ids already level-sorted */
    int32_t n_vertices, n_levels, R;
    const int32_t *level_off;         /* [n_levels+1]; level 0 = {source}, last level = {sink} */
    const int64_t *out_off;           /* [n_vertices+1] out-CSR, adjacency order preserved */
    const int32_t *out_dst;           /* every edge goes from level l to level l+1 */
    const uint8_t *out_w;             /* recombination weight 0/1 */
    const int64_t *hom_off, *het_off; /* [n_vertices+1] sorted-unique colour CSR (HOM / HET colours) */
    const int32_t *hom_col, *het_col; /* score deltas are 16 bits wide: 2 * (longest HOM list) + 4 * (longest HET list) must not exceed
                                         65535 and no list may hold more than 16383 ids, or the load fails with DG_ERR_UNSUPPORTED */
} dg_dp_graph;

typedef struct dg_dp_result {         /* sink state at r = R (approximator.cpp:774-785) */
    int32_t value, s_het, n_p1, n_p2;
    int32_t *p1_from, *p1_to, *p2_from, *p2_to;   /* caller-provided, capacity `cap` each (>= R+2) */
    int32_t cap;
    uint64_t cells, relaxations;      /* work counters: sum k^2(R+1), sum (sum outdeg)^2 (R+1) */
} dg_dp_result;

typedef struct dg_dp_timing {         /* HIP-event times of the last dg_dp_run, milliseconds */
    float delta_ms;                   /* score-delta precompute kernel(s) */
    float forward_ms;                 /* level sweep (segmented lattice: the value-only first pass) */
    float traceback_ms;               /* back-pointer walk + edge-list extraction (segmented lattice: plus the
                                         re-sweeps of the segments with back-pointers) */
    float total_ms;                   /* first launch -> last kernel done */
    int64_t n_forward_launches;
    uint64_t edge_pairs;              /* sum over levels of (in-edges into level)^2 */
    uint64_t colour_entries;          /* colour list entries read by the delta kernel */
    uint64_t state_bytes, bp_bytes, delta_bytes;   /* device allocations */
    int32_t n_segments;               /* 1: the back-pointer lattice was resident; > 1: checkpoint + recompute in that many segments */
    int32_t n_chunks;                 /* lattice chunks the levels were packed into */
} dg_dp_timing;

/* optional: reserve about `bytes` of back-pointer lattice (bytes <= 0: 60 % of the free HBM) in a background
 * thread, in 8 GB chunks; may be called again with a better figure (the latest call wins, chunks already mapped
 * are kept). Mapping 100+ GB takes seconds and stalls every other HIP call meanwhile, so the CLI issues it where
 * only host work follows; dg_dp_load_graph adopts the chunks and dg_dp_run waits for any still missing. */
int dg_dp_prealloc(dg_ctx *, int64_t bytes);
/* validate + upload + build in-CSR; resident until the next load.  The refusals, with the text of dg_last_error (U, V vertices, L a level):
 *   DG_ERR_ARG          a null array
 *   DG_ERR_ARG          "bad sizes": n_vertices < 2, n_levels < 2, or R outside 0..4096
 *   DG_ERR_ARG          "level_off must span [0, n_vertices]"; "level 0 must hold exactly the source vertex"; "level L is empty"
 *   DG_ERR_UNSUPPORTED  "level width W exceeds the supported 32768"
 *   DG_ERR_ARG          "out_off must start at 0"; "out_off not monotone at U" (a list that ends before it starts, or outside 0..out_off[n_vertices])
 *   DG_ERR_UNSUPPORTED  "unsupported number of edges": out_off[n_vertices] outside 0..2^31 - 1
 *   DG_ERR_ARG          "edge U->V does not go to the next level" (V outside 0..n_vertices - 1 included)
 *   DG_ERR_ARG          "edge weight W > 1"
 *   DG_ERR_UNSUPPORTED  "parallel edges with different weights into vertex V" (the tie order would depend on the schedule)
 *   DG_ERR_ARG          "colour offsets must start at 0" / "must be non-negative"; "colour offsets not monotone at V" (as for out_off)
 *   DG_ERR_ARG          "colour list of vertex V is not sorted-unique"
 *   DG_ERR_UNSUPPORTED  colour lists too long for the 16-bit score deltas (see dg_dp_graph)
 * and DG_ERR_OOM where state, tables or lattice do not fit.  Both constructions of the tables (device kernels; host threads: option
 * host_tables) refuse alike; where one defect shows at several vertices, which of them is named is not defined.  No array is read
 * outside [0, its offsets' last entry).  A refused load leaves NO graph loaded, whatever was resident before: the run, digest and
 * query entry points answer DG_ERR_STATE until a load succeeds, which then behaves as in a fresh context.
 * Valid and answered with value NEG_INF = INT32_MIN / 4 and empty edge lists where nothing reaches the sink: vertices without out-edges
 * (dead ends) on any level, levels that no edge enters, and a graph without any edge. */
int dg_dp_load_graph(dg_ctx *, const dg_dp_graph *);
int dg_dp_run(dg_ctx *, dg_dp_result *);               /* all kernels on the resident graph (dg_dp_run_budgets with the one budget R); synchronises */
int dg_dp_get_timing(dg_ctx *, dg_dp_timing *);
int dg_dp_solve_diploid(dg_ctx *, const dg_dp_graph *, dg_dp_result *);   /* = load_graph + run */
/* Every recombination budget from ONE pass.  The source level starts at 0 on all R + 1 planes and a cell of plane r gathers from
 * planes r, r - 1, r - 2 only, so after one sweep with the graph's R plane r of the sink is the cell a run with limit r reads out.
 * After dg_dp_load_graph: one sweep, then the read-out of every listed budget -- one chain walk per budget, all of a lattice chunk
 * in one launch, each re-scored against its plane's value.  budgets[q] in 0..R, distinct, any order; results[q] is filled as
 * dg_dp_run would fill it for a graph loaded with R = budgets[q] (value, s_het, both edge lists, n_p1, n_p2; cells / relaxations
 * are those of the one sweep that ran).  Caller-provided edge buffers per result, cap >= budgets[q] + 2.  An unreachable budget
 * answers value = NEG_INF (INT32_MIN / 4), n_p1 = n_p2 = 0 and is not an error.  DG_ERR_ARG (n_budgets <= 0, a budget outside
 * 0..R, a duplicate, a cap too small) and DG_ERR_STATE (no graph loaded) leave the context as it was; DG_ERR_STATE with the
 * budget named if any chain is corrupt or scores differently from its plane's value.  dg_dp_get_timing: traceback_ms covers all
 * chains.  Synchronises. */
int dg_dp_run_budgets(dg_ctx *, const int32_t *budgets, int32_t n_budgets, dg_dp_result *results);
/* the sink's value on planes 0..R (NEG_INF where unreachable) of the last dg_dp_run / dg_dp_run_budgets on the loaded graph;
 * out has n >= R + 1 entries */
int dg_dp_get_budget_values(dg_ctx *, int32_t *out, int32_t n);
/* Pinned run: dg_dp_run_budgets on the DP in which some cells of some levels are unreachable on every plane.  A pin matches cell
 * (i, j) of its level -- i the vertex of haplotype 1 (dg_dp_result's p1, row 0 of dg_dp_get_answer_paths), j that of haplotype 2 -- if
 * vertex1 is -1 or i and vertex2 is -1 or j; pins are ordered: (a, b) is not (b, a).  A cell of a level is allowed if the level has no
 * require-pin or one of them matches it, and no forbid-pin of the level matches it.  Recurrence, NEG_INF, tie order (the winner
 * among the candidates that remain), "at most" budgets, the finish kernel's check of every chain: the run's.  A constraint set that
 * no pair of paths satisfies within a budget is an answer, not an error: value NEG_INF and empty edge lists for that budget.
 * n_pins = 0 (pins may be NULL) is exactly dg_dp_run_budgets.  The sweep kernels run unchanged: after the launch that writes a
 * pinned level one mask launch stores NEG_INF over the level's cells that are not allowed, on all R + 1 planes (csrc/dg_dp_pins.hip);
 * a level pair whose earlier level is pinned runs as two launches in this call, a captured batch that holds a pinned level is issued
 * plainly in this call and the batch cache stays as it was.
 * DG_ERR_ARG, naming the first offending pin and leaving the state of the last run alone: a level outside 1 .. n_levels - 2, a vertex
 * that is neither -1 nor inside its level, a kind other than 0 or 1, n_pins < 0 or > 65536, null pins with n_pins > 0; the budget
 * rules are those of dg_dp_run_budgets.  DG_ERR_STATE: no graph loaded, or option digest 1 (the sweep accumulates a level's digest
 * before the mask runs).  The call is "the last run" for dg_dp_get_budget_values, dg_dp_get_answer_paths, dg_dp_answer_objectives,
 * dg_dp_get_timing and the launch and pair profiles; dg_dp_call_margins, which checks the run's value against an unconstrained
 * partner DP, answers DG_ERR_STATE after it until the next unpinned run.  Synchronises. */
typedef struct dg_dp_pin { int32_t level, vertex1, vertex2, kind; } dg_dp_pin;   /* kind: 0 require, 1 forbid; vertex -1 = any */
int dg_dp_run_pinned(dg_ctx *, const dg_dp_pin *pins, int64_t n_pins, const int32_t *budgets, int32_t n_budgets, dg_dp_result *results);
/* measurement: the last dg_dp_run_pinned with n_pins > 0 on this context: out[0] = pins, out[1] = pinned levels, out[2] = mask
 * launches (a segmented run masks a level once per pass), out[3] = level pairs run as two launches, out[4] = batches issued plainly
 * that would have been captured or replayed; n >= 5 (zeros before the first such call).  DG_ERR_ARG: null out or n < 5.
 * DG_ERR_STATE: no DP state on this context yet. */
int dg_dp_get_pin_stats(dg_ctx *, int64_t *out, int n);
/* What a pair of source -> sink paths is worth on the loaded graph (the question the sweep answers with a maximum: plane r of the
 * sink is the best `value` over all pairs with r1 + r2 <= r).  For the transition into level l the ordered pair (path 1, path 2)
 * contributes what the sweep adds to cell (i, j) for the in-edge pair (p1[l-1] -> p1[l], p2[l-1] -> p2[l]): |(Hom u Hom) n (Hom u Hom)|
 * + |(Het u Het) /\ (Het u Het)| of the two sources' against the two destinations' colour lists (approximator.cpp:604-624); a
 * transition without colours contributes 0.  Parallel edges between the same two vertices carry equal weights (checked at load) and
 * are one edge to the score. */
typedef struct dg_dp_pair_score {
    int32_t value;                    /* sum of the transitions' score deltas, as the sweep adds them */
    int32_t s_het;                    /* sum of their Het terms (approximator.cpp:662): dg_dp_result::s_het of a walked pair */
    int32_t r1, r2;                   /* weight-1 edges on path 1 / path 2; no budget applies, the caller compares r1 + r2 with one */
} dg_dp_pair_score;
/* paths (host) = [n_pairs][2][n_levels] vertex ids, one per level of the loaded graph: entry 0 the source, the last one the sink;
 * out (host) has n_pairs entries.  Needs dg_dp_load_graph only, and leaves the answers of an earlier run (dg_dp_get_budget_values,
 * dg_dp_get_level_digest, dg_dp_get_timing) as they were.  Validation and scoring run on the device, one lane per transition, the
 * paths going up in slabs of at most 256 MB (option score_slab_bytes).  DG_ERR_STATE: no graph loaded.  DG_ERR_ARG: a null
 * argument, n_pairs < 0, or a vertex that is not in its level / two consecutive vertices that no edge joins -- the message names
 * the first such (pair, path 0|1, level), in that order of significance (the level of a missing edge is its destination's), and
 * out is not written.  n_pairs = 0 is DG_OK.  Synchronises. */
int dg_dp_score_paths(dg_ctx *, const int32_t *paths, int64_t n_pairs, dg_dp_pair_score *out);
/* The best partner of a path that is already known: the DP with one haplotype fixed.  `given` is a source -> sink path, one vertex
 * per level; with it fixed, the in-edge (u -> v, w) into level l is worth what dg_dp_score_paths adds there for the ordered pair
 * (given, partner): inter + symd of the sources (given[l-1], u) against the destinations (given[l], v); parallel edges are one edge.
 * S_0[source][r] = 0 for r = 0..budget ("at most", as in the sweep); S_l[v][r] = max over the in-edges of v with r - w >= 0 and a
 * reachable source cell of S_{l-1}[u][r - w] + that score, the smallest source position winning among equals; NEG_INF = INT32_MIN / 4
 * where nothing arrives.  The answer is the sink's cell on plane `budget` and the path its winners lead back along. */
typedef struct dg_dp_partner {
    int32_t value;                    /* S[sink][budget]; NEG_INF: no path fits the budget (not an error: s_het = r2 = 0, the partner row is all -1) */
    int32_t s_het;                    /* sum of the symd terms of (given, partner) */
    int32_t r1, r2;                   /* weight-1 edges on the given path / on the partner (r2 <= budget) */
} dg_dp_partner;
/* given (host) = [n][n_levels] vertex ids; budgets (host) = [n], each >= 0 (independent of the graph's R); partners (host) =
 * [n][n_levels], may be NULL (values only); out (host) = [n].  Needs dg_dp_load_graph only and leaves the answers of an earlier run
 * (dg_dp_get_budget_values, dg_dp_get_level_digest, dg_dp_get_timing) as they were.  One workgroup per query keeps the
 * widest level x (budget + 1) cells of state in LDS and streams one 16-bit back-pointer per cell; every answered query is then
 * re-scored as the pair (given, partner) by the kernel of dg_dp_score_paths, which yields s_het, r1 and r2 and must reproduce
 * `value` with r2 <= budget (DG_ERR_STATE naming the query otherwise).  Queries go up in slabs, in order; option partner_slab_bytes
 * bounds the device memory of a slab, every query counting 2 * n_vertices * (bmax + 1) + 2 * n_edges + 8 * n_levels bytes, bmax the
 * largest budget of the call.  DG_ERR_STATE: no graph loaded.  DG_ERR_ARG: a null given, budgets or out, n < 0, a negative budget
 * (the message names the query), a given path with a vertex outside its level or a hop without an edge (the message names the first
 * such (query, level), in that order of significance; the level of a missing edge is its destination's).  DG_ERR_UNSUPPORTED: widest
 * level x (budget + 1) > 16384 cells for some query (the message names both numbers).  A failed call writes neither partners nor out.
 * n = 0 is DG_OK.  Synchronises.
 * Option partner_wide (default 0: all of the above) opens a second route that keeps the two level states in device memory, one
 * 1,024-lane workgroup per query: with 1 a call whose widest level x (bmax + 1) exceeds 16384 takes it as a whole, with 2 every call.
 * Same recurrence, ties and outputs.  Its limits: widest level <= 32767 (the back-pointer holds the source position in 15 bits) and
 * widest level x (budget + 1) <= 2^24 cells per query, DG_ERR_UNSUPPORTED beyond (the message names the query and both numbers).  On
 * that route a query counts 8 * widest level * (bmax + 1) bytes of state on top of the bytes above; the state buffer is released
 * when the call returns.  dg_dp_get_partner_route tells which route the last call took. */
int dg_dp_best_partners(dg_ctx *, const int32_t *given, int64_t n, const int32_t *budgets, int32_t *partners, dg_dp_partner *out);
/* Partner marginals: for a given path and a budget b, what the best partner through every vertex is worth, and per level the best
 * vertex, the best of the others and so the margin between them.  Notation of dg_dp_best_partners: d_l(u, v) is the score of the
 * in-edge u -> v into level l with `given` fixed, parallel edges are one edge.  Forward: F = the S of dg_dp_best_partners.  Backward:
 * B_{L-1}[sink][r] = 0 for r = 0..b; B_{l-1}[u][r] = max over the out-edges (u -> v, w) with r - w >= 0 and a reachable destination
 * cell of d_l(u, v) + B_l[v][r - w], NEG_INF where there is none.  M[v] = max over r = 0..b with both cells reachable of
 * F[v][r] + B[v][b - r], NEG_INF if there is no such r: the maximum of dg_dp_score_paths' value of (given, q) over all source -> sink
 * paths q through v with r(q) <= b (both tables mean "at most r", so the split over r loses nothing). */
typedef struct dg_dp_level_margin {
    int32_t best_vertex, best_value;      /* the vertex of the level with the largest M (the smallest id among equals) and its M: dg_dp_best_partners' value at every level */
    int32_t second_vertex, second_value;  /* the same choice among the level's other vertices; -1, NEG_INF if none of them has a reachable M */
} dg_dp_level_margin;
/* given, budgets (host): as for dg_dp_best_partners, one budget per query; levels (host) = [n][n_levels]; vertex_values (host) =
 * [n][n_vertices] receives M, may be NULL.  second_value == best_value: the data cannot tell the two vertices apart at that level;
 * best_value - second_value is the margin of the call there.  best_vertex[l] need not be dg_dp_best_partners' partner[l] where
 * values tie: that walk breaks a tie by the smallest source position of the in-edge it came through, this record by the smallest
 * vertex id among ALL vertices of the level that reach the value.  A query whose budget no path fits is an answer, not an error:
 * -1, NEG_INF, -1, NEG_INF on every level and NEG_INF for every vertex.  Needs dg_dp_load_graph only and leaves the answers of an
 * earlier run (dg_dp_get_budget_values, dg_dp_get_level_digest, dg_dp_get_timing) as they were.  Per query one workgroup runs the
 * forward recurrence, keeping every cell's value, and a second one the backward recurrence with the combination, both with
 * widest level x (budget + 1) cells of state in LDS.  Queries go up in slabs, in order; option partner_slab_bytes bounds the device
 * memory of a slab, every query counting 4 * n_vertices * (bmax + 1) bytes of forward values, 2 * n_edges of scores, 4 * n_vertices
 * of marginals and 20 * n_levels of path and level records, bmax the largest budget of the call.  Errors as for dg_dp_best_partners:
 * DG_ERR_STATE: no graph loaded.  DG_ERR_ARG: a null given, budgets or levels, n < 0, a negative budget (the message names the
 * query), a given path with a vertex outside its level or a hop without an edge (the message names the first such (query, level),
 * in that order of significance; the level of a missing edge is its destination's).  DG_ERR_UNSUPPORTED: widest level x (budget + 1)
 * > 16384 cells for some query (the message names both numbers).  A failed call writes neither levels nor vertex_values.  n = 0 is
 * DG_OK.  Synchronises.
 * Option partner_wide chooses the route as for dg_dp_best_partners, with the same limits.  On the device-memory route the forward
 * kernel reads the previous level back from the forward values it stores anyway, and the backward kernel keeps its two level states
 * in device memory: a query counts 8 * widest level * (bmax + 1) bytes of state on top of the bytes above, released when the call
 * returns. */
int dg_dp_partner_marginals(dg_ctx *, const int32_t *given, int64_t n, const int32_t *budgets, dg_dp_level_margin *levels, int32_t *vertex_values);
/* The answer of the last dg_dp_run / dg_dp_run_budgets at `budget` as the pair of paths it walked: paths (host) = [2][n_levels]
 * vertex ids, entry 0 the source, the last one the sink; row 0 is the path of dg_dp_result's p1 lists, row 1 that of p2 -- the rows
 * dg_dp_score_paths, dg_dp_best_partners and dg_dp_partner_marginals take.  (The weight-1 edge lists of dg_dp_result do not fix the
 * vertices in between on a general graph; the chain walk's hop words, which stay on the device, do: one kernel, one lane per level,
 * expands them.)  `budget` must be one the last run read out (dg_dp_run: R).  A budget that no pair of paths fits is an answer, not
 * an error: both rows are all -1, DG_OK.  DG_ERR_STATE: no graph loaded, no completed run since the last dg_dp_load_graph, or a budget
 * the last run did not read out (the message names it).  DG_ERR_ARG: null paths.  paths is written only on success.  Leaves the
 * run's answers (dg_dp_get_budget_values, dg_dp_get_level_digest, dg_dp_get_timing) as they were.  Synchronises. */
int dg_dp_get_answer_paths(dg_ctx *, int32_t budget, int32_t *paths);
/* Call margins: how sure each haplotype of the run's own answer is, per level.  With (p1, p2) the answer at `budget` b, r1 and r2 their
 * weight-1 hops and V the sink's value on plane b: row 0 describes p1 with given = p2 and the partner budget b - r2, row 1 describes p2
 * with given = p1 and b - r1; M is the quantity of dg_dp_partner_marginals for that given path and budget.  value == V on every level
 * of both rows (p_h is itself a partner within the budget, so M >= V; every partner within it forms a pair of at most b
 * recombinations, so M <= V; the score is symmetric in the two paths): the call checks it and answers DG_ERR_STATE naming the row
 * and the level otherwise. */
typedef struct dg_dp_call_margin {
    int32_t vertex, value;            /* p_h[l] and M[p_h[l]] */
    int32_t alt_vertex, alt_value;    /* the vertex of level l with the largest reachable M among those of another class than `vertex` (the smallest id among equals); -1, NEG_INF if there is none */
} dg_dp_call_margin;
/* levels (host) = [2][n_levels]; vertex_class (host) = [n_vertices], one int32 per vertex, or NULL: every vertex is its own class, so
 * the alternative is the best other vertex; paths (host) = [2][n_levels] or NULL receives what dg_dp_get_answer_paths returns.
 * value - alt_value is the margin of the call at that level; 0: the reads cannot tell the called allele from another one, given the
 * other haplotype.  The two paths go from the chain's hop words to the score kernel on the device, the marginals of the vertices stay
 * there too: after the backward pass one wave per (row, level) reduces the level's vertices of other classes to one record.  The two
 * queries form one slab if option partner_slab_bytes holds both (a query counts as for dg_dp_partner_marginals), two otherwise.
 * An unreachable budget is an answer: every record -1, NEG_INF, -1, NEG_INF, the paths all -1, DG_OK.  Errors as for
 * dg_dp_get_answer_paths (DG_ERR_ARG: null levels), and DG_ERR_UNSUPPORTED: widest level x (budget + 1) > 16384 cells (the message
 * names both numbers; on `budget` itself, not on what the other haplotype leaves of it, so that it is known before a run).  A failed
 * call writes nothing.  Leaves the run's answers as they were.  Synchronises.
 * With option partner_wide >= 1 the limits on `budget` are those of the device-memory route instead (widest level <= 32767, widest
 * level x (budget + 1) <= 2^24; the message names the budget and both numbers), and the two queries take that route together if widest
 * level x (the larger of their two budgets + 1) exceeds 16384 (with 2: always); a query then counts 8 * widest level * (that budget + 1)
 * bytes of backward state more, released when the call returns. */
int dg_dp_call_margins(dg_ctx *, int32_t budget, const int32_t *vertex_class, dg_dp_call_margin *levels, int32_t *paths);
/* Which route the last dg_dp_best_partners, dg_dp_partner_marginals or dg_dp_call_margins on this context took: *route = 0: none of them
 * has got as far as a launch since dg_create, 1: level state in LDS, 2: level state in device memory (option partner_wide); *cells =
 * that call's widest level x (largest budget + 1).  A call that fails before the route is chosen, or has nothing to launch (n = 0, an
 * unreachable budget of dg_dp_call_margins), leaves both as they were.  DG_ERR_ARG: a null argument. */
int dg_dp_get_partner_route(dg_ctx *, int32_t *route, int64_t *cells);
/* Genotype margins: the best pair of paths through every cell of a level, with BOTH haplotypes free (dg_dp_call_margins holds one
 * fixed).  d(u1, u2 -> v1, v2) is what the sweep adds for the transition: inter + symd; parallel edges are one edge; an edge pair
 * weighs w1 + w2, also when both paths take the same edge.  budget b >= 0 means "at most" and is independent of the graph's R.
 * Forward: F_0[src, src][r] = 0 for r = 0..b; F_l[i][j][r] = max over the in-edge pairs (u -> i, w1), (v -> j, w2) with
 * r - w1 - w2 >= 0 and a reachable source cell of F_{l-1}[u][v][r - w1 - w2] + d, NEG_INF where there is none (the sweep's values).
 * Backward: B_{L-1}[sink, sink][r] = 0; B_l[i][j][r] = max over the out-edge pairs (i -> i', w1), (j -> j', w2) with
 * r - w1 - w2 >= 0 and a reachable destination cell of d + B_{l+1}[i'][j'][r - w1 - w2].  Through-value: T_l[i][j] = max over
 * r = 0..b with both cells reachable of F_l[i][j][r] + B_l[i][j][b - r], NEG_INF if there is none: the best value of any ordered pair
 * of source -> sink paths (p, q) with p[l] = i, q[l] = j and r(p) + r(q) <= b.  T is symmetric.  V_b = F_{L-1}[sink, sink][b], and
 * on every level the maximum of T is V_b.  J[v] = max_j T_l[v][j], the joint marginal of vertex v (>= the M of
 * dg_dp_partner_marginals for either half of an optimal pair).  The genotype of a cell is the unordered pair of its vertices' classes. */
typedef struct dg_dp_genotype_margin {
    int32_t vertex1, vertex2;         /* the called cell of the level */
    int32_t value;                    /* T at the called cell (NEG_INF: no pair within the budget passes through it) */
    int32_t alt_vertex1, alt_vertex2; /* the cell with the largest T among the cells of another genotype than the called one, alt_vertex1 <= alt_vertex2; among equals the smallest alt_vertex1, then the smallest alt_vertex2; -1, -1 if no such cell is reachable */
    int32_t alt_value;                /* its T; NEG_INF if there is none */
    int32_t reserved[2];              /* written as 0 */
} dg_dp_genotype_margin;
/* called (host) = [n_called][2][n_levels] vertex ids: per query one cell per level (a list of cells: no edge is required between
 * levels), every id inside its level; 1 <= n_called <= 256.  vertex_class (host) = [n_vertices] or NULL (every vertex is its own
 * class), as for dg_dp_call_margins.  levels (host) = [n_called][n_levels]; vertex_values (host) = [n_vertices] receives J, may be
 * NULL; *best_value = V_b.  value - alt_value is the margin of the called genotype at that level: a per-site genotype quality.  It
 * is negative where the called cell is not optimal: an answer, not an error.  A budget that no pair fits is an answer too: NEG_INF /
 * -1 everywhere, DG_OK.  Needs dg_dp_load_graph only and leaves the sink values, answer paths, digests, timing and resident
 * score-delta window of an earlier run as they were.  Device memory: a level's state is 4 * width^2 * (b + 1) bytes; the forward
 * states are kept for one segment of levels at a time (option joint_state_bytes bounds a segment's states, a segment holds at least
 * one level) plus one state per segment, recomputed segment by segment from the last to the first, beside two backward states of the
 * widest level, one score matrix of the largest coloured transition (2 * in-edges^2 bytes) and 8 bytes per edge; all of it is reserved
 * inside the call and freed when it returns.  Closing check: the maximum of T is V_b on every level, DG_ERR_STATE naming the level
 * otherwise.  DG_ERR_STATE: no graph loaded.  DG_ERR_ARG: a null called, levels or best_value, n_called < 1, a negative budget, an id
 * outside its level (the message names the first such (query, row 0|1, level), in that order of significance).
 * DG_ERR_UNSUPPORTED (the message names both numbers): widest level > 32767, budget + 1 > 4096, n_called > 256.  A failed call
 * writes nothing.  Synchronises. */
int dg_dp_genotype_margins(dg_ctx *, const int32_t *called, int64_t n_called, int32_t budget, const int32_t *vertex_class,
                           dg_dp_genotype_margin *levels, int32_t *vertex_values, int32_t *best_value);
/* Genotype table: for every level l and every genotype g = (class1 <= class2, compared as signed integers) with a reachable cell,
 * G_l[g] = the largest T_l[i][j] over the cells of that genotype, and its representative cell: the one attaining it with
 * vertex1 <= vertex2, among equals the smallest vertex1, then the smallest vertex2 (the rule of alt_vertex1 / alt_vertex2 above).  A
 * genotype without a reachable cell is not listed.  This is the integer analogue of a PL vector per site: the largest value of a
 * level is V_b; with vertex_class = NULL the entries of a level are its reachable cells i <= j; the margin record of a called cell is
 * the entry of its genotype (if the called cell is its genotype's best) against the best entry of another genotype, ties to the
 * smallest vertex1, then vertex2; J[v] <= the largest entry whose genotype contains the class of v, with equality for NULL classes. */
typedef struct dg_dp_genotype_entry {
    int32_t class1, class2;           /* the genotype, class1 <= class2 */
    int32_t vertex1, vertex2;         /* its best cell, vertex1 <= vertex2 by id, ties as above */
    int32_t value;                    /* G_l[g] */
    int32_t reserved;                 /* written as 0 */
} dg_dp_genotype_entry;
/* budget, vertex_class, the recurrences, the limits and the errors are those of dg_dp_genotype_margins, from the same pass.  called /
 * levels are optional: both NULL with n_called = 0, or 0 < n_called <= 256 and levels receives exactly the records
 * dg_dp_genotype_margins writes for the same arguments (called without levels, the reverse, or NULL with n_called != 0: DG_ERR_ARG).
 * level_off (host) = [n_levels + 1]: entries level_off[l] .. level_off[l + 1] are level l's, in ascending (class1, class2); *entries is
 * malloc'ed by the library (dg_free), *n_entries = level_off[n_levels], *best_value = V_b.  A budget that no pair fits is an answer:
 * *n_entries = 0, *entries = NULL, level_off all 0, *best_value = NEG_INF, levels as dg_dp_genotype_margins fills them, DG_OK.
 * Plan, before any launch: the classes of a level are ranked densely (A_l distinct ones, = the width with NULL classes); the level can
 * hold up to A_l (A_l + 1) / 2 genotypes.  Finished entries are staged on the device in at most option genotype_table_bytes (default
 * 256 MB) and copied to the host when the next level's bound no longer fits, at the latest once per segment, so a result of any size
 * comes out; a level whose bound alone does not fit is DG_ERR_UNSUPPORTED (the message names the level, the bound and the option's
 * value; nothing was launched, the statistics are those of the call before).  Beside what dg_dp_genotype_margins reserves the call
 * holds T of the widest level (4 * width^2 bytes), one key per (row, class) and per possible genotype of a level (8 bytes each) and
 * 12 bytes per vertex; all of it counts in the peak bytes.  Closing check: on every level the level maximum and the largest entry are
 * V_b, DG_ERR_STATE otherwise.  DG_ERR_ARG also for a null level_off, entries, n_entries or best_value.  A failed call writes nothing
 * to any output and allocates nothing the caller must free.  Needs dg_dp_load_graph only and leaves a run's sink values, answer paths,
 * digests, timing and resident score-delta window as they were.  Synchronises. */
int dg_dp_genotype_table(dg_ctx *, int32_t budget, const int32_t *vertex_class, const int32_t *called, int64_t n_called,
                         dg_dp_genotype_margin *levels, int64_t *level_off, dg_dp_genotype_entry **entries, int64_t *n_entries,
                         int32_t *best_value);
/* measurement: the last successful dg_dp_genotype_margins / dg_dp_genotype_table on this context: out[0] = segments, out[1] = levels
 * whose forward state was computed twice, out[2] = peak bytes of device memory the call had reserved, out[3] = kernel launches; n >= 4
 * (zeros before the first call).  With n >= 6 also out[4] = entries of the last call's table (0 after dg_dp_genotype_margins) and
 * out[5] = its copies of the staging to the host.  With n >= 8 also out[6] = pins of the last call and out[7] = its mask launches
 * (both 0 after an unpinned call).  DG_ERR_ARG: null out or n < 4.  DG_ERR_STATE: no DP state on this context yet. */
int dg_dp_get_genotype_stats(dg_ctx *, int64_t *out, int n);
/* The joint pass on the pinned DP: dg_dp_genotype_margins / dg_dp_genotype_table with the cell constraints of dg_dp_run_pinned (the
 * pins, "allowed", the limits and the DG_ERR_ARG cases are that call's; the messages name the entry point at hand and the first
 * offending pin).  With a pin set P, F_l and B_l are the recurrences above with NEG_INF on every plane of every cell of level l that
 * is not allowed, so T_l[i][j | P] is the best value of any ORDERED pair (p, q) of source -> sink paths that satisfies P with
 * p[l] = i, q[l] = j and r(p) + r(q) <= b: plane b of dg_dp_run_pinned(P + require (l, i, j)).  V_b(P) = F_{L-1}[sink, sink][b] is
 * plane b of dg_dp_run_pinned(P), and on every level the maximum of T is V_b(P) (the closing check).  T(. | P) <= T(.) cell by cell.
 * Pins are ordered, so T is NOT symmetric in general: the called cell's value is T at the ordered called cell (vertex1 = haplotype 1)
 * and J[v] = max_j T_l[v][j] over the ordered row, while a genotype is unordered: the alternative of a record and the entries of the
 * table take the cells vertex1 <= vertex2 as above with the value max(T[i][j], T[j][i]), ties by the same rule.  That maximum changes
 * nothing where P is symmetric or empty.  A pin set that no pair satisfies within the budget is an answer: NEG_INF / -1 everywhere,
 * an empty table, DG_OK.  n_pins = 0 (pins may be NULL) is the unpinned call: the same pass, no mask launch, every output identical.
 * Device: after every launch that writes a forward or backward state of a pinned level (the checkpointing pass, every segment's
 * recompute, the backward recurrence) one launch of jt_pin_mask_kernel (csrc/dg_dp_pins.hip) stores NEG_INF over all b + 1 planes of
 * the level's cells that are not allowed; no other kernel changes, the combination of a pinned call takes both orders of a cell.  The
 * sorted pins live in a buffer of the call.  Like their twins the calls read and write nothing of a run: the pins, statistics and
 * "pinned" state of an earlier dg_dp_run_pinned stay as they were, and a failed call writes nothing.  Synchronises. */
int dg_dp_genotype_margins_pinned(dg_ctx *, const dg_dp_pin *pins, int64_t n_pins, const int32_t *called, int64_t n_called, int32_t budget,
                                  const int32_t *vertex_class, dg_dp_genotype_margin *levels, int32_t *vertex_values, int32_t *best_value);
int dg_dp_genotype_table_pinned(dg_ctx *, const dg_dp_pin *pins, int64_t n_pins, int32_t budget, const int32_t *vertex_class, const int32_t *called,
                                int64_t n_called, dg_dp_genotype_margin *levels, int64_t *level_off, dg_dp_genotype_entry **entries,
                                int64_t *n_entries, int32_t *best_value);
/* Genotype margins with one budget per query, from ONE joint pass.  F_l[i][j][r] and B_l[i][j][r] mean "at most r", so they do not
 * depend on the budget a call is made with, and T^b_l[i][j] = max over r = 0..b of F_l[i][j][r] + B_l[i][j][b - r]: the states of one
 * pass at bmax = the largest of budgets hold T^b for every b <= bmax.  Query q (called[q] = [2][n_levels], budgets[q]) is answered
 * exactly as dg_dp_genotype_margins_pinned(pins, n_pins, called[q], 1, budgets[q], ...) answers it -- with n_pins = 0 (pins may be
 * NULL) as dg_dp_genotype_margins does -- in every field of the record: the tie order of the alternative, NEG_INF / -1 where nothing
 * is reachable, the better of the two orders of a cell under pins.  best_values (host) = [n_called], best_values[q] = V at budgets[q].
 * Budgets may repeat and come in any order; a query whose budget no pair fits gets NEG_INF / -1 records beside its neighbours'
 * answers, DG_OK.  Per-vertex joint marginals are not offered (they would be n_called * n_vertices words): the one-budget call keeps
 * them.  Device: the schedule of dg_dp_genotype_margins once, with bmax + 1 planes (segments by joint_state_bytes at that size): the
 * forward, recompute and backward recurrences, the score matrices and the pin masks are launched once; only the combination runs per
 * distinct budget, in the same two launches per level (jt_combine_budgets_kernel: one more grid dimension over the distinct budgets,
 * each workgroup serves the queries of its budget).  Beside that call's buffers: one row maximum per (distinct budget, position of
 * the widest level) and bmax + 1 words for the sink's values; the scratch rows of T are shared among the budgets, not multiplied.
 * Closing check per distinct budget b: the level maximum of T^b is V_b on every level, DG_ERR_STATE naming level and budget otherwise.
 * Limits and errors are those of dg_dp_genotype_margins taken at bmax: DG_ERR_UNSUPPORTED for a widest level > 32767,
 * bmax + 1 > 4096, n_called > 256; DG_ERR_ARG for a negative budget (the message names the first such query), n_called < 1, a null
 * called, budgets, levels or best_values, an id outside its level (first (query, row, level) named), a bad pin as dg_dp_run_pinned
 * refuses it; DG_ERR_STATE without a graph.  A failed call writes nothing.  Reads and writes nothing of a run, pinned or not.
 * dg_dp_get_genotype_stats describes the call in its existing fields (entries and staging copies 0; pins and mask launches when pins
 * are given).  Synchronises. */
int dg_dp_genotype_margins_budgets(dg_ctx *, const dg_dp_pin *pins, int64_t n_pins, const int32_t *called, const int32_t *budgets, int64_t n_called,
                                   const int32_t *vertex_class, dg_dp_genotype_margin *levels, int32_t *best_values);
/* Phase margins: cis against trans for neighbouring heterozygous sites of a called pair of cells per level.  d, F, B, "reachable",
 * budget and vertex_class are those of dg_dp_genotype_margins.  called (host) = [2][n_levels] vertex ids, one cell per level, every id
 * inside its level; c_h[l] = the class of called[h][l].  The het levels are those with c_0[l] != c_1[l], ascending:
 * h_0 < ... < h_{m-1}.  For a neighbouring pair (a, e) = (h_t, h_{t+1}) and an ordered pair of classes X at a, W(X) = the largest value
 * of any ORDERED pair (p, q) of source -> sink paths with r(p) + r(q) <= b, (cls p[a], cls q[a]) = X and
 * (cls p[e], cls q[e]) = (c_0[e], c_1[e]); NEG_INF if there is none.  cis = W(c_0[a], c_1[a]), trans = W(c_1[a], c_0[a]);
 * cis - trans is the phase margin of the two sites: what the answer loses by switching the phase between them.  By the symmetry of d,
 * trans is also the value of the pairs that keep the called order at a and swap it at e.  Recurrence, over l = e - 1 .. a:
 * S_e[i][j][r] = B_e[i][j][r] where (cls i, cls j) = (c_0[e], c_1[e]), NEG_INF elsewhere; S_l from S_{l+1} by the backward recurrence,
 * unchanged; U_a[i][j] = max over r = 0..b with both reachable of F_a[i][j][r] + S_a[i][j][b - r]; cis = the maximum of U_a over the
 * cells of classes (c_0[a], c_1[a]), trans over those of classes (c_1[a], c_0[a]); after the read-out S_a is seeded again from B_a with
 * the called ordered classes of a.  So one more rolling backward state answers every neighbouring pair in the same pass. */
typedef struct dg_dp_phase_margin {
    int32_t level_a, level_b;             /* the two neighbouring het levels, level_a < level_b */
    int32_t cis_value;                    /* W of the called order at level_a; NEG_INF if nothing is reachable */
    int32_t cis_vertex1, cis_vertex2;     /* the cell of level_a (haplotype 1, haplotype 2) that attains it; among equals the smallest position of vertex1, then of vertex2; -1, -1 if there is none */
    int32_t trans_value;                  /* W of the swapped order at level_a; NEG_INF if nothing is reachable */
    int32_t trans_vertex1, trans_vertex2; /* its cell, ties as above; -1, -1 if there is none */
    int32_t reserved[2];                  /* written as 0 */
} dg_dp_phase_margin;
/* records (host) has room for n_levels - 1 entries; the call writes *n_records = m - 1 of them (0 when m < 2: DG_OK), ascending by
 * level, and *best_value = V_b.  A budget that no pair fits is an answer: NEG_INF / -1 in every record, DG_OK.  The call checks that
 * max(cis, trans) <= V_b in every record, DG_ERR_STATE naming the record otherwise.  Not checked, but true: if called is a pair of
 * real paths with r1 + r2 <= b, cis >= its score (dg_dp_score_paths); if called is an optimal pair at b, cis = V_b in every record.
 * Device: the schedule of dg_dp_genotype_margins (segments by option joint_state_bytes, forward checkpoints, the segments from the last
 * to the first, B rolling in two states) with two more states of the widest level for S, reserved by this call only.  From the level
 * below h_{m-1} down to h_0 the backward kernel runs a second time per level, on S, with the score matrix the first launch used;
 * below h_0 nothing backward is launched.  At every het level but the last a read-out kernel forms U on the rows of the two called
 * classes and a one-workgroup finish writes the record on the device; at every het level but the first a seed kernel writes S from B
 * under the class mask.  The records are copied out once, at the end.  The combination, record and table kernels of the other entry
 * points are not launched.  Limits and errors are those of dg_dp_genotype_margins with n_called = 1: DG_ERR_STATE without a graph;
 * DG_ERR_ARG for a null called, records, n_records or best_value, a negative budget, an id outside its level (the message names the
 * first such (row 0|1, level)); DG_ERR_UNSUPPORTED for a widest level > 32767 or budget + 1 > 4096.  Needs dg_dp_load_graph only, reads
 * and writes nothing of a run, and leaves what dg_dp_get_genotype_stats reports as it was.  A failed call writes nothing.  Synchronises.
 * There is no pinned variant: pins are ordered, and the single seeded state rests on the symmetry of the unpinned DP in its two
 * haplotypes (trans read off the same S as cis); under ordered pins the two orders would need a state each. */
int dg_dp_phase_margins(dg_ctx *, const int32_t *called, int32_t budget, const int32_t *vertex_class, dg_dp_phase_margin *records,
                        int64_t *n_records, int32_t *best_value);
/* measurement: the last successful dg_dp_phase_margins on this context: out[0] = het levels, out[1] = records, out[2] = backward
 * launches on the seeded state S, out[3] = read-out launches, out[4] = segments, out[5] = peak bytes of device memory the call had
 * reserved; n >= 6 (zeros before the first call).  DG_ERR_ARG: null out or n < 6.  DG_ERR_STATE: no DP state on this context yet. */
int dg_dp_get_phase_stats(dg_ctx *, int64_t *out, int n);
/* Phase margins for many called pairs, each at a budget of its own, from ONE joint pass.  Query q = (called[q] = [2][n_levels],
 * budgets[q]) gets records[record_off[q] .. record_off[q + 1]) and best_values[q] = V at budgets[q]; its records are, field for field,
 * what dg_dp_phase_margins(called[q], budgets[q], vertex_class) writes (reserved words, NEG_INF / -1 of a budget nobody fits, ties).
 * called (host) = [n_called][2][n_levels]; budgets (host) = [n_called], >= 0, in any order, repeats allowed; records (host) has room for
 * n_called * (n_levels - 1) entries; record_off (host) = [n_called + 1], record_off[0] = 0; a query with fewer than two het levels gets
 * an empty range.  Why one pass serves all: F, B and the seeded state S mean "at most r", so the states of a pass with bmax + 1 planes
 * (bmax = the largest of budgets) hold on planes 0..b exactly the states of a call at budget b, and query q reads out
 * U = max over r = 0..b_q of F[r] + S[b_q - r].  S is seeded again from B at every het level and never accumulates: between a het
 * level e and the next one below it S depends only on its seed key (e, c_0[e], c_1[e]) and on B, not on the query that asked for it.
 * Device: the schedule of dg_dp_phase_margins at bmax + 1 planes with a pool of slots in place of the one S, a slot being two rolling
 * states of the widest level.  The host plans before the first launch: going down the levels a query carries on h_0 <= l < h_last with
 * the key of its nearest het level above l; the live keys of a level are the distinct keys of the carrying queries, one slot each; a
 * slot is freed when no query carries its key any more and may be taken by a key seeded at that same level; the number of slots is the
 * largest live count.  The per-level tables (slot lists; per read-out slot, classes, budget, record; per seed slot, classes) are uploaded
 * once.  Per level with a live slot ONE backward launch carries every live slot down (a grid dimension over the slot list, the
 * recurrence and the score matrix of the B launch); per level with read-outs ONE read-out launch (a grid dimension over the queries)
 * and one finish launch; then one seed launch over the keys created there.  V_b of every budget comes from the sink's bmax + 1 planes
 * of F, copied once.  Closing check per query: max(cis, trans) <= V at budgets[q] in every record, DG_ERR_STATE naming query and record.
 * Keys with the classes swapped, (e, c_1, c_0), are each other's transpose in the unpinned DP and could share a slot; they do not here.
 * Limits and errors are those of dg_dp_phase_margins taken at bmax, and: DG_ERR_ARG for n_called < 1, a null called, budgets, records,
 * record_off or best_values, a negative budget (the message names the first such query), an id outside its level (the first such
 * (query, row, level)); DG_ERR_UNSUPPORTED for n_called > 256.  A failed call writes nothing, the statistics included.  Reads and
 * writes nothing of a run and leaves what dg_dp_get_phase_stats and dg_dp_get_genotype_stats report as it was.  Synchronises.  There is
 * no pinned variant, for the reason given above. */
int dg_dp_phase_margins_budgets(dg_ctx *, const int32_t *called, const int32_t *budgets, int64_t n_called, const int32_t *vertex_class,
                                dg_dp_phase_margin *records, int64_t *record_off, int32_t *best_values);
/* measurement: the last successful dg_dp_phase_margins_budgets on this context: out[0] = queries, out[1] = records, out[2] = distinct
 * seed keys created, out[3] = slot-levels (the sum over the levels of the live slots: the backward work on S), out[4] = backward
 * launches on S, out[5] = read-out launches, out[6] = the largest number of live slots, out[7] = slots allocated, out[8] = segments,
 * out[9] = peak bytes of device memory the call had reserved; n >= 10 (zeros before the first call).  DG_ERR_ARG: null out or n < 10.
 * DG_ERR_STATE: no DP state on this context yet. */
int dg_dp_get_phase_budget_stats(dg_ctx *, int64_t *out, int n);
/* Recombination margins: what a crossover at each transition is worth.  F, B, d, "reachable" and V_b are those of
 * dg_dp_genotype_margins; both states mean "at most r".  For the transition t = l -> l + 1 (0 <= l < n_levels - 1) and s in {0, 1, 2}:
 *   E_t[s] = max over the ORDERED hop pairs (i -> i', w1), (j -> j', w2) of that transition with w1 + w2 = s, s <= b, and over
 *            r = 0 .. b - s with F_l[i][j][r] and B_{l+1}[i'][j'][b - s - r] both reachable, of
 *            F_l[i][j][r] + d(i, j -> i', j') + B_{l+1}[i'][j'][b - s - r];
 * NEG_INF where there is none: the value of the best pair of paths that spends exactly s of its crossovers at t.  The argument is the
 * hop pair that attains E_t[s]: value descending, then the smallest (i, j, i', j') in that lexicographic order of positions inside the
 * levels.  d is symmetric in the two haplotypes, so the winning tuple has i <= j.  The loader refuses parallel edges of different
 * weights, so a hop is its two vertices. */
typedef struct dg_dp_recombination_margin {
    int32_t level;                        /* l: the transition l -> l + 1 */
    int32_t value[3];                     /* E_t[0], E_t[1], E_t[2]; NEG_INF if no pair of paths spends that many there */
    int32_t from1[3], from2[3];           /* the vertices i, j of level l of the winning hop pair per s; -1 with NEG_INF */
    int32_t to1[3], to2[3];               /* the vertices i', j' of level l + 1; -1 with NEG_INF */
} dg_dp_recombination_margin;
/* records (host) = [n_levels - 1], ascending by level; they do not depend on called.  called (host) = [n_called][2][n_levels] vertex
 * ids, one cell per level, every id inside its level, or NULL with n_called = 0; called_out (host) = [n_called][n_levels - 1][2]:
 * per query and transition s_called = the sum of the weights of the two called hops (called[q][h][l] -> called[q][h][l + 1]), -1 if
 * either is no edge, and called_value = the value above restricted to the called ordered hop pair (NEG_INF if it is unreachable, no
 * edge, or s_called > b).  *best_value = V_b.  Closing check: max over s of E_t[s] == V_b at every transition, DG_ERR_STATE naming the
 * level otherwise.  A budget nobody fits is an answer: NEG_INF / -1 in every record, DG_OK.
 * Device: rb_call, the schedule of dg_dp_genotype_margins (segments by option joint_state_bytes, forward checkpoints, the segments
 * from the last to the first with F recomputed, B rolling in two states) with that call's combination, record and table launches
 * replaced, per level l < n_levels - 1, by two gathers that run after the transition's score matrix is formed and while B_{l+1} is
 * still the "next" state: rb_edges_kernel (row i = blockIdx.y, the lanes over (j >= i, r): F_l[i][j][r] loaded once, out(i) x out(j)
 * walked, three running maxima, one per s, of one 64-bit word value | i' | j' each; wave and workgroup reduction to one two-word key
 * (value, i | j, i', j') per (s, row, workgroup of the row)) and rb_finish_kernel (one workgroup per s reduces the keys to the level's record in a device array that is
 * copied out once; in the same launch one wave per query finds the ranks of the called hops among the in-edges, reads d and walks r).
 * B_0 is not formed: nothing reads it.  No atomics, every word has one owner, nothing depends on the order of lanes or workgroups.
 * Limits and errors are those of dg_dp_phase_margins: DG_ERR_UNSUPPORTED for a widest level > 32767, budget + 1 > 4096 or
 * n_called > 256; DG_ERR_ARG for a null records or best_value, n_called < 0, n_called > 0 with a null called or called_out, a negative
 * budget, an id outside its level (the message names the first such (query, row, level)); DG_ERR_STATE without a graph.  Results are
 * staged on the host: a refused or failed call writes nothing, the statistics included.  Needs dg_dp_load_graph only, reads and writes
 * nothing of a run, and leaves what the genotype, phase and pin statistics report as it was.  Synchronises.
 * A budget per query: dg_dp_recombination_margins_budgets below.  Not here: a pinned form, more than one GPU, and windows of several
 * transitions -- a breakpoint that can slide by one level shows as margin 0 at both transitions, and that is the intended reading. */
int dg_dp_recombination_margins(dg_ctx *, int32_t budget, const int32_t *called, int64_t n_called, dg_dp_recombination_margin *records,
                                int32_t *called_out, int32_t *best_value);
/* measurement: the last successful dg_dp_recombination_margins on this context: out[0] = transitions, out[1] = edge-kernel launches,
 * out[2] = finish launches, out[3] = segments, out[4] = levels swept forward twice, out[5] = peak bytes of device memory the call had
 * reserved, out[6] = launches in all; n >= 7 (zeros before the first call).  DG_ERR_ARG: null out or n < 7.  DG_ERR_STATE: no DP state
 * on this context yet. */
int dg_dp_get_recombination_stats(dg_ctx *, int64_t *out, int n);
/* The same for every listed budget from ONE joint pass.  n queries (1 .. 256); query q has the budget budgets[q] >= 0, in any order, with
 * repeats.  called (host) = NULL or [n][2][n_levels], one pair of cells per level for every query, every id inside its level; with a
 * non-null called, called_out is required.  records (host) = [n][n_levels - 1], called_out (host) = [n][n_levels - 1][2],
 * best_values (host) = [n].  Query q gets, field for field, what dg_dp_recombination_margins(budgets[q], called[q], 1, ...) writes: the
 * tie order of the hop pair, NEG_INF / -1 where nothing is reachable, s_called and called_value at that query's own budget, and
 * best_values[q] = V_{budgets[q]}.  Queries of one budget share one set of records: they are computed once per DISTINCT budget and
 * copied to each such query.  A budget nobody fits gives its queries NEG_INF / -1 records and DG_OK while their neighbours get answers.
 * Why one pass suffices: both states mean "at most r", so plane p of F_l and of B_{l+1} computed at bmax = the largest budget is plane
 * p at any b <= bmax, and E^b_t[s] = max F_l[i][j][r] + d + B_{l+1}[i'][j'][b - s - r] reads planes of that one pass; V_b is plane b of
 * the sink's cell.  Only the planes paired in the gather depend on b.
 * Closing check, per distinct budget b: max over s of E^b_t[s] == V_b at every transition; DG_ERR_STATE naming the level and the budget
 * otherwise.
 * Device: the schedule of dg_dp_recombination_margins run once with bmax + 1 planes (the plan by joint_state_bytes at that size, forward
 * checkpoints, the segments from the last to the first with F recomputed, B rolling in two states, one score matrix per transition,
 * B_0 not formed), with two launches per transition whatever the number of budgets, so a call issues as many launches as
 * dg_dp_recombination_margins(bmax).  The host sorts the distinct budgets bud[0 .. nd).  rb_edges_budgets_kernel is rb_edges_kernel
 * with one more grid dimension: workgroup (x, i, d) handles row i at budget bud[d], its lanes stride over (j >= i, r <= bud[d]), the
 * state stride is bmax + 1 and the B plane bud[d] - w - r; the same three running 64-bit maxima, packed candidate, two-word key and
 * wave and workgroup reduction, to part[d][s][i][x].  A row of budget b has k * (b + 1) lanes, so of the x workgroups of a row only
 * the first ceil(k * (b + 1) / 256) (at most 4096, the lanes striding beyond) store a key and are read.  rb_finish_budgets_kernel:
 * 3 * nd workgroups reduce part[d][s] to record d of the level in a device array [nd][n_levels - 1] that is copied out once; the
 * workgroups behind them answer called_out, one wave per query, with the query's own budget in the r loop.  V_b for all planes is one
 * copy of bmax + 1 words.  No atomics, every word has one owner, nothing depends on the order of lanes or workgroups.
 * Limits and errors are those of dg_dp_recombination_margins at the largest budget: DG_ERR_UNSUPPORTED for a widest level > 32767,
 * bmax + 1 > 4096 or n > 256; DG_ERR_ARG for n < 1, a null budgets, records or best_values, called without called_out, a negative
 * budget (the message names the first such query), an id outside its level (the first such (query, row, level)); DG_ERR_STATE without
 * a graph.  Results and statistics are staged on the host: a refused or failed call writes nothing.  Needs dg_dp_load_graph only,
 * reads and writes nothing of a run, and leaves every other statistics block as it was, that of dg_dp_recombination_margins included.
 * Synchronises.  Not here: a pinned form, more than one GPU, windows of several transitions. */
int dg_dp_recombination_margins_budgets(dg_ctx *, const int32_t *budgets, int64_t n, const int32_t *called, dg_dp_recombination_margin *records,
                                        int32_t *called_out, int32_t *best_values);
/* measurement: the last successful dg_dp_recombination_margins_budgets on this context: out[0] = queries, out[1] = distinct budgets,
 * out[2] = transitions, out[3] = edge-kernel launches, out[4] = finish launches, out[5] = segments, out[6] = levels swept forward
 * twice, out[7] = peak bytes of device memory the call had reserved, out[8] = launches in all; n >= 9 (zeros before the first call).
 * DG_ERR_ARG: null out or n < 9.  DG_ERR_STATE: no DP state on this context yet. */
int dg_dp_get_recombination_budget_stats(dg_ctx *, int64_t *out, int n);
/* What a pair of source -> sink paths is worth in the objective that the sweep's value approximates: every colour counts once, however
 * many vertices of a path carry it.  Hom(p) = the union of the hom colour lists of p's vertices, Het(p) that of its het lists; hom ids
 * and het ids are two separate id spaces, as in the transition score (an id present in both kinds is two colours).  All four numbers are
 * symmetric in the two paths; no budget applies.  objective = hom_shared + het_single: the hom colours both haplotypes cover plus
 * the het colours exactly one covers; hom_single and het_both are reached but not credited. */
typedef struct dg_dp_pair_objective {
    int32_t hom_shared, hom_single;   /* |Hom(p1) n Hom(p2)|, |Hom(p1) /\ Hom(p2)| */
    int32_t het_single, het_both;     /* |Het(p1) /\ Het(p2)|, |Het(p1) n Het(p2)| */
} dg_dp_pair_objective;
/* paths (host) = [n_pairs][2][n_levels] vertex ids and out (host) = [n_pairs], as for dg_dp_score_paths, whose guarantees and error
 * contract this call shares: needs dg_dp_load_graph only, and leaves the answers of an earlier run (dg_dp_get_budget_values,
 * dg_dp_get_level_digest, dg_dp_get_timing, dg_dp_get_answer_paths) as they were.  The first call after a load builds the graph's colour
 * dictionary on the device (per kind the sorted distinct ids, and one rank per colour-list entry: colour ids are arbitrary int32
 * values and never index anything); a run neither needs nor disturbs it.  One workgroup per pair validates the paths as
 * dg_dp_score_paths does and ORs the ranks of their vertices' colours into four bitmaps, (distinct hom + distinct het colours) / 4
 * bytes in all, which live in LDS up to option objective_lds_bytes and in device memory beyond.  The pairs go up in slabs bounded by
 * option score_slab_bytes, a pair counting 8 * n_levels bytes of paths plus, on the device-memory route, its bitmaps.  DG_ERR_STATE:
 * no graph loaded.  DG_ERR_ARG: a null argument, n_pairs < 0, or a vertex that is not in its level / two consecutive vertices that
 * no edge joins -- the message names the first such (pair, path 0|1, level), in that order of significance (the level of a missing
 * edge is its destination's), and out is not written.  n_pairs = 0 is DG_OK.  Synchronises. */
int dg_dp_objective_paths(dg_ctx *, const int32_t *paths, int64_t n_pairs, dg_dp_pair_objective *out);
/* The same record for the answers of the last dg_dp_run / dg_dp_run_budgets: out[q] describes the pair of paths the run walked for
 * budgets[q] (dg_dp_get_answer_paths).  The paths never leave the device: the chains' hop words are expanded where the objective
 * kernel reads them.  A budget that no pair of paths fits is an answer, not an error: -1 in all four fields, DG_OK.  Errors as for
 * dg_dp_get_answer_paths: DG_ERR_STATE without a graph, without a completed run since the last dg_dp_load_graph, or for a budget the
 * last run did not read out (the message names it); DG_ERR_ARG: a null argument or n_budgets <= 0.  out is written only on success.
 * Leaves the run's answers as they were.  Synchronises. */
int dg_dp_answer_objectives(dg_ctx *, const int32_t *budgets, int32_t n_budgets, dg_dp_pair_objective *out);
/* debug/parity: copy the per-level digest (same definition as the oracle's level_digest) of the
 * last run; out has n_levels entries, entry 0 unused. Requires dg_dp_set_option("digest",1). */
int dg_dp_get_level_digest(dg_ctx *, uint64_t *out, int64_t n);
/* parity / test / tuning knobs of the DP (none is needed in normal use; unknown keys fail with DG_ERR_ARG):
 *   digest 0|1            accumulate the per-level digests
 *   fast 0|1              0: generic sweep kernel only          adaptive_rc 0|1   0: one chunk of all r per task
 *   coop 0|1|2            cooperative fan-in rows off / by cost model / whenever possible
 *   rowx 0|1              row in-edge matrices (next load)      lean_chain 0|1    1: lean chain walk where the lattice allows it, 0: the general one (next load)
 *   graph_batch n         levels per hipGraph batch (-1: default 1000, 0: plain launches)
 *   l2_prefetch n         levels the per-XCD table prefetcher runs ahead of the sweep (0: off)
 *   pf_far n              levels ahead at which the prefetcher's far blocks pull tables into the Infinity Cache (0: periodic launches instead)
 *   delta_overlap 0|1|2   score deltas beside the sweep: off / on graphs of >= 32,000 levels / whenever possible (tests)
 *   warm_ahead n          levels per Infinity-Cache look-ahead batch (0: off)
 *   segment_cells, lattice_chunk_cells, delta_cap_entries   force checkpoint + recompute / chunk size / delta windows (tests)
 *   plane_limit 0|1       lattice beyond HBM: re-sweep every segment only up to the recombination plane its path leaves it on (default 1; 0: all planes)
 *   sync_every n          drain the stream every n level launches (rocprofv3 --pmc)
 *   side_stream -1|0|1    L2 prefetcher + score deltas beside the sweep: -1 (default) while this is the only DP state on its device, 0 never, 1 always
 *   test_poison_level l, test_poison_byte b   tests: fill level l of the back-pointer lattice with byte b between sweep and walk (dg_dp_run must answer DG_ERR_STATE)
 *   test_force_rc n       tests: n != 0 = every level's chunk-size choice considers the chunk of n recombination counts only (with coop 0|2: one kernel variant per run);
 *                         a level on which n is no candidate (not instantiated, above the run's all-planes chunk, no cooperative form) runs the all-planes chunk as with adaptive_rc 0
 *   score_slab_bytes n    bound of the path staging buffer of dg_dp_score_paths (default 256 MB, n <= 0 restores it; a slab holds at least one pair)
 *   partner_slab_bytes n  bound of the back-pointers, edge scores and paths of one slab of dg_dp_best_partners, and of what a slab of dg_dp_partner_marginals holds (default 4 GB, n <= 0 restores it; a slab holds at least one query)
 *   partner_wide 0|1|2    level state of dg_dp_best_partners / dg_dp_partner_marginals / dg_dp_call_margins in device memory: 0 (default) never -- beyond 16384 cells the call is refused; 1 for a call beyond 16384 cells; 2 for every call (tests, A/B timing)
 *   joint_state_bytes n   bound of the forward states that dg_dp_genotype_margins keeps for one segment of levels (default 8 GB, n <= 0 restores it; a segment holds at least one level)
 *   genotype_table_bytes n  bound of the device staging of finished entries of dg_dp_genotype_table (default 256 MB, a guess that nothing has measured; n <= 0 restores it; one level's bound must fit)
 *   genotype_table_lanes n  lanes that reduce one genotype of dg_dp_genotype_table over its rows: 0 (default) = the level's mean rows per class, else n; rounded down to a power of two in 1..64 (tests: 1 and 64)
 *   genotype_table_tile_keys n   keys of a level's dense genotype triangle per workgroup of dg_dp_genotype_table's compaction: 256..2048 in steps of 256 (default 2048, n <= 0 restores it; tests: 256)
 *   genotype_table_scan_tiles n  tiles that the workgroup scanning a level's tile counts takes per pass: 64..1024 in steps of 64 (default 1024, n <= 0 restores it; tests: 64, so that 65 tiles make a second pass)
 *   objective_lds_bytes n largest size of a pair's four colour bitmaps that dg_dp_objective_paths / dg_dp_answer_objectives keep in LDS; larger ones live in device memory (default 131072, n <= 0 restores it; clamped to the device's LDS per workgroup)
 *   pair_levels 0|1       1 (default): adjacent low-fan-in levels run as one composed launch where the run allows it (unsegmented, all planes, digest 0,
 *                         fast 1, adaptive_rc 1, test_force_rc 0); 0: every level its own launch (next load)
 *   pair_min n            the composed tables are built and used only for a graph with at least n such pairs (default 4096; next load)
 *   pair_fanin 0|1        1 (default): pairs whose later level has rows of composed in-degree 9..32 (big rows, walked by four waves each:
 *                         dp_sweep_pair_coop_kernel) are chosen too, on a graph that has enough of them (pair_fanin_min); 0: never (next load)
 *   pair_fanin_min n      ... only on a graph with at least n such pairs (default 4096); below, the pairs are exactly those of pair_fanin 0 (next load)
 *   pair_fanin_max_big n, pair_fanin_max_indeg n   a fan-in pair has at most n big rows (default 4) / a largest composed in-degree of n (default and at most 32): the measured gate (next load)
 *   pair_wide 0|1         1 (default): pairs in which the source, middle or later level holds 256..1,023 vertices are chosen too (records with 10-bit
 *                         positions: dp_sweep_pair_wide_kernel, dp_sweep_pair_coop_wide_kernel), on a graph that has enough of them (pair_wide_min); 0: never (next load)
 *   pair_wide_min n       ... only on a graph with at least n such pairs (default 1024); below, the pairs are exactly those of pair_wide 0 (next load)
 *   pair_wide_fanin 0|1   1 (default): a wide pair may have big rows, under the gate of pair_fanin_max_*; 0: light wide pairs only (next load)
 *   pair_wide_max_width n, pair_wide_rc n   measurement: the widest level of a wide pair (default and at most 1023; next load) / n one of the chunk
 *                         sizes (1, 2, 4) = every wide pair launch takes it, any other value (default 0): the cost model
 *   pair_digest 0|1       tests: 1 = with digest 1 the pair launches stay and run the pair kernel's digest form: the later level of a pair gets the
 *                         oracle's digest, the earlier level (never materialised) keeps 0; 0 (default): digest 1 refuses pair launches
 *   test_force_pair_rc n  tests: n one of the pair kernel's chunk sizes (1, 2, 4) = every pair launch takes it; any other value (default 0): the cost model
 *   host_tables 0|1       0 (default): the sweep's tables are built by device kernels from the uploaded graph; 1: on the host, then uploaded (parity twin; next load)
 *   rc_t0_ns, rc_tg_ps, rc_tw_ps, rc_cap, bp_nt_min_cells, max_blocks, host_threads   cost model / launch tuning
 * This list is documentation: struct DpOptions (csrc/dg_dp.hpp) is authoritative for the defaults, the key table beside dg_dp_set_option for the clamps. */
int dg_dp_set_option(dg_ctx *, const char *key, int64_t value);
/* the stored value of a key (what a set clamped or rounded it to), so that set(key, get(key)) changes nothing; DG_ERR_ARG like the setter */
int dg_dp_get_option(dg_ctx *, const char *key, int64_t *value);
/* parity: FNV-1a digests of the 12 tables built by dg_dp_load_graph (level descriptors, in-CSR offsets / sources / destinations,
 * coloured transitions, their delta blocks, column groups, dead columns, heavy rows, row records, row in-edge matrices, slot
 * records): the device construction and the host construction (option host_tables) must agree.  out has n >= 12 words. */
int dg_dp_get_table_digest(dg_ctx *, uint64_t *out, int n);
/* measurement: which sweep kernel variants the last dg_dp_run launched, as "name:count name:count ..." (the names
 * rocprofv3 reports, abbreviated); lets a profile taken in another process be matched against this run. */
int dg_dp_get_launch_profile(dg_ctx *, char *buf, int cap);
/* parity: the names of every sweep kernel variant the dispatch can launch, space-separated, in the order the launch profile prints
 * them: the generic kernel, then per chunk size fast<rc,lean>, coop<rc,lean>, fast<rc,general>, coop<rc,general> (the cooperative
 * ones for the chunk sizes that have them).  Needs no context.  DG_ERR_ARG: buf is null or too small. */
int dg_dp_list_sweep_variants(char *buf, int cap);
/* measurement: the level-pair launches of the last dg_dp_run (two adjacent low-fan-in levels composed into one launch, options
 * pair_levels / pair_min), as "dp_sweep_pair_kernel<rc>:count ...", followed by the fan-in pairs (options pair_fanin / pair_fanin_min) as
 * "dp_sweep_pair_coop_kernel<rc>:count ...", then the wide pairs (options pair_wide / pair_wide_min) as "dp_sweep_pair_wide_kernel<rc>:count ..."
 * and "dp_sweep_pair_coop_wide_kernel<rc>:count ..."; empty if there were none.  dg_dp_get_launch_profile and
 * dg_dp_list_sweep_variants list the single-level launches only; dg_dp_timing::n_forward_launches counts both kinds. */
int dg_dp_get_pair_profile(dg_ctx *, char *buf, int cap);
/* parity: the names of every light pair kernel the dispatch can launch, space-separated, in the order of the pair profile (the fan-in form has
 * dp_sweep_pair_coop_kernel<rc>, the wide forms dp_sweep_pair_wide_kernel<rc> and dp_sweep_pair_coop_wide_kernel<rc> for the same chunk sizes).  Needs no context. */
int dg_dp_list_pair_variants(char *buf, int cap);

/* ---- haploid (vertex, r) DP ---- */
typedef struct dg_hap_graph {         /* expanded graph after topologically_reorder: every edge u -> v has u < v */
    int32_t n_vertices, R;
    const int64_t *out_off;           /* [n_vertices+1] out-CSR, adjacency order preserved */
    const int32_t *out_dst;
    const uint8_t *out_w;             /* recombination weight 0/1 */
    const int32_t *n_colours;         /* |color[v]| */
} dg_hap_graph;
/* replaces the scatter loop of Approximator::dp_approximation_solver (src/approximator.cpp:44-72): fills the caller's
 * dp / back_vtx / back_r arrays, each [n_vertices * (R+1)], index v * (R+1) + r; the per-r backtracks and the choice of
 * best_r (:74-153, double arithmetic) stay with the caller.  Synchronises. */
int dg_dp_solve_haploid(dg_ctx *, const dg_hap_graph *, int32_t *dp, int32_t *back_vtx, int32_t *back_r);

/* ---- (w,k)-minimizer sketching ---- */
/* reads: concatenated bases + offsets [n_reads+1] (host). Outputs (malloc'ed by the library, release
 * with dg_free): globally sorted distinct minimizer hashes and the number of reads containing each
 * (== Sp_R keys in order / kmer_count values). */
int dg_sketch_reads(dg_ctx *, const char *bases, const int64_t *read_off, int64_t n_reads, int k, int w,
                    uint64_t **hash, int32_t **n_reads_with_hash, int64_t *n_distinct);
/* one haplotype string (host): the emitted-on-hash-change minimizer list in sequence order.
 * pos = start of the winning k-mer. Outputs malloc'ed by the library (dg_free). */
int dg_sketch_haplotype(dg_ctx *, const char *seq, int64_t len, int k, int w,
                        uint64_t **hash, int64_t **pos, int64_t *n);
/* hash n k-mers of length k stored back to back (host) with h1^h2 of MurmurHash3_x64_128, seed 0 */
int dg_hash_kmers(dg_ctx *, const char *kmers, int64_t n, int k, uint64_t *out);
void dg_free(void *);

/* which of two hash lists the minimizers of every read support (read-backed phasing: A / B = dg_sketch_haplotype of the two
 * haplotypes).  reads as for dg_sketch_reads; S = the read's set of distinct minimizer hashes (exactly what Solver::compute_hashes
 * collects); A, B = the SETS of the values in hash_a[n_a], hash_b[n_b]: any order, duplicates allowed, any 64-bit value (0 and
 * 2^64 - 1 included, nothing is reserved), empty lists may be NULL.  out[r] for every read r; a read without a window
 * (len < k + w - 1) answers all zeros; a hash counts once per read however often the read emits it.  All pointers are host memory.
 * DG_ERR_ARG (out is not written): k or w outside 1..255, n_reads < 0, null read_off or out with n_reads > 0, negative n_a / n_b, a
 * null list of positive length, a tag_table_bits (below) that leaves no empty slot.  n_reads = 0 is DG_OK.  Synchronises.  Leaves the
 * spectrum options and every stat of dg_sketch_reads as they were; like any sketch call it ends the life of device pointers an
 * earlier one returned.  dg_sketch_get_timing afterwards: kernel_ms = the tile pass, sort_ms = dictionary + tagging, total_ms = both,
 * n_emitted = emissions before the per-read dedup. */
typedef struct dg_read_tag {
    int32_t n_min;              /* distinct minimizer hashes of the read: |S| */
    int32_t only_a, only_b;     /* |S n (A \ B)|, |S n (B \ A)| */
    int32_t both;               /* |S n A n B| */
} dg_read_tag;                  /* 16 bytes */
int dg_sketch_tag_reads(dg_ctx *, const char *bases, const int64_t *read_off, int64_t n_reads, int k, int w,
                        const uint64_t *hash_a, int64_t n_a, const uint64_t *hash_b, int64_t n_b, dg_read_tag *out);

typedef struct dg_sketch_timing { float kernel_ms, sort_ms, total_ms; int64_t n_emitted; } dg_sketch_timing;
int dg_sketch_get_timing(dg_ctx *, dg_sketch_timing *);
/* parity / test knobs of the read spectrum (Sp_R, src/solver.cpp:526-546; none is needed in normal use):
 *   spectrum_mode m        0 (default): the tile kernel drops every minimizer into the bucket of its hash range, one LDS table
 *                          per bucket resolves it (dg_sketch_spectrum.hip); full buckets spill into one shared list, and only when
 *                          that runs over is the pass repeated with exact placement.  2: exact placement at once.  1: the generic path, a stable 64-bit radix sort of
 *                          all (hash, read) pairs + reduce-by-key.  The output is the same bit for bit.
 *   bucket_bits b          0 (default): buckets sized to the input; 1..15: 2^b buckets
 *   bucket_stride n        0 (default): 12288 slots per bucket in mode 0
 *   spill_cap n            0 (default): 2^20 pairs in the shared spill list of full buckets; -1: none (a full bucket repeats the pass
 *                          with exact placement at once)
 *   residual_cap n         0 (default): 1024 residual entries per bucket (third hashes of a table entry); fewer (-1: none)
 *                          leave more buckets to the host's per-segment finish
 *   host_buckets n         0 (default): up to 256 buckets may be left to the host before the generic path takes over; 1..256
 * and of dg_sketch_tag_reads:
 *   tag_lds_entries n      0 (default): a read of up to 1024 emissions is deduplicated in an LDS set, longer ones by a sort of their
 *                          segment; 1..1024: that limit (tests: both routes give the same records)
 *   tag_table_bits b       0 (default): the dictionary table has the power of two >= 2 x distinct hashes slots; 1..30: 2^b slots
 *                          (DG_ERR_ARG from the call if that leaves no empty slot)
 * dg_sketch_get_stat names, about the last dg_sketch_reads / dg_sketch_reads_dev call: spectrum_path (0 buckets filled by the
 * tile kernel, 1 exact placement, 2 generic), buckets, overflow_buckets (finished by the host per segment), spilled_pairs;
 * about the last dg_sketch_tag_reads call: tag_long_reads (reads that took the sort), tag_dict_distinct, tag_table_slots
 * This list is documentation: the option table beside dg_sketch_set_option (csrc/dg_sketch.hip) is authoritative for names, ranges and defaults. */
int dg_sketch_set_option(dg_ctx *, const char *name, int64_t value);
int dg_sketch_get_option(dg_ctx *, const char *name, int64_t *value);   /* the stored value (0 = the default of every option) */
int dg_sketch_get_stat(dg_ctx *, const char *name, int64_t *value);

/* Device-resident variants for the read-sharded multi-GPU path (one rank per GPU; collectives are
 * done by the caller over RCCL on the same buffers).
 *  dg_sketch_reads_dev: bases/read_off are DEVICE pointers; writes up to cap distinct (hash,count)
 *  pairs of THIS shard, sorted by hash, into device buffers; *n_distinct on host. Synchronises. */
int dg_sketch_reads_dev(dg_ctx *, const char *bases_dev, const int64_t *read_off_dev, int64_t n_reads,
                        int64_t n_bases, int k, int w, uint64_t *hash_dev, int32_t *count_dev, int64_t cap,
                        int64_t *n_distinct);
/* counts_dev[i] += count of dict_dev[i] in the shard's (hash,count) list (both sorted); the caller
 * then all-reduces counts_dev (uint32 per dictionary minimizer). Asynchronous on the ctx stream. */
int dg_sketch_count_dictionary_dev(dg_ctx *, const uint64_t *dict_dev, int64_t n_dict,
                                   const uint64_t *hash_dev, const int32_t *count_dev, int64_t n,
                                   int32_t *counts_dev);
/* merge several sorted (hash,count) runs stored back to back (device) into one sorted distinct
 * list with summed counts (device, capacity cap). Synchronises.  Entries (0xFFFFFFFFFFFFFFFF, 0) are the padding of
 * a fixed-size exchange: a last entry with that hash and summed count 0 is dropped (a real hash has count >= 1). */
int dg_sketch_merge_runs_dev(dg_ctx *, const uint64_t *hash_dev, const int32_t *count_dev, int64_t n_total,
                             uint64_t *out_hash_dev, int32_t *out_count_dev, int64_t cap, int64_t *n_out);

/* Read-sharded scoring across ranks (semantics of solver.cpp:526-555, 711-755): the uint64 hash space is
 * cut into `world` equal ranges, rank r owns range r of the global spectrum.
 *  dg_sketch_partition_dev: split_dev[r] (r = 0..world) = first index of the sorted list hash_dev[n] owned by a rank
 *  >= r, i.e. the send offsets of the all-to-all of (hash,count) runs.  Asynchronous on the ctx stream. */
int dg_sketch_partition_dev(dg_ctx *, const uint64_t *hash_dev, int64_t n, int world, int64_t *split_dev);
/* rank1_dev[i] += base + idx + 1 for every dictionary hash that is entry idx of this rank's merged range hash_dev[n]
 * (base = number of distinct read hashes in lower ranges): after a sum over ranks rank1 - 1 is the Sp_R id
 * (solver.cpp:541-546), -1 = not a read minimizer.  Asynchronous on the ctx stream. */
int dg_sketch_rank_dictionary_dev(dg_ctx *, const uint64_t *dict_dev, int64_t n_dict, const uint64_t *hash_dev, int64_t n,
                                  int64_t base, int64_t *rank1_dev);
/* dg_sketch_count_dictionary_dev and dg_sketch_rank_dictionary_dev against the SAME list in one pass (one rank: the local
 * spectrum is the global one).  Asynchronous. */
int dg_sketch_count_rank_dictionary_dev(dg_ctx *, const uint64_t *dict_dev, int64_t n_dict, const uint64_t *hash_dev,
                                        const int32_t *count_dev, int64_t n, int64_t base, int32_t *counts_dev, int64_t *rank1_dev);
/* hist_dev[min(max(count, 0), n_bins-1)] += 1 per entry: this range's share of Hist_kmer (solver.cpp:745-755).  Asynchronous.
 * The count / merge / partition / rank / count_rank / histogram entry points above answer DG_ERR_ARG ("<entry point>: bad arguments") to a negative size and to a null pointer whose
 * size is positive, and write nothing then; a size of 0 with null pointers is no error. */
int dg_sketch_histogram_dev(dg_ctx *, const int32_t *count_dev, int64_t n, int n_bins, uint64_t *hist_dev);

/* ---- read-sharded scoring inside ONE process (bin/DipGenie --gpus N; SURVEY.md s8e, BASELINE configs[3]) ----
 * One host thread and one dg_ctx per rank; transport 0 = RCCL (librccl is dlopen-ed here, an in-process communicator over the
 * `devices`, one device per rank), transport 1 = the same exchange staged through host memory between the rank threads (tests on a
 * one-GPU box, where several ranks share a device).  dg_shard_ctx(s, r) is rank r's context: the caller sketches the haplotypes
 * h = r (mod N) on it from N threads of its own (index_kmers is independent per haplotype, solver.cpp:470-473) and runs the rest of
 * the pipeline on rank 0's.
 * dg_shard_score_reads replaces compute_hashes over all reads + Sp_R + kmer_count + Hist_kmer (solver.cpp:526-555, 711-755):
 * every rank sketches its contiguous block of the reads, the hit vector of the haplotype-minimizer dictionary (the sorted distinct
 * set of hap_hash[n_hap_hash], built on every device) is all-reduced over RCCL, the (hash, #reads) runs are exchanged by hash range
 * in one grouped send / receive and merged by their owners.  Out: sp_hash / sp_count (malloc-ed, dg_free) = Sp_R's keys in ascending
 * order with kmer_count; hist[n_bins] (multiplicities >= n_bins - 1 share the last bin); n_dict, dict_hits = size of the dictionary and
 * how many of its hashes some read holds; the slowest rank's sketch and exchange times (HIP events, ms).  Any of the last five may be NULL. */
typedef struct dg_shard dg_shard;
dg_shard *dg_shard_create(int n_ranks, const int *devices, int transport);   /* devices NULL: 0 .. n_ranks-1; NULL on error (dg_last_error) */
void      dg_shard_destroy(dg_shard *);
int       dg_shard_n_ranks(dg_shard *);
dg_ctx   *dg_shard_ctx(dg_shard *, int rank);
int       dg_shard_score_reads(dg_shard *, const char *bases, const int64_t *read_off, int64_t n_reads, int k, int w,
                               const uint64_t *hap_hash, int64_t n_hap_hash, uint64_t **sp_hash, int32_t **sp_count, int64_t *n_sp,
                               int64_t *hist, int n_bins, int64_t *n_dict, int64_t *dict_hits, double *ms_sketch_max, double *ms_exchange_max);

/* ---- haplotype index with vertex spans + anchor join / filter / sort ----
 * Replaces, for all haplotypes at once, Solver::index_kmers including its position -> vertex-list mapping
 * (src/solver.cpp:277-363), Solver::compute_anchors and the Anchor_hits assembly (:415-446, 560-575), the shared-anchor
 * filter (:590-638) and the occurrence sort (:641-663).  Call order: dg_anchor_begin, dg_anchor_add_haplotype for
 * h = 0 .. n_haps-1, dg_sketch_reads (any time), dg_anchor_finish.  All pointers are host memory. */
int dg_anchor_begin(dg_ctx *, int32_t n_haps, int32_t n_vertices, const int32_t *top_order_map /* [n_vertices], solver.cpp:174-199 */,
                    int k, int w);
/* seq = the haplotype's bases (node_seq concatenated along paths[h], :283-288); step_vtx[n_steps] = paths[h];
 * step_start[n_steps + 1] = base offset of every step (step_start[n_steps] = len, so a walk of zero steps has len = 0; anything
 * else is DG_ERR_ARG).  *n_minimizers = |index_kmers(h)|. */
int dg_anchor_add_haplotype(dg_ctx *, int32_t h, const char *seq, int64_t len, const int32_t *step_vtx, const int64_t *step_start,
                            int64_t n_steps, int64_t *n_minimizers);
/* the same for a haplotype whose minimizer list (hash / pos = the output of dg_sketch_haplotype on its sequence, host memory) was
 * computed elsewhere: in a haplotype-sharded run every rank sketches its share of the haplotypes (src/solver.cpp:470-473 runs
 * index_kmers once per haplotype, independently) and the rank that owns the anchor stage imports them. */
int dg_anchor_add_haplotype_sketched(dg_ctx *, int32_t h, int64_t len, const uint64_t *hash, const int64_t *pos, int64_t n,
                                     const int32_t *step_vtx, const int64_t *step_start, int64_t n_steps);
typedef struct dg_anchor_result {     /* Anchor_hits flattened: occurrence i = (occ_id[i], occ_hap[i], vpool[occ_off[i] .. +occ_len[i])), */
    int64_t n_occ, n_vtx;             /* in Anchor_hits order (id asc, haplotype asc, occurrence order of :641-663)                     */
    int32_t *occ_id, *occ_hap;        /* malloc'ed by the library: dg_free each                                                         */
    uint32_t *occ_off, *occ_len;
    int32_t *vpool;
    int64_t n_candidates;             /* occurrences before the shared-anchor filter                                                    */
    int64_t n_unstable_groups;        /* (id, haplotype) groups of > 16 occurrences holding different vertex lists with equal (front,  */
} dg_anchor_result;                   /* back): their order would depend on std::sort's unstable partitioning -- redo the stage on the host */
/* sp_hash[n_sp] = sorted distinct read-minimizer hashes (Sp_R keys, the output of dg_sketch_reads); min_shared =
 * threshold * num_walks as float (:618).  Consumes the index built since dg_anchor_begin.  Environment, read at call time:
 * DG_DEBUG (stage timings and counts on stderr), DG_ANCHOR_FP_BITS = 0..64 (tests: keep that many bits of the filter's list
 * fingerprints, to force the collisions that take its exact order). */
int dg_anchor_finish(dg_ctx *, const uint64_t *sp_hash, int64_t n_sp, float min_shared, dg_anchor_result *out);

#ifdef __cplusplus
}
#endif
#endif

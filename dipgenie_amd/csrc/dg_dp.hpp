// Diploid pair-of-paths DP: types and entry points shared by the translation units of the DP
// (dg_dp_tables.hip, dg_dp_pairs.hip, dg_dp_delta.hip, dg_dp_sweep.hip, dg_dp_trace.hip, dg_dp_budgets.hip, dg_dp_run.hip, dg_dp_score.hip, dg_dp_partner.hip, dg_dp_marginals.hip,
// dg_dp_objective.hip, dg_dp_joint.hip, dg_dp_pins.hip).
//
// Replaces the level loop + sink read-out of Approximator::diploid_dp_approximation_solver
// (/root/reference/src/approximator.cpp:532-716, 757-785).  Design:
//   * gather form: every destination cell (i2, j2, r2) of level l+1 reduces over in(u2) x in(v2) -- one wave per
//     (destination row, group of <= 64 column in-edges, chunk of recombination counts), lanes on the column
//     in-edges; in-edges are stored sorted by source position, so a lexicographic max over (value, in-edge ranks)
//     reproduces the reference's take-if total order (value desc, pred_i asc, pred_j asc, :657-659) without locks
//     or atomics, and no destination is ever "reset" (:565-576 disappears);
//   * rolling value state is 4 B/cell, layout [i][r][j] (j fastest); s_het / edge chains are not carried
//     (reference cell = 40 B).  Every cell streams one 2-byte back-pointer (ranks of the winning in-edges) to HBM
//     and a traceback walks the lattice from the sink, emitting the weighted-edge lists (:757-764, :673-692) and
//     re-deriving s_het from the colour lists of the L winning edge pairs;
//   * score deltas (:604-624) do not depend on r nor on other levels: a launch fills, for every transition that
//     touches a colour, the T x T matrix delta[e_u][e_v] (uint16), T = #in-edges of the destination level;
//   * one launch per level (the levels are a dependency chain); the host picks the chunk size RC per level from a
//     cost model and gives rows with many in-edges cooperative workgroups.  (Several levels per dispatch with row-completion
//     counters in place of the kernel boundary were built and measured 3-6x slower: profiles/r03_chained_dispatch_ab.txt.)
#pragma once
#include <condition_variable>
#include <atomic>
#include <map>
#include <mutex>
#include <thread>
#include <tuple>

#include "dg_internal.hpp"

namespace dgi {

constexpr int32_t NEG_INF = INT32_MIN / 4;              // approximator.cpp:413
constexpr uint32_t BP_NONE = 0xFFFFFFFFu;              // wide (32-bit) back-pointer of an unreachable cell
constexpr int MAX_K = 1 << 15;                          // hop words pack positions in 15 bits
// Back-pointers are 16 bits per cell: (eu << 8) | ev, the ranks of the winning in-edges inside the destination row's
// and column's in-edge lists (sorted by source position, so rank order IS the reference's (pred_i asc, pred_j asc)
// tie order); 0xFFFF = unreachable.  Only a level with an in-degree > 255 keeps the wide word
// pred_i | pred_j << 15 | wu << 30 | wv << 31 (two 16-bit units per cell) and runs on the generic kernel.
constexpr int BP_MAX_RANK = 255;
constexpr int COOP_MIN = 8;                             // rows with more in-edges get cooperative workgroups
constexpr int HEAVY_INLINE = 8;                         // heavy rows of a level whose index rides in the kernel arguments
constexpr int ROWX_MAX = 64;                            // widest row in-edge matrix (in-edges per row)
constexpr int DELTA_PER_BLOCK = 256 * 16;
constexpr int DELTA_PAD = 8;                            // delta[0..8) stays zero: the colourless transitions' slot
constexpr int32_t CHAIN_CORRUPT = INT32_MIN;            // ChainState::value after a hop left its level
// Score deltas are stored as uint16.  A delta is |(Hom u1 u Hom v1) n (Hom u2 u Hom v2)| + |(Het u1 u Het v1) /\ (Het u2 u Het v2)|:
// the intersection has at most as many ids as one of its sides, 2 * max_hom, the symmetric difference at most as many as the four
// het lists together, 4 * max_het.  Hom and het are separate lists, so the two terms add up.  (A single list stays below 16,384 ids.)
constexpr int64_t DELTA_MAX = 65535, COLOUR_LIST_MAX = 16383;
inline bool colour_lists_fit_delta(int64_t max_hom, int64_t max_het) {
    return max_hom <= COLOUR_LIST_MAX && max_het <= COLOUR_LIST_MAX && 2 * max_hom + 4 * max_het <= DELTA_MAX;
}

struct LevelDesc {                                      // transition (l-1) -> l, indexed by l; passed BY VALUE to the sweep
    int32_t a0, k;                                      // source level: first vertex id, width
    int32_t b0, k2;                                     // destination level
    uint32_t in_base;                                   // first in-edge of the destination level
    int32_t T;                                          // in-edges into the destination level
    int64_t delta_off;                                  // offset of the T*T uint16 matrix, -1 if all zero
    int64_t bp_off;                                     // offset of this level in the bp lattice, in 16-bit units (even)
    int32_t grp_first, ngroups;                         // column groups (runs of <=64 in-edges covering whole columns)
    int32_t dead_first, ndead;                          // destination columns with no in-edge
    int64_t slot_first;                                 // first entry of this level in the 64-wide slot table
    int32_t fast_ok, nblocks;                           // fast kernel usable; number of 64-slot blocks (>= ngroups: giant columns take several)
    int32_t heavy_first, n_heavy;                       // rows with more than COOP_MIN in-edges: slice of the heavy-row table
    int32_t bp_wide, bp_nt;                             // wide back-pointers on this level; stream them with non-temporal stores
    // Row in-edge matrix: rowx[rowx_off + i2 * rowx_stride + t] = t-th in-edge word of destination row i2 (0 beyond its
    // in-degree).  Its address needs nothing but kernel arguments, so the in-edge list of a fan-in row arrives in the
    // task's first load round together with the row and slot records (rowx_stride = 0: the level has no such matrix and
    // rows with more than two in-edges fetch their list from in_edge[] once the row record is in).
    int64_t rowx_off;
    int32_t rowx_stride;
    int16_t heavy_in[HEAVY_INLINE];                     // the level's first heavy rows (cooperative region: no table lookup)
    int32_t dmax;                                       // largest in-degree among the level's vertices (host: choice of RC)
};

struct TraceOut { int32_t value, s_het, n_e, overflow, corrupt, path_score; };   // path_score: sum of the score deltas along the walked path (must equal value)
struct ChainState { int32_t i, j, r, value; };
// walker block q of the chain launch walks chain `chain` (the caller's index; dg_dp_run: its one chain) from plane `budget` of the
// sink; blocks 0 .. G - 1 hold the group leaders, whose helpers read `planes` planes per level (dg_dp_trace.hip)
struct BudgetSlot { int32_t chain, budget, planes, pad_; };
constexpr int BUDGET_SYNC_STRIDE = 128;                 // bytes between the ChainSync records of two chains (a cache line each)
constexpr int BUDGET_HELPER_BLOCKS = 80;                // blocks beyond the walkers: ten per XCD, LEAN_PREFETCHERS of them find a ticket
struct ColourCsr { const int64_t *hom_off, *het_off; const int32_t *hom_col, *het_col; };

struct SweepArgs {                                      // generic sweep kernel
    const LevelDesc *descs;
    const uint32_t *in_off, *in_edge, *grp_begin;
    const int32_t *in_dst, *dead_cols;
    const uint16_t *delta, *delta_zero;                 // delta: biased so that delta[d.delta_off] is valid for the resident window
    char *ring;                                         // the two state slots (ping-pong: level l in slot l & 1), each slot_bytes long, data starts pad_bytes in
    size_t slot_bytes, pad_bytes;
    uint16_t *bp;
    unsigned long long *digest;
    int RP;
    int *progress;                                      // PfCtl::level: the level whose launch is running (dg_dp_sweep.hip: L2 prefetcher)
    int flip;                                           // 1: an odd number of level pairs ran before this level, so level l lives in slot (l & 1) ^ 1 (SweepLaunch::flip)
};

struct FastArgs {                                       // fast sweep kernel
    const uint4 *rowrec;
    const uint2 *slots;
    const uint32_t *in_edge, *rowx;
    const int32_t *dead_cols;
    const uint16_t *delta, *delta_zero;
    char *ring;                                         // padded allocation start of state slot 0; slot s starts at ring + s * slot_bytes
    uint16_t *bp;                                       // fast-form levels always store narrow back-pointers
    unsigned long long *digest;
    int RP, pad_bytes;                                  // pad_bytes: front padding of the state buffers
    uint32_t buf_bytes;                                 // size of one padded state buffer (what a buffer resource covers)
    uint32_t slot_bytes;                                // distance between two state slots
    int *progress;                                      // PfCtl::level: the level whose launch is running (L2 prefetcher)
    int flip;                                           // as SweepArgs::flip
#ifdef DG_SWEEP_PROBE
    unsigned long long *probe;                          // measurement build: 8 words per level
#endif
};

// DP states alive per device.  The side-stream features (L2 table prefetcher, score deltas beside the sweep) assume that nothing
// else shares the device's hardware queues with the sweep: with a second state on the SAME device a side-stream kernel of one may
// sit in front of the other's sweep.  States on other devices do not matter.
inline std::atomic<int> &dp_states_on_device(int device) { static std::atomic<int> n[64]; return n[device & 63]; }

// One instantiated sweep kernel: rc = its chunk of recombination counts, 0 for the generic kernel (one name for all its chunks).  Defined
// in dg_dp_sweep.hip beside the RC table and the dispatch: index() is dense (0 .. count() - 1, the order the launch profile prints).
struct SweepVariant {
    int rc;
    bool general, coop;
    int index() const;
    std::string name() const;                           // as rocprof prints the kernel, without its DIGEST argument
    bool exists() const;                                // the dispatch instantiates it (cooperative: the RC_COOP entries only)
    static int count();
    static SweepVariant at(int index);
};
// ---- level pairs (dg_dp_pairs.hip: tables; dg_dp_sweep.hip: dp_sweep_pair_kernel) ----
// Two adjacent low-fan-in levels (l - 1, l) composed into ONE transition from level l - 2: a cell of level l reduces over the composed
// in-edges (eu2, eu1) x (ev2, ev1); the state of level l - 1 is never written, its back-pointers only where a cell of level l wins through it.
constexpr int PAIR_MAX_INDEG = 8;                       // composed in-degree of a vertex (sum over its in-edges of their sources' in-degrees)
constexpr int PAIR_MAX_WIDTH = 255;                     // widths of both levels of a pair (8-bit positions in the records)
constexpr int PAIR_MAX_T = 2047;                        // in-edges into either level (11-bit score-delta rows)
constexpr int PAIR_RCS[] = {1, 2, 4};                   // chunk sizes dp_sweep_pair_kernel is instantiated for
constexpr int N_PAIR_RCS = (int)(sizeof PAIR_RCS / sizeof PAIR_RCS[0]);
// Fan-in pairs (dp_sweep_pair_coop_kernel): the later level may hold BIG rows, vertices of composed in-degree PAIR_MAX_INDEG + 1 ..
// PAIR_BIG_MAX_INDEG.  A big row has PAIR_BIG_MAX_INDEG wider records of its own (5-bit ranks) and a cooperative workgroup per
// (slot block, chunk) whose four waves walk a quarter of them each; its PAIR_MAX_INDEG light records carry PAIR_ROW_BIG as in-degree.
constexpr int PAIR_BIG_MAX_INDEG = 32;
constexpr int PAIR_BIG_INLINE = 8;                      // big rows of a narrow pair whose position rides in the kernel arguments (8 bits each); entries of PairDesc::big_in
constexpr uint32_t PAIR_ROW_BIG = 15;                   // in-degree field of a light row record: the row is a big one
// Wide pairs (option pair_wide): one of the three levels (source l - 2, middle l - 1, later l) is wider than PAIR_MAX_WIDTH.  The same
// records with 10-bit positions (PairLayout<true>), the same kernels instantiated for them (template parameter WIDE).
constexpr int PAIR_WIDE_MAX_WIDTH = 1023;               // widths of all three levels of a wide pair (10-bit positions in the records)
constexpr int PAIR_WIDE_BIG_INLINE = 4;                 // big rows of a wide pair whose position rides in the kernel arguments (16 bits each)
// Where the fields of a pair's records lie (dg_dp_pairs.hip writes them, pair_task reads them).  Row-record and slot x: source position,
// w1 at W1, middle position at MID, w2 at W2, (row records) composed in-degree at DEG; slot z: destination column at bit 20; the winner's
// mid word: middle row at MID_ROW, middle column at MID_COL, w2u + w2v below; kk = k1 | k2 << KK.  y and the ord word are the same in both.
template <bool WIDE> struct PairLayout;
template <> struct PairLayout<false> { static constexpr uint32_t POS = 0x7FFFu, W1 = 15, MID = 16, MID_MASK = 0xFFu, W2 = 24, DEG = 25, COL_MASK = 0xFFu, MID_ROW = 16, MID_COL = 8, MID_W = 0xFFu, KK = 8; };
template <> struct PairLayout<true> { static constexpr uint32_t POS = 0x3FFu, W1 = 10, MID = 11, MID_MASK = 0x3FFu, W2 = 21, DEG = 22, COL_MASK = 0x3FFu, MID_ROW = 13, MID_COL = 3, MID_W = 0x7u, KK = 10; };
struct PairDesc {                                       // pair of destination levels (l - 1, l); on the host and on the device (L2 prefetcher)
    int32_t l, nblocks;                                 // the later level; 64-slot blocks of composed column in-edges
    int32_t k0, k1, k2;                                 // widths of levels l - 2, l - 1, l
    int32_t dmax;                                       // largest composed in-degree among the vertices of level l
    int64_t row_first;                                  // first composed row record (PAIR_MAX_INDEG per vertex of level l)
    int64_t slot_first;                                 // first composed slot record
    int32_t n_big, dmax_light;                          // big rows (0: a light pair, dp_sweep_pair_kernel); largest composed in-degree among the light rows
    int64_t big_first;                                  // first entry of the big-row list (positions in level l, ascending); its records start at PAIR_BIG_MAX_INDEG * big_first
    uint16_t big_in[PAIR_BIG_INLINE];                   // the pair's first big rows (a wide pair passes the first PAIR_WIDE_BIG_INLINE of them)
    int32_t wide;                                       // 1: its records are PairLayout<true>'s (one of k0, k1, k2 exceeds PAIR_MAX_WIDTH)
};
// pair launches per kernel: light pairs by index into PAIR_RCS, fan-in pairs N_PAIR_RCS further on, then the same two of the wide layout
constexpr int PAIR_HIST_WIDE = 2 * N_PAIR_RCS, N_PAIR_HIST = 2 * PAIR_HIST_WIDE;
struct PairHist {
    int64_t n[N_PAIR_HIST] = {};
    void add(const PairHist &o, int64_t sign = 1) { for (int q = 0; q < N_PAIR_HIST; ++q) n[q] += sign * o.n[q]; }
};

struct SweepHist {                                      // launches per variant, by SweepVariant::index()
    std::vector<int64_t> n = std::vector<int64_t>((size_t)SweepVariant::count(), 0);
    void add(const SweepHist &o, int64_t sign = 1) { for (size_t q = 0; q < n.size(); ++q) n[q] += sign * o.n[q]; }
};

// Every option of dg_dp_set_option / dg_dp_get_option (key table: dg_dp_run.hip).  These initialisers are the defaults, written nowhere else.
struct DpOptions {
    int64_t side_stream = -1;                           // side_stream: -1 = on while this is the device's only DP state (and the concurrency probe agrees), 0 = off, 1 = on
    int64_t plane_limit = 1;                            // plane_limit: beyond HBM, re-sweep every segment only up to the plane its path leaves it on (0: all planes)
    int64_t want_digest = 0;                            // digest: accumulate per-level digests (values + back-pointers)
    int64_t use_fast = 1;                               // fast: 0 forces the generic kernel
    int64_t adaptive_rc = 1;                            // adaptive_rc: 0 = one chunk of all recombination counts per task
    int64_t use_coop = 1;                               // coop: cooperative tasks for rows with many in-edges (2: whenever possible)
    int64_t max_blocks = 1024;                          // max_blocks: grid of the generic kernel
    int64_t segment_cells = 0;                          // segment_cells: force lattice segments of at most this many cells (tests)
    int64_t host_threads = 16;                          // host_threads: threads of dg_dp_load_graph's host table construction
    int64_t test_poison_level = 0, test_poison_byte = 0xFF;   // test_poison_*: overwrite one level of the lattice between sweep and walk (tests of the corrupt-lattice path)
    int64_t test_force_rc = 0;                          // test_force_rc: n != 0 = the per-level RC choice considers the table entry of n recombination counts only (tests: one variant per run)
    int64_t host_tables = 0;                            // host_tables: 1 = build the tables on the host and upload them (dg_dp_tables.hip; parity twin of dg_dp_build.hip)
    int64_t bp_nt_min_cells = 262144;                   // bp_nt_min_cells: levels this big stream their back-pointers non-temporally
    int64_t graph_batch = -1;                           // graph_batch: levels per captured hipGraph (0 = plain launches, -1 = the default of 1,000)
    int64_t warm_ahead = 128;                           // warm_ahead: sweep look-ahead, levels per batch (0 = off)
    int64_t sync_every = 0;                             // sync_every: drain the stream every N level launches (profiler aid)
    int64_t l2_prefetch = 6;                            // l2_prefetch: levels the per-XCD table prefetcher runs ahead of the sweep (0: off)
    int64_t use_lean_chain = 1;                         // lean_chain: 1 the lean walk where the lattice allows it, 0 always the general one; next load
    int64_t delta_overlap = 1;                          // delta_overlap: 0 = the whole window before the sweep
    int64_t pf_far = 128;                               // pf_far: > 0 = prefetcher blocks also pull the tables pf_far levels ahead into the Infinity Cache (then no periodic look-ahead launches)
    int64_t use_rowx = 1;                               // rowx: row in-edge matrices (0: every fan-in row fetches its list from in_edge[])
    int64_t delta_cap_entries = (int64_t)4 << 30;       // delta_cap_entries: budget of resident score-delta entries
    int64_t rc_cap = 65536, rc_t0_ns = 3000, rc_tg_ps = 20000, rc_tw_ps = 50;   // rc_*: cost model of the per-level RC choice
    int64_t chunk_units_cfg = (int64_t)4 << 30;         // lattice_chunk_cells: size of one lattice chunk (16-bit units, even: 8 GB)
    int64_t score_slab_bytes = (int64_t)256 << 20;      // score_slab_bytes: bound of the path staging buffer of dg_dp_score_paths (a slab holds at least one pair)
    int64_t partner_slab_bytes = (int64_t)4 << 30;      // partner_slab_bytes: bound of the back-pointers, edge scores and paths of one slab of dg_dp_best_partners, of the forward values, edge scores, marginals and records of one slab of dg_dp_partner_marginals (a slab holds at least one query)
    int64_t partner_wide = 0;                           // partner_wide: the level state of dg_dp_best_partners / dg_dp_partner_marginals / dg_dp_call_margins in device memory: 0 never (LDS only), 1 for a call beyond the LDS limit, 2 always
    int64_t pair_levels = 1;                            // pair_levels: adjacent low-fan-in levels run as one composed launch (dg_dp_pairs.hip); next load
    int64_t pair_min = 4096;                            // pair_min: the composed tables are built and used only for a graph with at least this many pairs; next load
    int64_t pair_fanin = 1;                             // pair_fanin: pairs whose later level has rows of composed in-degree 9..32 (big rows, dp_sweep_pair_coop_kernel); next load
    int64_t pair_fanin_min = 4096;                      // pair_fanin_min: ... only on a graph that has at least this many of them; below, the pairs are chosen as with pair_fanin 0; next load
    int64_t pair_fanin_max_big = 4, pair_fanin_max_indeg = PAIR_BIG_MAX_INDEG;     // pair_fanin_max_*: a fan-in pair has at most this many big rows / this largest composed in-degree; the gate measured on MHC-24: every big row adds four rows of workgroups, and from five big rows on a pair costs more than its two single launches (DESIGN s3.3); next load
    int64_t pair_wide = 1;                              // pair_wide: pairs with a level of 256..1,023 vertices (10-bit records: the WIDE instantiations of the pair kernels); next load
    int64_t pair_wide_min = 1024;                       // pair_wide_min: ... only on a graph that has at least this many of them; below, the pairs are chosen as with pair_wide 0; next load
    int64_t pair_wide_fanin = 1;                        // pair_wide_fanin: 0 = a wide pair has no big rows; next load
    int64_t pair_wide_max_width = PAIR_WIDE_MAX_WIDTH;  // pair_wide_max_width: widest level of a wide pair (measurement: 511 against 1,023); next load
    int64_t pair_wide_rc = 0;                           // pair_wide_rc: n in PAIR_RCS = every wide pair launch takes chunks of n recombination counts (measurement); any other value: the cost model
    int64_t pair_digest = 0;                            // pair_digest: 1 = with digest 1 the pair launches stay, in the pair kernel's digest form (tests: the later level's digest; the earlier level's entry stays 0)
    int64_t test_force_pair_rc = 0;                     // test_force_pair_rc: n in PAIR_RCS = every pair launch takes chunks of n recombination counts; any other value: the cost model
    int64_t joint_state_bytes = (int64_t)8 << 30;       // joint_state_bytes: bound of the forward states of one segment of dg_dp_genotype_margins (a segment holds at least one level)
    int64_t genotype_table_bytes = (int64_t)256 << 20;  // genotype_table_bytes: bound of the staging of finished entries of dg_dp_genotype_table, copied to the host when it fills and once per segment (a guess: nothing has measured another value); one level's bound A (A + 1) / 2 entries must fit
    int64_t genotype_table_lanes = 0;                   // genotype_table_lanes: lanes that reduce one genotype over its rows in dg_dp_genotype_table: 0 = the level's mean rows per class, else n, either rounded down to a power of two in 1..64
    int64_t genotype_table_tile_keys = 2048;            // genotype_table_tile_keys: keys of a level's dense genotype triangle that one workgroup of dg_dp_genotype_table's compaction counts and writes: 256 lanes x 1..8 keys, so 256..2048 in steps of 256
    int64_t genotype_table_scan_tiles = 1024;           // genotype_table_scan_tiles: tiles that the one workgroup scanning a level's tile counts takes per pass (a carry links the passes): its lanes, 64..1024 in steps of 64
    int64_t objective_lds_bytes = 131072;              // objective_lds_bytes: the four colour bitmaps of a pair of dg_dp_objective_paths / dg_dp_answer_objectives live in LDS up to this size, in device memory beyond (clamped to the device's LDS per workgroup)
};

struct DpState {
    explicit DpState(int dev) : device(dev) { ++dp_states_on_device(device); }
    ~DpState() { --dp_states_on_device(device); }
    const int device;
    DpOptions opt;
    bool side_stream_ok() const { return opt.side_stream < 0 ? dp_states_on_device(device).load() <= 1 : opt.side_stream != 0; }
    DpState(const DpState &) = delete;
    DpState &operator=(const DpState &) = delete;
    int32_t nV = 0, L = 0, R = 0, RP = 0, cap = 0;
    bool loaded = false;
    bool lean_chain = false;
    // single-window score deltas computed beside the sweep: piece k (transitions of levels >= delta_piece_level[k]) signals delta_piece_ev[k]
    std::vector<hipEvent_t> delta_piece_ev;
    std::vector<int32_t> delta_piece_level;
    int delta_piece_next = 0;                           // first piece the sweep has not waited for yet
    hipStream_t pf_stream = nullptr;                    // the ONE side stream: score-delta pieces, then the L2 table prefetcher (dg_dp_sweep.hip)
    hipEvent_t pf_ev = nullptr;
    int pf_seq = 0;
    bool pf_active = false;                             // a prefetcher accompanies the sweep range being issued
    int pf_tested = 0;                                  // 0: the side stream's concurrency with the sweep's stream not yet probed, 1: probed
    // ---- lattice segments: destination levels [seg_begin[s], seg_begin[s+1]); one segment = whole lattice resident.
    // More than one = checkpoint + recompute (value-only pass, then each segment re-swept with back-pointers, last first).
    std::vector<int> seg_begin;
    std::vector<int64_t> ckpt_off;                     // element offset of checkpoint s (state of level seg_begin[s]-1)
    bool graph_failed = false;                          // capture or instantiation failed once: plain launches from then on
    typedef std::tuple<int, int, const void *, int> GraphKey;     // (first level, end level, biased lattice pointer, look-ahead launches left to the prefetcher | state-slot flip on entry << 1 | planes swept << 2)
    struct Batch { hipGraphExec_t exec = nullptr; SweepHist hist; PairHist pair_hist; int64_t n_launch = 0; int flips = 0; };   // flips: parity of its pair launches
    std::map<GraphKey, Batch> graphs;                             // -> replayable batch and its launches by kernel variant
    bool all_fast = false;
    size_t state_alloc_bytes = 0;
    std::vector<LevelDesc> descs;
    uint64_t cells = 0, relaxations = 0, edge_pairs = 0, colour_entries = 0;
    int64_t total_units = 0, max_level_units = 0;       // back-pointer lattice, in 16-bit units (1 per cell, 2 on wide levels)
    int64_t max_level_cells = 0, delta_entries = 0, n_delta_blocks = 0, pad_front = 0;
    std::vector<int64_t> level_units;                   // units of every level (even)
    // score-delta windows: coloured transitions [dwin_t[w], dwin_t[w+1]) are resident together (one window = everything
    // unless the matrices outgrow delta_cap_entries; then each window is recomputed right before its first level)
    std::vector<int32_t> dwin_t, level_win;             // level_win[l] = window of level l's transition, -1 if colourless
    int cur_win = -1;                                   // window whose matrices are in d_delta right now
    std::vector<int32_t> dtrans_host;
    std::vector<int64_t> dblk_first_host;
    int64_t delta_buf_entries = 0;
    std::vector<int32_t> level_dmax;                    // largest in-degree among the level's vertices
    int64_t n_grp = 0, n_dead = 0, n_heavy_rows = 0, n_slot_records = 0, n_rowx_words = 0, n_dtrans = 0, n_edges = 0;   // logical table sizes (dg_dp_get_table_digest)
    DevBuf d_descs, d_in_off, d_in_edge, d_in_dst, d_hom_off, d_het_off, d_hom_col, d_het_col, d_eflag, d_eself;
    // level pairs: pair_at[l] = index of the pair whose later level is l, -2 for the earlier level of a pair, -1 otherwise (empty: no pairs)
    std::vector<PairDesc> pairs;
    std::vector<int32_t> pair_at;
    DevBuf d_pairs, d_pair_at, d_prow, d_pslots, d_pbig, d_pbig_rows;   // d_pbig: the big rows' records (uint2), d_pbig_rows: their positions (int32)
    PairHist pair_hist;                                 // pair launches of the last run (dg_dp_get_pair_profile)
    DevBuf d_delta, d_bp, d_ring, d_digest, d_dblk_first, d_dtrans, d_grp, d_dead, d_heavy, d_rowrec, d_rowx, d_slots, d_ckpt, d_pfctl;
#ifdef DG_SWEEP_PROBE
    DevBuf d_probe;
#endif
    std::vector<uint64_t> digest_host;
    SweepHist launch_hist;                              // launches of the last run per sweep kernel variant (dg_dp_get_launch_profile)
    dg_dp_timing timing;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    // The resident back-pointer lattice lives in a pool of equal chunks that a background thread allocates one by
    // one (a 100+ GB hipMalloc takes seconds, more when another process has just freed HBM): reservation can start
    // before the graph exists (dg_dp_prealloc) without starving the small allocations of the sketch stage.
    // Levels never straddle chunks.
    struct Pool {
        std::mutex mu;
        std::condition_variable cv;
        std::vector<void *> chunks;           // each chunk_units * 2 bytes
        size_t chunk_units = (size_t)DpOptions().chunk_units_cfg;
        size_t target = 0;                     // chunks wanted
        size_t cap_chunks = 0;                 // upper bound for reservations made before the graph is known
        bool running = false, failed = false, paused = false;
        std::thread th;
    } pool;
    std::vector<int> chunk_begin;              // destination levels [chunk_begin[c], chunk_begin[c+1]) live in chunk c
    int seg_chunks = 1;                        // chunks per lattice segment (= all of them when the lattice is resident)
    // ---- the chains of a run (dg_dp_budgets.hip): one per requested budget, dg_dp_run = the one chain of budget R ----
    // Every chain has its own path slice (L hop words), ChainState, ChainSync, TraceOut and edge block; d_ch_tab holds the budgets
    // and the walker placement (BudgetSlot per block).  d_sink keeps the sink's RP values of the last run, taken when the sweep
    // reaches the sink (the second pass of a segmented run overwrites the state ring).
    DevBuf d_sink, d_ch_path, d_ch_state, d_ch_sync, d_ch_trace, d_ch_edges, d_ch_tab;
    std::vector<int32_t> sink_host;            // the sink's value on planes 0..R (dg_dp_get_budget_values); empty before the first run
    std::vector<BudgetSlot> tab_host;          // host copy of d_ch_tab (the run at hand)
    int n_groups = 0;                          // walker groups of the run at hand (chains of neighbouring budgets share an XCD and its helpers)
    mutable int walk_seq = 0;                  // per-launch number of the chain walk (ChainSync; counted from 0 in every run)
    // ---- dg_dp_score_paths (dg_dp_score.hip): staging of one slab of caller paths, its result words, the first-bad-hop word ----
    DevBuf d_sc_paths, d_sc_out, d_sc_err;
    // ---- dg_dp_best_partners (dg_dp_partner.hip): one slab of queries -- (given, partner) pairs, budgets, sink cells, the re-scoring
    // pass's records, the two first-bad-hop words; back-pointers and edge scores (released when the call returns) ----
    DevBuf d_pt_pairs, d_pt_bud, d_pt_val, d_pt_out, d_pt_err, d_pt_bp, d_pt_scores;
    // the device-memory route (option partner_wide) of these calls and of the two below: per query two level states of kmax * (bmax + 1)
    // int32 (released when the call returns); the route and the cells of the last call that chose one (dg_dp_get_partner_route)
    DevBuf d_pt_state;
    int32_t pt_route = 0;
    int64_t pt_route_cells = 0;
    // ---- dg_dp_partner_marginals (dg_dp_marginals.hip): the level records and the marginals of one slab; the given paths, budgets, sink
    // cells, first-bad-hop word, forward values (in d_pt_bp) and edge scores live in the buffers above ----
    DevBuf d_mg_levels, d_mg_vertex;
    // ---- the answer of the last run as paths, and its call margins (dg_dp_budgets.hip, dg_dp_marginals.hip) ----
    bool run_ok = false;                       // the last dg_dp_run / dg_dp_run_budgets on the loaded graph returned DG_OK: d_ch_path and d_ch_state hold its chains (sink_host is emptied by a load)
    DevBuf d_ans_paths, d_ans_cnt;             // dg_dp_get_answer_paths: the [2][L] vertex ids and the two counts of weight-1 hops
    DevBuf d_cm_class, d_cm_out;               // dg_dp_call_margins: the caller's classes (released when the call returns) and the [2][L] records
    // ---- dg_dp_objective_paths / dg_dp_answer_objectives (dg_dp_objective.hip): the colour dictionary of the loaded graph -- per kind the
    // number of distinct ids and one rank per colour-list entry, parallel to d_hom_col / d_het_col -- built by the first of these calls
    // after a load (a load only clears ob_dict; a run neither reads nor writes any of this), and one slab's paths, records, first-bad-hop
    // word and, on the global route, bitmaps ----
    bool ob_dict = false;
    int64_t ob_ch = 0, ob_ct = 0;              // distinct hom / het colours
    DevBuf d_ob_hom_rank, d_ob_het_rank, d_ob_paths, d_ob_out, d_ob_err, d_ob_bits;
    // ---- dg_dp_genotype_margins / dg_dp_genotype_table (dg_dp_joint.hip): nothing but the statistics of the last call outlives it
    // (dg_dp_get_genotype_stats: segments, levels swept forward twice, peak bytes reserved, launches, table entries, staging copies, pins,
    // mask launches: the last two are 0 after an unpinned call) ----
    int64_t jt_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // dg_dp_phase_margins (dg_dp_joint.hip) likewise (dg_dp_get_phase_stats: het levels, records, backward launches on the seeded state,
    // read-out launches, segments, peak bytes reserved)
    int64_t ph_stats[6] = {0, 0, 0, 0, 0, 0};
    // dg_dp_phase_margins_budgets likewise (dg_dp_get_phase_budget_stats: queries, records, seed keys created, slot-levels, backward launches
    // on the slots, read-out launches, largest number of live slots, slots allocated, segments, peak bytes reserved)
    int64_t phb_stats[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    // dg_dp_recombination_margins likewise (dg_dp_get_recombination_stats: transitions, edge-kernel launches, finish launches, segments,
    // levels swept forward twice, peak bytes reserved, launches in all)
    int64_t rb_stats[7] = {0, 0, 0, 0, 0, 0, 0};
    // dg_dp_recombination_margins_budgets likewise (dg_dp_get_recombination_budget_stats: queries, distinct budgets, transitions, edge-kernel
    // launches, finish launches, segments, levels swept forward twice, peak bytes reserved, launches in all)
    int64_t rbb_stats[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    // ---- dg_dp_run_pinned (dg_dp_pins.hip): the call's pins sorted by level (uploaded once per call), whether the last run on the loaded
    // graph was a pinned one, and the statistics of the last pinned run (dg_dp_get_pin_stats: pins, pinned levels, mask launches, pairs
    // run as singles, batches issued plainly) ----
    DevBuf d_pins;
    bool run_pinned = false;
    int64_t pin_stats[5] = {0, 0, 0, 0, 0};
};

inline ColourCsr colour_csr(const DpState &S) {
    return ColourCsr{S.d_hom_off.as<int64_t>(), S.d_het_off.as<int64_t>(), S.d_hom_col.as<int32_t>(), S.d_het_col.as<int32_t>()};
}

// ---- lattice chunk pool (dg_dp_run.hip) ----
void pool_request(DpState &S, int device, size_t target);
void pool_trim(DpState &S, size_t keep);
inline void pool_clear(DpState &S) { pool_trim(S, 0); }
void *pool_wait(DpState &S, size_t c);
struct PoolPause {                       // hipMalloc calls queue behind the one in flight: hold the pool thread between chunks
    DpState &S;
    explicit PoolPause(DpState &s);
    ~PoolPause();
};
void graphs_clear(DpState &S);
double wall_s();

// ---- table construction (dg_dp_tables.hip: entry, host construction, lattice plan; dg_dp_build.hip: device construction) ----
int dp_load(dg_ctx *c, const dg_dp_graph *g);
int dp_build_tables_device(dg_ctx *c, const dg_dp_graph *g, DpState &S, std::vector<int32_t> &dtrans, std::vector<int64_t> &dblk_first, int &max_k);
int dp_table_digest(dg_ctx *c, uint64_t *out, int n);
int dp_build_pairs(dg_ctx *c, const dg_dp_graph *g, DpState &S);           // dg_dp_pairs.hip: chooses the level pairs and builds their tables (host)

// ---- score deltas (dg_dp_delta.hip) ----
void delta_launch_edge_flags(const DpState &S, hipStream_t s);
// (re)computes the matrices of window w into d_delta; returns the pointer biased so that ptr[LevelDesc::delta_off] is valid
const uint16_t *delta_launch_window(DpState &S, int w, hipStream_t s);
const uint16_t *delta_launch_overlapped(DpState &S, hipStream_t s);          // one window: first piece on s, the rest on a side stream (events in delta_piece_*)
void delta_overlap_free(DpState &S);

// ---- level sweep (dg_dp_sweep.hip) ----
struct SweepLaunch {                     // per-run launch context
    SweepArgs A;
    FastArgs F;
    bool small_state = true;
    int rc_sel = 0;                      // chunk of "all recombination counts": the table's first all-planes entry that holds R + 1
    bool digest = false;                 // this pass accumulates the level digests (the re-sweeps of a segmented run do not: pass 1 did)
    int rp_active = 0;                   // planes [0, rp_active) are swept by the fast kernels (= RP except while a segment is re-swept below its path's plane)
    SweepHist hist;                      // launches of this run by kernel variant
    PairHist pair_hist;                  // its pair launches
    bool pairs_ok = false;               // this pass may launch level pairs (dg_dp_run.hip decides)
    int flip = 0;                        // parity of the pair launches so far: level l's state lives in slot (l & 1) ^ flip
};
void sweep_prepare(const DpState &S, SweepLaunch &X);
void sweep_init_state(const DpState &S, hipStream_t s);                  // level 0: every r starts at 0 (:534-535)
int sweep_launch_level(const DpState &S, SweepLaunch &X, int l, hipStream_t s);
int sweep_launch_pair(const DpState &S, SweepLaunch &X, int l, hipStream_t s);   // levels l - 1 and l (S.pair_at[l] >= 0) in one launch
std::string pair_variant_name(int q);                                      // of PairHist::n[q], as rocprof prints the kernel
void sweep_warm_tables(const DpState &S, const SweepLaunch &X, int q0, int q1, hipStream_t s);
int sweep_prefetch_begin(DpState &S, const SweepLaunch &X, int lb, int le, bool delta_resident, hipStream_t s);
void sweep_prefetch_end(DpState &S, int le, hipStream_t s);
void sweep_prefetch_free(DpState &S);

// ---- traceback (dg_dp_trace.hip) ----
void trace_launch_warm_rows(const DpState &S, int lb, int le, hipStream_t s);
void trace_launch_chains(const DpState &S, int n, int l_hi, int l_lo, const uint16_t *bp_biased, const int32_t *final_val, hipStream_t s);   // all n chains, one launch
void trace_launch_finish_chain(const DpState &S, const uint2 *path, int32_t *edges, const ChainState *st, TraceOut *out, hipStream_t s);   // the finish kernel on one chain's buffers
void trace_debug_report(const DpState &S, int n);

// ---- the chains of a run: buffers, placement, sink values, finish (dg_dp_budgets.hip) ----
void budgets_launch_sink_copy(const DpState &S, const int32_t *sink_state, hipStream_t s);   // sink values of planes 0..R -> d_sink
int budgets_reserve(DpState &S, int n);                                                      // buffers of n chains (grow-only)
int budgets_prepare(DpState &S, const int32_t *budgets, int n, hipStream_t s);                // buffers of n chains + walker placement
void budgets_launch_finish(const DpState &S, int n, hipStream_t s);                           // the finish kernel once per chain
// the chain that the last run walked for `budget` (fn: the entry point's name, for the messages): DG_ERR_STATE without a graph, without a
// run since the load, or for a budget that run did not read out
int budgets_find_chain(const char *fn, const DpState *S, int32_t budget, int &chain);
// the chain's path slice expanded into vertex ids: row h of the pair goes to out + (h ^ swap) * L (device), the weight-1 hops of row h
// are added to cnt[h] (device, zeroed here).  A chain whose budget nothing fits writes -1 everywhere.
void budgets_launch_expand(const DpState &S, int chain, int swap, int32_t *out, int32_t *cnt, hipStream_t s);
int dp_get_answer_paths(dg_ctx *c, int32_t budget, int32_t *paths);

// ---- caller-supplied pairs of paths scored on the resident graph (dg_dp_score.hip) ----
int dp_score_paths(dg_ctx *c, const int32_t *paths, int64_t n_pairs, dg_dp_pair_score *out);
int score_pair_blocks(const DpState &S);                                                     // workgroups per pair of the scoring kernel
// the scoring kernel on n pairs [n][2][L] resident on the device; out (4 words per pair) zeroed and *err all ones beforehand
void score_launch_pairs(const DpState &S, const int32_t *pairs, int64_t n, int32_t *out, unsigned long long *err, hipStream_t s);

// ---- pairs of paths by the distinct-colour objective (dg_dp_objective.hip) ----
int dp_objective_paths(dg_ctx *c, const int32_t *paths, int64_t n_pairs, dg_dp_pair_objective *out);
int dp_answer_objectives(dg_ctx *c, const int32_t *budgets, int32_t n_budgets, dg_dp_pair_objective *out);
int64_t objective_lds_limit(const dg_ctx *c);                                                // the largest objective_lds_bytes the device allows

// ---- the best partner of a given path: the DP with one haplotype fixed (dg_dp_partner.hip) ----
int dp_best_partners(dg_ctx *c, const int32_t *given, int64_t n, const int32_t *budgets, int32_t *partners, dg_dp_partner *out);

// ---- partner marginals: that DP forward and backward, combined per vertex (dg_dp_marginals.hip; shares dg_dp_partner.hpp with the above) ----
int dp_partner_marginals(dg_ctx *c, const int32_t *given, int64_t n, const int32_t *budgets, dg_dp_level_margin *levels, int32_t *vertex_values);
int dp_call_margins(dg_ctx *c, int32_t budget, const int32_t *vertex_class, dg_dp_call_margin *levels, int32_t *paths);

// ---- pinned calls (dg_dp_pins.hip): the per-level cell constraints of one dg_dp_run_pinned, dg_dp_genotype_margins_pinned or
// dg_dp_genotype_table_pinned ----
struct PinSet {
    std::vector<int32_t> off;            // [L + 1]: the pins of level l are d_pins[off[l] .. off[l + 1]) (sorted by level, input order inside a level)
    const dg_dp_pin *d_pins = nullptr;   // device
    int64_t n_mask = 0, n_pairs_split = 0, n_batches_plain = 0;   // what the run at hand issued because of them
    bool has(int l) const { return off[(size_t)l + 1] > off[(size_t)l]; }
    bool any_in(int l0, int l1) const { return off[(size_t)l1] > off[(size_t)l0]; }
};
// validates the pins against the loaded graph (DG_ERR_ARG naming fn, the entry point, and the first offending pin), sorts them by level
// and uploads them into buf (the run: DpState::d_pins; the joint pass: a buffer of the call)
int pins_prepare(const char *fn, const DpState &S, const dg_dp_pin *pins, int64_t n, PinSet &P, DevBuf &buf);
// stores NEG_INF into the cells of `level` that its pins do not allow, on all RP planes of the level's state slab `state` ([i][r][j])
void pins_launch_mask(const DpState &S, PinSet &P, int level, int32_t *state, hipStream_t s);
// the same for a state of the joint pass: [i][j][r] with `planes` planes, k = the level's width
void pins_launch_joint_mask(PinSet &P, int level, int32_t *state, int k, int planes, hipStream_t s);

// ---- genotype margins: the DP forward and backward with both haplotypes free, combined per cell (dg_dp_joint.hip) ----
// pinned = false: the unpinned entry points (pins ignored); true: the *_pinned ones, which with n_pins = 0 run the same pass
int dp_genotype_margins(dg_ctx *c, bool pinned, const dg_dp_pin *pins, int64_t n_pins, const int32_t *called, int64_t n, int32_t budget, const int32_t *vertex_class,
                        dg_dp_genotype_margin *levels, int32_t *vertex_values, int32_t *best_value);
int dp_genotype_table(dg_ctx *c, bool pinned, const dg_dp_pin *pins, int64_t n_pins, int32_t budget, const int32_t *vertex_class, const int32_t *called, int64_t n,
                      dg_dp_genotype_margin *levels, int64_t *level_off, dg_dp_genotype_entry **entries, int64_t *n_entries, int32_t *best_value);
// one budget per query, from one pass at the largest (n_pins = 0: unpinned)
int dp_genotype_margins_budgets(dg_ctx *c, const dg_dp_pin *pins, int64_t n_pins, const int32_t *called, const int32_t *budgets, int64_t n, const int32_t *vertex_class,
                                dg_dp_genotype_margin *levels, int32_t *best_values);
int dp_genotype_stats(dg_ctx *c, int64_t *out, int n);
// phase margins: cis against trans for neighbouring het levels of one called pair, from the same pass with one more backward state
int dp_phase_margins(dg_ctx *c, const int32_t *called, int32_t budget, const int32_t *vertex_class, dg_dp_phase_margin *records, int64_t *n_records, int32_t *best_value);
int dp_phase_stats(dg_ctx *c, int64_t *out, int n);
// the same for many called pairs, each at a budget of its own, from one pass at the largest: a pool of seeded states, one per live seed key
int dp_phase_margins_budgets(dg_ctx *c, const int32_t *called, const int32_t *budgets, int64_t n, const int32_t *vertex_class, dg_dp_phase_margin *records, int64_t *record_off,
                             int32_t *best_values);
int dp_phase_budget_stats(dg_ctx *c, int64_t *out, int n);
// recombination margins: per transition the best pair of paths that spends 0, 1 or 2 crossovers there, from the same pass with one more gather
int dp_recombination_margins(dg_ctx *c, int32_t budget, const int32_t *called, int64_t n, dg_dp_recombination_margin *records, int32_t *called_out, int32_t *best_value);
int dp_recombination_stats(dg_ctx *c, int64_t *out, int n);
// the same for every listed budget from one pass at the largest: only the planes paired in the gather depend on the budget
int dp_recombination_margins_budgets(dg_ctx *c, const int32_t *budgets, int64_t n, const int32_t *called, dg_dp_recombination_margin *records, int32_t *called_out,
                                     int32_t *best_values);
int dp_recombination_budget_stats(dg_ctx *c, int64_t *out, int n);

}  // namespace dgi

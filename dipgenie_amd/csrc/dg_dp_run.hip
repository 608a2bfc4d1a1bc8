// dg_dp_run and the DP entry points of the C ABI: issues the level chain (plain launches or replayed hipGraph batches),
// drives lattice chunks / segments (checkpoint + recompute when the back-pointer lattice outgrows HBM), the score-delta
// windows and the traceback, and turns the edge records into the two weighted-edge lists (approximator.cpp:757-785).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <ctime>

#include "dg_dp.hpp"

namespace dgi {

constexpr int DELTA_NO_PIECES = 1 << 30;

double wall_s() { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec + 1e-9 * ts.tv_nsec; }

void graphs_clear(DpState &S) {                 // captured level batches: stale as soon as the graph, the lattice or an option changes
    for (auto &kv : S.graphs) if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
    S.graphs.clear();
}

void dp_state_free(DpState *s) {
    if (!s) return;
    graphs_clear(*s);
    sweep_prefetch_free(*s);
    delta_overlap_free(*s);
    { std::unique_lock<std::mutex> lk(s->pool.mu); s->pool.target = 0; }
    s->pool.cv.notify_all();
    if (s->pool.th.joinable()) s->pool.th.join();
    const double tf0 = wall_s();
    for (void *q : s->pool.chunks) (void)hipFree(q);
    if (getenv("DG_DEBUG")) fprintf(stderr, "[dipgenie_hip] destroy: %zu lattice chunks freed in %.3f s\n", s->pool.chunks.size(), wall_s() - tf0);
    for (auto &e : s->ev) if (e) (void)hipEventDestroy(e);
    delete s;
}

// ---------------------------------------------------------------------------------------------
// lattice chunk pool
// ---------------------------------------------------------------------------------------------
// Ask for `target` chunks (the latest request wins): starts the allocation thread if chunks are missing.  Chunks
// already mapped beyond the target are kept (hipFree of 8 GB costs ~0.1 s) unless pool_trim is called.  Returns at once.
void pool_request(DpState &S, int device, size_t target) {
    std::unique_lock<std::mutex> lk(S.pool.mu);
    S.pool.target = std::max(target, S.pool.chunks.size());
    if (S.pool.running || S.pool.chunks.size() >= S.pool.target) return;
    if (S.pool.th.joinable()) { lk.unlock(); S.pool.th.join(); lk.lock(); }
    S.pool.running = true;
    S.pool.failed = false;
    DpState *Sp = &S;
    S.pool.th = std::thread([Sp, device]() {
        (void)hipSetDevice(device);
        for (;;) {
            size_t bytes;
            {
                std::unique_lock<std::mutex> lk2(Sp->pool.mu);
                // (a lowered target must get through a pause: pool_trim joins this thread while dg_dp_load_graph holds the pause)
                Sp->pool.cv.wait(lk2, [&] { return !Sp->pool.paused || Sp->pool.chunks.size() >= Sp->pool.target; });
                if (Sp->pool.chunks.size() >= Sp->pool.target) { Sp->pool.running = false; Sp->pool.cv.notify_all(); return; }
                bytes = Sp->pool.chunk_units * 2;
            }
            void *q = nullptr;
            const hipError_t e = hipMalloc(&q, bytes);
            std::unique_lock<std::mutex> lk2(Sp->pool.mu);
            if (e != hipSuccess) { (void)hipGetLastError(); Sp->pool.failed = true; Sp->pool.running = false; Sp->pool.cv.notify_all(); return; }
            Sp->pool.chunks.push_back(q);
            Sp->pool.cv.notify_all();
            lk2.unlock();
            // HIP calls of other threads queue on a runtime lock this thread would otherwise win again at once
            std::this_thread::sleep_for(std::chrono::milliseconds(1));
        }
    });
}
PoolPause::PoolPause(DpState &s) : S(s) { std::unique_lock<std::mutex> lk(S.pool.mu); S.pool.paused = true; }
PoolPause::~PoolPause() { { std::unique_lock<std::mutex> lk(S.pool.mu); S.pool.paused = false; } S.pool.cv.notify_all(); }
// free chunks beyond `keep` (and stop asking for more than that)
void pool_trim(DpState &S, size_t keep) {
    { std::unique_lock<std::mutex> lk(S.pool.mu); S.pool.target = std::min(std::min(S.pool.target, keep), S.pool.chunks.size()); }
    S.pool.cv.notify_all();
    if (S.pool.th.joinable()) S.pool.th.join();               // it stops at the next chunk boundary (a paused one: at once)
    std::unique_lock<std::mutex> lk(S.pool.mu);
    while (S.pool.chunks.size() > keep) { (void)hipFree(S.pool.chunks.back()); S.pool.chunks.pop_back(); }
    S.pool.running = false;
}
// wait until chunk c exists; nullptr if the allocation failed
void *pool_wait(DpState &S, size_t c) {
    std::unique_lock<std::mutex> lk(S.pool.mu);
    S.pool.cv.wait(lk, [&] { return S.pool.chunks.size() > c || S.pool.failed || !S.pool.running; });
    return S.pool.chunks.size() > c ? S.pool.chunks[c] : nullptr;
}

// ---------------------------------------------------------------------------------------------
// one DP pass over the resident graph
// ---------------------------------------------------------------------------------------------
namespace {

struct Run {
    dg_ctx *c;
    DpState &S;
    hipStream_t s;
    SweepLaunch X;
    int64_t n_launch = 0;
    int next_warm = 0;                                  // next level at which the look-ahead launch is due
    double host_enqueue_s = 0;                          // host time spent issuing the sweep's launches (DG_DEBUG)
    int n_chains = 1;                                   // chains walked from the sink, one per budget (dg_dp_run: 1)
    std::vector<uint16_t *> pool_base;
    PinSet *P;                                          // dg_dp_run_pinned: the call's cell constraints; null in every other run

    Run(dg_ctx *c_, DpState &S_, PinSet *P_ = nullptr) : c(c_), S(S_), s(c_->stream), P(P_) { sweep_prepare(S, X); }
    int n_win() const { return (int)S.dwin_t.size() - 1; }
    int32_t *state_ptr(int level) const { return (int32_t *)(S.d_ring.as<char>() + (size_t)((level & 1) ^ X.flip) * S.state_alloc_bytes) + S.pad_front; }   // (the slot parity as the launches issued so far left it)
    size_t level_cells(int level) const {               // state size of a level (level 0: the source, k = 1)
        const int64_t k = level == 0 ? 1 : S.descs[level].k2;
        return (size_t)(k * k * S.RP);
    }
    void load_window(int w) { X.A.delta = X.F.delta = delta_launch_window(S, w, s); }

    // issues the launches of destination levels [l0, l1) of the range that began at lb
    int issue_levels(int l0, int l1, int lb, int le) {
        for (int l = l0; l < l1; ++l) {
            if (S.level_win[l] >= 0 && S.level_win[l] != S.cur_win) load_window(S.level_win[l]);
            if (S.opt.warm_ahead > 0 && l >= next_warm && (l == lb || !(S.pf_active && S.opt.pf_far > 0))) {
                // tables of the batch after this one (and, at the start of a range, of this one too)
                const int q0 = l == lb ? l : (int)std::min<int64_t>(l + S.opt.warm_ahead, le), q1 = (int)std::min<int64_t>(l + 2 * S.opt.warm_ahead, le);
                if (q1 > q0) sweep_warm_tables(S, X, q0, q1, s);
            }
            if (l >= next_warm) next_warm = l + (int)std::max<int64_t>(S.opt.warm_ahead, 1);
            // a level pair (dg_dp_pairs.hip) runs as one launch where both of its levels lie inside this batch; else each level as ever
            // (a pinned run: the pair kernel never writes the state of its earlier level, so a pin there makes the pair two single launches)
            const bool pair_here = X.pairs_ok && l + 1 < l1 && S.pair_at[l + 1] >= 0;
            if (pair_here && !(P && P->has(l))) {
                if (S.level_win[l + 1] >= 0 && S.level_win[l + 1] != S.cur_win) load_window(S.level_win[l + 1]);
                if (int rc = sweep_launch_pair(S, X, ++l, s)) return rc;
            } else {
                if (pair_here) ++P->n_pairs_split;
                if (int rc = sweep_launch_level(S, X, l, s)) return rc;
            }
            ++n_launch;
            // The mask of a pinned level follows the launch that wrote it, on the same stream: whatever reads the level next -- the next
            // launch, the checkpoint copy in front of a segment (a pin on a segment's last level is in the checkpoint), the sink copy --
            // is ordered behind it.  state_ptr: the slot parity as that launch left it, a pair's flip included.
            if (P && P->has(l)) pins_launch_mask(S, *P, l, state_ptr(l), s);
            // profiling aid: rocprofv3 --pmc crashes when ~10^5 dispatches are queued without a drain
            if (S.opt.sync_every > 0 && n_launch % S.opt.sync_every == 0) DG_HIP(hipStreamSynchronize(s));
        }
        return DG_OK;
    }

    // Sweeps destination levels [lb, le).  bp_biased = lattice pointer minus the offset of level lb's first cell
    // (so the kernels keep using the global LevelDesc::bp_off), or nullptr for a value-only pass.
    // Issuing a level costs the host 2.3-5.4 us (hipLaunchKernelGGL; it varies from run to run on a shared host), the GPU
    // 2.7-4.2 us: since the sweep's own period came down to ~4.1 us the chain is host-bound as often as not (MHC-24 sweeps of
    // 596-742 ms with plain launches, pass after pass of one process).  So the levels are captured into hipGraphs of 1,000
    // launches and replayed: 590.5-593 ms on MHC-24, the capturing pass included, 320 ms on MHC_4 (option graph_batch: 0 =
    // plain launches, which at their best are 2 % faster).
    // A stream that cannot be captured (e.g. a caller-provided legacy stream) or a failed instantiation switches the
    // context back to plain launches for good; the batch at hand is then issued again, plainly.
    int sweep_range(int lb, int le, uint16_t *bp_biased) {
        X.A.bp = bp_biased; X.F.bp = bp_biased;
        next_warm = lb;
        if (int rc = sweep_prefetch_begin(S, X, lb, le, n_win() == 1, s)) return rc;
        const int64_t gb = S.opt.graph_batch >= 0 ? S.opt.graph_batch : 1000;
        // what issue_levels bakes into a captured batch besides the levels: whether the periodic look-ahead launches are left to the
        // prefetcher's far blocks -- part of the cache key (a second DP state on the device switches the prefetcher off)
        for (int l0 = lb; l0 < le;) {
            const int pf_key = ((S.pf_active && S.opt.pf_far > 0) ? 1 : 0) | (X.flip << 1) | (X.rp_active << 2);
            const bool graph_ok = gb > 0 && n_win() == 1 && S.opt.sync_every == 0 && !S.graph_failed;
            const int l1 = graph_ok ? (int)std::min<int64_t>((int64_t)l0 + gb, le) : le;
            // a pinned run: a batch that holds a pinned level is issued plainly, neither replayed from S.graphs nor stored there (the batch
            // bounds stay, so the batches around it find their cache entries; the slot flip on entry is part of their key)
            const bool pinned_batch = P && P->any_in(l0, l1);
            if (graph_ok && pinned_batch) ++P->n_batches_plain;
            const bool use_graph = graph_ok && !pinned_batch;
            // score deltas computed beside the sweep (delta_launch_overlapped): the stream waits for the pieces that hold a level below l1
            while (S.delta_piece_next < (int)S.delta_piece_level.size() && S.delta_piece_level[S.delta_piece_next] < l1) {
                DG_HIP(hipStreamWaitEvent(s, S.delta_piece_ev[S.delta_piece_next], 0));
                ++S.delta_piece_next;
            }
            const DpState::GraphKey key(l0, l1, (const void *)bp_biased, pf_key);
            DpState::Batch *slot = nullptr;
            bool capturing = false;
            if (use_graph) {
                slot = &S.graphs[key];
                if (slot->exec) {
                    DG_HIP(hipGraphLaunch(slot->exec, s));
                    X.hist.add(slot->hist); X.pair_hist.add(slot->pair_hist);
                    n_launch += slot->n_launch; X.flip ^= slot->flips; l0 = l1;
                    continue;
                }
                if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) == hipSuccess) capturing = true;
                else { (void)hipGetLastError(); S.graph_failed = true; continue; }
            }
            const int64_t n_launch_before = n_launch;
            const SweepHist hist_before = X.hist;
            const PairHist pair_hist_before = X.pair_hist;
            const int flip_before = X.flip;
            if (int rc = issue_levels(l0, l1, lb, le)) {
                if (capturing) {                                    // leave the stream usable: end the capture, drop the half-built graph
                    hipGraph_t cg = nullptr;
                    (void)hipStreamEndCapture(s, &cg);
                    if (cg) (void)hipGraphDestroy(cg);
                    (void)hipGetLastError();
                    S.graphs.erase(key);
                }
                return rc;
            }
            if (capturing) {
                hipGraph_t cg = nullptr;
                const bool ok = hipStreamEndCapture(s, &cg) == hipSuccess && cg && hipGraphInstantiate(&slot->exec, cg, nullptr, nullptr, 0) == hipSuccess;
                if (cg) (void)hipGraphDestroy(cg);
                if (!ok) {                                          // nothing of this batch has run: issue it again without a graph
                    (void)hipGetLastError();
                    slot->exec = nullptr; S.graph_failed = true; n_launch = n_launch_before; X.hist = hist_before; X.pair_hist = pair_hist_before; X.flip = flip_before;
                    continue;
                }
                slot->hist = X.hist;
                slot->hist.add(hist_before, -1);
                slot->pair_hist = X.pair_hist;
                slot->pair_hist.add(pair_hist_before, -1);
                slot->n_launch = n_launch - n_launch_before; slot->flips = X.flip ^ flip_before;
                DG_HIP(hipGraphLaunch(slot->exec, s));
            }
            l0 = l1;
        }
        sweep_prefetch_end(S, le, s);
        return DG_OK;
    }

    // Launches issued while the pool thread is still mapping chunks would each queue behind a multi-GB hipMalloc,
    // so there is nothing to overlap: wait for every chunk this run uses first.
    int wait_for_chunks() {
        if (S.d_bp.p) return DG_OK;
        const double tw0 = wall_s();
        const size_t need = (size_t)std::min(S.seg_chunks, (int)S.chunk_begin.size() - 1);
        if (!pool_wait(S, need - 1)) { set_error("back-pointer lattice: hipMalloc of a %.1f GB chunk failed", S.pool.chunk_units * 2 / 1e9); return DG_ERR_OOM; }
        std::unique_lock<std::mutex> lk(S.pool.mu);
        for (size_t q = 0; q < need; ++q) pool_base.push_back((uint16_t *)S.pool.chunks[q]);
        if (getenv("DG_DEBUG")) fprintf(stderr, "[dipgenie_hip] run: waited %.3f s for lattice chunks\n", wall_s() - tw0);
        return DG_OK;
    }

    // lattice chunk ch of a run of chunks that begins with c0: its destination levels [lb, le) and its back-pointers (pool chunk ch - c0, or
    // the one exact buffer) biased as sweep_range takes them
    std::tuple<int, int, uint16_t *> chunk(int ch, int c0) const {
        const int lb = S.d_bp.p ? 1 : S.chunk_begin[ch], le = S.d_bp.p ? S.L : S.chunk_begin[ch + 1];
        return {lb, le, (S.d_bp.p ? S.d_bp.as<uint16_t>() : pool_base[ch - c0]) - S.descs[lb].bp_off};
    }

    // Sweeps the chunks [c0, c1) with back-pointers into pool chunks 0 .. c1-c0-1 (or the one exact buffer), then walks
    // them last first; from_sink = this is the walk that starts at the sink.
    int sweep_and_walk(int c0, int c1, bool from_sink, bool mark_forward_end) {
        for (int ch = c0; ch < c1; ++ch) {
            const auto [lb, le, bp] = chunk(ch, c0);
            const double th0 = wall_s();
            if (int rc = sweep_range(lb, le, bp)) return rc;
            host_enqueue_s += wall_s() - th0;
        }
        if (mark_forward_end) { DG_HIP(hipEventRecord(S.ev[2], s)); budgets_launch_sink_copy(S, state_ptr(S.L - 1), s); }
        if (S.opt.test_poison_level > 0 && S.opt.test_poison_level < S.L)        // tests: a level nobody swept / a damaged lattice
            for (int ch = c0; ch < c1; ++ch) {
                const auto [lb, le, bp] = chunk(ch, c0);
                const int lp = (int)S.opt.test_poison_level;
                if (lp >= lb && lp < le) DG_HIP(hipMemsetAsync(bp + S.descs[lp].bp_off, (int)S.opt.test_poison_byte, 2 * (size_t)S.level_units[lp], s));
            }
        for (int ch = c1 - 1; ch >= c0; --ch) {
            const auto [lb, le, bp] = chunk(ch, c0);
            trace_launch_warm_rows(S, lb, le, s);
            const int32_t *final_val = from_sink && ch == c1 - 1 ? state_ptr(S.L - 1) : (const int32_t *)nullptr;
            trace_launch_chains(S, n_chains, le - 1, lb, bp, final_val, s);
        }
        return DG_OK;
    }

    int forward_and_trace() {
        const int n_seg = (int)S.seg_begin.size() - 1, n_chunks_all = (int)S.chunk_begin.size() - 1;
        DG_HIP(hipEventRecord(S.ev[0], s));
        S.cur_win = -1;
        S.delta_piece_next = DELTA_NO_PIECES;
        if (n_win() == 1 && S.n_delta_blocks > 0) X.A.delta = X.F.delta = delta_launch_overlapped(S, s);   // everything fits: the head up front (delta_ms), the rest beside the sweep
        DG_HIP(hipEventRecord(S.ev[1], s));
        if (S.opt.want_digest) DG_HIP(hipMemsetAsync(S.d_digest.p, 0, 8 * (size_t)S.L, s));
#ifdef DG_SWEEP_PROBE
        {   // slot 0 of every level takes an atomicMin: start from all ones
            std::vector<unsigned long long> init((size_t)S.L * 8, 0ULL);
            for (int l = 0; l < S.L; ++l) init[(size_t)l * 8] = ~0ULL;
            DG_HIP(hipMemcpy(S.d_probe.p, init.data(), 8 * init.size(), hipMemcpyHostToDevice));
        }
#endif
        sweep_init_state(S, s);
        // level pairs: the unsegmented pass over all planes, digests off (or pair_digest: the pair kernel's digest form), the per-level choice
        // of the fast kernels left free
        X.pairs_ok = !S.pairs.empty() && S.opt.pair_levels && n_seg == 1 && n_win() == 1 && (!X.digest || S.opt.pair_digest) && S.opt.use_fast && S.opt.adaptive_rc && S.opt.test_force_rc == 0 &&
                     X.small_state && X.rp_active == S.RP;
        if (n_seg == 1) {
            // whole lattice resident: one sweep with back-pointers, then the chain walk chunk by chunk, last first
            if (int rc = sweep_and_walk(0, S.d_bp.p ? 1 : n_chunks_all, true, true)) return rc;
        } else {
            // pass 1: values only, keeping the state in front of every segment
            int64_t planes_swept = 0;
            for (int sg = 0; sg < n_seg; ++sg) {
                if (sg > 0)
                    DG_HIP(hipMemcpyAsync(S.d_ckpt.as<int32_t>() + S.ckpt_off[sg], state_ptr(S.seg_begin[sg] - 1),
                                          4 * level_cells(S.seg_begin[sg] - 1), hipMemcpyDeviceToDevice, s));
                if (int rc = sweep_range(S.seg_begin[sg], S.seg_begin[sg + 1], nullptr)) return rc;
            }
            DG_HIP(hipEventRecord(S.ev[2], s));                 // (the re-sweeps below are booked under traceback_ms)
            budgets_launch_sink_copy(S, state_ptr(S.L - 1), s);  // the second pass overwrites the state ring
            // pass 2: last segment first -- restore its input state, re-sweep its chunks with back-pointers, walk them
            X.digest = false;                                       // digests were accumulated in pass 1
            // Along a path the recombination count only grows, and a cell of plane r gathers from planes r, r - 1, r - 2 of the level
            // before: once the walk has left segment sg on plane r*, the cells it can meet in the segments before lie on planes
            // <= r*, and those depend on planes <= r* only.  Every earlier segment is therefore re-swept up to the plane its
            // successor's walk ended on (one 16-byte read per chain and segment; several chains: the largest plane any of them left
            // on, an unreachable budget walks nothing) -- the path uses its recombinations along the whole panel, so about half of
            // the second pass goes away.  (The finish kernel re-scores the walked path against the DP value as ever.)
            for (int sg = n_seg - 1; sg >= 0; --sg) {
                const int lb = S.seg_begin[sg];
                if (sg > 0)
                    DG_HIP(hipMemcpyAsync(state_ptr(lb - 1), S.d_ckpt.as<int32_t>() + S.ckpt_off[sg], 4 * level_cells(lb - 1), hipMemcpyDeviceToDevice, s));
                else
                    sweep_init_state(S, s);
                const int c0 = sg * S.seg_chunks, c1 = std::min(n_chunks_all, c0 + S.seg_chunks);
                if (int rc = sweep_and_walk(c0, c1, sg == n_seg - 1, false)) return rc;
                if (S.opt.plane_limit && sg > 0) {
                    std::vector<ChainState> cs((size_t)n_chains);
                    DG_HIP(hipMemcpyAsync(cs.data(), S.d_ch_state.p, sizeof(ChainState) * cs.size(), hipMemcpyDeviceToHost, s));
                    DG_HIP(hipStreamSynchronize(s));
                    int planes = 1;
                    for (const ChainState &q : cs) {
                        if (q.value == NEG_INF) continue;
                        planes = std::max(planes, (q.value != CHAIN_CORRUPT && q.r >= 0 && q.r < S.RP) ? q.r + 1 : S.RP);
                    }
                    X.rp_active = planes;
                    planes_swept += (int64_t)planes * (S.seg_begin[sg] - S.seg_begin[sg - 1]);
                }
            }
            if (getenv("DG_DEBUG") && S.opt.plane_limit) fprintf(stderr, "[dipgenie_hip] run: second pass swept %.1f %% of the (level, plane) pairs before the last segment\n",
                                                              100.0 * (double)planes_swept / std::max(1.0, (double)S.RP * (S.seg_begin[n_seg - 1] - 1)));
        }
        budgets_launch_finish(S, n_chains, s);
        DG_HIP(hipEventRecord(S.ev[3], s));
        DG_HIP(hipGetLastError());
        return DG_OK;
    }
};

}  // namespace

// checks one chain's TraceOut and turns its edge records into the two weighted-edge lists; budget < 0: not named in the messages (dg_dp_run)
static int emit_result(const DpState &S, const TraceOut &to, const int32_t *edges, dg_dp_result *res, int budget) {
    char who[32] = "";
    if (budget >= 0) snprintf(who, sizeof who, " (budget %d)", budget);
    if (to.value == CHAIN_CORRUPT || to.corrupt) { set_error("back-pointer lattice is corrupt: the chain walk left its level (a level was not swept?)%s", who); return DG_ERR_STATE; }
    if (to.value != NEG_INF && to.path_score != to.value) {
        set_error("traceback path scores %d but the DP value is %d: sweep, lattice and walk disagree%s", to.path_score, to.value, who); return DG_ERR_STATE;
    }
    if (to.overflow || to.n_e > S.cap) { set_error("traceback edge list overflow (%d > %d)%s", to.n_e, S.cap, who); return DG_ERR_STATE; }
    res->value = to.value; res->s_het = to.s_het;
    res->cells = S.cells; res->relaxations = S.relaxations;
    // records arrive in arbitrary order: path order = ascending level (the two records of the last level are equal)
    std::vector<int> order(to.n_e);
    for (int q = 0; q < to.n_e; ++q) order[q] = q;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return edges[a] < edges[b]; });
    int n1 = 0, n2 = 0;
    for (int q : order) {
        const int from = edges[S.cap + q], tov = edges[2 * S.cap + q];
        if (edges[3 * S.cap + q] == 0) { if (n1 < res->cap && res->p1_from && res->p1_to) { res->p1_from[n1] = from; res->p1_to[n1] = tov; } ++n1; }
        else { if (n2 < res->cap && res->p2_from && res->p2_to) { res->p2_from[n2] = from; res->p2_to[n2] = tov; } ++n2; }
    }
    res->n_p1 = n1; res->n_p2 = n2;
    return DG_OK;
}

// One pass over the resident graph (the callers have checked that one is loaded): one chain per budgets[q] into res[q], all walked
// by one launch per lattice chunk (dg_dp_trace.hip).  name_budget: error texts say which budget's chain failed.
static int dp_run(dg_ctx *c, const int32_t *budgets, int n_budgets, dg_dp_result *res, bool name_budget, PinSet *P = nullptr) {
    DpState &S = *c->dp;
    Run run(c, S, P);
    hipStream_t s = c->stream;
    if (int rc = run.wait_for_chunks()) return rc;
    std::vector<TraceOut> to((size_t)n_budgets);
    std::vector<int32_t> edges(4 * (size_t)S.cap * (size_t)n_budgets);
    S.run_ok = false;                                                   // the chains' buffers are about to be rewritten
    S.run_pinned = P != nullptr;
    if (int rc = budgets_prepare(S, budgets, n_budgets, s)) return rc;
    run.n_chains = n_budgets;
    S.sink_host.clear();
    const int rc_run = run.forward_and_trace();
    S.launch_hist = run.X.hist;
    S.pair_hist = run.X.pair_hist;
    if (rc_run) return rc_run;
    DG_HIP(hipMemcpyAsync(to.data(), S.d_ch_trace.p, sizeof(TraceOut) * to.size(), hipMemcpyDeviceToHost, s));
    DG_HIP(hipMemcpyAsync(edges.data(), S.d_ch_edges.p, 4 * edges.size(), hipMemcpyDeviceToHost, s));
    std::vector<int32_t> sink((size_t)S.RP);
    DG_HIP(hipMemcpyAsync(sink.data(), S.d_sink.p, 4 * sink.size(), hipMemcpyDeviceToHost, s));
    if (S.opt.want_digest) {
        S.digest_host.assign(S.L, 0);
        DG_HIP(hipMemcpyAsync(S.digest_host.data(), S.d_digest.p, 8 * (size_t)S.L, hipMemcpyDeviceToHost, s));
    }
    DG_HIP(hipStreamSynchronize(s));
    S.sink_host.swap(sink);
#ifdef DG_SWEEP_PROBE
    if (const char *po = getenv("DG_PROBE_OUT")) {
        std::vector<unsigned long long> pr((size_t)S.L * 8);
        DG_HIP(hipMemcpy(pr.data(), S.d_probe.p, 8 * pr.size(), hipMemcpyDeviceToHost));
        if (FILE *f = fopen(po, "wb")) { fwrite(pr.data(), 8, pr.size(), f); fclose(f); }
    }
#endif
    if (getenv("DG_DEBUG") && S.lean_chain) trace_debug_report(S, n_budgets);
    if (getenv("DG_DEBUG") && S.pf_stream) {
        int w[4] = {0, 0, 0, 0};
        if (hipStreamSynchronize(S.pf_stream) == hipSuccess && hipMemcpy(w, S.d_pfctl.p, sizeof w, hipMemcpyDeviceToHost) == hipSuccess)
            fprintf(stderr, "[dipgenie_hip] run: L2 table prefetcher covered %d levels (since load)\n", w[2]);
    }
    if (getenv("DG_DEBUG"))
        fprintf(stderr, "[dipgenie_hip] run: host issued %lld sweep launches in %.1f ms (%.2f us each)\n", (long long)run.n_launch, 1e3 * run.host_enqueue_s,
                1e6 * run.host_enqueue_s / (double)std::max<int64_t>(run.n_launch, 1));
    DG_HIP(hipEventElapsedTime(&S.timing.delta_ms, S.ev[0], S.ev[1]));
    DG_HIP(hipEventElapsedTime(&S.timing.forward_ms, S.ev[1], S.ev[2]));
    DG_HIP(hipEventElapsedTime(&S.timing.traceback_ms, S.ev[2], S.ev[3]));
    DG_HIP(hipEventElapsedTime(&S.timing.total_ms, S.ev[0], S.ev[3]));
    S.timing.n_forward_launches = run.n_launch;
    S.timing.n_segments = (int32_t)S.seg_begin.size() - 1;
    S.timing.n_chunks = (int32_t)S.chunk_begin.size() - 1;
    for (int q = 0; q < n_budgets; ++q)                                  // any corrupt or mis-scored chain fails the call
        if (int rc = emit_result(S, to[q], edges.data() + 4 * (size_t)S.cap * (size_t)q, res + q, name_budget ? budgets[q] : -1)) return rc;
    S.run_ok = true;                                                    // every chain's path slice is a checked pair of paths (dg_dp_get_answer_paths)
    return DG_OK;
}

// the budget rules of dg_dp_run_budgets and dg_dp_run_pinned (fn: the entry point's name, for the messages)
static int check_budgets(const char *fn, const DpState *Sp, const int32_t *budgets, int32_t n, const dg_dp_result *results) {
    if (!Sp || !Sp->loaded) { set_error("%s: no graph loaded", fn); return DG_ERR_STATE; }
    if (!budgets || !results || n <= 0) { set_error("%s: budgets, results and n_budgets > 0 are required", fn); return DG_ERR_ARG; }
    std::vector<char> seen((size_t)Sp->RP, 0);
    for (int q = 0; q < n; ++q) {
        const int b = budgets[q];
        if (b < 0 || b > Sp->R) { set_error("%s: budget %d (entry %d) outside 0..%d, the R of the loaded graph", fn, b, q, Sp->R); return DG_ERR_ARG; }
        if (seen[b]) { set_error("%s: budget %d listed twice", fn, b); return DG_ERR_ARG; }
        seen[b] = 1;
        if (results[q].cap < b + 2) { set_error("%s: results[%d].cap = %d, budget %d needs %d", fn, q, results[q].cap, b, b + 2); return DG_ERR_ARG; }
    }
    return DG_OK;
}

static int dp_run_budgets(dg_ctx *c, const int32_t *budgets, int32_t n, dg_dp_result *results) {
    if (int rc = check_budgets("dg_dp_run_budgets", c->dp, budgets, n, results)) return rc;
    return dp_run(c, budgets, n, results, true);
}

// dg_dp_run_pinned: every argument is checked before anything of the last run is touched
static int dp_run_pinned(dg_ctx *c, const dg_dp_pin *pins, int64_t n_pins, const int32_t *budgets, int32_t n, dg_dp_result *results) {
    if (n_pins == 0) return dp_run_budgets(c, budgets, n, results);
    if (int rc = check_budgets("dg_dp_run_pinned", c->dp, budgets, n, results)) return rc;
    DpState &S = *c->dp;
    if (S.opt.want_digest) {
        set_error("dg_dp_run_pinned: option digest is 1: the sweep accumulates a level's digest before the level's mask runs, so the digest would describe another DP");
        return DG_ERR_STATE;
    }
    PinSet P;
    if (int rc = pins_prepare("dg_dp_run_pinned", S, pins, n_pins, P, S.d_pins)) return rc;
    const int rc = dp_run(c, budgets, n, results, true, &P);
    int64_t n_levels = 0;
    for (int l = 1; l < S.L; ++l) n_levels += P.has(l);
    const int64_t st[5] = {n_pins, n_levels, P.n_mask, P.n_pairs_split, P.n_batches_plain};
    memcpy(S.pin_stats, st, sizeof st);
    return rc;
}

// dg_dp_run: the one-chain case -- the chain of budget R, named by no budget in its messages.  (No check of res->cap against the
// budget: edges beyond cap are counted, not stored.)
static int dp_run_single(dg_ctx *c, dg_dp_result *res) {
    if (!c->dp || !c->dp->loaded) { set_error("dg_dp_run: no graph loaded"); return DG_ERR_STATE; }
    if (!res) { set_error("dg_dp_run: null result"); return DG_ERR_ARG; }
    const int32_t budget = c->dp->R;
    return dp_run(c, &budget, 1, res, false);
}

}  // namespace dgi

extern "C" int dg_dp_load_graph(dg_ctx *c, const dg_dp_graph *g) {
    if (int rc = dgi::bind(c)) return rc;
    return dgi::dp_load(c, g);
}
extern "C" int dg_dp_run(dg_ctx *c, dg_dp_result *r) {
    if (int rc = dgi::bind(c)) return rc;
    return dgi::dp_run_single(c, r);
}
extern "C" int dg_dp_run_budgets(dg_ctx *c, const int32_t *budgets, int32_t n_budgets, dg_dp_result *results) {
    if (int rc = dgi::bind(c)) return rc;
    return dgi::dp_run_budgets(c, budgets, n_budgets, results);
}
extern "C" int dg_dp_run_pinned(dg_ctx *c, const dg_dp_pin *pins, int64_t n_pins, const int32_t *budgets, int32_t n_budgets, dg_dp_result *results) {
    if (int rc = dgi::bind(c)) return rc;
    return dgi::dp_run_pinned(c, pins, n_pins, budgets, n_budgets, results);
}
extern "C" int dg_dp_get_pin_stats(dg_ctx *c, int64_t *out, int n) {
    if (!c || !c->dp) { dgi::set_error("dg_dp_get_pin_stats: no state"); return DG_ERR_STATE; }
    if (!out || n < 5) { dgi::set_error("dg_dp_get_pin_stats: out with n >= 5 entries is required"); return DG_ERR_ARG; }
    memcpy(out, c->dp->pin_stats, sizeof c->dp->pin_stats);
    return DG_OK;
}
extern "C" int dg_dp_get_budget_values(dg_ctx *c, int32_t *out, int32_t n) {
    if (!c || !c->dp || !out) { dgi::set_error("dg_dp_get_budget_values: no state"); return DG_ERR_STATE; }
    const std::vector<int32_t> &v = c->dp->sink_host;
    if (v.empty()) { dgi::set_error("dg_dp_get_budget_values: no completed dg_dp_run / dg_dp_run_budgets on the loaded graph"); return DG_ERR_STATE; }
    if (n < (int32_t)v.size()) { dgi::set_error("dg_dp_get_budget_values: out has %d entries, R + 1 = %zu needed", n, v.size()); return DG_ERR_ARG; }
    memcpy(out, v.data(), 4 * v.size());
    return DG_OK;
}
extern "C" int dg_dp_solve_diploid(dg_ctx *c, const dg_dp_graph *g, dg_dp_result *r) {
    if (int rc = dg_dp_load_graph(c, g)) return rc;
    return dg_dp_run(c, r);
}
extern "C" int dg_dp_prealloc(dg_ctx *c, int64_t bytes) {
    if (int rc = dgi::bind(c)) return rc;
    if (!c->dp) c->dp = new dgi::DpState(c->device);
    dgi::DpState &S = *c->dp;
    if (S.pool.chunk_units != (size_t)S.opt.chunk_units_cfg) { dgi::pool_clear(S); S.pool.chunk_units = (size_t)S.opt.chunk_units_cfg; }
    const size_t chunk_bytes = S.pool.chunk_units * 2;
    if (S.pool.cap_chunks == 0) {          // first call only: later ones may arrive while chunks are being mapped
        size_t free_b = 0, total_b = 0;
        DG_HIP(hipMemGetInfo(&free_b, &total_b));
        S.pool.cap_chunks = std::max<size_t>(1, (size_t)(0.6 * (double)free_b) / chunk_bytes);
    }
    const size_t want_chunks = bytes > 0 ? std::min(((size_t)bytes + chunk_bytes - 1) / chunk_bytes, S.pool.cap_chunks) : S.pool.cap_chunks;
    dgi::pool_request(S, c->device, want_chunks);   // whole chunks; returns immediately
    return DG_OK;
}
extern "C" int dg_dp_get_timing(dg_ctx *c, dg_dp_timing *t) {
    if (!c || !c->dp || !t) { dgi::set_error("dg_dp_get_timing: no state"); return DG_ERR_STATE; }
    *t = c->dp->timing;
    return DG_OK;
}
extern "C" int dg_dp_get_level_digest(dg_ctx *c, uint64_t *out, int64_t n) {
    if (!c || !c->dp || !out) { dgi::set_error("dg_dp_get_level_digest: no state"); return DG_ERR_STATE; }
    if ((int64_t)c->dp->digest_host.size() != n) { dgi::set_error("digest not collected (set option digest=1) or size mismatch"); return DG_ERR_STATE; }
    memcpy(out, c->dp->digest_host.data(), 8 * (size_t)n);
    return DG_OK;
}
extern "C" int dg_dp_get_table_digest(dg_ctx *c, uint64_t *out, int n) {
    if (int rc = dgi::bind(c)) return rc;
    return dgi::dp_table_digest(c, out, n);
}
extern "C" int dg_dp_get_launch_profile(dg_ctx *c, char *buf, int cap) {
    if (!c || !c->dp || !buf || cap < 2) { dgi::set_error("dg_dp_get_launch_profile: no state"); return DG_ERR_STATE; }
    std::string out;
    for (int q = 0; q < dgi::SweepVariant::count(); ++q)
        if (const int64_t n = c->dp->launch_hist.n[(size_t)q]) out += (out.empty() ? "" : " ") + dgi::SweepVariant::at(q).name() + ':' + std::to_string(n);
    if ((int)out.size() + 1 > cap) { dgi::set_error("dg_dp_get_launch_profile: buffer too small (%zu needed)", out.size() + 1); return DG_ERR_ARG; }
    memcpy(buf, out.c_str(), out.size() + 1);
    return DG_OK;
}
extern "C" int dg_dp_get_pair_profile(dg_ctx *c, char *buf, int cap) {
    if (!c || !c->dp || !buf || cap < 2) { dgi::set_error("dg_dp_get_pair_profile: no state"); return DG_ERR_STATE; }
    std::string out;
    for (int q = 0; q < dgi::N_PAIR_HIST; ++q)
        if (const int64_t n = c->dp->pair_hist.n[q]) out += (out.empty() ? "" : " ") + dgi::pair_variant_name(q) + ':' + std::to_string(n);
    if ((int)out.size() + 1 > cap) { dgi::set_error("dg_dp_get_pair_profile: buffer too small (%zu needed)", out.size() + 1); return DG_ERR_ARG; }
    memcpy(buf, out.c_str(), out.size() + 1);
    return DG_OK;
}
extern "C" int dg_dp_list_pair_variants(char *buf, int cap) {
    std::string out;
    for (int q = 0; q < dgi::N_PAIR_RCS; ++q) out += (out.empty() ? "" : " ") + dgi::pair_variant_name(q);
    if (!buf || (int)out.size() + 1 > cap) { dgi::set_error("dg_dp_list_pair_variants: buffer too small (%zu needed)", out.size() + 1); return DG_ERR_ARG; }
    memcpy(buf, out.c_str(), out.size() + 1);
    return DG_OK;
}
extern "C" int dg_dp_list_sweep_variants(char *buf, int cap) {
    std::string out;
    for (int q = 0; q < dgi::SweepVariant::count(); ++q)
        if (dgi::SweepVariant::at(q).exists()) out += (out.empty() ? "" : " ") + dgi::SweepVariant::at(q).name();
    if (!buf || (int)out.size() + 1 > cap) { dgi::set_error("dg_dp_list_sweep_variants: buffer too small (%zu needed)", out.size() + 1); return DG_ERR_ARG; }
    memcpy(buf, out.c_str(), out.size() + 1);
    return DG_OK;
}
// Options: parity / test knobs (digest, fast, adaptive_rc, coop, rowx, lean_chain, segment_cells, delta_cap_entries, lattice_chunk_cells,
// graph_batch, warm_ahead, score_slab_bytes, partner_slab_bytes, partner_wide, joint_state_bytes, genotype_table_bytes, genotype_table_lanes, genotype_table_tile_keys, genotype_table_scan_tiles, objective_lds_bytes), profiler aid (sync_every), tuning (rc_*, bp_nt_min_cells, max_blocks, host_threads).
// One row per key: its DpOptions field, the lower clamp, whether v <= 0 asks for the default (that of a fresh DpOptions).
typedef dgi::DpOptions DpO;
static const struct DpOptionKey { const char *key; int64_t DpO::*field; int64_t lo; bool nonpos_is_default; } dp_option_keys[] = {
    // read by every run or call: in effect at once
    {"digest", &DpO::want_digest, 0, false}, {"fast", &DpO::use_fast, 0, false}, {"adaptive_rc", &DpO::adaptive_rc, 0, false}, {"coop", &DpO::use_coop, 0, false},
    {"sync_every", &DpO::sync_every, 0, false}, {"rc_t0_ns", &DpO::rc_t0_ns, 0, false}, {"rc_tg_ps", &DpO::rc_tg_ps, 0, false}, {"rc_tw_ps", &DpO::rc_tw_ps, 0, false},
    {"rc_cap", &DpO::rc_cap, 0, true}, {"max_blocks", &DpO::max_blocks, 0, true}, {"bp_nt_min_cells", &DpO::bp_nt_min_cells, 0, false}, {"warm_ahead", &DpO::warm_ahead, 0, false},
    {"graph_batch", &DpO::graph_batch, -1, false}, {"l2_prefetch", &DpO::l2_prefetch, 0, false}, {"delta_overlap", &DpO::delta_overlap, 0, false}, {"pf_far", &DpO::pf_far, 0, false},
    {"side_stream", &DpO::side_stream, -1, false}, {"plane_limit", &DpO::plane_limit, 0, false}, {"test_poison_level", &DpO::test_poison_level, 0, false},
    {"test_poison_byte", &DpO::test_poison_byte, 0, false}, {"test_force_rc", &DpO::test_force_rc, 0, false}, {"pair_digest", &DpO::pair_digest, 0, false}, {"test_force_pair_rc", &DpO::test_force_pair_rc, 0, false},
    {"pair_wide_rc", &DpO::pair_wide_rc, 0, false},
    {"score_slab_bytes", &DpO::score_slab_bytes, 0, true}, {"partner_slab_bytes", &DpO::partner_slab_bytes, 0, true},
    {"partner_wide", &DpO::partner_wide, 0, false},                // 0..2: clamped from above below
    {"joint_state_bytes", &DpO::joint_state_bytes, 0, true},
    {"genotype_table_bytes", &DpO::genotype_table_bytes, 0, true}, {"genotype_table_lanes", &DpO::genotype_table_lanes, 0, false},
    {"genotype_table_tile_keys", &DpO::genotype_table_tile_keys, 256, true}, {"genotype_table_scan_tiles", &DpO::genotype_table_scan_tiles, 64, true},   // rounded down to a multiple of 256 / 64, clamped from above below
    {"objective_lds_bytes", &DpO::objective_lds_bytes, 0, true},   // clamped from above to objective_lds_limit(): the device's LDS per workgroup
    // read by dg_dp_load_graph: in effect at the next load
    {"rowx", &DpO::use_rowx, 0, false}, {"lean_chain", &DpO::use_lean_chain, 0, false}, {"segment_cells", &DpO::segment_cells, 0, false},
    {"host_threads", &DpO::host_threads, 1, false}, {"host_tables", &DpO::host_tables, 0, false}, {"delta_cap_entries", &DpO::delta_cap_entries, 0, true},
    {"pair_levels", &DpO::pair_levels, 0, false}, {"pair_min", &DpO::pair_min, 1, false}, {"pair_fanin", &DpO::pair_fanin, 0, false}, {"pair_fanin_min", &DpO::pair_fanin_min, 1, false},
    {"pair_fanin_max_big", &DpO::pair_fanin_max_big, 0, false}, {"pair_fanin_max_indeg", &DpO::pair_fanin_max_indeg, 0, false},
    {"pair_wide", &DpO::pair_wide, 0, false}, {"pair_wide_min", &DpO::pair_wide_min, 1, false}, {"pair_wide_fanin", &DpO::pair_wide_fanin, 0, false},
    {"pair_wide_max_width", &DpO::pair_wide_max_width, 0, true},
    {"lattice_chunk_cells", &DpO::chunk_units_cfg, 1, false},   // 16-bit back-pointer units; below 1 is an error, else rounded up to even; empties the chunk pool at once
};
static int dp_option(dg_ctx *c, const char *what, const char *key, const int64_t *set, int64_t *get) {   // set or get, the other is null
    if (!c || !key || (!set && !get)) { dgi::set_error("%s: null", what); return DG_ERR_ARG; }
    if (!c->dp) c->dp = new dgi::DpState(c->device);
    dgi::DpState &S = *c->dp;
    if (set) dgi::graphs_clear(S);
    for (const DpOptionKey &o : dp_option_keys) {
        if (strcmp(key, o.key)) continue;
        if (!set) { *get = S.opt.*o.field; return DG_OK; }
        int64_t v = *set;
        if (o.field == &DpO::chunk_units_cfg) {
            if (v < o.lo) { dgi::set_error("lattice_chunk_cells must be positive"); return DG_ERR_ARG; }
            dgi::pool_clear(S);
            v = (int64_t)(S.pool.chunk_units = ((size_t)v + 1) & ~(size_t)1);
        }
        if (o.field == &DpO::objective_lds_bytes) v = std::min(v, dgi::objective_lds_limit(c));
        if (o.field == &DpO::partner_wide) v = std::min<int64_t>(v, 2);
        if (o.field == &DpO::genotype_table_tile_keys && v > 0) v = std::min<int64_t>(std::max<int64_t>(v / 256, 1) * 256, 2048);
        if (o.field == &DpO::genotype_table_scan_tiles && v > 0) v = std::min<int64_t>(std::max<int64_t>(v / 64, 1) * 64, 1024);
        S.opt.*o.field = o.nonpos_is_default && v <= 0 ? DpO().*o.field : v < o.lo ? o.lo : v;
        return DG_OK;
    }
    dgi::set_error("unknown option %s", key);
    return DG_ERR_ARG;
}
extern "C" int dg_dp_set_option(dg_ctx *c, const char *key, int64_t v) { return dp_option(c, "dg_dp_set_option", key, &v, nullptr); }
extern "C" int dg_dp_get_option(dg_ctx *c, const char *key, int64_t *value) { return dp_option(c, "dg_dp_get_option", key, nullptr, value); }

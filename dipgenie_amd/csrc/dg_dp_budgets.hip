// Every recombination budget from one DP pass (dg_dp_run_budgets; dg_dp_run is the list {R}), host side of the read-out.
// The source level starts at 0 on all R + 1 planes, a cell of plane r gathers from planes r, r - 1, r - 2 only, and the levelized
// graph does not depend on R: after ONE sweep with limit R, plane r of the sink is the cell a run with limit r reads out -- same
// value, same winning predecessors all the way back.  What a budget costs is therefore its chain walk and its finish, not a sweep.
// Here: the sink's value per plane (kept when the sweep reaches the sink -- a segmented second pass overwrites the state ring), the
// buffers of n chains, the placement of their walkers (the walkers and their helpers: dg_dp_trace.hip), and the finish kernel per chain.
// dg_dp_get_answer_paths: after the run, a chain's path slice -- one hop word per haplotype and level, source position | weight << 31
// -- expanded into the pair of paths it stands for, one vertex id per level, by one lane per level.  The run's buffers are only read.
#include <algorithm>
#include <cstring>
#include <numeric>

#include "dg_dp.hpp"

namespace dgi {

// the sink level in layout [i][r][j] (j fastest): cell (0, r, 0)
__global__ __launch_bounds__(256) void dp_sink_values_kernel(const int32_t *__restrict__ sink_state, int k2, int RP, int32_t *__restrict__ out) {
    const int r = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (r < RP) out[r] = sink_state[(int64_t)r * k2];
}

void budgets_launch_sink_copy(const DpState &S, const int32_t *sink_state, hipStream_t s) {
    hipLaunchKernelGGL(dp_sink_values_kernel, dim3((unsigned)((S.RP + 255) / 256)), dim3(256), 0, s, sink_state, S.descs[S.L - 1].k2, S.RP, S.d_sink.as<int32_t>());
}

int budgets_reserve(DpState &S, int n) {                                // (dg_dp_load_graph reserves one chain's: what dg_dp_run needs)
    if (int rc = S.d_ch_path.ensure(8 * (size_t)S.L * (size_t)n)) return rc;
    if (int rc = S.d_ch_state.ensure(sizeof(ChainState) * (size_t)n)) return rc;
    if (int rc = S.d_ch_sync.ensure((size_t)BUDGET_SYNC_STRIDE * (size_t)n)) return rc;
    if (int rc = S.d_ch_trace.ensure(sizeof(TraceOut) * (size_t)n)) return rc;
    if (int rc = S.d_ch_edges.ensure(4 * 4 * (size_t)S.cap * (size_t)n)) return rc;
    return S.d_ch_tab.ensure(sizeof(BudgetSlot) * (size_t)n);
}

int budgets_prepare(DpState &S, const int32_t *budgets, int n, hipStream_t s) {
    if (int rc = budgets_reserve(S, n)) return rc;
    // Placement (dg_dp_trace.hip): chains by falling budget, dealt into G contiguous groups; group g owns the blocks g, g + G, ...
    // (one XCD under the observed round-robin dispatch), its largest budget -- the leader -- sits in block g.
    std::vector<int> order(n);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return budgets[a] > budgets[b]; });
    const int G = std::min(8, n);
    std::vector<int> start(G + 1, 0);
    for (int g = 0; g < G; ++g) start[g + 1] = start[g] + n / G + (g < n % G ? 1 : 0);
    std::vector<BudgetSlot> &tab = S.tab_host;                          // outlives the call: the copy below is asynchronous
    tab.resize(n);
    for (int b = 0; b < n; ++b) {
        const int g = b % G, chain = order[start[g] + b / G];
        tab[b] = BudgetSlot{chain, budgets[chain], start[g + 1] - start[g] + 1, 0};
    }
    S.n_groups = G;
    S.walk_seq = 0;
    // on the run's stream, like everything else of a run: a blocking copy goes through the legacy stream, which must not meet the
    // stream of another context (another host thread) while that one captures its level batches
    DG_HIP(hipMemcpyAsync(S.d_ch_tab.p, tab.data(), sizeof(BudgetSlot) * (size_t)n, hipMemcpyHostToDevice, s));
    DG_HIP(hipMemsetAsync(S.d_ch_sync.p, 0, (size_t)BUDGET_SYNC_STRIDE * (size_t)n, s));
    DG_HIP(hipMemsetAsync(S.d_ch_state.p, 0, sizeof(ChainState) * (size_t)n, s));
    return DG_OK;
}

void budgets_launch_finish(const DpState &S, int n, hipStream_t s) {
    (void)hipMemsetAsync(S.d_ch_trace.p, 0, sizeof(TraceOut) * (size_t)n, s);
    for (int q = 0; q < n; ++q)
        trace_launch_finish_chain(S, S.d_ch_path.as<uint2>() + (size_t)q * (size_t)S.L, S.d_ch_edges.as<int32_t>() + 4 * (size_t)S.cap * (size_t)q,
                                  S.d_ch_state.as<ChainState>() + q, S.d_ch_trace.as<TraceOut>() + q, s);
}

// path = the chain's slice: path[l], l = 1 .. L - 1, holds the positions in level l - 1 that the pair came through and the weights of
// its two hops into level l (the finish kernel has checked every position against its level's width); out = [2][L], cnt = [2]
__global__ __launch_bounds__(256) void dp_answer_paths_kernel(const LevelDesc *__restrict__ descs, int L, int nV, const uint2 *__restrict__ path,
                                                              const ChainState *__restrict__ st, int swap, int32_t *__restrict__ out, int32_t *__restrict__ cnt) {
    const int l = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const bool none = st->value == NEG_INF;                             // no pair of paths fits the budget: nothing was walked
    int w0 = 0, w1 = 0;
    if (l < L) {
        int v0 = -1, v1 = -1;
        if (!none) {
            if (l == L - 1) v0 = v1 = nV - 1;                           // the sink
            else {
                const uint2 w = path[l + 1];
                const int a0 = descs[l + 1].a0;
                v0 = a0 + (int)(w.x & 0x7FFFu); v1 = a0 + (int)(w.y & 0x7FFFu);
                w0 = (int)(w.x >> 31); w1 = (int)(w.y >> 31);
            }
        }
        out[(int64_t)swap * L + l] = v0;
        out[(int64_t)(1 - swap) * L + l] = v1;
    }
    for (int sft = 32; sft > 0; sft >>= 1) { w0 += __shfl_down(w0, sft); w1 += __shfl_down(w1, sft); }
    if ((threadIdx.x & 63) == 0) {
        if (w0) atomicAdd(&cnt[0], w0);
        if (w1) atomicAdd(&cnt[1], w1);
    }
}

int budgets_find_chain(const char *fn, const DpState *S, int32_t budget, int &chain) {
    if (!S || !S->loaded) { set_error("%s: no graph loaded", fn); return DG_ERR_STATE; }
    if (!S->run_ok || S->sink_host.empty()) { set_error("%s: no completed dg_dp_run / dg_dp_run_budgets on the loaded graph", fn); return DG_ERR_STATE; }
    for (const BudgetSlot &b : S->tab_host)
        if (b.budget == budget) { chain = b.chain; return DG_OK; }
    set_error("%s: budget %d is not among the budgets the last run read out", fn, budget);
    return DG_ERR_STATE;
}

void budgets_launch_expand(const DpState &S, int chain, int swap, int32_t *out, int32_t *cnt, hipStream_t s) {
    (void)hipMemsetAsync(cnt, 0, 8, s);
    hipLaunchKernelGGL(dp_answer_paths_kernel, dim3((unsigned)((S.L + 255) / 256)), dim3(256), 0, s, S.d_descs.as<LevelDesc>(), S.L, S.nV,
                       S.d_ch_path.as<uint2>() + (size_t)chain * (size_t)S.L, S.d_ch_state.as<ChainState>() + chain, swap, out, cnt);
}

int dp_get_answer_paths(dg_ctx *c, int32_t budget, int32_t *paths) {
    static const char *const FN = "dg_dp_get_answer_paths";
    int chain = 0;
    if (int rc = budgets_find_chain(FN, c->dp, budget, chain)) return rc;
    if (!paths) { set_error("%s: paths is required", FN); return DG_ERR_ARG; }
    DpState &S = *c->dp;
    hipStream_t s = c->stream;
    if (int rc = S.d_ans_paths.ensure(8 * (size_t)S.L)) return rc;
    if (int rc = S.d_ans_cnt.ensure(8)) return rc;
    std::vector<int32_t> rows(2 * (size_t)S.L);                         // the caller's array is written only on success
    budgets_launch_expand(S, chain, 0, S.d_ans_paths.as<int32_t>(), S.d_ans_cnt.as<int32_t>(), s);
    DG_HIP(hipGetLastError());
    DG_HIP(hipMemcpyAsync(rows.data(), S.d_ans_paths.p, 4 * rows.size(), hipMemcpyDeviceToHost, s));
    DG_HIP(hipStreamSynchronize(s));
    memcpy(paths, rows.data(), 4 * rows.size());
    return DG_OK;
}

}  // namespace dgi

extern "C" int dg_dp_get_answer_paths(dg_ctx *c, int32_t budget, int32_t *paths) {
    if (int rc = dgi::bind(c)) return rc;
    return dgi::dp_get_answer_paths(c, budget, paths);
}

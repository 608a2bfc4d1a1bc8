// Every recombination budget from one DP pass (dg_dp_run_budgets; dg_dp_run is the list {R}), host side of the read-out.
// The source level starts at 0 on all R + 1 planes, a cell of plane r gathers from planes r, r - 1, r - 2 only, and the levelized
// graph does not depend on R: after ONE sweep with limit R, plane r of the sink is the cell a run with limit r reads out -- same
// value, same winning predecessors all the way back.  What a budget costs is therefore its chain walk and its finish, not a sweep.
// Here: the sink's value per plane (kept when the sweep reaches the sink -- a segmented second pass overwrites the state ring), the
// buffers of n chains, the placement of their walkers (the walkers and their helpers: dg_dp_trace.hip), and the finish kernel per chain.
#include <algorithm>
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

}  // namespace dgi

// dg_dp_best_partners: the best second path for a first path that is already known -- the DP with one haplotype fixed.
// With `given` fixed, the transition into level l over the in-edge e = (u -> v, w) is worth d_l(u, v) = inter + symd of the sources
// (given[l-1], u) against the destinations (given[l], v) -- what dg_dp_score_paths adds for the ordered pair (given, partner) -- and
//   S_0[source][r] = 0,   S_l[v][r] = max over in-edges of v with r - w >= 0 and a reachable source cell of S_{l-1}[u][r - w] + d_l(u, v),
// ties to the smallest source position (the in-edge slice is sorted that way), NEG_INF where nothing arrives.  The state of a level
// is k x (budget + 1) cells, so a query is one workgroup and thousands of them run side by side.  Three kernels per slab of queries:
//   * dp_partner_scores_kernel: one workgroup per (query, 64 destination levels).  One lane per level checks given[l-1], given[l]
//     against the level descriptor and looks the hop up (first bad (query, level) by atomicMin, as dg_dp_score.hip does); then one
//     lane per in-edge of those levels runs the two 4-way merges and stores d as 16 bits (load rejects graphs whose longest
//     hom and het lists allow more: 2 max_hom + 4 max_het > 65535, colour_lists_fit_delta).  All merges are done here, off the serial path.
//   * dp_partner_sweep_kernel: one persistent workgroup per query, no synchronisation between workgroups.  Two copies of the state
//     in LDS ([vertex][r], r fastest: the lanes of a vertex read consecutive words of a source row and share the in-edge records);
//     the in-edge words, their scores and the in-edge offsets of level l + 1 are loaded into registers before the cells of level l
//     are computed and go to an LDS stage (two buffers) after them, one barrier per level.  A level with more than 1,024 in-edges
//     or vertices is read from global memory instead.  One 16-bit back-pointer per cell: source position | weight << 15, 0xFFFF
//     for an unreachable cell (positions stay below 2^14: a level is at most 16,384 cells wide).
//   * dp_partner_walk_kernel: one lane per query walks the winners back from (sink, budget) and writes the partner next to the
//     given path, as the pair that dp_score_paths_kernel then re-scores: s_het, r1, r2 come from that pass, its value must be the
//     DP's cell and r2 must fit the budget, or the call fails with DG_ERR_STATE.
// Nothing of a run is read or written.  Per query a slab holds 2 * n_vertices * (bmax + 1) bytes of back-pointers (bmax: the largest
// budget of the call), 2 bytes per in-edge of scores and 8 * n_levels bytes of paths; partner_slab_bytes bounds their sum.
// With option partner_wide a call whose kmax x (bmax + 1) cells exceed PT_MAX_CELLS (1), or every call (2), takes the device-memory
// route: dp_partner_sweep_wide_kernel in place of the second kernel, one 1,024-lane workgroup per query, the two level states in a
// per-query device buffer of 2 * kmax * (bmax + 1) int32 (8 bytes per cell more in the slab's sum; released when the call returns),
// only the in-edge stage in LDS.  Same recurrence, ties, back-pointers and walk; kmax <= 32,767 and 2^24 cells per query.
// dg_dp_partner_marginals (dg_dp_marginals.hip) runs the first two kernels as well, the second one storing every cell's int32 value
// in place of the back-pointer (VALUES): what the two files share is declared in dg_dp_partner.hpp.
#include <algorithm>
#include <cstring>

#include "dg_dp_partner.hpp"
#include "dg_dp_setops.hpp"

namespace dgi {

namespace {

constexpr uint32_t PT_BP_NONE = 0xFFFFu;
constexpr size_t PT_STAGE_BYTES = 2 * PT_STAGE_BUF_BYTES;

// grid: n * nblk workgroups; query q's given path = given_all + q * given_stride ([n][2][L], row 0, for dg_dp_best_partners); scores = [n][E]
__global__ __launch_bounds__(PT_THREADS) void dp_partner_scores_kernel(const LevelDesc *__restrict__ descs, int L, int nblk,
                                                                       const uint32_t *__restrict__ in_off, const uint32_t *__restrict__ in_edge,
                                                                       const int32_t *__restrict__ in_dst, ColourCsr col, const int32_t *__restrict__ given_all,
                                                                       int64_t given_stride, uint16_t *__restrict__ scores, int64_t E, unsigned long long *__restrict__ err) {
    __shared__ uint32_t s_base[PT_SCORE_LEVELS + 1];
    __shared__ int32_t s_a0[PT_SCORE_LEVELS], s_gu[PT_SCORE_LEVELS], s_gv[PT_SCORE_LEVELS], s_ok[PT_SCORE_LEVELS];
    const int64_t q = (int64_t)(blockIdx.x / (unsigned)nblk);
    const int l0 = 1 + (int)(blockIdx.x % (unsigned)nblk) * PT_SCORE_LEVELS;
    const int nl = min(PT_SCORE_LEVELS, L - l0);
    const int32_t *given = given_all + q * given_stride;
    const int t = (int)threadIdx.x;
    if (t < nl) {
        const int l = l0 + t;
        const LevelDesc &d = descs[l];
        const int a0 = d.a0, k = d.k, b0 = d.b0, k2 = d.k2;
        const int gu = given[l - 1], gv = given[l];
        // (unsigned compare: a negative id fails too)  A source id is reported at its own level l - 1, as the lane of that level does
        const bool gu_ok = (uint32_t)gu - (uint32_t)a0 < (uint32_t)k, gv_ok = (uint32_t)gv - (uint32_t)b0 < (uint32_t)k2;
        if (!gu_ok) atomicMin(err, partner_err_key(q, l - 1, 0));
        if (!gv_ok) atomicMin(err, partner_err_key(q, l, 0));
        if (gu_ok && gv_ok && score_edge_weight(in_off, in_edge, gv, (uint32_t)(gu - a0)) < 0) atomicMin(err, partner_err_key(q, l, 1));
        s_base[t] = d.in_base;
        if (t == nl - 1) s_base[nl] = d.in_base + (uint32_t)d.T;
        s_a0[t] = a0; s_gu[t] = gu; s_gv[t] = gv; s_ok[t] = gu_ok && gv_ok;      // ids outside their level never index a colour list
    }
    __syncthreads();
    uint16_t *sc = scores + q * E;
    for (uint32_t e = s_base[0] + (uint32_t)t; e < s_base[nl]; e += PT_THREADS) {
        int lo = 0, hi = nl - 1;                                        // the last level of the block whose first in-edge is <= e
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (s_base[mid] <= e) lo = mid; else hi = mid - 1;
        }
        int d = 0;
        if (s_ok[lo]) {
            const int u = s_a0[lo] + (int)(in_edge[e] & 0x7FFFFFFFu), v = in_dst[e];
            d = score_symd(col, s_gu[lo], u, s_gv[lo], v) + score_inter(col, s_gu[lo], u, s_gv[lo], v);
        }
        sc[e] = (uint16_t)d;
    }
}

// What a cell leaves in global memory: its 16-bit back-pointer (dg_dp_best_partners) or its int32 value (VALUES: dg_dp_partner_marginals)
template <bool VALUES> struct PtStore { typedef uint16_t type; };
template <> struct PtStore<true> { typedef int32_t type; };

// The cells of one level.  STAGED: edge / sc / off are the LDS stage (indices relative to the level's first in-edge / vertex);
// otherwise the global arrays (off = in_off + b0, absolute in-edge indices).
template <bool STAGED, bool VALUES>
__device__ __forceinline__ void pt_cells(const PtLevel &lv, int B1, int vrow, int rows, int r0, int rstep, const int32_t *prev, int32_t *cur,
                                         const uint32_t *edge, const uint16_t *sc, const uint32_t *off, typename PtStore<VALUES>::type *__restrict__ bp) {
    for (int v = vrow; v < lv.k2; v += rows) {
        const uint32_t e0 = off[v], e1 = off[v + 1];
        for (int r = r0; r < B1; r += rstep) {
            int best = NEG_INF;
            uint32_t word = PT_BP_NONE;
            for (uint32_t e = e0; e < e1; ++e) {                        // sorted by source position: a strict > keeps the smallest among equals
                const uint32_t rec = edge[e];
                const int pos = (int)(rec & 0x7FFFFFFFu), w = (int)(rec >> 31);
                if (r - w < 0) continue;
                const int s = prev[pos * B1 + r - w];
                if (s == NEG_INF) continue;
                const int cand = s + (int)sc[e];
                if (cand > best) { best = cand; word = (uint32_t)pos | ((uint32_t)w << 15); }
            }
            cur[v * B1 + r] = best;
            if constexpr (VALUES) bp[((int64_t)lv.b0 + v) * B1 + r] = best;
            else bp[((int64_t)lv.b0 + v) * B1 + r] = (uint16_t)word;
        }
    }
}

// grid: n workgroups of PT_THREADS; dynamic LDS = two states of `cells` int32 each, then the two stage buffers
template <bool VALUES>
__global__ __launch_bounds__(PT_THREADS) void dp_partner_sweep_kernel(const LevelDesc *__restrict__ descs, int L, int nV, int cells,
                                                                      const uint32_t *__restrict__ in_off, const uint32_t *__restrict__ in_edge,
                                                                      const uint16_t *__restrict__ scores, int64_t E, const int32_t *__restrict__ budgets,
                                                                      typename PtStore<VALUES>::type *__restrict__ bp_all, int64_t bp_stride, int32_t *__restrict__ value) {
    extern __shared__ int32_t pt_lds[];
    const int64_t q = blockIdx.x;
    const int t = (int)threadIdx.x;
    const int B1 = budgets[q] + 1;
    const uint16_t *__restrict__ sc_g = scores + q * E;
    typename PtStore<VALUES>::type *__restrict__ bp = bp_all + q * bp_stride;
    int32_t *const state0 = pt_lds, *const state1 = pt_lds + cells;     // level l lives in state (l & 1)
    // stage buffer b: PT_STAGE in-edge words, PT_STAGE + 4 in-edge offsets, PT_STAGE scores
    uint32_t *const st_edge0 = (uint32_t *)(pt_lds + 2 * (size_t)cells), *const st_off0 = st_edge0 + 2 * PT_STAGE;
    uint16_t *const st_sc0 = (uint16_t *)(st_off0 + 2 * (PT_STAGE + 4));
#define PT_EDGE(b) (st_edge0 + (b) * PT_STAGE)
#define PT_OFF(b) (st_off0 + (b) * (PT_STAGE + 4))
#define PT_SC(b) (st_sc0 + (b) * PT_STAGE)
    // lanes -> cells: whole rows of B1 planes per pass while a row fits the workgroup, else one row with the lanes striding over r
    int rows, vrow, r0, rstep;
    if (B1 <= PT_THREADS) { rows = PT_THREADS / B1; vrow = t / B1; r0 = t - vrow * B1; rstep = B1; if (vrow >= rows) vrow = 1 << 30; }
    else { rows = 1; vrow = 0; r0 = t; rstep = PT_THREADS; }

    for (int r = t; r < B1; r += PT_THREADS) {                        // level 0 is the source alone
        state0[r] = 0;
        if constexpr (VALUES) bp[(int64_t)descs[1].a0 * B1 + r] = 0;
    }
    PtLevel lv = pt_level(descs, 1);
    PtLevel ln = L > 2 ? pt_level(descs, 2) : lv;
    if (pt_staged(lv)) {
        for (int i = t; i < lv.T; i += PT_THREADS) { PT_EDGE(1)[i] = in_edge[lv.in_base + i]; PT_SC(1)[i] = sc_g[lv.in_base + i]; }
        for (int i = t; i <= lv.k2; i += PT_THREADS) PT_OFF(1)[i] = in_off[lv.b0 + i] - lv.in_base;
    }
    __syncthreads();
    for (int l = 1; l < L; ++l) {
        const bool more = l + 1 < L, stage_next = more && pt_staged(ln);
        const PtLevel lnn = l + 2 < L ? pt_level(descs, l + 2) : ln;
        // level l + 1's records: issued here, consumed after this level's cells
        uint32_t pf_edge[PT_PF], pf_off[PT_PF + 1], pf_sc[PT_PF];          // (scores in full registers: packed halves would chain the loads)
        if (stage_next) {
#pragma unroll
            for (int j = 0; j < PT_PF; ++j) {
                const int i = t + j * PT_THREADS;
                if (i < ln.T) { pf_edge[j] = in_edge[ln.in_base + i]; pf_sc[j] = sc_g[ln.in_base + i]; }
            }
#pragma unroll
            for (int j = 0; j <= PT_PF; ++j) {
                const int i = t + j * PT_THREADS;
                if (i <= ln.k2) pf_off[j] = in_off[ln.b0 + i];
            }
        }
        const int32_t *prev = (l & 1) ? state0 : state1;
        int32_t *cur = (l & 1) ? state1 : state0;
        if (pt_staged(lv)) pt_cells<true, VALUES>(lv, B1, vrow, rows, r0, rstep, prev, cur, PT_EDGE(l & 1), PT_SC(l & 1), PT_OFF(l & 1), bp);
        else pt_cells<false, VALUES>(lv, B1, vrow, rows, r0, rstep, prev, cur, in_edge, sc_g, in_off + lv.b0, bp);
        if (stage_next) {
            const int nb = (l + 1) & 1;
#pragma unroll
            for (int j = 0; j < PT_PF; ++j) {
                const int i = t + j * PT_THREADS;
                if (i < ln.T) { PT_EDGE(nb)[i] = pf_edge[j]; PT_SC(nb)[i] = (uint16_t)pf_sc[j]; }
            }
#pragma unroll
            for (int j = 0; j <= PT_PF; ++j) {
                const int i = t + j * PT_THREADS;
                if (i <= ln.k2) PT_OFF(nb)[i] = pf_off[j] - ln.in_base;
            }
        }
        __syncthreads();
        lv = ln; ln = lnn;
    }
    if (t == 0) value[q] = (((L - 1) & 1) ? state1 : state0)[(nV - 1 - lv.b0) * B1 + B1 - 1];      // lv: the sink's level
}

#undef PT_EDGE
#undef PT_OFF
#undef PT_SC

// ---- the device-memory route (option partner_wide): the same recurrence with the level states in device memory ----
// The cells of one level, as pt_cells.  prev / cur: the states of level l - 1 / l as [position][r] in device memory, written and read
// by this workgroup alone.  They are plain pointers on purpose -- not const, not __restrict__, no non-temporal access: the loads of
// level l must follow the barrier that ends level l - 1, and only a pointer the compiler has to assume written lets it neither hoist
// such a load over the barrier nor turn it into a scalar (constant-cache) load.  All waves of a workgroup share one CU and its L1,
// through which both the stores and the loads go, so the barrier is all the ordering they need.
template <bool STAGED, bool VALUES>
__device__ __forceinline__ void ptw_cells(const PtLevel &lv, int B1, int vrow, int rows, int r0, int rstep, int32_t *prev, int32_t *cur,
                                          const uint32_t *edge, const uint16_t *sc, const uint32_t *off, uint16_t *bp) {
    for (int v = vrow; v < lv.k2; v += rows) {
        const uint32_t e0 = off[v], e1 = off[v + 1];
        for (int r = r0; r < B1; r += rstep) {
            int best = NEG_INF;
            uint32_t word = PT_BP_NONE;
            for (uint32_t e = e0; e < e1; ++e) {                        // sorted by source position: a strict > keeps the smallest among equals
                const uint32_t rec = edge[e];
                const int pos = (int)(rec & 0x7FFFFFFFu), w = (int)(rec >> 31);
                if (r - w < 0) continue;
                const int s = prev[pos * B1 + r - w];
                if (s == NEG_INF) continue;
                const int cand = s + (int)sc[e];
                if (cand > best) { best = cand; word = (uint32_t)pos | ((uint32_t)w << 15); }
            }
            cur[v * B1 + r] = best;
            if constexpr (!VALUES) bp[((int64_t)lv.b0 + v) * B1 + r] = (uint16_t)word;
        }
    }
}

// grid: n workgroups of PTW_THREADS; static LDS: the two stage buffers.  !VALUES: state_all = [n][2][cells] int32, level l in copy
// (l & 1), store_all = the back-pointers.  VALUES: store_all = the values [vertex][r], which are the state as well (level l - 1 is
// read back from where it was stored); state_all is not used
template <bool VALUES>
__global__ __launch_bounds__(PTW_THREADS) void dp_partner_sweep_wide_kernel(const LevelDesc *__restrict__ descs, int L, int nV, int cells,
                                                                            const uint32_t *__restrict__ in_off, const uint32_t *__restrict__ in_edge,
                                                                            const uint16_t *__restrict__ scores, int64_t E, const int32_t *__restrict__ budgets,
                                                                            int32_t *state_all, typename PtStore<VALUES>::type *store_all, int64_t stride,
                                                                            int32_t *__restrict__ value) {
    __shared__ uint32_t st_edge[2][PT_STAGE], st_off[2][PT_STAGE + 4];
    __shared__ uint16_t st_sc[2][PT_STAGE];
    const int64_t q = blockIdx.x;
    const int t = (int)threadIdx.x;
    const int B1 = budgets[q] + 1;
    const uint16_t *__restrict__ sc_g = scores + q * E;
    typename PtStore<VALUES>::type *store = store_all + q * stride;
    int32_t *state0 = nullptr, *state1 = nullptr;
    uint16_t *bp = nullptr;
    if constexpr (!VALUES) { state0 = state_all + q * 2 * (int64_t)cells; state1 = state0 + cells; bp = store; }
    // lanes -> cells as in dp_partner_sweep_kernel: whole rows of B1 planes per pass while a row fits the workgroup, else one row with the lanes striding over r
    int rows, vrow, r0, rstep;
    if (B1 <= PTW_THREADS) { rows = PTW_THREADS / B1; vrow = t / B1; r0 = t - vrow * B1; rstep = B1; if (vrow >= rows) vrow = 1 << 30; }
    else { rows = 1; vrow = 0; r0 = t; rstep = PTW_THREADS; }

    int prev_b0 = descs[1].a0;                                          // first vertex of level l - 1
    {                                                                   // level 0 is the source alone
        int32_t *lev0;
        if constexpr (VALUES) lev0 = store + (int64_t)prev_b0 * B1; else lev0 = state0;
        for (int r = t; r < B1; r += PTW_THREADS) lev0[r] = 0;
    }
    PtLevel lv = pt_level(descs, 1);
    PtLevel ln = L > 2 ? pt_level(descs, 2) : lv;
    if (pt_staged(lv)) {
        for (int i = t; i < lv.T; i += PTW_THREADS) { st_edge[1][i] = in_edge[lv.in_base + i]; st_sc[1][i] = sc_g[lv.in_base + i]; }
        for (int i = t; i <= lv.k2; i += PTW_THREADS) st_off[1][i] = in_off[lv.b0 + i] - lv.in_base;
    }
    __syncthreads();
    for (int l = 1; l < L; ++l) {
        const bool more = l + 1 < L, stage_next = more && pt_staged(ln);
        const PtLevel lnn = l + 2 < L ? pt_level(descs, l + 2) : ln;
        // level l + 1's records: issued here, consumed after this level's cells
        uint32_t pf_edge[PTW_PF], pf_off[PTW_PF + 1], pf_sc[PTW_PF];
        if (stage_next) {
#pragma unroll
            for (int j = 0; j < PTW_PF; ++j) {
                const int i = t + j * PTW_THREADS;
                if (i < ln.T) { pf_edge[j] = in_edge[ln.in_base + i]; pf_sc[j] = sc_g[ln.in_base + i]; }
            }
#pragma unroll
            for (int j = 0; j <= PTW_PF; ++j) {
                const int i = t + j * PTW_THREADS;
                if (i <= ln.k2) pf_off[j] = in_off[ln.b0 + i];
            }
        }
        int32_t *prev, *cur;
        if constexpr (VALUES) { prev = store + (int64_t)prev_b0 * B1; cur = store + (int64_t)lv.b0 * B1; }
        else { prev = (l & 1) ? state0 : state1; cur = (l & 1) ? state1 : state0; }
        const int b = l & 1;
        if (pt_staged(lv)) ptw_cells<true, VALUES>(lv, B1, vrow, rows, r0, rstep, prev, cur, st_edge[b], st_sc[b], st_off[b], bp);
        else ptw_cells<false, VALUES>(lv, B1, vrow, rows, r0, rstep, prev, cur, in_edge, sc_g, in_off + lv.b0, bp);
        if (stage_next) {
            const int nb = (l + 1) & 1;
#pragma unroll
            for (int j = 0; j < PTW_PF; ++j) {
                const int i = t + j * PTW_THREADS;
                if (i < ln.T) { st_edge[nb][i] = pf_edge[j]; st_sc[nb][i] = (uint16_t)pf_sc[j]; }
            }
#pragma unroll
            for (int j = 0; j <= PTW_PF; ++j) {
                const int i = t + j * PTW_THREADS;
                if (i <= ln.k2) st_off[nb][i] = pf_off[j] - ln.in_base;
            }
        }
        __syncthreads();                                                // level l's stores before level l + 1's loads
        prev_b0 = lv.b0;
        lv = ln; ln = lnn;
    }
    if (t == 0) {                                                       // lv: the sink's level
        if constexpr (VALUES) value[q] = store[(int64_t)(nV - 1) * B1 + B1 - 1];
        else value[q] = (((L - 1) & 1) ? state1 : state0)[(nV - 1 - lv.b0) * B1 + B1 - 1];
    }
}

// one lane per query; pairs = [n][2][L]: row 1 receives the partner (the given path itself where the budget reaches nothing: the
// re-scoring pass then still counts r1, and the host hands out a row of -1)
__global__ __launch_bounds__(64) void dp_partner_walk_kernel(const LevelDesc *__restrict__ descs, int L, int nV, int64_t n, const int32_t *__restrict__ budgets,
                                                             const uint16_t *__restrict__ bp_all, int64_t bp_stride, const int32_t *__restrict__ value,
                                                             int32_t *__restrict__ pairs) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    int32_t *given = pairs + q * 2 * (int64_t)L, *partner = given + L;
    if (value[q] == NEG_INF) {
        for (int l = 0; l < L; ++l) partner[l] = given[l];
        return;
    }
    const int B1 = budgets[q] + 1;
    const uint16_t *__restrict__ bp = bp_all + q * bp_stride;
    int id = nV - 1, r = B1 - 1;
    partner[L - 1] = id;
    for (int l = L - 1; l >= 1; --l) {
        const uint32_t word = bp[(int64_t)id * B1 + r];
        const int pos = (int)(word & 0x7FFFu);
        r -= (int)(word >> 15);
        if (word == PT_BP_NONE || pos >= descs[l].k || r < 0) {         // cannot happen on an intact lattice: the re-scoring pass rejects the -1
            for (int m = l - 1; m >= 0; --m) partner[m] = -1;
            return;
        }
        id = descs[l].a0 + pos;
        partner[l - 1] = id;
    }
}

}  // namespace

int partner_check_wide(const char *fn, const char *who, long long which, int kmax, int64_t budget) {
    if (kmax > PTW_MAX_K) {
        set_error("%s: %s %lld: widest level %d exceeds the %d vertices of the device-memory route (budget + 1 = %lld)", fn, who, which, kmax, PTW_MAX_K, (long long)budget + 1);
        return DG_ERR_UNSUPPORTED;
    }
    if ((int64_t)kmax * (budget + 1) > PTW_MAX_CELLS) {
        set_error("%s: %s %lld: widest level %d x (budget + 1) %lld exceeds the %d cells of the device-memory route", fn, who, which, kmax, (long long)budget + 1, PTW_MAX_CELLS);
        return DG_ERR_UNSUPPORTED;
    }
    return DG_OK;
}

int partner_check_budgets(const char *fn, const DpState &S, int64_t n, const int32_t *budgets, int &kmax, int &bmax, bool &wide) {
    kmax = 1;
    for (int l = 1; l < S.L; ++l) kmax = std::max(kmax, S.descs[l].k2);
    bmax = 0;
    for (int64_t q = 0; q < n; ++q) {
        if (budgets[q] < 0) { set_error("%s: query %lld: budget %d is negative", fn, (long long)q, budgets[q]); return DG_ERR_ARG; }
        if (S.opt.partner_wide >= 1) {
            if (int rc = partner_check_wide(fn, "query", (long long)q, kmax, budgets[q])) return rc;
        } else if ((int64_t)kmax * ((int64_t)budgets[q] + 1) > PT_MAX_CELLS) {
            set_error("%s: query %lld: widest level %d x (budget + 1) %lld exceeds %d cells", fn, (long long)q, kmax, (long long)budgets[q] + 1, PT_MAX_CELLS);
            return DG_ERR_UNSUPPORTED;
        }
        bmax = std::max(bmax, budgets[q]);
    }
    wide = partner_route_wide(S, kmax, bmax);                           // per call, not per query: one launch serves a slab
    return DG_OK;
}

static int partner_score_blocks(const DpState &S) { return (S.L - 1 + PT_SCORE_LEVELS - 1) / PT_SCORE_LEVELS; }

int64_t partner_slab_limit(const DpState &S) { return std::max<int64_t>(1, ((int64_t)1 << 30) / std::max(partner_score_blocks(S), score_pair_blocks(S))); }

int partner_bad_hop(const char *fn, unsigned long long key, int64_t first, const int32_t *given, int L) {
    const int64_t q = first + (int64_t)(key >> 33);
    const int level = (int)((uint32_t)key >> 1), kind = (int)(key & 1u);
    const int32_t *pp = given + q * L;
    if (kind == 0) set_error("%s: query %lld level %d: vertex %d is not in that level", fn, (long long)q, level, pp[level]);
    else set_error("%s: query %lld level %d: no edge %d -> %d", fn, (long long)q, level, pp[level - 1], pp[level]);
    return DG_ERR_ARG;
}

void partner_launch_scores(const DpState &S, const int32_t *given, int64_t given_stride, int64_t m, uint16_t *scores, unsigned long long *err, hipStream_t s) {
    const int nblk = partner_score_blocks(S);
    hipLaunchKernelGGL(dp_partner_scores_kernel, dim3((unsigned)(m * nblk)), dim3(PT_THREADS), 0, s, S.d_descs.as<LevelDesc>(), S.L, nblk,
                       S.d_in_off.as<uint32_t>(), S.d_in_edge.as<uint32_t>(), S.d_in_dst.as<int32_t>(), colour_csr(S), given, given_stride, scores, S.n_edges, err);
}

// the recurrence on m queries; store = back-pointers (16 bits per cell) or values (32 bits), stride in those units.  wide: the
// device-memory route, state = [m][2][cells] int32 for the back-pointer form (the values form needs none)
template <bool VALUES>
static int partner_launch_sweep(const DpState &S, bool wide, int cells, int64_t m, const uint16_t *scores, const int32_t *budgets, int32_t *state,
                                typename PtStore<VALUES>::type *store, int64_t stride, int32_t *value, hipStream_t s) {
    if (wide) {
        hipLaunchKernelGGL(dp_partner_sweep_wide_kernel<VALUES>, dim3((unsigned)m), dim3(PTW_THREADS), 0, s, S.d_descs.as<LevelDesc>(), S.L, S.nV, cells,
                           S.d_in_off.as<uint32_t>(), S.d_in_edge.as<uint32_t>(), scores, S.n_edges, budgets, state, store, stride, value);
        DG_HIP(hipGetLastError());
        return DG_OK;
    }
    const size_t lds_bytes = 2 * (size_t)cells * 4 + PT_STAGE_BYTES;
    if (lds_bytes > 65536) DG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(dp_partner_sweep_kernel<VALUES>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    hipLaunchKernelGGL(dp_partner_sweep_kernel<VALUES>, dim3((unsigned)m), dim3(PT_THREADS), lds_bytes, s, S.d_descs.as<LevelDesc>(), S.L, S.nV, cells,
                       S.d_in_off.as<uint32_t>(), S.d_in_edge.as<uint32_t>(), scores, S.n_edges, budgets, store, stride, value);
    DG_HIP(hipGetLastError());
    return DG_OK;
}

int partner_launch_forward_values(const DpState &S, bool wide, int cells, int64_t m, const uint16_t *scores, const int32_t *budgets, int32_t *values, int64_t stride,
                                  int32_t *value, hipStream_t s) {
    return partner_launch_sweep<true>(S, wide, cells, m, scores, budgets, nullptr, values, stride, value, s);
}

int dp_best_partners(dg_ctx *c, const int32_t *given, int64_t n, const int32_t *budgets, int32_t *partners, dg_dp_partner *out) {
    DpState *Sp = c->dp;
    if (!Sp || !Sp->loaded) { set_error("dg_dp_best_partners: no graph loaded"); return DG_ERR_STATE; }
    if (n < 0) { set_error("dg_dp_best_partners: n = %lld", (long long)n); return DG_ERR_ARG; }
    if (n == 0) return DG_OK;
    if (!given || !budgets || !out) { set_error("dg_dp_best_partners: given, budgets and out are required"); return DG_ERR_ARG; }
    DpState &S = *Sp;
    hipStream_t s = c->stream;
    const int L = S.L, nV = S.nV;
    const int64_t E = S.n_edges;
    int kmax, bmax;
    bool wide;
    if (int rc = partner_check_budgets("dg_dp_best_partners", S, n, budgets, kmax, bmax, wide)) return rc;
    const int cells = kmax * (bmax + 1);
    partner_note_route(S, wide, cells);
    // queries per slab: what partner_slab_bytes holds (at least one), every query sized for the call's largest budget
    const int64_t bp_stride = (int64_t)nV * (bmax + 1);                 // 16-bit units
    const int64_t pair_words = 2 * (int64_t)L;
    const int64_t state_words = wide ? 2 * (int64_t)cells : 0;         // the device-memory route: two level states per query
    const int64_t query_bytes = 2 * bp_stride + 2 * E + 4 * pair_words + 4 * state_words;
    int64_t per_slab = std::max<int64_t>(1, S.opt.partner_slab_bytes / query_bytes);
    per_slab = std::min(per_slab, partner_slab_limit(S));
    per_slab = std::min(per_slab, n);
    if (int rc = S.d_pt_pairs.ensure((size_t)(per_slab * pair_words) * 4)) return rc;
    if (int rc = S.d_pt_bud.ensure((size_t)per_slab * 4)) return rc;
    if (int rc = S.d_pt_val.ensure((size_t)per_slab * 4)) return rc;
    if (int rc = S.d_pt_out.ensure((size_t)per_slab * sizeof(dg_dp_pair_score))) return rc;
    if (int rc = S.d_pt_err.ensure(2 * sizeof(unsigned long long))) return rc;
    // the large buffers live for the call only: the lattice pool of a later run may need the memory
    struct Release { DpState &S; ~Release() { S.d_pt_bp.release(); S.d_pt_scores.release(); S.d_pt_state.release(); } } release{S};
    if (int rc = S.d_pt_bp.ensure((size_t)(per_slab * bp_stride) * 2)) return rc;
    if (int rc = S.d_pt_scores.ensure((size_t)(per_slab * E) * 2 + 16)) return rc;
    if (wide)
        if (int rc = S.d_pt_state.ensure((size_t)(per_slab * state_words) * 4)) return rc;
    // the caller's arrays are written only if every query is answered
    std::vector<dg_dp_partner> res((size_t)n);
    std::vector<int32_t> val((size_t)per_slab), rows;
    std::vector<dg_dp_pair_score> sc((size_t)per_slab);
    if (partners) rows.resize((size_t)(n * L));
    int32_t *pairs = S.d_pt_pairs.as<int32_t>();
    unsigned long long *d_err = S.d_pt_err.as<unsigned long long>();
    for (int64_t first = 0; first < n; first += per_slab) {
        const int64_t m = std::min(per_slab, n - first);
        unsigned long long err[2] = {PT_NO_ERROR, PT_NO_ERROR};       // [0]: the given paths, [1]: the re-scored pairs
        DG_HIP(hipMemcpy2DAsync(pairs, (size_t)pair_words * 4, given + first * L, (size_t)L * 4, (size_t)L * 4, (size_t)m, hipMemcpyHostToDevice, s));
        DG_HIP(hipMemcpyAsync(S.d_pt_bud.p, budgets + first, (size_t)m * 4, hipMemcpyHostToDevice, s));
        DG_HIP(hipMemsetAsync(S.d_pt_out.p, 0, (size_t)m * sizeof(dg_dp_pair_score), s));
        DG_HIP(hipMemsetAsync(d_err, 0xFF, sizeof err, s));
        partner_launch_scores(S, pairs, pair_words, m, S.d_pt_scores.as<uint16_t>(), d_err, s);
        DG_HIP(hipGetLastError());
        if (int rc = partner_launch_sweep<false>(S, wide, cells, m, S.d_pt_scores.as<uint16_t>(), S.d_pt_bud.as<int32_t>(), S.d_pt_state.as<int32_t>(), S.d_pt_bp.as<uint16_t>(), bp_stride, S.d_pt_val.as<int32_t>(), s)) return rc;
        hipLaunchKernelGGL(dp_partner_walk_kernel, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, s, S.d_descs.as<LevelDesc>(), L, nV, m, S.d_pt_bud.as<int32_t>(),
                           S.d_pt_bp.as<uint16_t>(), bp_stride, S.d_pt_val.as<int32_t>(), pairs);
        DG_HIP(hipGetLastError());
        score_launch_pairs(S, pairs, m, S.d_pt_out.as<int32_t>(), d_err + 1, s);
        DG_HIP(hipGetLastError());
        DG_HIP(hipMemcpyAsync(val.data(), S.d_pt_val.p, (size_t)m * 4, hipMemcpyDeviceToHost, s));
        DG_HIP(hipMemcpyAsync(sc.data(), S.d_pt_out.p, (size_t)m * sizeof(dg_dp_pair_score), hipMemcpyDeviceToHost, s));
        DG_HIP(hipMemcpyAsync(err, d_err, sizeof err, hipMemcpyDeviceToHost, s));
        if (partners)
            DG_HIP(hipMemcpy2DAsync(rows.data() + first * L, (size_t)L * 4, pairs + L, (size_t)pair_words * 4, (size_t)L * 4, (size_t)m, hipMemcpyDeviceToHost, s));
        DG_HIP(hipStreamSynchronize(s));
        if (err[0] != PT_NO_ERROR) return partner_bad_hop("dg_dp_best_partners", err[0], first, given, L);   // slabs go up in order: the first slab with a bad hop holds the first bad hop
        if (err[1] != PT_NO_ERROR) {
            set_error("dg_dp_best_partners: query %lld: the walked partner is not a path (level %d)", (long long)(first + (int64_t)(err[1] >> 33)), (int)((uint32_t)err[1] >> 1));
            return DG_ERR_STATE;
        }
        for (int64_t i = 0; i < m; ++i) {
            const int64_t q = first + i;
            if (val[i] == NEG_INF) {
                res[q] = dg_dp_partner{NEG_INF, 0, sc[i].r1, 0};
                if (partners) std::fill(rows.begin() + q * L, rows.begin() + (q + 1) * L, -1);
                continue;
            }
            if (sc[i].value != val[i] || sc[i].r2 > budgets[q]) {
                set_error("dg_dp_best_partners: query %lld: the walked partner scores %d with %d recombinations, the DP's cell holds %d at budget %d",
                          (long long)q, sc[i].value, sc[i].r2, val[i], budgets[q]);
                return DG_ERR_STATE;
            }
            res[q] = dg_dp_partner{sc[i].value, sc[i].s_het, sc[i].r1, sc[i].r2};
        }
    }
    memcpy(out, res.data(), (size_t)n * sizeof(dg_dp_partner));
    if (partners) memcpy(partners, rows.data(), rows.size() * 4);
    return DG_OK;
}

}  // namespace dgi

extern "C" int dg_dp_get_partner_route(dg_ctx *c, int32_t *route, int64_t *cells) {
    if (!c || !route || !cells) { dgi::set_error("dg_dp_get_partner_route: null"); return DG_ERR_ARG; }
    *route = c->dp ? c->dp->pt_route : 0;
    *cells = c->dp ? c->dp->pt_route_cells : 0;
    return DG_OK;
}

extern "C" int dg_dp_best_partners(dg_ctx *c, const int32_t *given, int64_t n, const int32_t *budgets, int32_t *partners, dg_dp_partner *out) {
    if (int rc = dgi::bind(c)) return rc;
    return dgi::dp_best_partners(c, given, n, budgets, partners, out);
}

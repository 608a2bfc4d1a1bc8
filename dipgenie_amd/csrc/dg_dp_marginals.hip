// dg_dp_partner_marginals: the max-marginals of the DP with one haplotype fixed -- for every vertex v the best value(given, q) over
// the source -> sink paths q through v with r(q) <= budget, and per level the best vertex, the best of the others and so the margin.
// Notation of dg_dp_partner.hip: d_l(u, v) scores the in-edge u -> v into level l with `given` fixed.
//   forward   F = the S of dg_dp_best_partners: F_0[source][r] = 0, F_l[v][r] = max over in-edges of F_{l-1}[u][r - w] + d_l(u, v);
//   backward  B_{L-1}[sink][r] = 0, B_{l-1}[u][r] = max over the out-edges (u -> v, w) with r - w >= 0 and a reachable destination
//             cell of d_l(u, v) + B_l[v][r - w];
//   marginal  M[v] = max over r = 0..b with both cells reachable of F[v][r] + B[v][b - r]; NEG_INF where there is none.
// Both tables mean "at most r", so a path with r1 recombinations up to v and r2 after it is counted at r = r1 whenever r1 + r2 <= b.
// Three kernels per slab of queries, two of them dg_dp_partner.hip's (dg_dp_partner.hpp):
//   * dp_partner_scores_kernel: d of every in-edge as 16 bits, and the validation of the given paths.
//   * dp_partner_sweep_kernel<VALUES>: the forward recurrence, storing every cell's int32 value as [vertex][r] in global memory.
//   * dp_marginals_back_kernel (here): one persistent 256-lane workgroup per query, launched after the forward kernel on the same
//     stream -- the kernel boundary is what makes the forward values visible.  Two copies of the backward state in LDS, [vertex][r],
//     r fastest.  The device has no out-CSR, so level l - 1 is filled from the in-edges of level l with the loops of the forward
//     recurrence turned round: the lane of (destination row v, plane r) does, per in-edge (pos, w) of v, an LDS atomicMax of
//     B_l[v][r - w] + d on B_{l-1}[pos][r] -- an integer maximum into a level that was set to NEG_INF before, so the order of the
//     lanes does not matter.  Per level, between two barriers: the scatter of level l into level l - 1 and, on the same (now
//     read-only) state of level l, the combination: groups of G = min(64, next power of two >= budget + 1) lanes per vertex form
//     F[v][r] + B[v][b - r], reduce it by shuffles to M[v], store it where the caller wants the vertex values, and keep the top two
//     keys (value << 32 | INT32_MAX - id: value descending, id ascending) seen by the lane; waves reduce them by shuffles, one lane
//     merges the four waves' pairs after the barrier and writes the level's 16-byte record.  A group's first forward value is loaded
//     before the scatter, as are the in-edge words, scores and offsets of level l - 1, which go to the LDS stage (one buffer) in
//     the second phase of the level together with the NEG_INF fill of level l - 2.  A level with more than 1,024 in-edges or
//     vertices is read from global memory instead of the stage.
// Nothing of a run is read or written.  Per query a slab holds 4 * n_vertices * (bmax + 1) bytes of forward values (bmax: the
// largest budget of the call), 2 bytes per in-edge of scores, 4 * n_vertices bytes of marginals and 20 * n_levels bytes of path and
// level records; partner_slab_bytes bounds their sum.
// With option partner_wide (dg_dp_partner.hip) the forward kernel is dp_partner_sweep_wide_kernel<VALUES>, which reads level l - 1 back
// from the forward values and needs no other state, and the backward kernel dp_marginals_back_wide_kernel, whose two level states live
// in a per-query device buffer (8 * kmax * (bmax + 1) bytes more per query, released when the call returns).
#include <algorithm>
#include <cstring>

#include "dg_dp_partner.hpp"

namespace dgi {

namespace {

constexpr long long MG_NO_KEY = INT64_MIN;              // no vertex (every key of a vertex is larger: its value is >= 0)

// any level as PtLevel: level 0 (the source level) has no in-edges
__device__ __forceinline__ PtLevel mg_level(const LevelDesc *__restrict__ descs, int l) {
    if (l >= 1) return pt_level(descs, l);
    const LevelDesc &d = descs[1];
    return PtLevel{d.a0, d.k, 0u, 0};
}

__device__ __forceinline__ long long mg_key(int value, int id) { return (long long)(((unsigned long long)(uint32_t)value << 32) | (uint32_t)(INT32_MAX - id)); }

// (a1 >= a2) and (b1 >= b2), keys of distinct vertices or MG_NO_KEY -> the two largest of the four
__device__ __forceinline__ void mg_merge(long long &a1, long long &a2, long long b1, long long b2) {
    const long long hi = a1 > b1 ? a1 : b1, lo = a1 > b1 ? b1 : a1, rest = a2 > b2 ? a2 : b2;
    a1 = hi;
    a2 = lo > rest ? lo : rest;
}

// Level l scattered into level l - 1.  STAGED: edge / sc / off are the LDS stage (indices relative to the level's first in-edge /
// vertex); otherwise the global arrays (off = in_off + b0, absolute in-edge indices).
template <bool STAGED>
__device__ __forceinline__ void mg_scatter(const PtLevel &lv, int B1, int vrow, int rows, int r0, int rstep, const int32_t *src, int32_t *dst,
                                           const uint32_t *edge, const uint16_t *sc, const uint32_t *off) {
    for (int v = vrow; v < lv.k2; v += rows) {
        const uint32_t e0 = off[v], e1 = off[v + 1];
        for (int r = r0; r < B1; r += rstep) {
            const int s0 = src[v * B1 + r], s1 = r ? src[v * B1 + r - 1] : NEG_INF;          // the destination cell an in-edge of weight 0 / 1 reads
            for (uint32_t e = e0; e < e1; ++e) {
                const uint32_t rec = edge[e];
                const int pos = (int)(rec & 0x7FFFFFFFu);
                const int s = (rec >> 31) ? s1 : s0;
                if (s == NEG_INF) continue;
                atomicMax(&dst[pos * B1 + r], s + (int)sc[e]);
            }
        }
    }
}

// grid: n workgroups of PT_THREADS; dynamic LDS = two states of `cells` int32 each, then one stage buffer.  fwd = [n][fwd_stride]
// forward values; levels = [n][L]; vertex_values = [n][nV] or null
__global__ __launch_bounds__(PT_THREADS) void dp_marginals_back_kernel(const LevelDesc *__restrict__ descs, int L, int nV, int cells,
                                                                       const uint32_t *__restrict__ in_off, const uint32_t *__restrict__ in_edge,
                                                                       const uint16_t *__restrict__ scores, int64_t E, const int32_t *__restrict__ budgets,
                                                                       const int32_t *__restrict__ fwd_all, int64_t fwd_stride,
                                                                       dg_dp_level_margin *__restrict__ levels, int32_t *__restrict__ vertex_values) {
    extern __shared__ int32_t mg_lds[];
    __shared__ long long s_top[PT_THREADS / 64][2];
    const int64_t q = blockIdx.x;
    const int t = (int)threadIdx.x;
    const int B1 = budgets[q] + 1;
    const uint16_t *__restrict__ sc_g = scores + q * E;
    const int32_t *__restrict__ fwd = fwd_all + q * fwd_stride;
    dg_dp_level_margin *__restrict__ out = levels + q * (int64_t)L;
    int32_t *__restrict__ vv = vertex_values ? vertex_values + q * (int64_t)nV : nullptr;
    int32_t *const state0 = mg_lds, *const state1 = mg_lds + cells;     // level l lives in state (l & 1)
    uint32_t *const st_edge = (uint32_t *)(mg_lds + 2 * (size_t)cells), *const st_off = st_edge + PT_STAGE;
    uint16_t *const st_sc = (uint16_t *)(st_off + PT_STAGE + 4);
    // scatter, lanes -> cells as in the forward recurrence: whole rows of B1 planes per pass while a row fits the workgroup, else one
    // row with the lanes striding over r
    int rows, vrow, r0, rstep;
    if (B1 <= PT_THREADS) { rows = PT_THREADS / B1; vrow = t / B1; r0 = t - vrow * B1; rstep = B1; if (vrow >= rows) vrow = 1 << 30; }
    else { rows = 1; vrow = 0; r0 = t; rstep = PT_THREADS; }
    // combination: G lanes per vertex (a power of two, inside one wave), PT_THREADS / G vertices per pass
    int G = 1;
    while (G < 64 && G < B1) G <<= 1;
    const int gv = t / G, gj = t & (G - 1), gper = PT_THREADS / G;

    PtLevel lv = mg_level(descs, L - 1);                                // level l
    PtLevel ln = mg_level(descs, L - 2);                                // level l - 1
    {                                                                   // the sink's level: 0 on every plane of the sink, NEG_INF elsewhere; level L - 2: NEG_INF
        int32_t *top = ((L - 1) & 1) ? state1 : state0, *below = ((L - 1) & 1) ? state0 : state1;
        const int sink_lo = (nV - 1 - lv.b0) * B1;
        for (int i = t; i < lv.k2 * B1; i += PT_THREADS) top[i] = (i >= sink_lo && i < sink_lo + B1) ? 0 : NEG_INF;
        for (int i = t; i < ln.k2 * B1; i += PT_THREADS) below[i] = NEG_INF;
        if (pt_staged(lv)) {
            for (int i = t; i < lv.T; i += PT_THREADS) { st_edge[i] = in_edge[lv.in_base + i]; st_sc[i] = sc_g[lv.in_base + i]; }
            for (int i = t; i <= lv.k2; i += PT_THREADS) st_off[i] = in_off[lv.b0 + i] - lv.in_base;
        }
    }
    __syncthreads();
    for (int l = L - 1; l >= 0; --l) {
        const PtLevel lnn = mg_level(descs, l >= 2 ? l - 2 : 0);        // level l - 2 (its width: the fill below)
        const bool stage_next = l >= 2 && pt_staged(ln);                // level l - 1 has in-edges to stage
        // issued here, consumed after the scatter: the records of level l - 1 and the first forward value of this lane's group
        uint32_t pf_edge[PT_PF], pf_off[PT_PF + 1], pf_sc[PT_PF];
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
        int f_first = 0;                                                // F of level 0 is 0 on every plane and is not read
        if (l >= 1 && gv < lv.k2 && gj < B1) f_first = fwd[((int64_t)lv.b0 + gv) * B1 + gj];
        const int32_t *cur = (l & 1) ? state1 : state0;
        int32_t *below = (l & 1) ? state0 : state1;
        if (l >= 1) {
            if (pt_staged(lv)) mg_scatter<true>(lv, B1, vrow, rows, r0, rstep, cur, below, st_edge, st_sc, st_off);
            else mg_scatter<false>(lv, B1, vrow, rows, r0, rstep, cur, below, in_edge, sc_g, in_off + lv.b0);
        }
        long long k1 = MG_NO_KEY, k2 = MG_NO_KEY;
        for (int v0 = 0; v0 < lv.k2; v0 += gper) {                      // the same trips for every lane: the shuffles below find their group whole
            const int v = v0 + gv;
            int m = NEG_INF;
            if (v < lv.k2) {
                for (int r = gj; r < B1; r += G) {
                    const int f = (v0 == 0 && r == gj) ? f_first : (l >= 1 ? fwd[((int64_t)lv.b0 + v) * B1 + r] : 0);
                    const int b = cur[v * B1 + (B1 - 1 - r)];
                    if (f != NEG_INF && b != NEG_INF) m = max(m, f + b);
                }
            }
            for (int d = G >> 1; d; d >>= 1) m = max(m, __shfl_xor(m, d));
            if (v < lv.k2 && gj == 0) {
                if (vv) vv[lv.b0 + v] = m;
                if (m != NEG_INF) mg_merge(k1, k2, mg_key(m, lv.b0 + v), MG_NO_KEY);
            }
        }
        for (int d = 32; d; d >>= 1) {
            const long long o1 = __shfl_xor(k1, d), o2 = __shfl_xor(k2, d);
            mg_merge(k1, k2, o1, o2);
        }
        if ((t & 63) == 0) { s_top[t >> 6][0] = k1; s_top[t >> 6][1] = k2; }
        __syncthreads();
        if (t == 0) {
            for (int w = 1; w < PT_THREADS / 64; ++w) mg_merge(k1, k2, s_top[w][0], s_top[w][1]);
            dg_dp_level_margin rec;
            rec.best_vertex = k1 == MG_NO_KEY ? -1 : INT32_MAX - (int)(uint32_t)k1;
            rec.best_value = k1 == MG_NO_KEY ? NEG_INF : (int)(k1 >> 32);
            rec.second_vertex = k2 == MG_NO_KEY ? -1 : INT32_MAX - (int)(uint32_t)k2;
            rec.second_value = k2 == MG_NO_KEY ? NEG_INF : (int)(k2 >> 32);
            out[l] = rec;
        }
        if (l >= 2) {                                                   // level l's state has been read: it becomes level l - 2
            int32_t *nxt = (l & 1) ? state1 : state0;
            for (int i = t; i < lnn.k2 * B1; i += PT_THREADS) nxt[i] = NEG_INF;
        }
        if (stage_next) {
#pragma unroll
            for (int j = 0; j < PT_PF; ++j) {
                const int i = t + j * PT_THREADS;
                if (i < ln.T) { st_edge[i] = pf_edge[j]; st_sc[i] = (uint16_t)pf_sc[j]; }
            }
#pragma unroll
            for (int j = 0; j <= PT_PF; ++j) {
                const int i = t + j * PT_THREADS;
                if (i <= ln.k2) st_off[i] = pf_off[j] - ln.in_base;
            }
        }
        __syncthreads();
        lv = ln; ln = lnn;
    }
}

// ---- the device-memory route (option partner_wide): the same backward pass with the two level states in device memory ----
// The scatter's atomicMax is executed by the L2, past this CU's L1; a plain load of the same word may be served from an L1 line that
// was filled before the atomics arrived (the combination of level l + 1 read the neighbouring words of the same state copy two levels
// ago, the scatter itself reads rows next to the ones other lanes add to).  So every access to a backward state is an atomic one at
// agent scope, which goes to the L2 as well: the NEG_INF fill and the sink's row are atomic stores, the reads atomic loads.  With the
// barrier between the phases that orders fill, scatter and read of a word, whatever the L1 holds.  The forward values, written by
// the kernel before this one, are read with plain loads as in the LDS kernel.  (What the L1 bypass costs against plain loads is not
// measured: a plain load is not known to be correct here, so there is nothing to compare it with.)
__device__ __forceinline__ int mgw_ld(int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void mgw_st(int32_t *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Level l scattered into level l - 1, as mg_scatter
template <bool STAGED>
__device__ __forceinline__ void mgw_scatter(const PtLevel &lv, int B1, int vrow, int rows, int r0, int rstep, int32_t *src, int32_t *dst,
                                            const uint32_t *edge, const uint16_t *sc, const uint32_t *off) {
    for (int v = vrow; v < lv.k2; v += rows) {
        const uint32_t e0 = off[v], e1 = off[v + 1];
        for (int r = r0; r < B1; r += rstep) {
            const int s0 = mgw_ld(src + v * B1 + r), s1 = r ? mgw_ld(src + v * B1 + r - 1) : NEG_INF;   // the destination cell an in-edge of weight 0 / 1 reads
            for (uint32_t e = e0; e < e1; ++e) {
                const uint32_t rec = edge[e];
                const int pos = (int)(rec & 0x7FFFFFFFu);
                const int s = (rec >> 31) ? s1 : s0;
                if (s == NEG_INF) continue;
                atomicMax(&dst[pos * B1 + r], s + (int)sc[e]);
            }
        }
    }
}

// grid: n workgroups of PTW_THREADS; state_all = [n][2][cells] int32, level l in copy (l & 1); static LDS: one stage buffer and the
// waves' top-two keys.  Phases, barriers and outputs are those of dp_marginals_back_kernel
__global__ __launch_bounds__(PTW_THREADS) void dp_marginals_back_wide_kernel(const LevelDesc *__restrict__ descs, int L, int nV, int cells,
                                                                             const uint32_t *__restrict__ in_off, const uint32_t *__restrict__ in_edge,
                                                                             const uint16_t *__restrict__ scores, int64_t E, const int32_t *__restrict__ budgets,
                                                                             const int32_t *__restrict__ fwd_all, int64_t fwd_stride, int32_t *state_all,
                                                                             dg_dp_level_margin *__restrict__ levels, int32_t *__restrict__ vertex_values) {
    __shared__ uint32_t st_edge[PT_STAGE], st_off[PT_STAGE + 4];
    __shared__ uint16_t st_sc[PT_STAGE];
    __shared__ long long s_top[PTW_THREADS / 64][2];
    const int64_t q = blockIdx.x;
    const int t = (int)threadIdx.x;
    const int B1 = budgets[q] + 1;
    const uint16_t *__restrict__ sc_g = scores + q * E;
    const int32_t *__restrict__ fwd = fwd_all + q * fwd_stride;
    dg_dp_level_margin *__restrict__ out = levels + q * (int64_t)L;
    int32_t *__restrict__ vv = vertex_values ? vertex_values + q * (int64_t)nV : nullptr;
    int32_t *const state0 = state_all + q * 2 * (int64_t)cells, *const state1 = state0 + cells;
    // scatter, lanes -> cells as in the forward recurrence
    int rows, vrow, r0, rstep;
    if (B1 <= PTW_THREADS) { rows = PTW_THREADS / B1; vrow = t / B1; r0 = t - vrow * B1; rstep = B1; if (vrow >= rows) vrow = 1 << 30; }
    else { rows = 1; vrow = 0; r0 = t; rstep = PTW_THREADS; }
    // combination: G lanes per vertex (a power of two, inside one wave), PTW_THREADS / G vertices per pass
    int G = 1;
    while (G < 64 && G < B1) G <<= 1;
    const int gv = t / G, gj = t & (G - 1), gper = PTW_THREADS / G;

    PtLevel lv = mg_level(descs, L - 1);                                // level l
    PtLevel ln = mg_level(descs, L - 2);                                // level l - 1
    {                                                                   // the sink's level: 0 on every plane of the sink, NEG_INF elsewhere; level L - 2: NEG_INF
        int32_t *top = ((L - 1) & 1) ? state1 : state0, *below = ((L - 1) & 1) ? state0 : state1;
        const int sink_lo = (nV - 1 - lv.b0) * B1;
        for (int i = t; i < lv.k2 * B1; i += PTW_THREADS) mgw_st(top + i, (i >= sink_lo && i < sink_lo + B1) ? 0 : NEG_INF);
        for (int i = t; i < ln.k2 * B1; i += PTW_THREADS) mgw_st(below + i, NEG_INF);
        if (pt_staged(lv)) {
            for (int i = t; i < lv.T; i += PTW_THREADS) { st_edge[i] = in_edge[lv.in_base + i]; st_sc[i] = sc_g[lv.in_base + i]; }
            for (int i = t; i <= lv.k2; i += PTW_THREADS) st_off[i] = in_off[lv.b0 + i] - lv.in_base;
        }
    }
    __syncthreads();
    for (int l = L - 1; l >= 0; --l) {
        const PtLevel lnn = mg_level(descs, l >= 2 ? l - 2 : 0);        // level l - 2 (its width: the fill below)
        const bool stage_next = l >= 2 && pt_staged(ln);                // level l - 1 has in-edges to stage
        // issued here, consumed after the scatter: the records of level l - 1 and the first forward value of this lane's group
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
        int f_first = 0;                                                // F of level 0 is 0 on every plane and is not read
        if (l >= 1 && gv < lv.k2 && gj < B1) f_first = fwd[((int64_t)lv.b0 + gv) * B1 + gj];
        int32_t *cur = (l & 1) ? state1 : state0;
        int32_t *below = (l & 1) ? state0 : state1;
        if (l >= 1) {
            if (pt_staged(lv)) mgw_scatter<true>(lv, B1, vrow, rows, r0, rstep, cur, below, st_edge, st_sc, st_off);
            else mgw_scatter<false>(lv, B1, vrow, rows, r0, rstep, cur, below, in_edge, sc_g, in_off + lv.b0);
        }
        long long k1 = MG_NO_KEY, k2 = MG_NO_KEY;
        for (int v0 = 0; v0 < lv.k2; v0 += gper) {                      // the same trips for every lane: the shuffles below find their group whole
            const int v = v0 + gv;
            int m = NEG_INF;
            if (v < lv.k2) {
                for (int r = gj; r < B1; r += G) {
                    const int f = (v0 == 0 && r == gj) ? f_first : (l >= 1 ? fwd[((int64_t)lv.b0 + v) * B1 + r] : 0);
                    const int b = mgw_ld(cur + v * B1 + (B1 - 1 - r));
                    if (f != NEG_INF && b != NEG_INF) m = max(m, f + b);
                }
            }
            for (int d = G >> 1; d; d >>= 1) m = max(m, __shfl_xor(m, d));
            if (v < lv.k2 && gj == 0) {
                if (vv) vv[lv.b0 + v] = m;
                if (m != NEG_INF) mg_merge(k1, k2, mg_key(m, lv.b0 + v), MG_NO_KEY);
            }
        }
        for (int d = 32; d; d >>= 1) {
            const long long o1 = __shfl_xor(k1, d), o2 = __shfl_xor(k2, d);
            mg_merge(k1, k2, o1, o2);
        }
        if ((t & 63) == 0) { s_top[t >> 6][0] = k1; s_top[t >> 6][1] = k2; }
        __syncthreads();
        if (t == 0) {
            for (int w = 1; w < PTW_THREADS / 64; ++w) mg_merge(k1, k2, s_top[w][0], s_top[w][1]);
            dg_dp_level_margin rec;
            rec.best_vertex = k1 == MG_NO_KEY ? -1 : INT32_MAX - (int)(uint32_t)k1;
            rec.best_value = k1 == MG_NO_KEY ? NEG_INF : (int)(k1 >> 32);
            rec.second_vertex = k2 == MG_NO_KEY ? -1 : INT32_MAX - (int)(uint32_t)k2;
            rec.second_value = k2 == MG_NO_KEY ? NEG_INF : (int)(k2 >> 32);
            out[l] = rec;
        }
        if (l >= 2) {                                                   // level l's state has been read: it becomes level l - 2
            int32_t *nxt = (l & 1) ? state1 : state0;
            for (int i = t; i < lnn.k2 * B1; i += PTW_THREADS) mgw_st(nxt + i, NEG_INF);
        }
        if (stage_next) {
#pragma unroll
            for (int j = 0; j < PTW_PF; ++j) {
                const int i = t + j * PTW_THREADS;
                if (i < ln.T) { st_edge[i] = pf_edge[j]; st_sc[i] = (uint16_t)pf_sc[j]; }
            }
#pragma unroll
            for (int j = 0; j <= PTW_PF; ++j) {
                const int i = t + j * PTW_THREADS;
                if (i <= ln.k2) st_off[i] = pf_off[j] - ln.in_base;
            }
        }
        __syncthreads();
        lv = ln; ln = lnn;
    }
}

// dg_dp_call_margins, after the backward kernel: one wave per (query, level).  Query q of the slab is row `first + q` of the call: its
// marginals are those of the partners of the OTHER row's path, the called vertex is its own path's (given = the two paths in the
// order of the queries, so the path of row r is given + (1 - r) * L).  The lanes stride over the level's vertices and keep the
// largest key among those of another class than the called vertex's (cls null: every vertex is its own class).
__global__ __launch_bounds__(PT_THREADS) void dp_call_margins_kernel(const LevelDesc *__restrict__ descs, int L, int nV, int m, int first,
                                                                     const int32_t *__restrict__ given, const int32_t *__restrict__ vertex_values,
                                                                     const int32_t *__restrict__ cls, dg_dp_call_margin *__restrict__ out) {
    const int64_t wave = ((int64_t)blockIdx.x * PT_THREADS + threadIdx.x) >> 6;
    const int lane = (int)(threadIdx.x & 63);
    if (wave >= (int64_t)m * L) return;                                 // whole waves leave
    const int q = (int)(wave / L), l = (int)(wave - (int64_t)q * L), row = first + q;
    const PtLevel lv = mg_level(descs, l);
    const int32_t *__restrict__ vv = vertex_values + (int64_t)q * nV;
    const int called = given[(int64_t)(1 - row) * L + l];
    dg_dp_call_margin rec{called, NEG_INF, -1, NEG_INF};
    if ((uint32_t)called - (uint32_t)lv.b0 < (uint32_t)lv.k2) {         // (the expansion writes nothing else)
        const int cc = cls ? cls[called] : called;
        long long key = MG_NO_KEY;
        for (int v = lane; v < lv.k2; v += 64) {
            const int id = lv.b0 + v;
            if ((cls ? cls[id] : id) == cc) continue;
            const int mv = vv[id];
            if (mv != NEG_INF) key = max(key, mg_key(mv, id));
        }
        for (int d = 32; d; d >>= 1) key = max(key, __shfl_xor(key, d));
        rec.value = vv[called];
        if (key != MG_NO_KEY) { rec.alt_vertex = INT32_MAX - (int)(uint32_t)key; rec.alt_value = (int)(key >> 32); }
    }
    if (lane == 0) out[(int64_t)row * L + l] = rec;
}

// What a call's slabs share: LDS sizes, strides, and the buffers of `per_slab` queries (grow-only but for the two large ones, which the
// caller releases).  vertex: the marginals of every vertex are kept (on the device)
struct MgPlan { int cells; bool wide; size_t lds_bytes; int64_t fwd_stride, per_slab; };

// wide: the call takes the device-memory route (option partner_wide): no LDS to ask for, two backward states per query in d_pt_state
int mg_plan(DpState &S, int64_t n, int kmax, int bmax, bool wide, bool vertex, MgPlan &P) {
    const int L = S.L, nV = S.nV;
    const int64_t E = S.n_edges;
    P.cells = kmax * (bmax + 1);
    P.wide = wide;
    P.lds_bytes = wide ? 0 : 2 * (size_t)P.cells * 4 + PT_STAGE_BUF_BYTES;
    if (P.lds_bytes > 65536) DG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(dp_marginals_back_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)P.lds_bytes));
    // queries per slab: what partner_slab_bytes holds (at least one), every query sized for the call's largest budget
    P.fwd_stride = (int64_t)nV * (bmax + 1);                            // int32 units
    const int64_t query_bytes = 4 * P.fwd_stride + 2 * E + 4 * (int64_t)nV + 20 * (int64_t)L + (wide ? 8 * (int64_t)P.cells : 0);
    int64_t per_slab = std::max<int64_t>(1, S.opt.partner_slab_bytes / query_bytes);
    per_slab = std::min(std::min(per_slab, partner_slab_limit(S)), n);
    P.per_slab = per_slab;
    if (int rc = S.d_pt_pairs.ensure((size_t)(per_slab * L) * 4)) return rc;
    if (int rc = S.d_pt_bud.ensure((size_t)per_slab * 4)) return rc;
    if (int rc = S.d_pt_val.ensure((size_t)per_slab * 4)) return rc;
    if (int rc = S.d_pt_err.ensure(2 * sizeof(unsigned long long))) return rc;
    if (int rc = S.d_mg_levels.ensure((size_t)(per_slab * L) * sizeof(dg_dp_level_margin))) return rc;
    if (vertex)
        if (int rc = S.d_mg_vertex.ensure((size_t)(per_slab * nV) * 4)) return rc;
    partner_note_route(S, wide, P.cells);
    return DG_OK;
}

// the large buffers live for the call only: the lattice pool of a later run may need the memory
struct MgRelease { DpState &S; ~MgRelease() { S.d_pt_bp.release(); S.d_pt_scores.release(); S.d_pt_state.release(); S.d_cm_class.release(); } };

int mg_plan_large(DpState &S, const MgPlan &P) {
    if (int rc = S.d_pt_bp.ensure((size_t)(P.per_slab * P.fwd_stride) * 4)) return rc;
    if (P.wide)
        if (int rc = S.d_pt_state.ensure((size_t)(P.per_slab * 2 * P.cells) * 4)) return rc;
    return S.d_pt_scores.ensure((size_t)(P.per_slab * S.n_edges) * 2 + 16);
}

// The core: m queries of one slab whose given paths are on the device (query q's: given + q * L) and whose budgets are in d_pt_bud;
// scores + validation, forward values, backward pass.  Leaves the level records in d_mg_levels, the marginals (vertex) in
// d_mg_vertex and the first-bad-hop word in d_pt_err, all on the device; nothing is waited for.
int mg_launch_slab(DpState &S, const MgPlan &P, const int32_t *d_given, int64_t m, bool vertex, hipStream_t s) {
    unsigned long long *d_err = S.d_pt_err.as<unsigned long long>();
    DG_HIP(hipMemsetAsync(d_err, 0xFF, sizeof(unsigned long long), s));
    partner_launch_scores(S, d_given, S.L, m, S.d_pt_scores.as<uint16_t>(), d_err, s);
    DG_HIP(hipGetLastError());
    if (int rc = partner_launch_forward_values(S, P.wide, P.cells, m, S.d_pt_scores.as<uint16_t>(), S.d_pt_bud.as<int32_t>(), S.d_pt_bp.as<int32_t>(), P.fwd_stride,
                                               S.d_pt_val.as<int32_t>(), s))
        return rc;
    if (P.wide) {
        hipLaunchKernelGGL(dp_marginals_back_wide_kernel, dim3((unsigned)m), dim3(PTW_THREADS), 0, s, S.d_descs.as<LevelDesc>(), S.L, S.nV, P.cells,
                           S.d_in_off.as<uint32_t>(), S.d_in_edge.as<uint32_t>(), S.d_pt_scores.as<uint16_t>(), S.n_edges, S.d_pt_bud.as<int32_t>(),
                           S.d_pt_bp.as<int32_t>(), P.fwd_stride, S.d_pt_state.as<int32_t>(), S.d_mg_levels.as<dg_dp_level_margin>(),
                           vertex ? S.d_mg_vertex.as<int32_t>() : nullptr);
    } else {
        hipLaunchKernelGGL(dp_marginals_back_kernel, dim3((unsigned)m), dim3(PT_THREADS), P.lds_bytes, s, S.d_descs.as<LevelDesc>(), S.L, S.nV, P.cells,
                           S.d_in_off.as<uint32_t>(), S.d_in_edge.as<uint32_t>(), S.d_pt_scores.as<uint16_t>(), S.n_edges, S.d_pt_bud.as<int32_t>(),
                           S.d_pt_bp.as<int32_t>(), P.fwd_stride, S.d_mg_levels.as<dg_dp_level_margin>(), vertex ? S.d_mg_vertex.as<int32_t>() : nullptr);
    }
    DG_HIP(hipGetLastError());
    return DG_OK;
}

}  // namespace

int dp_partner_marginals(dg_ctx *c, const int32_t *given, int64_t n, const int32_t *budgets, dg_dp_level_margin *levels, int32_t *vertex_values) {
    static const char *const FN = "dg_dp_partner_marginals";
    DpState *Sp = c->dp;
    if (!Sp || !Sp->loaded) { set_error("%s: no graph loaded", FN); return DG_ERR_STATE; }
    if (n < 0) { set_error("%s: n = %lld", FN, (long long)n); return DG_ERR_ARG; }
    if (n == 0) return DG_OK;
    if (!given || !budgets || !levels) { set_error("%s: given, budgets and levels are required", FN); return DG_ERR_ARG; }
    DpState &S = *Sp;
    hipStream_t s = c->stream;
    const int L = S.L, nV = S.nV;
    int kmax, bmax;
    bool wide;
    if (int rc = partner_check_budgets(FN, S, n, budgets, kmax, bmax, wide)) return rc;
    MgPlan P;
    if (int rc = mg_plan(S, n, kmax, bmax, wide, vertex_values != nullptr, P)) return rc;
    const int64_t per_slab = P.per_slab;
    MgRelease release{S};
    if (int rc = mg_plan_large(S, P)) return rc;
    // the caller's arrays are written only if every query is answered
    std::vector<dg_dp_level_margin> recs((size_t)(n * L));
    std::vector<int32_t> vals;
    if (vertex_values) vals.resize((size_t)(n * nV));
    int32_t *d_given = S.d_pt_pairs.as<int32_t>();
    for (int64_t first = 0; first < n; first += per_slab) {
        const int64_t m = std::min(per_slab, n - first);
        unsigned long long err = PT_NO_ERROR;
        DG_HIP(hipMemcpyAsync(d_given, given + first * L, (size_t)(m * L) * 4, hipMemcpyHostToDevice, s));
        DG_HIP(hipMemcpyAsync(S.d_pt_bud.p, budgets + first, (size_t)m * 4, hipMemcpyHostToDevice, s));
        if (int rc = mg_launch_slab(S, P, d_given, m, vertex_values != nullptr, s)) return rc;
        DG_HIP(hipMemcpyAsync(recs.data() + first * L, S.d_mg_levels.p, (size_t)(m * L) * sizeof(dg_dp_level_margin), hipMemcpyDeviceToHost, s));
        if (vertex_values) DG_HIP(hipMemcpyAsync(vals.data() + first * nV, S.d_mg_vertex.p, (size_t)(m * nV) * 4, hipMemcpyDeviceToHost, s));
        DG_HIP(hipMemcpyAsync(&err, S.d_pt_err.p, sizeof err, hipMemcpyDeviceToHost, s));
        DG_HIP(hipStreamSynchronize(s));
        if (err != PT_NO_ERROR) return partner_bad_hop(FN, err, first, given, L);       // slabs go up in order: the first slab with a bad hop holds the first bad hop
    }
    memcpy(levels, recs.data(), recs.size() * sizeof(dg_dp_level_margin));
    if (vertex_values) memcpy(vertex_values, vals.data(), vals.size() * 4);
    return DG_OK;
}

// dg_dp_call_margins: both haplotypes of the last run's answer at `budget`, each against the best vertex of another class per level.
// Row 0: haplotype 1 with haplotype 2 given and the budget that haplotype 2 leaves, row 1 the mirror image.  The two paths go from the
// chain's hop words straight to where the score kernel reads them (budgets_launch_expand); back come the two hop counts, 16 bytes
// per (row, level) and, if asked for, the paths.
int dp_call_margins(dg_ctx *c, int32_t budget, const int32_t *vertex_class, dg_dp_call_margin *levels, int32_t *paths) {
    static const char *const FN = "dg_dp_call_margins";
    DpState *Sp = c->dp;
    if (!Sp || !Sp->loaded) { set_error("%s: no graph loaded", FN); return DG_ERR_STATE; }
    DpState &S = *Sp;
    if (S.run_pinned) {
        set_error("%s: the last run was dg_dp_run_pinned: the margins check the run's value against an unconstrained partner DP, which a constrained answer need not reach", FN);
        return DG_ERR_STATE;
    }
    const int L = S.L, nV = S.nV;
    int kmax = 1;
    for (int l = 1; l < L; ++l) kmax = std::max(kmax, S.descs[l].k2);
    // on the budget itself, not on what the other haplotype leaves: known before a run
    if (budget >= 0 && S.opt.partner_wide >= 1) {
        if (int rc = partner_check_wide(FN, "budget", budget, kmax, budget)) return rc;
    } else if (budget >= 0 && (int64_t)kmax * ((int64_t)budget + 1) > PT_MAX_CELLS) {
        set_error("%s: widest level %d x (budget + 1) %lld exceeds %d cells", FN, kmax, (long long)budget + 1, PT_MAX_CELLS);
        return DG_ERR_UNSUPPORTED;
    }
    int chain = 0;
    if (int rc = budgets_find_chain(FN, Sp, budget, chain)) return rc;
    if (!levels) { set_error("%s: levels is required", FN); return DG_ERR_ARG; }
    hipStream_t s = c->stream;
    std::vector<dg_dp_call_margin> recs(2 * (size_t)L, dg_dp_call_margin{-1, NEG_INF, -1, NEG_INF});
    std::vector<int32_t> rows(paths ? 2 * (size_t)L : 0, -1);
    const int32_t V = S.sink_host[(size_t)budget];
    if (V != NEG_INF) {
        // the two queries, in order: given = haplotype 2 (row 0), given = haplotype 1 (row 1) -- the expansion writes them swapped
        if (int rc = S.d_pt_pairs.ensure(2 * (size_t)L * 4)) return rc;
        if (int rc = S.d_ans_cnt.ensure(8)) return rc;
        int32_t *d_given = S.d_pt_pairs.as<int32_t>();
        int32_t cnt[2] = {0, 0};
        budgets_launch_expand(S, chain, 1, d_given, S.d_ans_cnt.as<int32_t>(), s);
        DG_HIP(hipGetLastError());
        DG_HIP(hipMemcpyAsync(cnt, S.d_ans_cnt.p, sizeof cnt, hipMemcpyDeviceToHost, s));
        DG_HIP(hipStreamSynchronize(s));
        if (cnt[0] < 0 || cnt[1] < 0 || cnt[0] + cnt[1] > budget) {
            set_error("%s: the answer at budget %d has %d + %d recombinations", FN, budget, cnt[0], cnt[1]);
            return DG_ERR_STATE;
        }
        const int32_t budgets[2] = {budget - cnt[1], budget - cnt[0]};
        MgPlan P;
        const int bmax = std::max(budgets[0], budgets[1]);
        if (int rc = mg_plan(S, 2, kmax, bmax, partner_route_wide(S, kmax, bmax), true, P)) return rc;      // (d_pt_pairs holds both paths already: it only grows)
        MgRelease release{S};
        if (int rc = mg_plan_large(S, P)) return rc;
        if (int rc = S.d_cm_out.ensure(2 * (size_t)L * sizeof(dg_dp_call_margin))) return rc;
        if (vertex_class) {
            if (int rc = S.d_cm_class.ensure((size_t)nV * 4)) return rc;
            DG_HIP(hipMemcpyAsync(S.d_cm_class.p, vertex_class, (size_t)nV * 4, hipMemcpyHostToDevice, s));
        }
        for (int first = 0; first < 2; first += (int)P.per_slab) {
            const int m = (int)std::min<int64_t>(P.per_slab, 2 - first);
            unsigned long long err = PT_NO_ERROR;
            DG_HIP(hipMemcpyAsync(S.d_pt_bud.p, budgets + first, (size_t)m * 4, hipMemcpyHostToDevice, s));
            if (int rc = mg_launch_slab(S, P, d_given + (size_t)first * L, m, true, s)) return rc;
            const int64_t waves = (int64_t)m * L;
            hipLaunchKernelGGL(dp_call_margins_kernel, dim3((unsigned)((waves + PT_THREADS / 64 - 1) / (PT_THREADS / 64))), dim3(PT_THREADS), 0, s,
                               S.d_descs.as<LevelDesc>(), L, nV, m, first, d_given, S.d_mg_vertex.as<int32_t>(),
                               vertex_class ? S.d_cm_class.as<int32_t>() : nullptr, S.d_cm_out.as<dg_dp_call_margin>());
            DG_HIP(hipGetLastError());
            DG_HIP(hipMemcpyAsync(&err, S.d_pt_err.p, sizeof err, hipMemcpyDeviceToHost, s));
            DG_HIP(hipStreamSynchronize(s));
            if (err != PT_NO_ERROR) {
                set_error("%s: row %d: the run's path is not a path of the graph (level %d)", FN, first + (int)(err >> 33), (int)((uint32_t)err >> 1));
                return DG_ERR_STATE;
            }
        }
        DG_HIP(hipMemcpyAsync(recs.data(), S.d_cm_out.p, recs.size() * sizeof(dg_dp_call_margin), hipMemcpyDeviceToHost, s));
        if (paths) {                                                    // rows 0 and 1 of the caller are haplotypes 1 and 2: the second and the first given path
            DG_HIP(hipMemcpyAsync(rows.data(), d_given + L, (size_t)L * 4, hipMemcpyDeviceToHost, s));
            DG_HIP(hipMemcpyAsync(rows.data() + L, d_given, (size_t)L * 4, hipMemcpyDeviceToHost, s));
        }
        DG_HIP(hipStreamSynchronize(s));
        // the closing check: the answer's own haplotype is a partner within the budget (M >= V), and no partner within it beats plane `budget` (M <= V)
        for (int row = 0; row < 2; ++row)
            for (int l = 0; l < L; ++l)
                if (recs[(size_t)row * L + l].value != V) {
                    set_error("%s: row %d level %d: the marginal of the called vertex %d is %d, the run's value at budget %d is %d", FN, row, l,
                              recs[(size_t)row * L + l].vertex, recs[(size_t)row * L + l].value, budget, V);
                    return DG_ERR_STATE;
                }
    }
    memcpy(levels, recs.data(), recs.size() * sizeof(dg_dp_call_margin));
    if (paths) memcpy(paths, rows.data(), rows.size() * 4);
    return DG_OK;
}

}  // namespace dgi

extern "C" int dg_dp_call_margins(dg_ctx *c, int32_t budget, const int32_t *vertex_class, dg_dp_call_margin *levels, int32_t *paths) {
    if (int rc = dgi::bind(c)) return rc;
    return dgi::dp_call_margins(c, budget, vertex_class, levels, paths);
}

extern "C" int dg_dp_partner_marginals(dg_ctx *c, const int32_t *given, int64_t n, const int32_t *budgets, dg_dp_level_margin *levels, int32_t *vertex_values) {
    if (int rc = dgi::bind(c)) return rc;
    return dgi::dp_partner_marginals(c, given, n, budgets, levels, vertex_values);
}

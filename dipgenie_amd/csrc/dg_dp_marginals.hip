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
    const int64_t E = S.n_edges;
    int kmax, bmax;
    if (int rc = partner_check_budgets(FN, S, n, budgets, kmax, bmax)) return rc;
    const int cells = kmax * (bmax + 1);
    const size_t lds_bytes = 2 * (size_t)cells * 4 + PT_STAGE_BUF_BYTES;
    if (lds_bytes > 65536) DG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(dp_marginals_back_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    // queries per slab: what partner_slab_bytes holds (at least one), every query sized for the call's largest budget
    const int64_t fwd_stride = (int64_t)nV * (bmax + 1);                // int32 units
    const int64_t query_bytes = 4 * fwd_stride + 2 * E + 4 * (int64_t)nV + 20 * (int64_t)L;
    int64_t per_slab = std::max<int64_t>(1, S.opt.partner_slab_bytes / query_bytes);
    per_slab = std::min(std::min(per_slab, partner_slab_limit(S)), n);
    if (int rc = S.d_pt_pairs.ensure((size_t)(per_slab * L) * 4)) return rc;
    if (int rc = S.d_pt_bud.ensure((size_t)per_slab * 4)) return rc;
    if (int rc = S.d_pt_val.ensure((size_t)per_slab * 4)) return rc;
    if (int rc = S.d_pt_err.ensure(2 * sizeof(unsigned long long))) return rc;
    if (int rc = S.d_mg_levels.ensure((size_t)(per_slab * L) * sizeof(dg_dp_level_margin))) return rc;
    if (vertex_values)
        if (int rc = S.d_mg_vertex.ensure((size_t)(per_slab * nV) * 4)) return rc;
    // the two large buffers live for the call only: the lattice pool of a later run may need the memory
    struct Release { DpState &S; ~Release() { S.d_pt_bp.release(); S.d_pt_scores.release(); } } release{S};
    if (int rc = S.d_pt_bp.ensure((size_t)(per_slab * fwd_stride) * 4)) return rc;
    if (int rc = S.d_pt_scores.ensure((size_t)(per_slab * E) * 2 + 16)) return rc;
    // the caller's arrays are written only if every query is answered
    std::vector<dg_dp_level_margin> recs((size_t)(n * L));
    std::vector<int32_t> vals;
    if (vertex_values) vals.resize((size_t)(n * nV));
    int32_t *d_given = S.d_pt_pairs.as<int32_t>();
    unsigned long long *d_err = S.d_pt_err.as<unsigned long long>();
    for (int64_t first = 0; first < n; first += per_slab) {
        const int64_t m = std::min(per_slab, n - first);
        unsigned long long err = PT_NO_ERROR;
        DG_HIP(hipMemcpyAsync(d_given, given + first * L, (size_t)(m * L) * 4, hipMemcpyHostToDevice, s));
        DG_HIP(hipMemcpyAsync(S.d_pt_bud.p, budgets + first, (size_t)m * 4, hipMemcpyHostToDevice, s));
        DG_HIP(hipMemsetAsync(d_err, 0xFF, sizeof err, s));
        partner_launch_scores(S, d_given, L, m, S.d_pt_scores.as<uint16_t>(), d_err, s);
        DG_HIP(hipGetLastError());
        if (int rc = partner_launch_forward_values(S, cells, m, S.d_pt_scores.as<uint16_t>(), S.d_pt_bud.as<int32_t>(), S.d_pt_bp.as<int32_t>(), fwd_stride,
                                                   S.d_pt_val.as<int32_t>(), s))
            return rc;
        hipLaunchKernelGGL(dp_marginals_back_kernel, dim3((unsigned)m), dim3(PT_THREADS), lds_bytes, s, S.d_descs.as<LevelDesc>(), L, nV, cells,
                           S.d_in_off.as<uint32_t>(), S.d_in_edge.as<uint32_t>(), S.d_pt_scores.as<uint16_t>(), E, S.d_pt_bud.as<int32_t>(),
                           S.d_pt_bp.as<int32_t>(), fwd_stride, S.d_mg_levels.as<dg_dp_level_margin>(), vertex_values ? S.d_mg_vertex.as<int32_t>() : nullptr);
        DG_HIP(hipGetLastError());
        DG_HIP(hipMemcpyAsync(recs.data() + first * L, S.d_mg_levels.p, (size_t)(m * L) * sizeof(dg_dp_level_margin), hipMemcpyDeviceToHost, s));
        if (vertex_values) DG_HIP(hipMemcpyAsync(vals.data() + first * nV, S.d_mg_vertex.p, (size_t)(m * nV) * 4, hipMemcpyDeviceToHost, s));
        DG_HIP(hipMemcpyAsync(&err, d_err, sizeof err, hipMemcpyDeviceToHost, s));
        DG_HIP(hipStreamSynchronize(s));
        if (err != PT_NO_ERROR) return partner_bad_hop(FN, err, first, given, L);       // slabs go up in order: the first slab with a bad hop holds the first bad hop
    }
    memcpy(levels, recs.data(), recs.size() * sizeof(dg_dp_level_margin));
    if (vertex_values) memcpy(vertex_values, vals.data(), vals.size() * 4);
    return DG_OK;
}

}  // namespace dgi

extern "C" int dg_dp_partner_marginals(dg_ctx *c, const int32_t *given, int64_t n, const int32_t *budgets, dg_dp_level_margin *levels, int32_t *vertex_values) {
    if (int rc = dgi::bind(c)) return rc;
    return dgi::dp_partner_marginals(c, given, n, budgets, levels, vertex_values);
}

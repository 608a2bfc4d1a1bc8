// What the two entry points of the DP with one haplotype fixed share: dg_dp_best_partners (dg_dp_partner.hip) and
// dg_dp_partner_marginals (dg_dp_marginals.hip).  Constants of the one-workgroup-per-query kernels, the level record they step
// through, the first-bad-hop word, the checks of a call's queries, and the launches of the two kernels that dg_dp_partner.hip owns
// and dg_dp_marginals.hip runs as well: the edge scores with the validation of the given paths, and the forward recurrence.
#pragma once
#include "dg_dp.hpp"

namespace dgi {

constexpr unsigned long long PT_NO_ERROR = ~0ull;
constexpr int PT_THREADS = 256;
constexpr int PT_SCORE_LEVELS = 64;                     // destination levels per workgroup of the score kernel
constexpr int PT_PF = 4;                                // staged in-edges per lane
constexpr int PT_STAGE = PT_THREADS * PT_PF;            // in-edges (and vertices) of a level that the LDS stage holds
constexpr int PT_MAX_CELLS = 16384;                     // kmax * (budget + 1): two int32 copies = 128 KiB of the CU's 160 KiB
// one stage buffer: PT_STAGE in-edge words, PT_STAGE + 4 in-edge offsets, PT_STAGE 16-bit scores
constexpr size_t PT_STAGE_BUF_BYTES = (size_t)PT_STAGE * 4 + ((size_t)PT_STAGE + 4) * 4 + (size_t)PT_STAGE * 2;

// first bad (query, level) of a slab by atomicMin: kind 0 = a vertex outside its level, 1 = a hop without an edge
__device__ __forceinline__ unsigned long long partner_err_key(int64_t query, int level, int kind) {
    return ((unsigned long long)query << 33) | ((unsigned long long)(uint32_t)level << 1) | (unsigned long long)kind;
}

struct PtLevel { int b0, k2; uint32_t in_base; int T; };   // a level as the destination of its in-edges: first vertex, width, first in-edge, in-edges
__device__ __forceinline__ PtLevel pt_level(const LevelDesc *__restrict__ descs, int l) {
    const LevelDesc &d = descs[l];
    return PtLevel{d.b0, d.k2, d.in_base, d.T};
}
__device__ __forceinline__ bool pt_staged(const PtLevel &v) { return v.T <= PT_STAGE && v.k2 <= PT_STAGE; }

// ---- host side (dg_dp_partner.hip) ----
// the budgets of a call: none negative, widest level x (budget + 1) within PT_MAX_CELLS (fn: the entry point's name, for the
// message); kmax = the widest level, bmax = the largest budget
int partner_check_budgets(const char *fn, const DpState &S, int64_t n, const int32_t *budgets, int &kmax, int &bmax);
// the bound that the grids of the score kernels put on the queries of a slab
int64_t partner_slab_limit(const DpState &S);
// sets the message of the first-bad-hop word `key` of the slab that starts at query `first` (given = the call's [n][L]); DG_ERR_ARG
int partner_bad_hop(const char *fn, unsigned long long key, int64_t first, const int32_t *given, int L);
// dp_partner_scores_kernel on m queries: query q's given path starts at given + q * given_stride (device), its scores at
// scores + q * n_edges; *err all ones beforehand
void partner_launch_scores(const DpState &S, const int32_t *given, int64_t given_stride, int64_t m, uint16_t *scores, unsigned long long *err, hipStream_t s);
// the forward recurrence on m queries with every cell's int32 value kept: values + q * stride holds [vertex][r], r fastest with
// budgets[q] + 1 entries per vertex, the source's row included; value[q] = the sink's cell on plane budgets[q].  cells = kmax * (bmax + 1)
int partner_launch_forward_values(const DpState &S, int cells, int64_t m, const uint16_t *scores, const int32_t *budgets, int32_t *values, int64_t stride,
                                  int32_t *value, hipStream_t s);

}  // namespace dgi

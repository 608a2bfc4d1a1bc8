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
// The device-memory route (option partner_wide): the level states live in device memory, so no LDS bound applies.  One workgroup of
// PTW_THREADS lanes per query (the state loads are L2 round trips: more lanes keep more of them in flight; the stage stays PT_STAGE
// entries, PTW_PF per lane).  The 16-bit back-pointer holds the source position in 15 bits and 0xFFFF means "none": PTW_MAX_K.
constexpr int PTW_THREADS = 1024;
constexpr int PTW_PF = PT_STAGE / PTW_THREADS;
constexpr int PTW_MAX_K = 32767;
constexpr int PTW_MAX_CELLS = 1 << 24;                  // kmax * (budget + 1) of one query
static_assert(PTW_PF >= 1 && PTW_PF * PTW_THREADS == PT_STAGE, "the stage is a whole number of entries per lane");
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
// the budgets of a call: none negative, widest level x (budget + 1) within PT_MAX_CELLS -- with option partner_wide >= 1 within the
// limits of the device-memory route instead (fn: the entry point's name, for the message); kmax = the widest level, bmax = the
// largest budget, wide = the route of the call as a whole
int partner_check_budgets(const char *fn, const DpState &S, int64_t n, const int32_t *budgets, int &kmax, int &bmax, bool &wide);
// the limits of the device-memory route on one budget: kmax <= PTW_MAX_K, kmax x (budget + 1) <= PTW_MAX_CELLS, else the message and
// DG_ERR_UNSUPPORTED (who: "query 3" or "budget 31", for the message)
int partner_check_wide(const char *fn, const char *who, long long which, int kmax, int64_t budget);
// the route of a call of kmax x (bmax + 1) cells under option partner_wide
inline bool partner_route_wide(const DpState &S, int kmax, int bmax) { return S.opt.partner_wide >= 2 || (S.opt.partner_wide == 1 && (int64_t)kmax * ((int64_t)bmax + 1) > PT_MAX_CELLS); }
// what dg_dp_get_partner_route reports: set once a call has chosen its route
inline void partner_note_route(DpState &S, bool wide, int64_t cells) { S.pt_route = wide ? 2 : 1; S.pt_route_cells = cells; }
// the bound that the grids of the score kernels put on the queries of a slab
int64_t partner_slab_limit(const DpState &S);
// sets the message of the first-bad-hop word `key` of the slab that starts at query `first` (given = the call's [n][L]); DG_ERR_ARG
int partner_bad_hop(const char *fn, unsigned long long key, int64_t first, const int32_t *given, int L);
// dp_partner_scores_kernel on m queries: query q's given path starts at given + q * given_stride (device), its scores at
// scores + q * n_edges; *err all ones beforehand
void partner_launch_scores(const DpState &S, const int32_t *given, int64_t given_stride, int64_t m, uint16_t *scores, unsigned long long *err, hipStream_t s);
// the forward recurrence on m queries with every cell's int32 value kept: values + q * stride holds [vertex][r], r fastest with
// budgets[q] + 1 entries per vertex, the source's row included; value[q] = the sink's cell on plane budgets[q].  cells = kmax * (bmax + 1).
// wide: the kernel of the device-memory route, which reads level l - 1 back from `values` and keeps no other state
int partner_launch_forward_values(const DpState &S, bool wide, int cells, int64_t m, const uint16_t *scores, const int32_t *budgets, int32_t *values, int64_t stride,
                                  int32_t *value, hipStream_t s);

}  // namespace dgi

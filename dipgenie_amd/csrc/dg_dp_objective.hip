// dg_dp_objective_paths / dg_dp_answer_objectives: what pairs of source -> sink paths are worth in the objective that the sweep's value
// approximates.  The sweep adds inter + symd per transition, so a colour that sits on many vertices of a path counts many times; the
// objective counts every colour once: with Hom(p) / Het(p) the unions of the hom / het colour lists of p's vertices,
//   hom_shared = |Hom(p) n Hom(q)|   hom_single = |Hom(p) /\ Hom(q)|   het_single = |Het(p) /\ Het(q)|   het_both = |Het(p) n Het(q)|
// and objective = hom_shared + het_single.  Hom ids and het ids are two id spaces, as in the transition score.
//
// Colour dictionary (once per load, at the first call): colour ids are arbitrary int32 values, so nothing is indexed by one.  Per kind
// the uploaded colour pool is sorted and made distinct (rocPRIM), and a lower-bound kernel gives every colour-list entry its rank in that
// dictionary: d_ob_hom_rank / d_ob_het_rank run parallel to d_hom_col / d_het_col.  Ch, Ct = the numbers of distinct colours,
// Wh = ceil(Ch / 32), Wt = ceil(Ct / 32) the bitmap words per path.  Only the ranks and the two counts outlive the construction.
//
// LDS route: one workgroup per pair, four bitmaps (hom and het of either path, 8 * (Wh + Wt) bytes) in dynamic LDS.  Lanes stride over
// the levels: a lane checks its vertex and the hop into it exactly as dp_score_paths_kernel does (an id outside its level is never used
// as an index; the first bad hop in (pair, path, level) order is kept by atomicMin on the packed key), then ORs the ranks of the
// vertex's two lists into the bitmaps with LDS atomics.  After a barrier the lanes stride over the words and popcount a & b and a ^ b
// per kind; wave reduction by shuffles, LDS across the waves, one lane writes the 16-byte record.
// Global route, for bitmaps beyond option objective_lds_bytes: the slab's bitmaps live in device memory, zeroed per slab; one kernel on a
// grid of (pair, block of levels) validates and ORs with global atomics, a second one (one workgroup per pair) counts.  The kernel
// boundary is what makes the first kernel's ORs visible to the second.
// Host: slabs bounded by score_slab_bytes, a pair counting its 8 * L bytes of paths plus, on the global route, its bitmaps.
// dg_dp_answer_objectives: the chains of the last run are expanded (budgets_launch_expand) where the kernels read their pairs; a
// chain whose budget nothing fits is all -1 and answers -1 in all four fields.  Nothing of a run is written.
#include <algorithm>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "dg_dp_setops.hpp"

namespace dgi {

namespace {

constexpr unsigned long long OBJ_NO_ERROR = ~0ull;
constexpr int OBJ_BLOCK = 256;                          // lanes per workgroup: levels per block on the global route
constexpr int64_t OBJ_MAX_GRID = (int64_t)1 << 30;
constexpr int OBJ_STATIC_LDS = 64;                      // s_red of objective_count

// the key of dg_dp_score.hip: pair | path | level | kind (0: the vertex is not in its level, 1: no edge into it from the path's previous vertex)
__device__ __forceinline__ unsigned long long objective_err_key(int64_t pair, int path, int level, int kind) {
    return ((unsigned long long)pair << 33) | ((unsigned long long)path << 32) | ((unsigned long long)(uint32_t)level << 1) | (unsigned long long)kind;
}

// rank[e] = position of col[e] in the sorted distinct ids dict[0 .. C)
__global__ __launch_bounds__(256) void dp_objective_rank_kernel(const int32_t *__restrict__ col, int64_t n, const int32_t *__restrict__ dict, int C,
                                                                int32_t *__restrict__ rank) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const int32_t x = col[e];
        int lo = 0, hi = C;
        while (lo < hi) {                                               // first dictionary id >= x: x itself
            const int mid = lo + ((hi - lo) >> 1);
            if (dict[mid] < x) lo = mid + 1; else hi = mid;
        }
        rank[e] = lo;
    }
}

struct ObjGraph {                                       // what the kernels read of the resident graph
    const LevelDesc *descs;
    int L;
    const uint32_t *in_off, *in_edge;
    const int64_t *hom_off, *het_off;
    const int32_t *hom_rank, *het_rank;
    int Wh, Wt;
};

// vertex path[l] and the hop into it, checked as dp_score_paths_kernel checks them; true: the vertex is in its level
__device__ __forceinline__ bool objective_check(const ObjGraph &G, const int32_t *__restrict__ path, int l, int64_t pair, int which, unsigned long long *err) {
    const int v = path[l];
    const LevelDesc &d = G.descs[l > 0 ? l : 1];                        // level 0 is the source level of transition 1
    const int b0 = l > 0 ? d.b0 : d.a0, k2 = l > 0 ? d.k2 : d.k;
    const bool v_ok = (uint32_t)v - (uint32_t)b0 < (uint32_t)k2;        // (unsigned compare: a negative id fails too)
    if (!v_ok) atomicMin(err, objective_err_key(pair, which, l, 0));
    if (l > 0 && v_ok) {
        const int u = path[l - 1];                                      // outside its level: reported by the lane of level l - 1
        if ((uint32_t)u - (uint32_t)d.a0 < (uint32_t)d.k && score_edge_weight(G.in_off, G.in_edge, v, (uint32_t)(u - d.a0)) < 0)
            atomicMin(err, objective_err_key(pair, which, l, 1));
    }
    return v_ok;
}

// bits of the ranks of the list entries [off[v], off[v + 1]) of a checked vertex v
__device__ __forceinline__ void objective_mark(const int64_t *__restrict__ off, const int32_t *__restrict__ rank, int v, uint32_t *bits) {
    for (int64_t e = off[v], end = off[v + 1]; e < end; ++e) {
        const uint32_t r = (uint32_t)rank[e];
        atomicOr(&bits[r >> 5], 1u << (r & 31u));
    }
}

// level l of one pair: checks, then the colours of its two vertices into the pair's bitmaps [hom p][hom q][het p][het q]
__device__ __forceinline__ void objective_level(const ObjGraph &G, const int32_t *__restrict__ p, const int32_t *__restrict__ q, int l, int64_t pair,
                                                uint32_t *bits, unsigned long long *err) {
    if (objective_check(G, p, l, pair, 0, err)) {
        objective_mark(G.hom_off, G.hom_rank, p[l], bits);
        objective_mark(G.het_off, G.het_rank, p[l], bits + 2 * G.Wh);
    }
    if (objective_check(G, q, l, pair, 1, err)) {
        objective_mark(G.hom_off, G.hom_rank, q[l], bits + G.Wh);
        objective_mark(G.het_off, G.het_rank, q[l], bits + 2 * G.Wh + G.Wt);
    }
}

// the whole workgroup: the pair's record from its finished bitmaps
__device__ __forceinline__ void objective_count(const uint32_t *bits, int Wh, int Wt, dg_dp_pair_objective *__restrict__ out) {
    int hom_and = 0, hom_xor = 0, het_and = 0, het_xor = 0;
    const uint32_t *hp = bits, *hq = bits + Wh, *tp = bits + 2 * Wh, *tq = tp + Wt;
    for (int w = (int)threadIdx.x; w < Wh; w += (int)blockDim.x) { const uint32_t a = hp[w], b = hq[w]; hom_and += __popc(a & b); hom_xor += __popc(a ^ b); }
    for (int w = (int)threadIdx.x; w < Wt; w += (int)blockDim.x) { const uint32_t a = tp[w], b = tq[w]; het_and += __popc(a & b); het_xor += __popc(a ^ b); }
    for (int sft = 32; sft > 0; sft >>= 1) {
        hom_and += __shfl_down(hom_and, sft); hom_xor += __shfl_down(hom_xor, sft);
        het_and += __shfl_down(het_and, sft); het_xor += __shfl_down(het_xor, sft);
    }
    __shared__ int s_red[OBJ_BLOCK / 64][4];
    static_assert(sizeof(s_red) == OBJ_STATIC_LDS, "the LDS route leaves room for s_red");
    const int wave = (int)(threadIdx.x >> 6);
    if ((threadIdx.x & 63) == 0) { s_red[wave][0] = hom_and; s_red[wave][1] = hom_xor; s_red[wave][2] = het_xor; s_red[wave][3] = het_and; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int sum[4] = {0, 0, 0, 0};
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w)
            for (int f = 0; f < 4; ++f) sum[f] += s_red[w][f];
        *out = dg_dp_pair_objective{sum[0], sum[1], sum[2], sum[3]};
    }
}

// none_ok: a pair whose first entry is negative is the expansion of a chain that nothing fits (dg_dp_answer_objectives) and answers -1
__device__ __forceinline__ bool objective_is_none(const int32_t *__restrict__ p, int none_ok) { return none_ok && p[0] < 0; }

// LDS route.  grid: n pairs, OBJ_BLOCK lanes, 8 * (Wh + Wt) bytes of dynamic LDS; *err all ones beforehand
__global__ __launch_bounds__(OBJ_BLOCK) void dp_objective_lds_kernel(ObjGraph G, const int32_t *__restrict__ paths /* [n][2][L] */, int none_ok,
                                                                     dg_dp_pair_objective *__restrict__ out, unsigned long long *__restrict__ err) {
    extern __shared__ uint32_t ob_bits[];
    const int64_t pair = blockIdx.x;
    const int32_t *p = paths + pair * 2 * (int64_t)G.L, *q = p + G.L;
    if (objective_is_none(p, none_ok)) {                                // (the same for every lane: nobody reaches a barrier)
        if (threadIdx.x == 0) out[pair] = dg_dp_pair_objective{-1, -1, -1, -1};
        return;
    }
    const int words = 2 * (G.Wh + G.Wt);
    for (int w = (int)threadIdx.x; w < words; w += (int)blockDim.x) ob_bits[w] = 0;
    __syncthreads();
    for (int l = (int)threadIdx.x; l < G.L; l += (int)blockDim.x) objective_level(G, p, q, l, pair, ob_bits, err);
    __syncthreads();
    objective_count(ob_bits, G.Wh, G.Wt, out + pair);
}

// Global route, first kernel.  grid: n * nblk workgroups of OBJ_BLOCK lanes, one lane per level; bits ([n][2 * (Wh + Wt)] words) zeroed beforehand
__global__ __launch_bounds__(OBJ_BLOCK) void dp_objective_mark_kernel(ObjGraph G, int nblk, const int32_t *__restrict__ paths, int none_ok,
                                                                      uint32_t *__restrict__ bits, unsigned long long *__restrict__ err) {
    const int64_t pair = (int64_t)(blockIdx.x / (unsigned)nblk);
    const int64_t l = (int64_t)(blockIdx.x % (unsigned)nblk) * blockDim.x + threadIdx.x;
    const int32_t *p = paths + pair * 2 * (int64_t)G.L, *q = p + G.L;
    if (l >= G.L || objective_is_none(p, none_ok)) return;
    objective_level(G, p, q, (int)l, pair, bits + pair * 2 * ((int64_t)G.Wh + G.Wt), err);
}

// Global route, second kernel.  grid: n pairs
__global__ __launch_bounds__(OBJ_BLOCK) void dp_objective_count_kernel(int L, int Wh, int Wt, const int32_t *__restrict__ paths, int none_ok,
                                                                       const uint32_t *__restrict__ bits, dg_dp_pair_objective *__restrict__ out) {
    const int64_t pair = blockIdx.x;
    if (objective_is_none(paths + pair * 2 * (int64_t)L, none_ok)) {
        if (threadIdx.x == 0) out[pair] = dg_dp_pair_objective{-1, -1, -1, -1};
        return;
    }
    objective_count(bits + pair * 2 * ((int64_t)Wh + Wt), Wh, Wt, out + pair);
}

// sorted distinct ids of col[0 .. n) -> one rank per entry; *C = their number
int objective_rank_kind(const DevBuf &col, int64_t n, DevBuf &rank, int64_t *C, hipStream_t s) {
    *C = 0;
    if (int rc = rank.ensure(4 * (size_t)n)) return rc;
    if (n == 0) return DG_OK;
    DevBuf sorted, dict, cnt, tmp;
    if (int rc = sorted.ensure(4 * (size_t)n)) return rc;
    if (int rc = dict.ensure(4 * (size_t)n)) return rc;
    if (int rc = cnt.ensure(8)) return rc;
    size_t tb = 0;
    DG_HIP(rocprim::radix_sort_keys(nullptr, tb, col.as<int32_t>(), sorted.as<int32_t>(), (size_t)n, 0, 32, s));
    if (int rc = tmp.ensure(tb)) return rc;
    DG_HIP(rocprim::radix_sort_keys(tmp.p, tb, col.as<int32_t>(), sorted.as<int32_t>(), (size_t)n, 0, 32, s));
    size_t tu = 0;
    DG_HIP(rocprim::unique(nullptr, tu, sorted.as<int32_t>(), dict.as<int32_t>(), cnt.as<unsigned long long>(), (size_t)n, rocprim::equal_to<int32_t>(), s));
    if (tu > tb) { DG_HIP(hipStreamSynchronize(s)); if (int rc = tmp.ensure(tu)) return rc; }
    DG_HIP(rocprim::unique(tmp.p, tu, sorted.as<int32_t>(), dict.as<int32_t>(), cnt.as<unsigned long long>(), (size_t)n, rocprim::equal_to<int32_t>(), s));
    unsigned long long distinct = 0;
    DG_HIP(hipMemcpyAsync(&distinct, cnt.p, sizeof distinct, hipMemcpyDeviceToHost, s));
    DG_HIP(hipStreamSynchronize(s));
    *C = (int64_t)distinct;                                             // <= 2^32 int32 values; a rank is an int32
    const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, (int64_t)1 << 20);
    hipLaunchKernelGGL(dp_objective_rank_kernel, dim3(grid), dim3(256), 0, s, col.as<int32_t>(), n, dict.as<int32_t>(), (int)distinct, rank.as<int32_t>());
    DG_HIP(hipGetLastError());
    DG_HIP(hipStreamSynchronize(s));                                    // the temporaries go with this scope
    return DG_OK;
}

int objective_dictionary(dg_ctx *c, DpState &S) {
    if (S.ob_dict) return DG_OK;
    hipStream_t s = c->stream;
    int64_t n_hom = 0, n_het = 0;
    DG_HIP(hipMemcpyAsync(&n_hom, S.d_hom_off.as<int64_t>() + S.nV, 8, hipMemcpyDeviceToHost, s));
    DG_HIP(hipMemcpyAsync(&n_het, S.d_het_off.as<int64_t>() + S.nV, 8, hipMemcpyDeviceToHost, s));
    DG_HIP(hipStreamSynchronize(s));
    if (int rc = objective_rank_kind(S.d_hom_col, n_hom, S.d_ob_hom_rank, &S.ob_ch, s)) return rc;
    if (int rc = objective_rank_kind(S.d_het_col, n_het, S.d_ob_het_rank, &S.ob_ct, s)) return rc;
    if (S.ob_ch >= ((int64_t)1 << 31) || S.ob_ct >= ((int64_t)1 << 31)) { set_error("colour dictionary: %lld hom / %lld het distinct ids do not fit an int32 rank", (long long)S.ob_ch, (long long)S.ob_ct); return DG_ERR_UNSUPPORTED; }
    S.ob_dict = true;
    return DG_OK;
}

struct ObjPlan {                                        // one call: the route and the slab size
    ObjGraph G;
    int64_t pair_bits_bytes = 0;                        // 8 * (Wh + Wt)
    bool lds = true;
    int nblk = 1;                                       // global route: workgroups per pair of the first kernel
    int64_t per_slab = 1;
};

int objective_plan(dg_ctx *c, DpState &S, int64_t n_pairs, ObjPlan &P) {
    if (int rc = objective_dictionary(c, S)) return rc;
    const int64_t Wh = (S.ob_ch + 31) / 32, Wt = (S.ob_ct + 31) / 32;
    P.G = ObjGraph{S.d_descs.as<LevelDesc>(), S.L, S.d_in_off.as<uint32_t>(), S.d_in_edge.as<uint32_t>(), S.d_hom_off.as<int64_t>(), S.d_het_off.as<int64_t>(),
                   S.d_ob_hom_rank.as<int32_t>(), S.d_ob_het_rank.as<int32_t>(), (int)Wh, (int)Wt};
    P.pair_bits_bytes = 8 * (Wh + Wt);
    P.lds = P.pair_bits_bytes <= std::min(S.opt.objective_lds_bytes, objective_lds_limit(c));
    P.nblk = (S.L + OBJ_BLOCK - 1) / OBJ_BLOCK;
    // pairs per slab: what score_slab_bytes holds (at least one), a grid of at most 2^30 workgroups, a pair index of 31 bits
    const int64_t pair_bytes = 8 * (int64_t)S.L + (P.lds ? 0 : P.pair_bits_bytes);
    P.per_slab = std::max<int64_t>(1, S.opt.score_slab_bytes / pair_bytes);
    P.per_slab = std::min(P.per_slab, std::max<int64_t>(1, OBJ_MAX_GRID / P.nblk));
    P.per_slab = std::min(P.per_slab, n_pairs);
    if (int rc = S.d_ob_paths.ensure((size_t)(P.per_slab * 8 * (int64_t)S.L))) return rc;
    if (int rc = S.d_ob_out.ensure((size_t)P.per_slab * sizeof(dg_dp_pair_objective))) return rc;
    if (int rc = S.d_ob_err.ensure(sizeof(unsigned long long))) return rc;
    if (!P.lds) { if (int rc = S.d_ob_bits.ensure((size_t)(P.per_slab * P.pair_bits_bytes))) return rc; }
    else if (P.pair_bits_bytes > 65536 - OBJ_STATIC_LDS)
        DG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(dp_objective_lds_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)P.pair_bits_bytes));
    return DG_OK;
}

// the n pairs in d_ob_paths -> res (host) and *err; synchronises
int objective_slab(DpState &S, const ObjPlan &P, int64_t n, int none_ok, dg_dp_pair_objective *res, unsigned long long *err, hipStream_t s) {
    DG_HIP(hipMemsetAsync(S.d_ob_err.p, 0xFF, sizeof *err, s));
    const int32_t *pairs = S.d_ob_paths.as<int32_t>();
    dg_dp_pair_objective *out = S.d_ob_out.as<dg_dp_pair_objective>();
    unsigned long long *d_err = S.d_ob_err.as<unsigned long long>();
    if (P.lds) {
        hipLaunchKernelGGL(dp_objective_lds_kernel, dim3((unsigned)n), dim3(OBJ_BLOCK), (size_t)P.pair_bits_bytes, s, P.G, pairs, none_ok, out, d_err);
    } else {
        DG_HIP(hipMemsetAsync(S.d_ob_bits.p, 0, (size_t)(n * P.pair_bits_bytes), s));
        hipLaunchKernelGGL(dp_objective_mark_kernel, dim3((unsigned)(n * P.nblk)), dim3(OBJ_BLOCK), 0, s, P.G, P.nblk, pairs, none_ok, S.d_ob_bits.as<uint32_t>(), d_err);
        DG_HIP(hipGetLastError());
        hipLaunchKernelGGL(dp_objective_count_kernel, dim3((unsigned)n), dim3(OBJ_BLOCK), 0, s, S.L, P.G.Wh, P.G.Wt, pairs, none_ok, S.d_ob_bits.as<uint32_t>(), out);
    }
    DG_HIP(hipGetLastError());
    DG_HIP(hipMemcpyAsync(res, S.d_ob_out.p, (size_t)n * sizeof(dg_dp_pair_objective), hipMemcpyDeviceToHost, s));
    DG_HIP(hipMemcpyAsync(err, S.d_ob_err.p, sizeof *err, hipMemcpyDeviceToHost, s));
    DG_HIP(hipStreamSynchronize(s));
    return DG_OK;
}

}  // namespace

int64_t objective_lds_limit(const dg_ctx *c) {
    const int64_t lds = (int64_t)std::max(c->prop.sharedMemPerBlock, c->prop.sharedMemPerBlockOptin);
    return std::max<int64_t>(lds, 65536) - OBJ_STATIC_LDS;
}

int dp_objective_paths(dg_ctx *c, const int32_t *paths, int64_t n_pairs, dg_dp_pair_objective *out) {
    static const char *const FN = "dg_dp_objective_paths";
    DpState *Sp = c->dp;
    if (!Sp || !Sp->loaded) { set_error("%s: no graph loaded", FN); return DG_ERR_STATE; }
    if (n_pairs < 0) { set_error("%s: n_pairs = %lld", FN, (long long)n_pairs); return DG_ERR_ARG; }
    if (n_pairs == 0) return DG_OK;
    if (!paths || !out) { set_error("%s: paths and out are required", FN); return DG_ERR_ARG; }
    DpState &S = *Sp;
    hipStream_t s = c->stream;
    const int L = S.L;
    const int64_t pair_words = 2 * (int64_t)L;
    ObjPlan P;
    if (int rc = objective_plan(c, S, n_pairs, P)) return rc;
    static_assert(sizeof(dg_dp_pair_objective) == 16, "four result words per pair");
    std::vector<dg_dp_pair_objective> res((size_t)n_pairs);             // the caller's array is written only if every pair is valid
    for (int64_t first = 0; first < n_pairs; first += P.per_slab) {
        const int64_t n = std::min(P.per_slab, n_pairs - first);
        unsigned long long err = OBJ_NO_ERROR;
        DG_HIP(hipMemcpyAsync(S.d_ob_paths.p, paths + first * pair_words, (size_t)(n * pair_words) * 4, hipMemcpyHostToDevice, s));
        if (int rc = objective_slab(S, P, n, 0, res.data() + first, &err, s)) return rc;
        if (err != OBJ_NO_ERROR) {                                      // slabs go up in order: the first slab with a bad hop holds the first bad hop
            const int64_t pair = first + (int64_t)(err >> 33);
            const int path = (int)((err >> 32) & 1u), level = (int)((uint32_t)err >> 1), kind = (int)(err & 1u);
            const int32_t *pp = paths + pair * pair_words + (int64_t)path * L;
            if (kind == 0) set_error("%s: pair %lld path %d level %d: vertex %d is not in that level", FN, (long long)pair, path, level, pp[level]);
            else set_error("%s: pair %lld path %d level %d: no edge %d -> %d", FN, (long long)pair, path, level, pp[level - 1], pp[level]);
            return DG_ERR_ARG;
        }
    }
    memcpy(out, res.data(), (size_t)n_pairs * sizeof(dg_dp_pair_objective));
    return DG_OK;
}

int dp_answer_objectives(dg_ctx *c, const int32_t *budgets, int32_t n_budgets, dg_dp_pair_objective *out) {
    static const char *const FN = "dg_dp_answer_objectives";
    DpState *Sp = c->dp;
    if (!Sp || !Sp->loaded) { set_error("%s: no graph loaded", FN); return DG_ERR_STATE; }
    if (!budgets || !out || n_budgets <= 0) { set_error("%s: budgets, out and n_budgets > 0 are required", FN); return DG_ERR_ARG; }
    if (!Sp->run_ok || Sp->sink_host.empty()) { set_error("%s: budget %d: no completed dg_dp_run / dg_dp_run_budgets on the loaded graph", FN, budgets[0]); return DG_ERR_STATE; }
    std::vector<int> chains((size_t)n_budgets);
    for (int32_t q = 0; q < n_budgets; ++q)
        if (int rc = budgets_find_chain(FN, Sp, budgets[q], chains[(size_t)q])) return rc;
    DpState &S = *Sp;
    hipStream_t s = c->stream;
    ObjPlan P;
    if (int rc = objective_plan(c, S, n_budgets, P)) return rc;
    if (int rc = S.d_ans_cnt.ensure(8)) return rc;                      // the hop counts of the expansion: not asked for here
    std::vector<dg_dp_pair_objective> res((size_t)n_budgets);           // the caller's array is written only on success
    for (int64_t first = 0; first < n_budgets; first += P.per_slab) {
        const int64_t n = std::min<int64_t>(P.per_slab, n_budgets - first);
        unsigned long long err = OBJ_NO_ERROR;
        for (int64_t q = 0; q < n; ++q)
            budgets_launch_expand(S, chains[(size_t)(first + q)], 0, S.d_ob_paths.as<int32_t>() + q * 2 * (int64_t)S.L, S.d_ans_cnt.as<int32_t>(), s);
        DG_HIP(hipGetLastError());
        if (int rc = objective_slab(S, P, n, 1, res.data() + first, &err, s)) return rc;
        if (err != OBJ_NO_ERROR) {                                      // the run checked every chain: its path slice no longer describes a path
            set_error("%s: the answer at budget %d is not a pair of paths of the loaded graph (level %d)", FN, budgets[first + (int64_t)(err >> 33)], (int)((uint32_t)err >> 1));
            return DG_ERR_STATE;
        }
    }
    memcpy(out, res.data(), (size_t)n_budgets * sizeof(dg_dp_pair_objective));
    return DG_OK;
}

}  // namespace dgi

extern "C" int dg_dp_objective_paths(dg_ctx *c, const int32_t *paths, int64_t n_pairs, dg_dp_pair_objective *out) {
    if (int rc = dgi::bind(c)) return rc;
    return dgi::dp_objective_paths(c, paths, n_pairs, out);
}

extern "C" int dg_dp_answer_objectives(dg_ctx *c, const int32_t *budgets, int32_t n_budgets, dg_dp_pair_objective *out) {
    if (int rc = dgi::bind(c)) return rc;
    return dgi::dp_answer_objectives(c, budgets, n_budgets, out);
}

// dg_dp_score_paths: the value of caller-supplied pairs of source -> sink paths on the resident graph, thousands of pairs per launch.
// For the transition into level l a pair (p, q) contributes what the sweep adds to cell (p[l], q[l]) for the in-edge pair
// (p[l-1] -> p[l], q[l-1] -> q[l]): |(Hom(p[l-1]) u Hom(q[l-1])) n (Hom(p[l]) u Hom(q[l]))| + |(Het .. u ..) /\ (Het .. u ..)|
// (approximator.cpp:604-624, the merges of dg_dp_setops.hpp), the second term alone being the transition's share of s_het (:662).
// Nothing of a run is read or written: only the tables of dg_dp_load_graph (level descriptors, in-CSR, colour CSR).
//
// Kernel: one workgroup per (pair, block of destination levels), one lane per transition.  A lane first checks its four vertex ids
// against the level descriptor (an id outside its level is never used as an index), then looks both edges up by binary search of the
// destination's in-edge slice -- sorted by source position; parallel edges carry equal weights (checked at load), so any hit gives
// the weight -- and only then touches the colour lists.  Wave reduction by shuffles, LDS across the waves, one atomicAdd per
// workgroup and result word.  The first bad hop in (pair, path, level) order is kept by an atomicMin on one packed 64-bit word
// that the host reads once per slab.
// Host: the paths go up in slabs of at most score_slab_bytes (dg_dp_set_option), so n_pairs x n_levels is bounded by host memory only.
#include <algorithm>
#include <cstring>

#include "dg_dp_setops.hpp"

namespace dgi {

namespace {

constexpr unsigned long long SCORE_NO_ERROR = ~0ull;
constexpr int SCORE_BLOCK = 256;                        // transitions per workgroup (graphs of <= 65 levels: one wave)
constexpr int64_t SCORE_MAX_GRID = (int64_t)1 << 30;

// bad hop -> key, smaller = earlier: pair | path | level | kind (0: the vertex is not in its level, 1: no edge into it from the path's previous vertex)
__device__ __forceinline__ unsigned long long score_err_key(int64_t pair, int path, int level, int kind) {
    return ((unsigned long long)pair << 33) | ((unsigned long long)path << 32) | ((unsigned long long)(uint32_t)level << 1) | (unsigned long long)kind;
}

// grid: n_pairs * nblk workgroups of 64 or 256 lanes; out (4 words per pair: value, s_het, r1, r2) and *err are set by the host before the launch
__global__ __launch_bounds__(SCORE_BLOCK) void dp_score_paths_kernel(const LevelDesc *__restrict__ descs, int L, int nblk,
                                                                     const uint32_t *__restrict__ in_off, const uint32_t *__restrict__ in_edge, ColourCsr col,
                                                                     const int32_t *__restrict__ paths /* [n_pairs][2][L] */, int32_t *__restrict__ out,
                                                                     unsigned long long *__restrict__ err) {
    const int64_t pair = (int64_t)(blockIdx.x / (unsigned)nblk);
    const int blk = (int)(blockIdx.x % (unsigned)nblk);
    const int64_t lq = 1 + (int64_t)blk * blockDim.x + threadIdx.x;     // destination level of this lane's transition
    int value = 0, shet = 0, r1 = 0, r2 = 0;
    if (lq < L) {
        const int l = (int)lq;
        const int32_t *p = paths + pair * 2 * (int64_t)L, *q = p + L;
        const int pu = p[l - 1], pv = p[l], qu = q[l - 1], qv = q[l];
        const LevelDesc &d = descs[l];
        const int a0 = d.a0, k = d.k, b0 = d.b0, k2 = d.k2;
        // (unsigned compare: a negative id fails too)  A source id is reported at its own level l - 1, as the lane of that level does
        const bool pu_ok = (uint32_t)pu - (uint32_t)a0 < (uint32_t)k, qu_ok = (uint32_t)qu - (uint32_t)a0 < (uint32_t)k;
        const bool pv_ok = (uint32_t)pv - (uint32_t)b0 < (uint32_t)k2, qv_ok = (uint32_t)qv - (uint32_t)b0 < (uint32_t)k2;
        if (!pu_ok) atomicMin(err, score_err_key(pair, 0, l - 1, 0));
        if (!pv_ok) atomicMin(err, score_err_key(pair, 0, l, 0));
        if (!qu_ok) atomicMin(err, score_err_key(pair, 1, l - 1, 0));
        if (!qv_ok) atomicMin(err, score_err_key(pair, 1, l, 0));
        const int w1 = (pu_ok && pv_ok) ? score_edge_weight(in_off, in_edge, pv, (uint32_t)(pu - a0)) : -1;
        const int w2 = (qu_ok && qv_ok) ? score_edge_weight(in_off, in_edge, qv, (uint32_t)(qu - a0)) : -1;
        if (pu_ok && pv_ok && w1 < 0) atomicMin(err, score_err_key(pair, 0, l, 1));
        if (qu_ok && qv_ok && w2 < 0) atomicMin(err, score_err_key(pair, 1, l, 1));
        if (w1 >= 0 && w2 >= 0) {                                       // all four ids are inside their levels
            shet = score_symd(col, pu, qu, pv, qv);
            value = shet + score_inter(col, pu, qu, pv, qv);
            r1 = w1; r2 = w2;
        }
    }
    for (int sft = 32; sft > 0; sft >>= 1) {
        value += __shfl_down(value, sft); shet += __shfl_down(shet, sft);
        r1 += __shfl_down(r1, sft); r2 += __shfl_down(r2, sft);
    }
    __shared__ int s_red[SCORE_BLOCK / 64][4];
    const int wave = (int)(threadIdx.x >> 6);
    if ((threadIdx.x & 63) == 0) { s_red[wave][0] = value; s_red[wave][1] = shet; s_red[wave][2] = r1; s_red[wave][3] = r2; }
    __syncthreads();
    if (threadIdx.x < 4) {
        int sum = 0;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) sum += s_red[w][threadIdx.x];
        if (sum) atomicAdd(&out[pair * 4 + threadIdx.x], sum);
    }
}

inline int score_threads(int L) { return L - 1 <= 64 ? 64 : SCORE_BLOCK; }

}  // namespace

int score_pair_blocks(const DpState &S) { return (S.L - 1 + score_threads(S.L) - 1) / score_threads(S.L); }

void score_launch_pairs(const DpState &S, const int32_t *pairs, int64_t n, int32_t *out, unsigned long long *err, hipStream_t s) {
    const int nblk = score_pair_blocks(S);
    hipLaunchKernelGGL(dp_score_paths_kernel, dim3((unsigned)(n * nblk)), dim3((unsigned)score_threads(S.L)), 0, s, S.d_descs.as<LevelDesc>(), S.L, nblk,
                       S.d_in_off.as<uint32_t>(), S.d_in_edge.as<uint32_t>(), colour_csr(S), pairs, out, err);
}

int dp_score_paths(dg_ctx *c, const int32_t *paths, int64_t n_pairs, dg_dp_pair_score *out) {
    DpState *Sp = c->dp;
    if (!Sp || !Sp->loaded) { set_error("dg_dp_score_paths: no graph loaded"); return DG_ERR_STATE; }
    if (n_pairs < 0) { set_error("dg_dp_score_paths: n_pairs = %lld", (long long)n_pairs); return DG_ERR_ARG; }
    if (n_pairs == 0) return DG_OK;
    if (!paths || !out) { set_error("dg_dp_score_paths: paths and out are required"); return DG_ERR_ARG; }
    DpState &S = *Sp;
    hipStream_t s = c->stream;
    const int L = S.L;
    const int nblk = score_pair_blocks(S);
    const int64_t pair_words = 2 * (int64_t)L;
    // pairs per slab: what the staging bound holds (at least one), a grid of at most 2^30 workgroups, a pair index of 31 bits
    int64_t per_slab = std::max<int64_t>(1, S.opt.score_slab_bytes / (4 * pair_words));
    per_slab = std::min(per_slab, std::max<int64_t>(1, SCORE_MAX_GRID / nblk));
    per_slab = std::min(per_slab, n_pairs);
    if (int rc = S.d_sc_paths.ensure((size_t)(per_slab * pair_words) * 4)) return rc;
    if (int rc = S.d_sc_out.ensure((size_t)per_slab * sizeof(dg_dp_pair_score))) return rc;
    if (int rc = S.d_sc_err.ensure(sizeof(unsigned long long))) return rc;
    static_assert(sizeof(dg_dp_pair_score) == 16, "four result words per pair");
    std::vector<dg_dp_pair_score> res((size_t)n_pairs);                 // the caller's array is written only if every pair is valid
    for (int64_t first = 0; first < n_pairs; first += per_slab) {
        const int64_t n = std::min(per_slab, n_pairs - first);
        const int32_t *src = paths + first * pair_words;
        unsigned long long err = SCORE_NO_ERROR;
        DG_HIP(hipMemcpyAsync(S.d_sc_paths.p, src, (size_t)(n * pair_words) * 4, hipMemcpyHostToDevice, s));
        DG_HIP(hipMemsetAsync(S.d_sc_out.p, 0, (size_t)n * sizeof(dg_dp_pair_score), s));
        DG_HIP(hipMemsetAsync(S.d_sc_err.p, 0xFF, sizeof err, s));
        score_launch_pairs(S, S.d_sc_paths.as<int32_t>(), n, S.d_sc_out.as<int32_t>(), S.d_sc_err.as<unsigned long long>(), s);
        DG_HIP(hipGetLastError());
        DG_HIP(hipMemcpyAsync(res.data() + first, S.d_sc_out.p, (size_t)n * sizeof(dg_dp_pair_score), hipMemcpyDeviceToHost, s));
        DG_HIP(hipMemcpyAsync(&err, S.d_sc_err.p, sizeof err, hipMemcpyDeviceToHost, s));
        DG_HIP(hipStreamSynchronize(s));
        if (err != SCORE_NO_ERROR) {                                    // slabs go up in order: the first slab with a bad hop holds the first bad hop
            const int64_t pair = first + (int64_t)(err >> 33);
            const int path = (int)((err >> 32) & 1u), level = (int)((uint32_t)err >> 1), kind = (int)(err & 1u);
            const int32_t *pp = paths + pair * pair_words + (int64_t)path * L;
            if (kind == 0) set_error("dg_dp_score_paths: pair %lld path %d level %d: vertex %d is not in that level", (long long)pair, path, level, pp[level]);
            else set_error("dg_dp_score_paths: pair %lld path %d level %d: no edge %d -> %d", (long long)pair, path, level, pp[level - 1], pp[level]);
            return DG_ERR_ARG;
        }
    }
    memcpy(out, res.data(), (size_t)n_pairs * sizeof(dg_dp_pair_score));
    return DG_OK;
}

}  // namespace dgi

extern "C" int dg_dp_score_paths(dg_ctx *c, const int32_t *paths, int64_t n_pairs, dg_dp_pair_score *out) {
    if (int rc = dgi::bind(c)) return rc;
    return dgi::dp_score_paths(c, paths, n_pairs, out);
}

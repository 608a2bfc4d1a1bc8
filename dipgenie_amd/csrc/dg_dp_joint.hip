// dg_dp_genotype_margins: the max-marginals of the diploid DP with BOTH haplotypes free -- for every cell (i, j) of every level the
// best value of any ordered pair of source -> sink paths (p, q) with p[l] = i, q[l] = j and r(p) + r(q) <= budget, and per level and
// query the called cell's value against the best cell of another genotype.  Notation: d(u1, u2 -> v1, v2) = inter + symd of the
// transition, what the sweep adds (one T x T uint16 matrix per coloured transition, indexed by the ranks of the two in-edges).
//   forward   F_0[src, src][r] = 0; F_l[i][j][r] = max over the in-edge pairs (u -> i, w1), (v -> j, w2) with r - w1 - w2 >= 0 and a
//             reachable source cell of F_{l-1}[u][v][r - w1 - w2] + d; NEG_INF where there is none (the sweep's values);
//   backward  B_{L-1}[sink, sink][r] = 0; B_l[i][j][r] = max over the out-edge pairs (i -> i', w1), (j -> j', w2) with
//             r - w1 - w2 >= 0 and a reachable destination cell of d + B_{l+1}[i'][j'][r - w1 - w2];
//   through   T_l[i][j] = max over r = 0..b with both cells reachable of F_l[i][j][r] + B_l[i][j][b - r]; J[v] = max_j T_l[v][j].
// Both tables mean "at most r", so a pair that spends r1 up to the level and r2 after it is counted at r = r1 whenever r1 + r2 <= b.
// A level's state is int32 [i][j][r], r fastest, in device memory.  Every kernel is a gather: each cell is written once by one
// lane, no output is an atomic, and nothing depends on the order in which lanes or workgroups run:
//   * jt_scores_kernel: the T x T score matrix of one transition into a buffer of the call (the run's own window of matrices,
//     DpState::d_delta / cur_win, is neither read nor written); the pairs with at most one coloured edge are answered from the edge
//     flags and single-edge scores that dg_dp_load_graph leaves (read only), the others by the merges of dg_dp_setops.hpp;
//   * jt_forward_kernel: one lane per (i, j, r) of the destination level, looping over in(i) x in(j);
//   * jt_out_*: the device holds the in-CSR only, so once per call the in-edges are grouped by their source vertex (count, scan,
//     fill: a counting sort; the order inside a group is the order the lanes arrive in, and a maximum does not depend on it);
//   * jt_backward_kernel: one lane per (i, j, r) of level l, looping over out(i) x out(j) into level l + 1;
//   * jt_combine_kernel: one workgroup per row i forms T[i][.] over r, its maximum J, and per query the best cell (i, j >= i) of
//     another genotype than the called one as a key (value desc, i asc, j asc); T is symmetric, so the cells with j >= i are all of
//     them and the alternative comes out with alt_vertex1 <= alt_vertex2;
//   * jt_records_kernel: one workgroup per query reduces the rows' keys to the level's record, workgroup 0 the rows' maxima to
//     the level maximum (the closing check: it must be V_b on every level).
// One launch per level and pass: the kernel boundary orders the levels.  No cooperative launch, no grid barrier, no spinning.
// Memory: F of all levels is 4 * sum k^2 (b + 1) bytes, so the call keeps F only at the first level of each segment (option
// joint_state_bytes bounds the forward states of one segment; a segment holds at least one level) in a first forward pass, then
// visits the segments from the last to the first: the forward states of the segment's levels are recomputed and kept, the backward
// recurrence walks the segment with two rolling states, combination and records run per level.  With one segment the first pass
// has nothing to do.  Every buffer is reserved inside the call and freed when it returns; nothing of a run is read or written.
// dg_dp_genotype_table is the same pass with one more step per level: the combine kernel gets one scratch row per row of the level, so
// T of the level is whole, and the gt_* kernels below reduce it by genotype into a compacted list (their comment has the plan).
// dg_dp_genotype_margins launches none of them and reserves none of their buffers.
// dg_dp_genotype_margins_pinned / dg_dp_genotype_table_pinned are the same pass on the DP that per-level cell constraints leave (the pins
// of dg_dp_run_pinned): after every launch that writes a forward or backward state of a pinned level, jt_pin_mask_kernel
// (dg_dp_pins.hip) stores NEG_INF over the level's cells that are not allowed, and the recurrences, which skip a NEG_INF source cell,
// do the rest.  Pins are ordered, so T is no longer symmetric: the pinned calls run the ORDERED instantiations of jt_combine_kernel and
// gt_rows_kernel, which give the unordered cell (i, j >= i) the value max(T[i][j], T[j][i]); n_pins = 0 runs what the unpinned calls run.
// dg_dp_genotype_margins_budgets answers every query at a budget of its own from the same pass run once at the largest budget: the
// recurrences, score matrices and masks are launched once, jt_combine_budgets_kernel / jt_records_budgets_kernel (their comment has the
// plan) take the places of jt_combine_kernel / jt_records_kernel.  The other entry points launch neither and reserve none of their buffers.
// dg_dp_phase_margins (ph_call and the ph_* kernels, below jt_call: their comment has the plan) is the same schedule with a second rolling
// backward state, seeded at every het level of the called pair; it launches none of the combination, record or table kernels.
// dg_dp_phase_margins_budgets (phb_call and the phb_* kernels, below ph_call: their comment has the plan) is that schedule once at the
// largest budget for many called pairs, with a pool of seeded states, one per live seed key, planned on the host before the first launch.
// dg_dp_recombination_margins (rb_call and the rb_* kernels, below phb_call: their comment has the plan) is jt_call's schedule with one more
// gather per level in place of the combination and record kernels: per transition l -> l + 1 the best F_l + d + B_{l+1} over the hop pairs
// the backward kernel walks, bucketed by the number of weight-1 hops in the pair, with the hop pair that attains it, and per called pair what
// its own two hops are worth.  It launches none of the combination, record, table or phase kernels and reserves none of their buffers.  Out of
// scope there: a pinned form, more than one GPU, windows of several transitions.
// dg_dp_recombination_margins_budgets (rbb_call and the rb_*_budgets kernels, below rb_call: their comment has the plan) is that schedule
// once at the largest budget for queries with a budget each: the two gathers get one more grid dimension over the distinct budgets and
// pair the planes of the one pass per budget.  rb_call and its kernels are launched by the one-budget call alone, these by this one.
#include <algorithm>
#include <cstring>
#include <functional>
#include <map>

#include "dg_dp_setops.hpp"

namespace dgi {

namespace {

constexpr int JT_THREADS = 256;
constexpr int JT_MAX_K = 32767;                         // widest level: a cell's two positions take 15 bits each in the tie key
constexpr int JT_MAX_PLANES = 4096;                     // budget + 1
constexpr int JT_MAX_QUERIES = 256;                     // called genotypes per call (the combine kernel loops over them)
constexpr int JT_ROW_BLOCKS = 2048;                     // workgroups of the combine kernel (each owns one scratch row of T)
constexpr int JT_X_BLOCKS = 4096;                       // workgroups per row of the recurrences (the lanes stride beyond)
constexpr long long JT_NO_KEY = INT64_MIN;              // no cell (every key of a cell is larger: its value is >= 0)

// value descending, then i ascending, then j ascending (positions inside the level, both <= 32766)
__device__ __forceinline__ long long jt_key(int value, int i, int j) {
    return (long long)(((unsigned long long)(uint32_t)value << 32) | ((uint32_t)(JT_MAX_K - i) << 15) | (uint32_t)(JT_MAX_K - j));
}

// n cells of NEG_INF but for [hot, hot + planes): 0 (level 0: the source's cell; level L - 1: the sink's)
__global__ __launch_bounds__(JT_THREADS) void jt_fill_kernel(int32_t *__restrict__ st, int64_t n, int64_t hot, int planes) {
    for (int64_t x = (int64_t)blockIdx.x * JT_THREADS + threadIdx.x; x < n; x += (int64_t)gridDim.x * JT_THREADS) st[x] = (x >= hot && x < hot + planes) ? 0 : NEG_INF;
}

// out[eu * T + ev] for the transition whose T in-edges start at in_base and whose source level starts at vertex a0
__global__ __launch_bounds__(JT_THREADS) void jt_scores_kernel(int T, uint32_t in_base, int a0, const uint32_t *__restrict__ in_edge, const int32_t *__restrict__ in_dst,
                                                               ColourCsr col, const uint8_t *__restrict__ eflags, const uint16_t *__restrict__ eself,
                                                               uint16_t *__restrict__ out) {
    for (int eu = (int)blockIdx.y; eu < T; eu += (int)gridDim.y) {
        const uint32_t fu = eflags[in_base + eu];
        for (int ev = (int)(blockIdx.x * JT_THREADS + threadIdx.x); ev < T; ev += (int)(gridDim.x * JT_THREADS)) {
            const uint32_t fv = eflags[in_base + ev];
            int sc = 0;
            if ((fu | fv) == 0u) sc = 0;                                    // no colour on either edge
            else if (fv == 0u) sc = eself[in_base + eu];                    // one coloured edge: its own score
            else if (fu == 0u) sc = eself[in_base + ev];
            else {
                const int u1 = a0 + (int)(in_edge[in_base + eu] & 0x7FFFFFFFu), v1 = a0 + (int)(in_edge[in_base + ev] & 0x7FFFFFFFu);
                const int u2 = in_dst[in_base + eu], v2 = in_dst[in_base + ev];
                if (((fu | fv) & 3u) == 3u) sc += score_inter(col, u1, v1, u2, v2);
                if (((fu | fv) & 12u) != 0u) sc += score_symd(col, u1, v1, u2, v2);
            }
            out[(int64_t)eu * T + ev] = (uint16_t)sc;
        }
    }
}

// grid (x blocks, k): row i = blockIdx.y, the lanes stride over (j, r).  prev = level l - 1 [kprev][kprev][B1], cur = level l [k][k][B1];
// b0 = first vertex of level l, in_base / T = its in-edges; sc = its T x T scores, null: all zero
__global__ __launch_bounds__(JT_THREADS) void jt_forward_kernel(const int32_t *__restrict__ prev, int32_t *__restrict__ cur, int kprev, int k, int B1, int b0,
                                                                uint32_t in_base, int T, const uint32_t *__restrict__ in_off, const uint32_t *__restrict__ in_edge,
                                                                const uint16_t *__restrict__ sc) {
    const int i = (int)blockIdx.y;
    const uint32_t eu0 = in_off[b0 + i], eu1 = in_off[b0 + i + 1];
    const int n = k * B1;
    for (int x = (int)(blockIdx.x * JT_THREADS + threadIdx.x); x < n; x += (int)(gridDim.x * JT_THREADS)) {
        const int j = x / B1, r = x - j * B1;
        const uint32_t ev0 = in_off[b0 + j], ev1 = in_off[b0 + j + 1];
        int best = NEG_INF;
        for (uint32_t eu = eu0; eu < eu1; ++eu) {
            const uint32_t ru = in_edge[eu];
            const uint32_t pu = ru & 0x7FFFFFFFu;
            const int r1 = r - (int)(ru >> 31);
            if (pu >= (uint32_t)kprev || r1 < 0 || eu - in_base >= (uint32_t)T) continue;
            for (uint32_t ev = ev0; ev < ev1; ++ev) {
                const uint32_t rv = in_edge[ev];
                const uint32_t pv = rv & 0x7FFFFFFFu;
                const int r2 = r1 - (int)(rv >> 31);
                if (pv >= (uint32_t)kprev || r2 < 0 || ev - in_base >= (uint32_t)T) continue;
                const int s = prev[((int64_t)pu * kprev + pv) * B1 + r2];
                if (s == NEG_INF) continue;
                const int d = sc ? (int)sc[(int64_t)(eu - in_base) * T + (ev - in_base)] : 0;
                best = max(best, s + d);
            }
        }
        cur[((int64_t)i * k + j) * B1 + r] = best;
    }
}

// ---- the in-edges grouped by source vertex: cnt[v] = out-edges of v, then off = their exclusive scan, then oe[off[v] ..) = the in-edge
// indices.  One workgroup per destination level l = blockIdx.x + 1 for count and fill ----
__global__ __launch_bounds__(JT_THREADS) void jt_out_count_kernel(const LevelDesc *__restrict__ descs, int L, int nV, const uint32_t *__restrict__ in_edge,
                                                                  uint32_t *__restrict__ cnt) {
    const int l = (int)blockIdx.x + 1;
    if (l >= L) return;
    const LevelDesc d = descs[l];
    for (int e = (int)threadIdx.x; e < d.T; e += JT_THREADS) {
        const uint32_t pos = in_edge[d.in_base + e] & 0x7FFFFFFFu;
        if (pos < (uint32_t)d.k && (uint32_t)d.a0 + pos < (uint32_t)nV) atomicAdd(&cnt[d.a0 + (int)pos], 1u);
    }
}

// one workgroup: off[v] = sum of cnt[0 .. v), off[nV] = the total; cur (may be cnt itself) = a copy of off[0 .. nV) for the fill
__global__ __launch_bounds__(1024) void jt_out_scan_kernel(const uint32_t *cnt, uint32_t *__restrict__ off, uint32_t *cur, int nV) {
    __shared__ uint32_t s[1024];
    const int t = (int)threadIdx.x;
    uint32_t carry = 0;
    for (int base = 0; base < nV; base += 1024) {
        const int v = base + t;
        const uint32_t x = v < nV ? cnt[v] : 0u;
        s[t] = x;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {
            const uint32_t y = t >= d ? s[t - d] : 0u;
            __syncthreads();
            s[t] += y;
            __syncthreads();
        }
        const uint32_t excl = carry + s[t] - x;
        if (v < nV) { off[v] = excl; cur[v] = excl; }
        carry += s[1023];
        __syncthreads();
    }
    if (t == 0) off[nV] = carry;
}

__global__ __launch_bounds__(JT_THREADS) void jt_out_fill_kernel(const LevelDesc *__restrict__ descs, int L, int nV, const uint32_t *__restrict__ in_edge,
                                                                 uint32_t *__restrict__ cur, uint32_t *__restrict__ oe, uint32_t n_edges) {
    const int l = (int)blockIdx.x + 1;
    if (l >= L) return;
    const LevelDesc d = descs[l];
    for (int e = (int)threadIdx.x; e < d.T; e += JT_THREADS) {
        const uint32_t pos = in_edge[d.in_base + e] & 0x7FFFFFFFu;
        if (pos < (uint32_t)d.k && (uint32_t)d.a0 + pos < (uint32_t)nV) {
            const uint32_t at = atomicAdd(&cur[d.a0 + (int)pos], 1u);
            if (at < n_edges) oe[at] = d.in_base + (uint32_t)e;
        }
    }
}

// grid (x blocks, k): row i = blockIdx.y.  next = level l + 1 [kn][kn][B1], cur = level l [k][k][B1]; a0 = first vertex of level l, b0n = first
// vertex of level l + 1, in_base / T = the in-edges of level l + 1, sc = their scores (null: all zero); oo / oe = the out-index
__global__ __launch_bounds__(JT_THREADS) void jt_backward_kernel(const int32_t *__restrict__ next, int32_t *__restrict__ cur, int k, int kn, int B1, int a0, int b0n,
                                                                 uint32_t in_base, int T, const uint32_t *__restrict__ oo, const uint32_t *__restrict__ oe,
                                                                 const uint32_t *__restrict__ in_edge, const int32_t *__restrict__ in_dst,
                                                                 const uint16_t *__restrict__ sc) {
    const int i = (int)blockIdx.y;
    const uint32_t ou0 = oo[a0 + i], ou1 = oo[a0 + i + 1];
    const int n = k * B1;
    for (int x = (int)(blockIdx.x * JT_THREADS + threadIdx.x); x < n; x += (int)(gridDim.x * JT_THREADS)) {
        const int j = x / B1, r = x - j * B1;
        const uint32_t ov0 = oo[a0 + j], ov1 = oo[a0 + j + 1];
        int best = NEG_INF;
        for (uint32_t ou = ou0; ou < ou1; ++ou) {
            const uint32_t eu = oe[ou] - in_base;                           // rank among the in-edges of level l + 1
            if (eu >= (uint32_t)T) continue;
            const uint32_t pi = (uint32_t)(in_dst[in_base + eu] - b0n);
            const int r1 = r - (int)(in_edge[in_base + eu] >> 31);
            if (pi >= (uint32_t)kn || r1 < 0) continue;
            for (uint32_t ov = ov0; ov < ov1; ++ov) {
                const uint32_t ev = oe[ov] - in_base;
                if (ev >= (uint32_t)T) continue;
                const uint32_t pj = (uint32_t)(in_dst[in_base + ev] - b0n);
                const int r2 = r1 - (int)(in_edge[in_base + ev] >> 31);
                if (pj >= (uint32_t)kn || r2 < 0) continue;
                const int s = next[((int64_t)pi * kn + pj) * B1 + r2];
                if (s == NEG_INF) continue;
                const int d = sc ? (int)sc[(int64_t)eu * T + ev] : 0;
                best = max(best, s + d);
            }
        }
        cur[((int64_t)i * k + j) * B1 + r] = best;
    }
}

// grid: min(k, JT_ROW_BLOCKS) workgroups, rows strided.  F, B = the two states of level l; row = [gridDim.x][k] scratch; J = [nV];
// called = [n][2][L] vertex ids (validated by the host); cls = [nV] or null; part = [n][k] keys; cval = [n].
// ORDERED (a pinned call: T need not be symmetric): a second scratch row per workgroup, behind the gridDim.x first ones, takes the
// column T[.][i], and the key of the unordered cell (i, j >= i) holds max(T[i][j], T[j][i]); J and the called cell's value stay those
// of the ordered row.  ORDERED = false is the kernel as it was: no load, store or branch more.
template <bool ORDERED>
__global__ __launch_bounds__(JT_THREADS) void jt_combine_kernel(const int32_t *__restrict__ F, const int32_t *__restrict__ B, int k, int B1, int b0, int32_t *row_all,
                                                                int32_t *__restrict__ J, int n, const int32_t *__restrict__ called, int L, int l,
                                                                const int32_t *__restrict__ cls, long long *__restrict__ part, int32_t *__restrict__ cval) {
    __shared__ long long s_key[JT_MAX_QUERIES][JT_THREADS / 64];
    __shared__ int s_max[JT_THREADS / 64];
    const int t = (int)threadIdx.x;
    int32_t *row = row_all + (int64_t)blockIdx.x * k;
    int32_t *col = ORDERED ? row_all + ((int64_t)gridDim.x + blockIdx.x) * k : nullptr;
    for (int i = (int)blockIdx.x; i < k; i += (int)gridDim.x) {
        int m = NEG_INF;
        for (int j = t; j < k; j += JT_THREADS) {
            const int32_t *f = F + ((int64_t)i * k + j) * B1, *b = B + ((int64_t)i * k + j) * B1;
            int best = NEG_INF;
            for (int r = 0; r < B1; ++r) {
                const int fv = f[r], bv = b[B1 - 1 - r];
                if (fv != NEG_INF && bv != NEG_INF) best = max(best, fv + bv);
            }
            row[j] = best;
            m = max(m, best);
            if (ORDERED && j >= i) {
                const int32_t *f2 = F + ((int64_t)j * k + i) * B1, *b2 = B + ((int64_t)j * k + i) * B1;
                int other = NEG_INF;
                for (int r = 0; r < B1; ++r) {
                    const int fv = f2[r], bv = b2[B1 - 1 - r];
                    if (fv != NEG_INF && bv != NEG_INF) other = max(other, fv + bv);
                }
                col[j] = other;
            }
        }
        for (int d = 32; d; d >>= 1) m = max(m, __shfl_xor(m, d));
        if ((t & 63) == 0) s_max[t >> 6] = m;
        __syncthreads();                                                    // the row and the waves' maxima are in
        if (t == 0) {
            for (int w = 1; w < JT_THREADS / 64; ++w) m = max(m, s_max[w]);
            J[b0 + i] = m;
        }
        const int ci = cls ? cls[b0 + i] : b0 + i;
        for (int q = 0; q < n; ++q) {
            const int c1 = called[((int64_t)q * 2) * L + l], c2 = called[((int64_t)q * 2 + 1) * L + l];
            const int cc1 = cls ? cls[c1] : c1, cc2 = cls ? cls[c2] : c2;
            if (t == 0 && i == c1 - b0) cval[q] = row[c2 - b0];
            long long key = JT_NO_KEY;
            for (int j = i + t; j < k; j += JT_THREADS) {
                const int v = ORDERED ? max(row[j], col[j]) : row[j];
                if (v == NEG_INF) continue;
                const int cj = cls ? cls[b0 + j] : b0 + j;
                if ((ci == cc1 && cj == cc2) || (ci == cc2 && cj == cc1)) continue;      // the called genotype itself
                key = max(key, jt_key(v, i, j));
            }
            for (int d = 32; d; d >>= 1) key = max(key, __shfl_xor(key, d));
            if ((t & 63) == 0) s_key[q][t >> 6] = key;
        }
        __syncthreads();
        for (int q = t; q < n; q += JT_THREADS) {
            long long key = s_key[q][0];
            for (int w = 1; w < JT_THREADS / 64; ++w) key = max(key, s_key[q][w]);
            part[(int64_t)q * k + i] = key;
        }
        __syncthreads();                                                    // the next row overwrites the scratch row and the keys
    }
}

// grid: n workgroups.  Query q: the largest of its k row keys -> rec[q][l]; workgroup 0 also the level's maximum of J -> lvlmax[l]
__global__ __launch_bounds__(JT_THREADS) void jt_records_kernel(int k, int b0, const int32_t *__restrict__ J, const long long *__restrict__ part,
                                                                const int32_t *__restrict__ cval, const int32_t *__restrict__ called, int L, int l,
                                                                dg_dp_genotype_margin *__restrict__ rec, int32_t *__restrict__ lvlmax) {
    __shared__ long long s_key[JT_THREADS / 64];
    __shared__ int s_max[JT_THREADS / 64];
    const int t = (int)threadIdx.x, q = (int)blockIdx.x;
    long long key = JT_NO_KEY;
    int m = NEG_INF;
    for (int i = t; i < k; i += JT_THREADS) {
        key = max(key, part[(int64_t)q * k + i]);
        if (q == 0) m = max(m, J[b0 + i]);
    }
    for (int d = 32; d; d >>= 1) { key = max(key, __shfl_xor(key, d)); m = max(m, __shfl_xor(m, d)); }
    if ((t & 63) == 0) { s_key[t >> 6] = key; s_max[t >> 6] = m; }
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < JT_THREADS / 64; ++w) { key = max(key, s_key[w]); m = max(m, s_max[w]); }
        dg_dp_genotype_margin r;
        r.vertex1 = called[((int64_t)q * 2) * L + l];
        r.vertex2 = called[((int64_t)q * 2 + 1) * L + l];
        r.value = cval[q];
        if (key == JT_NO_KEY) { r.alt_vertex1 = -1; r.alt_vertex2 = -1; r.alt_value = NEG_INF; }
        else {
            const uint32_t lo = (uint32_t)key;
            r.alt_vertex1 = b0 + (JT_MAX_K - (int)((lo >> 15) & 0x7FFFu));
            r.alt_vertex2 = b0 + (JT_MAX_K - (int)(lo & 0x7FFFu));
            r.alt_value = (int)(key >> 32);
        }
        r.reserved[0] = 0; r.reserved[1] = 0;
        rec[(int64_t)q * L + l] = r;
        if (q == 0) lvlmax[l] = m;
    }
}

// ---- dg_dp_genotype_margins_budgets: the states are "at most r" planes, so F and B at B1 = bmax + 1 hold T^b for every b <= bmax:
// T^b[i][j] = max over r = 0..b of F[i][j][r] + B[i][j][b - r].  Siblings of the two kernels above with one more grid dimension:
//   * jt_combine_budgets_kernel: grid (row blocks, distinct budgets).  Workgroup (x, d) forms the rows of T^bud[d] in a scratch row of its
//     own, their maxima into Jb[d][.], and the keys of the queries of that budget only (qlist[qoff[d] .. qoff[d + 1])): part[q][i] and
//     cval[q] have one owner as before, since a query has one budget.  f / b of a cell are read once per distinct budget, by different
//     workgroups of the same launch: the repeats are served by the L2, and a narrow level gets nd times the workgroups it had;
//   * jt_records_budgets_kernel: one workgroup per query; the first query of each budget also reduces Jb[d][.] to lvlmax[d][l].
// bud[d] < B1 (the host sorts the distinct budgets, the largest is B1 - 1); Jb = [nd][kstride].
template <bool ORDERED>
__global__ __launch_bounds__(JT_THREADS) void jt_combine_budgets_kernel(const int32_t *__restrict__ F, const int32_t *__restrict__ B, int k, int B1, int b0, int32_t *row_all,
                                                                        int32_t *__restrict__ Jb, int kstride, const int32_t *__restrict__ bud, const int32_t *__restrict__ qoff,
                                                                        const int32_t *__restrict__ qlist, const int32_t *__restrict__ called, int L, int l,
                                                                        const int32_t *__restrict__ cls, long long *__restrict__ part, int32_t *__restrict__ cval) {
    __shared__ long long s_key[JT_MAX_QUERIES][JT_THREADS / 64];
    __shared__ int s_max[JT_THREADS / 64];
    const int t = (int)threadIdx.x, d = (int)blockIdx.y;
    const int bb = min(bud[d], B1 - 1);
    const int q0 = qoff[d], nq = min(qoff[d + 1] - q0, JT_MAX_QUERIES);
    const int64_t slot = (int64_t)blockIdx.y * gridDim.x + blockIdx.x, slots = (int64_t)gridDim.x * gridDim.y;
    int32_t *row = row_all + slot * k;
    int32_t *col = ORDERED ? row_all + (slots + slot) * k : nullptr;
    for (int i = (int)blockIdx.x; i < k; i += (int)gridDim.x) {
        int m = NEG_INF;
        for (int j = t; j < k; j += JT_THREADS) {
            const int32_t *f = F + ((int64_t)i * k + j) * B1, *b = B + ((int64_t)i * k + j) * B1;
            int best = NEG_INF;
            for (int r = 0; r <= bb; ++r) {
                const int fv = f[r], bv = b[bb - r];
                if (fv != NEG_INF && bv != NEG_INF) best = max(best, fv + bv);
            }
            row[j] = best;
            m = max(m, best);
            if (ORDERED && j >= i) {
                const int32_t *f2 = F + ((int64_t)j * k + i) * B1, *b2 = B + ((int64_t)j * k + i) * B1;
                int other = NEG_INF;
                for (int r = 0; r <= bb; ++r) {
                    const int fv = f2[r], bv = b2[bb - r];
                    if (fv != NEG_INF && bv != NEG_INF) other = max(other, fv + bv);
                }
                col[j] = other;
            }
        }
        for (int w = 32; w; w >>= 1) m = max(m, __shfl_xor(m, w));
        if ((t & 63) == 0) s_max[t >> 6] = m;
        __syncthreads();                                                    // the row and the waves' maxima are in
        if (t == 0) {
            for (int w = 1; w < JT_THREADS / 64; ++w) m = max(m, s_max[w]);
            Jb[(int64_t)d * kstride + i] = m;
        }
        const int ci = cls ? cls[b0 + i] : b0 + i;
        for (int x = 0; x < nq; ++x) {
            const int q = qlist[q0 + x];
            const int c1 = called[((int64_t)q * 2) * L + l], c2 = called[((int64_t)q * 2 + 1) * L + l];
            const int cc1 = cls ? cls[c1] : c1, cc2 = cls ? cls[c2] : c2;
            if (t == 0 && i == c1 - b0) cval[q] = row[c2 - b0];
            long long key = JT_NO_KEY;
            for (int j = i + t; j < k; j += JT_THREADS) {
                const int v = ORDERED ? max(row[j], col[j]) : row[j];
                if (v == NEG_INF) continue;
                const int cj = cls ? cls[b0 + j] : b0 + j;
                if ((ci == cc1 && cj == cc2) || (ci == cc2 && cj == cc1)) continue;      // the called genotype itself
                key = max(key, jt_key(v, i, j));
            }
            for (int w = 32; w; w >>= 1) key = max(key, __shfl_xor(key, w));
            if ((t & 63) == 0) s_key[x][t >> 6] = key;
        }
        __syncthreads();
        for (int x = t; x < nq; x += JT_THREADS) {
            long long key = s_key[x][0];
            for (int w = 1; w < JT_THREADS / 64; ++w) key = max(key, s_key[x][w]);
            part[(int64_t)qlist[q0 + x] * k + i] = key;
        }
        __syncthreads();                                                    // the next row overwrites the scratch row and the keys
    }
}

// grid: n workgroups.  Query q of budget index d = qd[q]: the largest of its k row keys -> rec[q][l]; the first query of d also the
// maximum of Jb[d][.] -> lvlmax[d][l]
__global__ __launch_bounds__(JT_THREADS) void jt_records_budgets_kernel(int k, int b0, const int32_t *__restrict__ Jb, int kstride, const int32_t *__restrict__ qd,
                                                                        const int32_t *__restrict__ qoff, const int32_t *__restrict__ qlist, const long long *__restrict__ part,
                                                                        const int32_t *__restrict__ cval, const int32_t *__restrict__ called, int L, int l,
                                                                        dg_dp_genotype_margin *__restrict__ rec, int32_t *__restrict__ lvlmax) {
    __shared__ long long s_key[JT_THREADS / 64];
    __shared__ int s_max[JT_THREADS / 64];
    const int t = (int)threadIdx.x, q = (int)blockIdx.x;
    const int d = qd[q];
    const bool lead = qlist[qoff[d]] == q;                                  // uniform per workgroup
    long long key = JT_NO_KEY;
    int m = NEG_INF;
    for (int i = t; i < k; i += JT_THREADS) {
        key = max(key, part[(int64_t)q * k + i]);
        if (lead) m = max(m, Jb[(int64_t)d * kstride + i]);
    }
    for (int w = 32; w; w >>= 1) { key = max(key, __shfl_xor(key, w)); m = max(m, __shfl_xor(m, w)); }
    if ((t & 63) == 0) { s_key[t >> 6] = key; s_max[t >> 6] = m; }
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < JT_THREADS / 64; ++w) { key = max(key, s_key[w]); m = max(m, s_max[w]); }
        dg_dp_genotype_margin r;
        r.vertex1 = called[((int64_t)q * 2) * L + l];
        r.vertex2 = called[((int64_t)q * 2 + 1) * L + l];
        r.value = cval[q];
        if (key == JT_NO_KEY) { r.alt_vertex1 = -1; r.alt_vertex2 = -1; r.alt_value = NEG_INF; }
        else {
            const uint32_t lo = (uint32_t)key;
            r.alt_vertex1 = b0 + (JT_MAX_K - (int)((lo >> 15) & 0x7FFFu));
            r.alt_vertex2 = b0 + (JT_MAX_K - (int)(lo & 0x7FFFu));
            r.alt_value = (int)(key >> 32);
        }
        r.reserved[0] = 0; r.reserved[1] = 0;
        rec[(int64_t)q * L + l] = r;
        if (lead) lvlmax[(int64_t)d * L + l] = m;
    }
}

// ---- dg_dp_genotype_table: a level's through-values reduced by genotype.  The call runs the combine kernel with one scratch row per
// row of the level, so T[k][k] of the level is whole when these run.  rank[v] = dense rank of v's class among the classes of its level
// (ascending, signed), perm = the level's positions ordered by (rank, position), goff[a] .. goff[a + 1] = the slice of perm with rank a
// (host-built, A + 1 offsets).  All gathers: every word has one owner.
//   * gt_rows_kernel: one wave per row i walks the row in perm order, 64 cells at a time: a segmented max-scan over the runs of equal
//     rank, the run's key so far carried from chunk to chunk; the lane at the end of a run writes part[i][a'] (every rank has a cell, so
//     every word of part is written);
//   * gt_pairs_kernel: 2^lp lanes per genotype (a <= a') take the maximum of part[i][a'] over the rows i of rank a -- T is symmetric and
//     the key holds (min, max), so this covers both orders of a cell -- into the dense triangle, row a at a * A - a (a - 1) / 2;
//   * gt_count_kernel / gt_scan_kernel / gt_scatter_kernel: the reachable genotypes of the triangle, in its order (ascending
//     (class1, class2)), go to the staging behind the levels before: per tile of 256 * items keys the count and the largest value, one
//     workgroup scans the tiles, blockDim.x of them per pass with a carry, and moves the call's cursor, the tiles write their entries.
constexpr int GT_MAX_ITEMS = 8;                         // most keys per lane of a tile (contiguous, so a tile's entries stay in order): option genotype_table_tile_keys / 256
constexpr int GT_MAX_SCAN = 1024;                       // most lanes of the scan's workgroup = tiles per pass: option genotype_table_scan_tiles

// ORDERED (a pinned call: T need not be symmetric): the unordered cell's value is max(T[i][j], T[j][i]), so what the later steps see is
// symmetric again; ORDERED = false is the kernel as it was.
template <bool ORDERED>
__global__ __launch_bounds__(JT_THREADS) void gt_rows_kernel(const int32_t *__restrict__ T, int k, int A, const int32_t *__restrict__ rank, const int32_t *__restrict__ perm,
                                                             long long *__restrict__ part) {
    const int lane = (int)threadIdx.x & 63;
    const int waves = (int)gridDim.x * (JT_THREADS / 64);
    for (int i = (int)blockIdx.x * (JT_THREADS / 64) + ((int)threadIdx.x >> 6); i < k; i += waves) {      // uniform per wave
        long long carry = JT_NO_KEY;
        int carry_c = -1;
        for (int base = 0; base < k; base += 64) {
            const int x = base + lane;
            int c = A;                                                      // beyond the row: a rank nobody has
            long long key = JT_NO_KEY;
            if (x < k) {
                const uint32_t j = (uint32_t)perm[x];
                if (j < (uint32_t)k) {
                    c = rank[j];
                    const int v = ORDERED ? max(T[(int64_t)i * k + j], T[(int64_t)j * k + i]) : T[(int64_t)i * k + j];
                    if (v != NEG_INF) key = jt_key(v, min(i, (int)j), max(i, (int)j));
                }
            }
            int cn = __shfl_down(c, 1);
            if (lane == 63) {
                cn = -1;
                if (x + 1 < k) { const uint32_t j = (uint32_t)perm[x + 1]; cn = j < (uint32_t)k ? rank[j] : A; }
            }
            if (lane == 0 && c == carry_c) key = max(key, carry);
            for (int d = 1; d < 64; d <<= 1) {
                const long long ok = __shfl_up(key, d);
                const int oc = __shfl_up(c, d);
                if (lane >= d && oc == c) key = max(key, ok);
            }
            if (cn != c && (uint32_t)c < (uint32_t)A) part[(int64_t)i * A + c] = key;
            carry = __shfl(key, 63);
            carry_c = __shfl(c, 63);
        }
    }
}

// grid (x, y): rank a = blockIdx.y (strided), the lanes of x cover a' = a .. A - 1, 1 << lp of them each
__global__ __launch_bounds__(JT_THREADS) void gt_pairs_kernel(const long long *__restrict__ part, int k, int A, const int32_t *__restrict__ perm, const int32_t *__restrict__ goff,
                                                              int lp, long long *__restrict__ dense) {
    const int sub = (int)threadIdx.x & ((1 << lp) - 1);
    for (int a = (int)blockIdx.y; a < A; a += (int)gridDim.y) {
        const int x0 = goff[a], x1 = min(goff[a + 1], k);
        const int64_t row0 = (int64_t)a * A - (int64_t)a * (a - 1) / 2, lanes = (int64_t)(A - a) << lp;
        for (int64_t t0 = (int64_t)blockIdx.x * JT_THREADS; t0 < lanes; t0 += (int64_t)gridDim.x * JT_THREADS) {      // uniform per workgroup
            const int g = (int)((t0 + threadIdx.x) >> lp);
            long long key = JT_NO_KEY;
            if (g < A - a && x0 >= 0)
                for (int x = x0 + sub; x < x1; x += 1 << lp) {
                    const uint32_t i = (uint32_t)perm[x];
                    if (i < (uint32_t)k) key = max(key, part[(int64_t)i * A + a + g]);
                }
            for (int d = (1 << lp) >> 1; d; d >>= 1) key = max(key, __shfl_xor(key, d));
            if (g < A - a && sub == 0) dense[row0 + g] = key;
        }
    }
}

// one workgroup per tile: cnt[tile] = its reachable genotypes, tmax[tile] = their largest value
__global__ __launch_bounds__(JT_THREADS) void gt_count_kernel(const long long *__restrict__ dense, int64_t n, int items, uint32_t *__restrict__ cnt, int32_t *__restrict__ tmax) {
    __shared__ uint32_t s_n[JT_THREADS / 64];
    __shared__ int s_m[JT_THREADS / 64];
    const int t = (int)threadIdx.x;
    const int64_t first = ((int64_t)blockIdx.x * JT_THREADS + t) * items;
    uint32_t c = 0;
    int m = NEG_INF;
    for (int q = 0; q < items; ++q)
        if (first + q < n) {
            const long long key = dense[first + q];
            if (key != JT_NO_KEY) { ++c; m = max(m, (int)(key >> 32)); }
        }
    for (int d = 32; d; d >>= 1) { c += __shfl_xor(c, d); m = max(m, __shfl_xor(m, d)); }
    if ((t & 63) == 0) { s_n[t >> 6] = c; s_m[t >> 6] = m; }
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < JT_THREADS / 64; ++w) { c += s_n[w]; m = max(m, s_m[w]); }
        cnt[blockIdx.x] = c;
        tmax[blockIdx.x] = m;
    }
}

// one workgroup: cnt[0 .. nt) becomes its exclusive scan; the level's entries start at *cursor, which moves on by their number.
// out = the level's three words: first entry in the staging, entries, largest value
__global__ __launch_bounds__(GT_MAX_SCAN) void gt_scan_kernel(uint32_t *cnt, const int32_t *__restrict__ tmax, int64_t nt, long long *cursor, long long *__restrict__ out) {
    __shared__ uint32_t s[GT_MAX_SCAN];
    __shared__ int s_m[GT_MAX_SCAN / 64];
    const int t = (int)threadIdx.x, W = (int)blockDim.x;                    // W: a multiple of 64, at most GT_MAX_SCAN
    long long carry = 0;
    int m = NEG_INF;
    for (int64_t base = 0; base < nt; base += W) {
        const int64_t b = base + t;
        const uint32_t x = b < nt ? cnt[b] : 0u;
        if (b < nt) m = max(m, tmax[b]);
        s[t] = x;
        __syncthreads();
        for (int d = 1; d < W; d <<= 1) {
            const uint32_t y = t >= d ? s[t - d] : 0u;
            __syncthreads();
            s[t] += y;
            __syncthreads();
        }
        if (b < nt) cnt[b] = (uint32_t)(carry + s[t] - x);                  // a level has fewer than 2^30 genotypes
        carry += s[W - 1];
        __syncthreads();
    }
    for (int d = 32; d; d >>= 1) m = max(m, __shfl_xor(m, d));
    if ((t & 63) == 0) s_m[t >> 6] = m;
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < W / 64; ++w) m = max(m, s_m[w]);
        const long long at = *cursor;
        out[0] = at; out[1] = carry; out[2] = m;
        *cursor = at + carry;
    }
}

// one workgroup per tile: its reachable genotypes as entries, from stage[lvl[0] + off[tile]] on (cap = entries the staging holds)
__global__ __launch_bounds__(JT_THREADS) void gt_scatter_kernel(const long long *__restrict__ dense, int64_t n, int items, const uint32_t *__restrict__ off, const long long *__restrict__ lvl,
                                                                int b0, const int32_t *__restrict__ cls, dg_dp_genotype_entry *__restrict__ stage, int64_t cap) {
    __shared__ uint32_t s[JT_THREADS];
    const int t = (int)threadIdx.x;
    const int64_t first = ((int64_t)blockIdx.x * JT_THREADS + t) * items;
    long long keys[GT_MAX_ITEMS];
    uint32_t c = 0;
    for (int q = 0; q < GT_MAX_ITEMS; ++q) {
        keys[q] = q < items && first + q < n ? dense[first + q] : JT_NO_KEY;
        c += keys[q] != JT_NO_KEY;
    }
    s[t] = c;
    __syncthreads();
    for (int d = 1; d < JT_THREADS; d <<= 1) {
        const uint32_t y = t >= d ? s[t - d] : 0u;
        __syncthreads();
        s[t] += y;
        __syncthreads();
    }
    int64_t at = (int64_t)lvl[0] + off[blockIdx.x] + (s[t] - c);
    for (int q = 0; q < GT_MAX_ITEMS; ++q) {
        if (keys[q] == JT_NO_KEY) continue;
        const uint32_t lo = (uint32_t)keys[q];
        dg_dp_genotype_entry e;
        e.vertex1 = b0 + (JT_MAX_K - (int)((lo >> 15) & 0x7FFFu));
        e.vertex2 = b0 + (JT_MAX_K - (int)(lo & 0x7FFFu));
        const int c1 = cls ? cls[e.vertex1] : e.vertex1, c2 = cls ? cls[e.vertex2] : e.vertex2;
        e.class1 = min(c1, c2);
        e.class2 = max(c1, c2);
        e.value = (int)(keys[q] >> 32);
        e.reserved = 0;
        if (at >= 0 && at < cap) stage[at] = e;
        ++at;
    }
}


struct JtLevel { int a0, k; uint32_t in_base; int T; bool coloured; int64_t cells; };   // cells: k * k * (b + 1)

// the buffers of one call: reserved here, released when the call returns; `now` / `peak` bytes for dg_dp_get_genotype_stats
struct JtMem {
    int64_t now = 0, peak = 0;
    int get(DevBuf &b, int64_t bytes) {
        if (int rc = b.ensure((size_t)std::max<int64_t>(bytes, 16))) return rc;
        now += (int64_t)b.bytes;
        peak = std::max(peak, now);
        return DG_OK;
    }
    void drop(DevBuf &b) { now -= (int64_t)b.bytes; b.release(); }
};

unsigned jt_blocks(int64_t lanes, int cap) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((lanes + JT_THREADS - 1) / JT_THREADS, cap)); }

}  // namespace

// the outputs of dg_dp_genotype_table (null for dg_dp_genotype_margins: then nothing of the table is reserved or launched)
struct JtTable { int64_t *level_off; dg_dp_genotype_entry **entries; int64_t *n_entries; };
// one budget per query (dg_dp_genotype_margins_budgets; null for the others: then `budget` holds for all and nothing here is reserved or launched)
struct JtBudgets { const int32_t *budgets; int32_t *best_values; };

namespace {

// all five entry points: tab = null is dg_dp_genotype_margins (_pinned); n_pins = 0 is the unpinned call -- no PinSet, no mask launch,
// the kernels' unordered instantiations; mb != null is dg_dp_genotype_margins_budgets: the same schedule once at the largest budget, the
// combination and the closing check per distinct budget (tab, vertex_values and best_value are null then, `budget` is ignored)
int jt_call(dg_ctx *c, const char *FN, const dg_dp_pin *pins, int64_t n_pins, const int32_t *called, int64_t n, int32_t budget, const int32_t *vertex_class, dg_dp_genotype_margin *levels,
            int32_t *vertex_values, int32_t *best_value, const JtTable *tab, const JtBudgets *mb = nullptr) {
    DpState *Sp = c->dp;
    if (!Sp || !Sp->loaded) { set_error("%s: no graph loaded", FN); return DG_ERR_STATE; }
    DpState &S = *Sp;
    if (tab) {
        if (!tab->level_off || !tab->entries || !tab->n_entries || !best_value) { set_error("%s: level_off, entries, n_entries and best_value are required", FN); return DG_ERR_ARG; }
        if (n < 0 || (n == 0) != (!called && !levels) || (!called) != (!levels)) {
            set_error("%s: called and levels go together, with n_called = %lld", FN, (long long)n);
            return DG_ERR_ARG;
        }
    } else {
        if (n < 1) { set_error("%s: n_called = %lld", FN, (long long)n); return DG_ERR_ARG; }
        if (mb) {
            if (!called || !levels || !mb->budgets || !mb->best_values) { set_error("%s: called, budgets, levels and best_values are required", FN); return DG_ERR_ARG; }
        } else if (!called || !levels || !best_value) { set_error("%s: called, levels and best_value are required", FN); return DG_ERR_ARG; }
    }
    if (mb && n <= JT_MAX_QUERIES) {                                        // the pass runs at the largest budget
        budget = 0;
        for (int64_t q = 0; q < n; ++q) {
            if (mb->budgets[q] < 0) { set_error("%s: query %lld: budget %d is negative", FN, (long long)q, mb->budgets[q]); return DG_ERR_ARG; }
            budget = std::max(budget, mb->budgets[q]);
        }
    }
    if (budget < 0) { set_error("%s: budget %d is negative", FN, budget); return DG_ERR_ARG; }
    if (n > JT_MAX_QUERIES) { set_error("%s: %lld called genotypes exceed %d per call", FN, (long long)n, JT_MAX_QUERIES); return DG_ERR_UNSUPPORTED; }
    if ((int64_t)budget + 1 > JT_MAX_PLANES) { set_error("%s: budget + 1 = %lld exceeds %d planes", FN, (long long)budget + 1, JT_MAX_PLANES); return DG_ERR_UNSUPPORTED; }
    const int L = S.L, nV = S.nV, B1 = budget + 1;
    if (L < 2 || (int)S.descs.size() < L) { set_error("%s: the loaded graph has %d levels", FN, L); return DG_ERR_STATE; }
    std::vector<JtLevel> lv((size_t)L);
    int kmax = 1;
    int64_t tmax = 0;
    for (int l = 0; l < L; ++l) {
        const LevelDesc &d = S.descs[(size_t)std::max(l, 1)];
        lv[l] = l ? JtLevel{d.b0, d.k2, d.in_base, d.T, d.delta_off >= 0, 0} : JtLevel{d.a0, d.k, 0u, 0, false, 0};
        lv[l].cells = (int64_t)lv[l].k * lv[l].k * B1;
        kmax = std::max(kmax, lv[l].k);
        if (lv[l].coloured) tmax = std::max<int64_t>(tmax, lv[l].T);
    }
    if (kmax > JT_MAX_K) { set_error("%s: widest level %d exceeds %d", FN, kmax, JT_MAX_K); return DG_ERR_UNSUPPORTED; }
    for (int64_t q = 0; q < n; ++q)
        for (int row = 0; row < 2; ++row)
            for (int l = 0; l < L; ++l) {
                const int32_t v = called[(q * 2 + row) * L + l];
                if ((uint32_t)(v - lv[l].a0) >= (uint32_t)lv[l].k) {
                    set_error("%s: query %lld row %d level %d: vertex %d is not in its level", FN, (long long)q, row, l, v);
                    return DG_ERR_ARG;
                }
            }
    // ---- the pins: validated, sorted by level and uploaded into a buffer of this call (DpState::d_pins belongs to the last pinned run) ----
    PinSet pin_set;
    DevBuf d_jpins;
    if (n_pins != 0) if (int rc = pins_prepare(FN, S, pins, n_pins, pin_set, d_jpins)) return rc;
    PinSet *const P = n_pins != 0 ? &pin_set : nullptr;
    // ---- the table's plan, before anything is launched: per level the dense rank of every vertex's class (ascending, signed), the
    // positions ordered by (rank, position), the A + 1 offsets of the ranks (level l's start at a0 + l: A <= k), the bound A (A + 1) / 2 ----
    std::vector<int32_t> t_rank, t_perm, t_goff, t_A;
    int64_t cap_entries = 0, bound_sum = 0, bound_max = 0, gpart_max = 1;
    // the two sizes of the compaction: keys per tile (256 lanes x 1..8 keys) and tiles per pass of the scan (its lanes, 64..1024 in whole waves)
    const int gt_items = (int)std::min<int64_t>(std::max<int64_t>(S.opt.genotype_table_tile_keys / JT_THREADS, 1), GT_MAX_ITEMS), gt_tile = gt_items * JT_THREADS;
    const int gt_scan = (int)std::min<int64_t>(std::max<int64_t>(S.opt.genotype_table_scan_tiles / 64, 1) * 64, GT_MAX_SCAN);
    const bool dbg = tab && getenv("DG_DEBUG") != nullptr;
    const double t_plan0 = wall_s();
    double t_copies = 0, t_plan = 0;
    if (tab) {
        cap_entries = S.opt.genotype_table_bytes / (int64_t)sizeof(dg_dp_genotype_entry);
        t_rank.resize((size_t)nV); t_perm.resize((size_t)nV); t_goff.assign((size_t)nV + (size_t)L, 0); t_A.resize((size_t)L);
        for (int l = 0; l < L; ++l) {
            const int a0 = lv[l].a0, k = lv[l].k;
            int32_t *perm = t_perm.data() + a0, *rank = t_rank.data() + a0, *goff = t_goff.data() + a0 + l;
            for (int x = 0; x < k; ++x) perm[x] = x;
            int A = k;
            if (vertex_class) {
                const int32_t *cl = vertex_class + a0;
                std::sort(perm, perm + k, [cl](int32_t x, int32_t y) { return cl[x] != cl[y] ? cl[x] < cl[y] : x < y; });
                A = 0;
                for (int x = 0; x < k; ++x) {
                    if (x == 0 || cl[perm[x]] != cl[perm[x - 1]]) goff[A++] = x;
                    rank[perm[x]] = A - 1;
                }
                goff[A] = k;
            } else
                for (int x = 0; x <= k; ++x) { if (x < k) rank[x] = x; goff[x] = x; }
            t_A[(size_t)l] = A;
            const int64_t bound = (int64_t)A * (A + 1) / 2;
            if (bound > cap_entries) {
                set_error("%s: level %d: up to %lld genotypes (%d classes) do not fit genotype_table_bytes = %lld (%lld entries)", FN, l, (long long)bound, A,
                          (long long)S.opt.genotype_table_bytes, (long long)cap_entries);
                return DG_ERR_UNSUPPORTED;
            }
            bound_sum += bound;
            bound_max = std::max(bound_max, bound);
            gpart_max = std::max(gpart_max, (int64_t)k * A);
        }
    }
    t_plan = wall_s() - t_plan0;
    // without a query the combine and record kernels still form T and the level maxima: one cell per level stands in, its records are dropped
    const bool want_levels = levels != nullptr;
    std::vector<int32_t> stand_in;
    if (n == 0) {
        stand_in.resize((size_t)2 * L);
        for (int l = 0; l < L; ++l) stand_in[(size_t)l] = stand_in[(size_t)L + l] = lv[l].a0;
        called = stand_in.data();
        n = 1;
    }
    // ---- the distinct budgets, ascending; per query its index among them; the queries grouped by it (in their own order) ----
    std::vector<int32_t> bud, bq;                                           // bq = [nd + 1] offsets, [n] the grouped queries, [n] the index per query
    int nd = 1;
    if (mb) {
        bud.assign(mb->budgets, mb->budgets + n);
        std::sort(bud.begin(), bud.end());
        bud.erase(std::unique(bud.begin(), bud.end()), bud.end());
        nd = (int)bud.size();
        bq.assign((size_t)nd + 1 + 2 * (size_t)n, 0);
        int32_t *qoff = bq.data(), *qlist = qoff + nd + 1, *qd = qlist + n;
        for (int64_t q = 0; q < n; ++q) {
            qd[q] = (int32_t)(std::lower_bound(bud.begin(), bud.end(), mb->budgets[q]) - bud.begin());
            ++qoff[qd[q] + 1];
        }
        for (int d = 0; d < nd; ++d) qoff[d + 1] += qoff[d];
        std::vector<int32_t> at(qoff, qoff + nd);
        for (int64_t q = 0; q < n; ++q) qlist[at[(size_t)qd[q]]++] = (int32_t)q;
    }
    hipStream_t s = c->stream;
    // ---- the plan: segments [seg[g], seg[g + 1]) whose forward states fit joint_state_bytes (at least one level each) ----
    std::vector<int> seg{0};
    {
        int64_t in_seg = 0;
        for (int l = 0; l < L; ++l) {
            const int64_t bytes = 4 * lv[l].cells;
            if (l > seg.back() && in_seg + bytes > S.opt.joint_state_bytes) { seg.push_back(l); in_seg = 0; }
            in_seg += bytes;
        }
    }
    const int n_seg = (int)seg.size();
    seg.push_back(L);
    std::vector<int64_t> ck_off((size_t)n_seg + 1, 0);                     // F of every segment's first level, int32 units
    int64_t seg_cells = 1, roll_cells = 0, level_cells = 1;
    for (int g = 0; g < n_seg; ++g) {
        ck_off[g + 1] = ck_off[g] + lv[seg[g]].cells;
        int64_t sum = 0;
        for (int l = seg[g] + 1; l < seg[g + 1]; ++l) { sum += lv[l].cells; if (g + 1 < n_seg) roll_cells = std::max(roll_cells, lv[l].cells); }
        seg_cells = std::max(seg_cells, sum);
    }
    for (int l = 0; l < L; ++l) level_cells = std::max(level_cells, lv[l].cells);
    int64_t launches = 0, twice = 0;
    JtMem M;
    if (P) { M.now += (int64_t)d_jpins.bytes; M.peak = M.now; }
    DevBuf d_called, d_cls, d_J, d_rec, d_lvlmax, d_cval, d_part, d_row, d_oo, d_ocur, d_oe, d_sc, d_ck, d_roll, d_seg, d_back;
    DevBuf d_bud, d_bq, d_Jb, d_V;
    DevBuf d_trank, d_tperm, d_tgoff, d_gpart, d_dense, d_tcnt, d_tmax, d_tlvl, d_stage;
    // the table keeps every row of T: one scratch row per row; the budgets share the rows of the one-budget call among them
    const int rows_per_budget = std::max(1, std::min(kmax, JT_ROW_BLOCKS / nd));
    const int row_blocks = tab ? kmax : mb ? rows_per_budget * nd : std::min(kmax, JT_ROW_BLOCKS);
    if (int rc = M.get(d_called, n * 2 * L * 4)) return rc;
    if (vertex_class) if (int rc = M.get(d_cls, (int64_t)nV * 4)) return rc;
    if (int rc = M.get(d_J, (int64_t)nV * 4)) return rc;
    if (int rc = M.get(d_rec, n * L * (int64_t)sizeof(dg_dp_genotype_margin))) return rc;
    if (int rc = M.get(d_lvlmax, mb ? (int64_t)nd * L * 4 : ((int64_t)L + 1) * 4)) return rc;       // entry L: V_b, the sink's cell on plane `budget` (budgets: [nd][L], V in d_V)
    if (mb) {
        if (int rc = M.get(d_bud, (int64_t)nd * 4)) return rc;
        if (int rc = M.get(d_bq, (int64_t)bq.size() * 4)) return rc;
        if (int rc = M.get(d_Jb, (int64_t)nd * kmax * 4)) return rc;
        if (int rc = M.get(d_V, (int64_t)B1 * 4)) return rc;                       // the sink's cell, every plane
    }
    if (int rc = M.get(d_cval, n * 4)) return rc;
    if (int rc = M.get(d_part, n * kmax * 8)) return rc;
    if (int rc = M.get(d_row, (int64_t)row_blocks * kmax * 4 * (P ? 2 : 1))) return rc;       // (pinned: the columns behind the rows)
    if (int rc = M.get(d_oo, ((int64_t)nV + 1) * 4)) return rc;
    if (int rc = M.get(d_ocur, (int64_t)nV * 4)) return rc;
    if (int rc = M.get(d_oe, S.n_edges * 4)) return rc;
    if (tmax) if (int rc = M.get(d_sc, tmax * tmax * 2)) return rc;
    if (int rc = M.get(d_ck, ck_off[n_seg] * 4)) return rc;
    const int64_t stage_cap = std::min(cap_entries, bound_sum), tiles_max = (bound_max + gt_tile - 1) / gt_tile;
    if (tab) {
        if (int rc = M.get(d_trank, (int64_t)nV * 4)) return rc;
        if (int rc = M.get(d_tperm, (int64_t)nV * 4)) return rc;
        if (int rc = M.get(d_tgoff, ((int64_t)nV + L) * 4)) return rc;
        if (int rc = M.get(d_gpart, gpart_max * 8)) return rc;
        if (int rc = M.get(d_dense, bound_max * 8)) return rc;
        if (int rc = M.get(d_tcnt, tiles_max * 4)) return rc;
        if (int rc = M.get(d_tmax, tiles_max * 4)) return rc;
        if (int rc = M.get(d_tlvl, ((int64_t)3 * L + 1) * 8)) return rc;                // per level: first entry in the staging, entries, largest value; then the cursor
        if (int rc = M.get(d_stage, stage_cap * (int64_t)sizeof(dg_dp_genotype_entry))) return rc;
        DG_HIP(hipMemcpyAsync(d_trank.p, t_rank.data(), (size_t)nV * 4, hipMemcpyHostToDevice, s));
        DG_HIP(hipMemcpyAsync(d_tperm.p, t_perm.data(), (size_t)nV * 4, hipMemcpyHostToDevice, s));
        DG_HIP(hipMemcpyAsync(d_tgoff.p, t_goff.data(), ((size_t)nV + (size_t)L) * 4, hipMemcpyHostToDevice, s));
        DG_HIP(hipMemsetAsync(d_tlvl.p, 0, ((size_t)3 * L + 1) * 8, s));
    }
    long long *const t_cursor = tab ? d_tlvl.as<long long>() + (int64_t)3 * L : nullptr;
    std::vector<dg_dp_genotype_entry> found;                               // the entries in the order the levels finish: L - 1 .. 0
    int64_t staged_bound = 0, copies = 0;
    auto flush = [&]() -> int {                                             // the staging's entries to the host; the cursor back to 0
        staged_bound = 0;
        long long have = 0;
        const double t0 = wall_s();
        DG_HIP(hipMemcpyAsync(&have, t_cursor, 8, hipMemcpyDeviceToHost, s));
        DG_HIP(hipStreamSynchronize(s));
        if (have < 0 || have > stage_cap) { set_error("%s: the staging holds %lld entries of %lld", FN, have, (long long)stage_cap); return DG_ERR_STATE; }
        if (!have) return DG_OK;
        const size_t at = found.size();
        found.resize(at + (size_t)have);
        DG_HIP(hipMemcpyAsync(found.data() + at, d_stage.p, (size_t)have * sizeof(dg_dp_genotype_entry), hipMemcpyDeviceToHost, s));
        DG_HIP(hipMemsetAsync(t_cursor, 0, 8, s));
        DG_HIP(hipStreamSynchronize(s));
        ++copies;
        t_copies += wall_s() - t0;                                          // (with the wait for the kernels still in flight)
        return DG_OK;
    };
    DG_HIP(hipMemcpyAsync(d_called.p, called, (size_t)(n * 2 * L) * 4, hipMemcpyHostToDevice, s));
    if (vertex_class) DG_HIP(hipMemcpyAsync(d_cls.p, vertex_class, (size_t)nV * 4, hipMemcpyHostToDevice, s));
    if (mb) {
        DG_HIP(hipMemcpyAsync(d_bud.p, bud.data(), (size_t)nd * 4, hipMemcpyHostToDevice, s));
        DG_HIP(hipMemcpyAsync(d_bq.p, bq.data(), bq.size() * 4, hipMemcpyHostToDevice, s));
    }
    const int32_t *d_qoff = d_bq.as<int32_t>(), *d_qlist = mb ? d_qoff + nd + 1 : nullptr, *d_qd = mb ? d_qlist + n : nullptr;
    const LevelDesc *descs = S.d_descs.as<LevelDesc>();
    const uint32_t *in_off = S.d_in_off.as<uint32_t>(), *in_edge = S.d_in_edge.as<uint32_t>();
    const int32_t *in_dst = S.d_in_dst.as<int32_t>();
    uint16_t *sc = d_sc.as<uint16_t>();
    // the in-edges grouped by source
    DG_HIP(hipMemsetAsync(d_ocur.p, 0, (size_t)nV * 4, s));
    hipLaunchKernelGGL(jt_out_count_kernel, dim3((unsigned)(L - 1)), dim3(JT_THREADS), 0, s, descs, L, nV, in_edge, d_ocur.as<uint32_t>());
    hipLaunchKernelGGL(jt_out_scan_kernel, dim3(1), dim3(1024), 0, s, d_ocur.as<uint32_t>(), d_oo.as<uint32_t>(), d_ocur.as<uint32_t>(), nV);
    hipLaunchKernelGGL(jt_out_fill_kernel, dim3((unsigned)(L - 1)), dim3(JT_THREADS), 0, s, descs, L, nV, in_edge, d_ocur.as<uint32_t>(), d_oe.as<uint32_t>(), (uint32_t)S.n_edges);
    DG_HIP(hipGetLastError());
    launches += 3;

    auto scores = [&](int l) -> const uint16_t * {                          // the matrix of the transition into level l, in d_sc
        const int T = lv[l].T;
        if (!lv[l].coloured || T < 1) return nullptr;
        hipLaunchKernelGGL(jt_scores_kernel, dim3(jt_blocks(T, 64), (unsigned)std::min(T, 16384)), dim3(JT_THREADS), 0, s, T, lv[l].in_base, lv[l - 1].a0, in_edge, in_dst,
                           colour_csr(S), S.d_eflag.as<uint8_t>(), S.d_eself.as<uint16_t>(), sc);
        ++launches;
        return sc;
    };
    auto fill = [&](int32_t *st, int l, int pos) {                          // level l: 0 on every plane of the cell (pos, pos)
        hipLaunchKernelGGL(jt_fill_kernel, dim3(jt_blocks(lv[l].cells, 65536)), dim3(JT_THREADS), 0, s, st, lv[l].cells, ((int64_t)pos * lv[l].k + pos) * B1, B1);
        ++launches;
    };
    auto forward = [&](const int32_t *prev, int32_t *cur, int l) {
        const uint16_t *m = scores(l);
        hipLaunchKernelGGL(jt_forward_kernel, dim3(jt_blocks((int64_t)lv[l].k * B1, JT_X_BLOCKS), (unsigned)lv[l].k), dim3(JT_THREADS), 0, s, prev, cur, lv[l - 1].k, lv[l].k, B1,
                           lv[l].a0, lv[l].in_base, lv[l].T, in_off, in_edge, m);
        ++launches;
        if (P && P->has(l)) { pins_launch_joint_mask(*P, l, cur, lv[l].k, B1, s); ++launches; }       // before anything reads the level
    };
    // ---- pass 1: the state at every segment's first level ----
    int32_t *ck = d_ck.as<int32_t>();
    fill(ck, 0, 0);
    if (n_seg > 1) {
        if (int rc = M.get(d_roll, 2 * roll_cells * 4)) return rc;
        int32_t *roll = d_roll.as<int32_t>();
        const int32_t *prev = ck;
        int g = 0;
        for (int l = 1; l <= seg[n_seg - 1]; ++l) {
            int32_t *dst;
            if (l == seg[g + 1]) dst = ck + ck_off[++g];
            else { dst = roll + (l & 1) * roll_cells; ++twice; }
            forward(prev, dst, l);
            prev = dst;
        }
        DG_HIP(hipGetLastError());
        DG_HIP(hipStreamSynchronize(s));                                    // the rolling states go before the segment buffers come
        M.drop(d_roll);
    }
    // ---- the segments, last first ----
    if (int rc = M.get(d_seg, seg_cells * 4)) return rc;
    if (int rc = M.get(d_back, 2 * level_cells * 4)) return rc;
    int32_t *back = d_back.as<int32_t>();
    const auto combine = P ? jt_combine_kernel<true> : jt_combine_kernel<false>;       // ordered pins: both orders of a cell
    const auto combine_budgets = P ? jt_combine_budgets_kernel<true> : jt_combine_budgets_kernel<false>;
    const auto gt_rows = P ? gt_rows_kernel<true> : gt_rows_kernel<false>;
    std::vector<const int32_t *> Fp((size_t)L, nullptr);
    for (int g = n_seg - 1; g >= 0; --g) {
        const int a = seg[g], e = seg[g + 1];
        Fp[a] = ck + ck_off[g];
        int64_t at = 0;
        for (int l = a + 1; l < e; ++l) {
            int32_t *dst = d_seg.as<int32_t>() + at;
            at += lv[l].cells;
            forward(Fp[l - 1], dst, l);
            Fp[l] = dst;
        }
        for (int l = e - 1; l >= a; --l) {
            int32_t *cur = back + (l & 1) * level_cells;
            if (l == L - 1) {
                const int sink = nV - 1 - lv[l].a0;
                fill(cur, l, sink);
                if (mb) DG_HIP(hipMemcpyAsync(d_V.p, Fp[l] + ((int64_t)sink * lv[l].k + sink) * B1, (size_t)B1 * 4, hipMemcpyDeviceToDevice, s));
                else DG_HIP(hipMemcpyAsync(d_lvlmax.as<int32_t>() + L, Fp[l] + ((int64_t)sink * lv[l].k + sink) * B1 + budget, 4, hipMemcpyDeviceToDevice, s));
            } else {
                const uint16_t *m = scores(l + 1);
                hipLaunchKernelGGL(jt_backward_kernel, dim3(jt_blocks((int64_t)lv[l].k * B1, JT_X_BLOCKS), (unsigned)lv[l].k), dim3(JT_THREADS), 0, s,
                                   (const int32_t *)(back + ((l + 1) & 1) * level_cells), cur, lv[l].k, lv[l + 1].k, B1, lv[l].a0, lv[l + 1].a0, lv[l + 1].in_base, lv[l + 1].T,
                                   d_oo.as<uint32_t>(), d_oe.as<uint32_t>(), in_edge, in_dst, m);
                ++launches;
                if (P && P->has(l)) { pins_launch_joint_mask(*P, l, cur, lv[l].k, B1, s); ++launches; }
            }
            if (mb) {
                hipLaunchKernelGGL(combine_budgets, dim3((unsigned)std::min(lv[l].k, rows_per_budget), (unsigned)nd), dim3(JT_THREADS), 0, s, Fp[l], (const int32_t *)cur, lv[l].k, B1,
                                   lv[l].a0, d_row.as<int32_t>(), d_Jb.as<int32_t>(), kmax, (const int32_t *)d_bud.as<int32_t>(), d_qoff, d_qlist, (const int32_t *)d_called.as<int32_t>(), L, l,
                                   vertex_class ? (const int32_t *)d_cls.as<int32_t>() : nullptr, d_part.as<long long>(), d_cval.as<int32_t>());
                hipLaunchKernelGGL(jt_records_budgets_kernel, dim3((unsigned)n), dim3(JT_THREADS), 0, s, lv[l].k, lv[l].a0, (const int32_t *)d_Jb.as<int32_t>(), kmax, d_qd, d_qoff, d_qlist,
                                   (const long long *)d_part.as<long long>(), (const int32_t *)d_cval.as<int32_t>(), (const int32_t *)d_called.as<int32_t>(), L, l,
                                   d_rec.as<dg_dp_genotype_margin>(), d_lvlmax.as<int32_t>());
                launches += 2;
                continue;
            }
            hipLaunchKernelGGL(combine, dim3((unsigned)std::min(lv[l].k, row_blocks)), dim3(JT_THREADS), 0, s, Fp[l], (const int32_t *)cur, lv[l].k, B1, lv[l].a0,
                               d_row.as<int32_t>(), d_J.as<int32_t>(), (int)n, d_called.as<int32_t>(), L, l, vertex_class ? d_cls.as<int32_t>() : nullptr,
                               d_part.as<long long>(), d_cval.as<int32_t>());
            hipLaunchKernelGGL(jt_records_kernel, dim3((unsigned)n), dim3(JT_THREADS), 0, s, lv[l].k, lv[l].a0, d_J.as<int32_t>(), d_part.as<long long>(), d_cval.as<int32_t>(),
                               d_called.as<int32_t>(), L, l, d_rec.as<dg_dp_genotype_margin>(), d_lvlmax.as<int32_t>());
            launches += 2;
            if (tab) {
                const int k = lv[l].k, A = t_A[(size_t)l];
                const int64_t bound = (int64_t)A * (A + 1) / 2, tiles = (bound + gt_tile - 1) / gt_tile;
                if (staged_bound + bound > stage_cap) if (int rc = flush()) return rc;
                staged_bound += bound;
                int lp = 0;                                                 // lanes per genotype: the mean rows per rank, as a power of two
                const int64_t per = S.opt.genotype_table_lanes > 0 ? S.opt.genotype_table_lanes : (k + A - 1) / A;
                while (lp < 6 && ((int64_t)1 << (lp + 1)) <= std::max<int64_t>(per, 1)) ++lp;
                const int32_t *perm = d_tperm.as<int32_t>() + lv[l].a0;
                long long *lvl3 = d_tlvl.as<long long>() + (int64_t)3 * l;
                hipLaunchKernelGGL(gt_rows, dim3((unsigned)((k + JT_THREADS / 64 - 1) / (JT_THREADS / 64))), dim3(JT_THREADS), 0, s, (const int32_t *)d_row.as<int32_t>(), k, A,
                                   (const int32_t *)(d_trank.as<int32_t>() + lv[l].a0), perm, d_gpart.as<long long>());
                hipLaunchKernelGGL(gt_pairs_kernel, dim3(jt_blocks((int64_t)A << lp, 65535), (unsigned)std::min(A, 65535)), dim3(JT_THREADS), 0, s,
                                   (const long long *)d_gpart.as<long long>(), k, A, perm, (const int32_t *)(d_tgoff.as<int32_t>() + lv[l].a0 + l), lp, d_dense.as<long long>());
                hipLaunchKernelGGL(gt_count_kernel, dim3((unsigned)tiles), dim3(JT_THREADS), 0, s, (const long long *)d_dense.as<long long>(), bound, gt_items,
                                   d_tcnt.as<uint32_t>(), d_tmax.as<int32_t>());
                hipLaunchKernelGGL(gt_scan_kernel, dim3(1), dim3((unsigned)gt_scan), 0, s, d_tcnt.as<uint32_t>(), (const int32_t *)d_tmax.as<int32_t>(), tiles, t_cursor, lvl3);
                hipLaunchKernelGGL(gt_scatter_kernel, dim3((unsigned)tiles), dim3(JT_THREADS), 0, s, (const long long *)d_dense.as<long long>(), bound, gt_items,
                                   (const uint32_t *)d_tcnt.as<uint32_t>(), (const long long *)lvl3, lv[l].a0, vertex_class ? (const int32_t *)d_cls.as<int32_t>() : nullptr,
                                   d_stage.as<dg_dp_genotype_entry>(), stage_cap);
                launches += 5;
            }
        }
        DG_HIP(hipGetLastError());
        if (tab) if (int rc = flush()) return rc;                           // at the latest once per segment
    }
    // the caller's arrays are written only if the call succeeds
    std::vector<dg_dp_genotype_margin> recs((size_t)(n * L));
    std::vector<int32_t> lvlmax(mb ? (size_t)nd * L : (size_t)L + 1), vals(vertex_values ? (size_t)nV : 0), Vs(mb ? (size_t)B1 : 0);
    std::vector<long long> tlvl(tab ? (size_t)3 * L : 0);
    if (tab) DG_HIP(hipMemcpyAsync(tlvl.data(), d_tlvl.p, tlvl.size() * 8, hipMemcpyDeviceToHost, s));
    DG_HIP(hipMemcpyAsync(recs.data(), d_rec.p, recs.size() * sizeof(dg_dp_genotype_margin), hipMemcpyDeviceToHost, s));
    DG_HIP(hipMemcpyAsync(lvlmax.data(), d_lvlmax.p, lvlmax.size() * 4, hipMemcpyDeviceToHost, s));
    if (mb) DG_HIP(hipMemcpyAsync(Vs.data(), d_V.p, Vs.size() * 4, hipMemcpyDeviceToHost, s));
    if (vertex_values) DG_HIP(hipMemcpyAsync(vals.data(), d_J.p, (size_t)nV * 4, hipMemcpyDeviceToHost, s));
    DG_HIP(hipStreamSynchronize(s));
    S.jt_stats[0] = n_seg; S.jt_stats[1] = twice; S.jt_stats[2] = M.peak; S.jt_stats[3] = launches;
    S.jt_stats[4] = (int64_t)found.size(); S.jt_stats[5] = copies;
    S.jt_stats[6] = P ? n_pins : 0; S.jt_stats[7] = P ? P->n_mask : 0;
    if (mb) {                                                               // the closing check, per distinct budget
        for (int d = 0; d < nd; ++d)
            for (int l = 0; l < L; ++l)
                if (lvlmax[(size_t)d * L + l] != Vs[(size_t)bud[(size_t)d]]) {
                    set_error("%s: level %d: the largest through-value at budget %d is %d, the sink's value at that budget is %d", FN, l, bud[(size_t)d], lvlmax[(size_t)d * L + l],
                              Vs[(size_t)bud[(size_t)d]]);
                    return DG_ERR_STATE;
                }
        memcpy(levels, recs.data(), recs.size() * sizeof(dg_dp_genotype_margin));
        for (int64_t q = 0; q < n; ++q) mb->best_values[q] = Vs[(size_t)mb->budgets[q]];
        return DG_OK;
    }
    const int32_t V = lvlmax[(size_t)L];
    // the closing check: on every level the best pair through any cell is the best pair
    for (int l = 0; l < L; ++l)
        if (lvlmax[l] != V) {
            set_error("%s: level %d: the largest through-value is %d, the sink's value at budget %d is %d", FN, l, lvlmax[l], budget, V);
            return DG_ERR_STATE;
        }
    if (tab) {                                                              // the levels came last first: turn them round
        const double t_turn0 = wall_s();
        std::vector<int64_t> off((size_t)L + 1, 0);
        for (int l = 0; l < L; ++l) {
            if (tlvl[(size_t)3 * l + 2] != V) {
                set_error("%s: level %d: the largest genotype value is %lld, the sink's value at budget %d is %d", FN, l, tlvl[(size_t)3 * l + 2], budget, V);
                return DG_ERR_STATE;
            }
            off[(size_t)l + 1] = off[(size_t)l] + tlvl[(size_t)3 * l + 1];
        }
        if (off[(size_t)L] != (int64_t)found.size()) { set_error("%s: %lld entries counted, %zu copied", FN, (long long)off[(size_t)L], found.size()); return DG_ERR_STATE; }
        dg_dp_genotype_entry *out = nullptr;
        if (!found.empty()) {
            out = (dg_dp_genotype_entry *)malloc(found.size() * sizeof(dg_dp_genotype_entry));
            if (!out) { set_error("%s: out of host memory for %zu entries", FN, found.size()); return DG_ERR_OOM; }
            size_t at = 0;
            for (int l = L - 1; l >= 0; --l) {
                const size_t cnt = (size_t)(off[(size_t)l + 1] - off[(size_t)l]);
                if (cnt) memcpy(out + off[(size_t)l], found.data() + at, cnt * sizeof(dg_dp_genotype_entry));
                at += cnt;
            }
        }
        memcpy(tab->level_off, off.data(), off.size() * 8);
        *tab->entries = out;
        *tab->n_entries = (int64_t)found.size();
        if (dbg) fprintf(stderr, "[dipgenie_hip] genotype_table: host plan %.3f s, %lld staging copies %.3f s (with their waits for the stream), turning the levels round %.3f s\n", t_plan,
                         (long long)copies, t_copies, wall_s() - t_turn0);
    }
    if (want_levels) memcpy(levels, recs.data(), recs.size() * sizeof(dg_dp_genotype_margin));
    if (vertex_values) memcpy(vertex_values, vals.data(), vals.size() * 4);
    *best_value = V;
    return DG_OK;
}

// ---- dg_dp_phase_margins: cis against trans for neighbouring het levels h_t < h_{t+1} of one called pair (include/dipgenie_hip.h has the
// definition).  Beside B a second backward state S rolls down the levels: seeded at a het level e with B_e restricted to the cells of the
// called ORDERED classes of e, carried down by jt_backward_kernel unchanged (launched a second time per level, on the score matrix the first
// launch left in the call's buffer), read out at the next het level a below against F_a, then seeded again from B_a.  Both states mean "at
// most r" and d is symmetric in the two haplotypes, so the one S answers both orders at a.  Every kernel is a gather as above: each word
// has one owner, nothing depends on the order of lanes or workgroups; the classes of the level come as kernel arguments (the host has them):
//   * ph_seed_kernel: grid (x blocks, k), row i = blockIdx.y: S[i][j][.] = B[i][j][.] where (cls i, cls j) = (c0, c1), NEG_INF elsewhere; a row
//     of another class stores NEG_INF without a load of B;
//   * ph_readout_kernel: one workgroup per row i.  The row's class is workgroup-uniform: a row of class c0 holds cells of the called order
//     (its columns of class c1), a row of class c1 cells of the swapped order (its columns of class c0), any other row has nothing and its
//     workgroup stores two empty keys and returns before a load of a state.  A lane takes a cell and walks r, as jt_combine_kernel does;
//     part = [2][k] keys (value desc, i asc, j asc), [0] = cis, [1] = trans;
//   * ph_finish_kernel: one workgroup reduces the two rows of keys to the record of the pair of sites, in a device array that is copied
//     out once when the call ends.
__global__ __launch_bounds__(JT_THREADS) void ph_seed_kernel(const int32_t *__restrict__ B, int32_t *__restrict__ S, int k, int B1, int b0, const int32_t *__restrict__ cls,
                                                             int c0, int c1) {
    const int i = (int)blockIdx.y;
    const bool row = (cls ? cls[b0 + i] : b0 + i) == c0;                    // uniform per workgroup
    const int n = k * B1;
    for (int x = (int)(blockIdx.x * JT_THREADS + threadIdx.x); x < n; x += (int)(gridDim.x * JT_THREADS)) {
        const int j = x / B1;
        const int64_t at = (int64_t)i * n + x;                              // ((i * k + j) * B1 + r)
        int v = NEG_INF;
        if (row && (cls ? cls[b0 + j] : b0 + j) == c1) v = B[at];
        S[at] = v;
    }
}

__global__ __launch_bounds__(JT_THREADS) void ph_readout_kernel(const int32_t *__restrict__ F, const int32_t *__restrict__ S, int k, int B1, int b0,
                                                                const int32_t *__restrict__ cls, int c0, int c1, long long *__restrict__ part) {
    __shared__ long long s_key[JT_THREADS / 64];
    const int t = (int)threadIdx.x, i = (int)blockIdx.x;
    const int ci = cls ? cls[b0 + i] : b0 + i;
    if (ci != c0 && ci != c1) {                                             // uniform: no cell of either order in this row
        if (t == 0) { part[i] = JT_NO_KEY; part[k + i] = JT_NO_KEY; }
        return;
    }
    const int cj_want = ci == c0 ? c1 : c0;                                 // c0 != c1: the level is het
    long long key = JT_NO_KEY;
    for (int j = t; j < k; j += JT_THREADS) {
        if ((cls ? cls[b0 + j] : b0 + j) != cj_want) continue;
        const int32_t *f = F + ((int64_t)i * k + j) * B1, *sv = S + ((int64_t)i * k + j) * B1;
        int best = NEG_INF;
        for (int r = 0; r < B1; ++r) {
            const int fv = f[r], bv = sv[B1 - 1 - r];
            if (fv != NEG_INF && bv != NEG_INF) best = max(best, fv + bv);
        }
        if (best != NEG_INF) key = max(key, jt_key(best, i, j));
    }
    for (int d = 32; d; d >>= 1) key = max(key, __shfl_xor(key, d));
    if ((t & 63) == 0) s_key[t >> 6] = key;
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < JT_THREADS / 64; ++w) key = max(key, s_key[w]);
        part[i] = ci == c0 ? key : JT_NO_KEY;
        part[k + i] = ci == c0 ? JT_NO_KEY : key;
    }
}

__global__ __launch_bounds__(JT_THREADS) void ph_finish_kernel(const long long *__restrict__ part, int k, int b0, int level_a, int level_b, dg_dp_phase_margin *__restrict__ rec) {
    __shared__ long long s_key[2][JT_THREADS / 64];
    const int t = (int)threadIdx.x;
    long long cis = JT_NO_KEY, trans = JT_NO_KEY;
    for (int i = t; i < k; i += JT_THREADS) { cis = max(cis, part[i]); trans = max(trans, part[k + i]); }
    for (int d = 32; d; d >>= 1) { cis = max(cis, __shfl_xor(cis, d)); trans = max(trans, __shfl_xor(trans, d)); }
    if ((t & 63) == 0) { s_key[0][t >> 6] = cis; s_key[1][t >> 6] = trans; }
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < JT_THREADS / 64; ++w) { cis = max(cis, s_key[0][w]); trans = max(trans, s_key[1][w]); }
        dg_dp_phase_margin r;
        r.level_a = level_a; r.level_b = level_b;
        r.cis_value = r.trans_value = NEG_INF;
        r.cis_vertex1 = r.cis_vertex2 = r.trans_vertex1 = r.trans_vertex2 = -1;
        if (cis != JT_NO_KEY) {
            const uint32_t lo = (uint32_t)cis;
            r.cis_vertex1 = b0 + (JT_MAX_K - (int)((lo >> 15) & 0x7FFFu));
            r.cis_vertex2 = b0 + (JT_MAX_K - (int)(lo & 0x7FFFu));
            r.cis_value = (int)(cis >> 32);
        }
        if (trans != JT_NO_KEY) {
            const uint32_t lo = (uint32_t)trans;
            r.trans_vertex1 = b0 + (JT_MAX_K - (int)((lo >> 15) & 0x7FFFu));
            r.trans_vertex2 = b0 + (JT_MAX_K - (int)(lo & 0x7FFFu));
            r.trans_value = (int)(trans >> 32);
        }
        r.reserved[0] = 0; r.reserved[1] = 0;
        *rec = r;
    }
}

// the schedule of jt_call (plan by joint_state_bytes, forward checkpoints, the segments from the last to the first, B rolling in two
// states) with S beside B; none of that call's combination, record or table kernels, and nothing backward below the first het level
int ph_call(dg_ctx *c, const int32_t *called, int32_t budget, const int32_t *vertex_class, dg_dp_phase_margin *records, int64_t *n_records, int32_t *best_value) {
    const char *FN = "dg_dp_phase_margins";
    DpState *Sp = c->dp;
    if (!Sp || !Sp->loaded) { set_error("%s: no graph loaded", FN); return DG_ERR_STATE; }
    DpState &S = *Sp;
    if (!called || !records || !n_records || !best_value) { set_error("%s: called, records, n_records and best_value are required", FN); return DG_ERR_ARG; }
    if (budget < 0) { set_error("%s: budget %d is negative", FN, budget); return DG_ERR_ARG; }
    if ((int64_t)budget + 1 > JT_MAX_PLANES) { set_error("%s: budget + 1 = %lld exceeds %d planes", FN, (long long)budget + 1, JT_MAX_PLANES); return DG_ERR_UNSUPPORTED; }
    const int L = S.L, nV = S.nV, B1 = budget + 1;
    if (L < 2 || (int)S.descs.size() < L) { set_error("%s: the loaded graph has %d levels", FN, L); return DG_ERR_STATE; }
    std::vector<JtLevel> lv((size_t)L);
    int kmax = 1;
    int64_t tmax = 0;
    for (int l = 0; l < L; ++l) {
        const LevelDesc &d = S.descs[(size_t)std::max(l, 1)];
        lv[l] = l ? JtLevel{d.b0, d.k2, d.in_base, d.T, d.delta_off >= 0, 0} : JtLevel{d.a0, d.k, 0u, 0, false, 0};
        lv[l].cells = (int64_t)lv[l].k * lv[l].k * B1;
        kmax = std::max(kmax, lv[l].k);
        if (lv[l].coloured) tmax = std::max<int64_t>(tmax, lv[l].T);
    }
    if (kmax > JT_MAX_K) { set_error("%s: widest level %d exceeds %d", FN, kmax, JT_MAX_K); return DG_ERR_UNSUPPORTED; }
    for (int row = 0; row < 2; ++row)
        for (int l = 0; l < L; ++l) {
            const int32_t v = called[(int64_t)row * L + l];
            if ((uint32_t)(v - lv[l].a0) >= (uint32_t)lv[l].k) { set_error("%s: row %d level %d: vertex %d is not in its level", FN, row, l, v); return DG_ERR_ARG; }
        }
    // ---- the het levels, ascending, and the called ordered classes of every level ----
    std::vector<int32_t> c0((size_t)L), c1((size_t)L);
    std::vector<int> het;
    for (int l = 0; l < L; ++l) {
        c0[(size_t)l] = vertex_class ? vertex_class[called[l]] : called[l];
        c1[(size_t)l] = vertex_class ? vertex_class[called[(int64_t)L + l]] : called[(int64_t)L + l];
        if (c0[(size_t)l] != c1[(size_t)l]) het.push_back(l);
    }
    const int nh = (int)het.size(), nrec = std::max(nh - 1, 0);
    const int h_first = nrec ? het.front() : L, h_last = nrec ? het.back() : L;        // fewer than two het levels: no backward state at all
    hipStream_t s = c->stream;
    // ---- the plan: segments [seg[g], seg[g + 1]) whose forward states fit joint_state_bytes (at least one level each) ----
    std::vector<int> seg{0};
    {
        int64_t in_seg = 0;
        for (int l = 0; l < L; ++l) {
            const int64_t bytes = 4 * lv[l].cells;
            if (l > seg.back() && in_seg + bytes > S.opt.joint_state_bytes) { seg.push_back(l); in_seg = 0; }
            in_seg += bytes;
        }
    }
    const int n_seg = (int)seg.size();
    seg.push_back(L);
    std::vector<int64_t> ck_off((size_t)n_seg + 1, 0);                     // F of every segment's first level, int32 units
    int64_t seg_cells = 1, roll_cells = 0, level_cells = 1;
    for (int g = 0; g < n_seg; ++g) {
        ck_off[g + 1] = ck_off[g] + lv[seg[g]].cells;
        int64_t sum = 0;
        for (int l = seg[g] + 1; l < seg[g + 1]; ++l) { sum += lv[l].cells; if (g + 1 < n_seg) roll_cells = std::max(roll_cells, lv[l].cells); }
        seg_cells = std::max(seg_cells, sum);
    }
    for (int l = 0; l < L; ++l) level_cells = std::max(level_cells, lv[l].cells);
    int64_t seeded = 0, readouts = 0;
    JtMem M;
    DevBuf d_cls, d_rec, d_V, d_part, d_oo, d_ocur, d_oe, d_sc, d_ck, d_roll, d_seg, d_back, d_sback;
    if (vertex_class) if (int rc = M.get(d_cls, (int64_t)nV * 4)) return rc;
    if (int rc = M.get(d_rec, (int64_t)std::max(nrec, 1) * (int64_t)sizeof(dg_dp_phase_margin))) return rc;
    if (int rc = M.get(d_V, 4)) return rc;
    if (int rc = M.get(d_part, (int64_t)2 * kmax * 8)) return rc;
    if (tmax) if (int rc = M.get(d_sc, tmax * tmax * 2)) return rc;
    if (int rc = M.get(d_ck, ck_off[n_seg] * 4)) return rc;
    if (vertex_class) DG_HIP(hipMemcpyAsync(d_cls.p, vertex_class, (size_t)nV * 4, hipMemcpyHostToDevice, s));
    const int32_t *cls = vertex_class ? (const int32_t *)d_cls.as<int32_t>() : nullptr;
    const LevelDesc *descs = S.d_descs.as<LevelDesc>();
    const uint32_t *in_off = S.d_in_off.as<uint32_t>(), *in_edge = S.d_in_edge.as<uint32_t>();
    const int32_t *in_dst = S.d_in_dst.as<int32_t>();
    uint16_t *sc = d_sc.as<uint16_t>();
    if (nrec) {                                                             // the in-edges grouped by source
        if (int rc = M.get(d_oo, ((int64_t)nV + 1) * 4)) return rc;
        if (int rc = M.get(d_ocur, (int64_t)nV * 4)) return rc;
        if (int rc = M.get(d_oe, S.n_edges * 4)) return rc;
        DG_HIP(hipMemsetAsync(d_ocur.p, 0, (size_t)nV * 4, s));
        hipLaunchKernelGGL(jt_out_count_kernel, dim3((unsigned)(L - 1)), dim3(JT_THREADS), 0, s, descs, L, nV, in_edge, d_ocur.as<uint32_t>());
        hipLaunchKernelGGL(jt_out_scan_kernel, dim3(1), dim3(1024), 0, s, d_ocur.as<uint32_t>(), d_oo.as<uint32_t>(), d_ocur.as<uint32_t>(), nV);
        hipLaunchKernelGGL(jt_out_fill_kernel, dim3((unsigned)(L - 1)), dim3(JT_THREADS), 0, s, descs, L, nV, in_edge, d_ocur.as<uint32_t>(), d_oe.as<uint32_t>(), (uint32_t)S.n_edges);
        DG_HIP(hipGetLastError());
    }
    auto scores = [&](int l) -> const uint16_t * {                          // the matrix of the transition into level l, in d_sc
        const int T = lv[l].T;
        if (!lv[l].coloured || T < 1) return nullptr;
        hipLaunchKernelGGL(jt_scores_kernel, dim3(jt_blocks(T, 64), (unsigned)std::min(T, 16384)), dim3(JT_THREADS), 0, s, T, lv[l].in_base, lv[l - 1].a0, in_edge, in_dst,
                           colour_csr(S), S.d_eflag.as<uint8_t>(), S.d_eself.as<uint16_t>(), sc);
        return sc;
    };
    auto fill = [&](int32_t *st, int l, int pos) {                          // level l: 0 on every plane of the cell (pos, pos)
        hipLaunchKernelGGL(jt_fill_kernel, dim3(jt_blocks(lv[l].cells, 65536)), dim3(JT_THREADS), 0, s, st, lv[l].cells, ((int64_t)pos * lv[l].k + pos) * B1, B1);
    };
    auto forward = [&](const int32_t *prev, int32_t *cur, int l) {
        const uint16_t *m = scores(l);
        hipLaunchKernelGGL(jt_forward_kernel, dim3(jt_blocks((int64_t)lv[l].k * B1, JT_X_BLOCKS), (unsigned)lv[l].k), dim3(JT_THREADS), 0, s, prev, cur, lv[l - 1].k, lv[l].k, B1,
                           lv[l].a0, lv[l].in_base, lv[l].T, in_off, in_edge, m);
    };
    auto backward = [&](const int32_t *next, int32_t *cur, int l, const uint16_t *m) {      // level l from level l + 1, whose scores are m
        hipLaunchKernelGGL(jt_backward_kernel, dim3(jt_blocks((int64_t)lv[l].k * B1, JT_X_BLOCKS), (unsigned)lv[l].k), dim3(JT_THREADS), 0, s, next, cur, lv[l].k, lv[l + 1].k, B1,
                           lv[l].a0, lv[l + 1].a0, lv[l + 1].in_base, lv[l + 1].T, d_oo.as<uint32_t>(), d_oe.as<uint32_t>(), in_edge, in_dst, m);
    };
    // ---- pass 1: the state at every segment's first level ----
    int32_t *ck = d_ck.as<int32_t>();
    fill(ck, 0, 0);
    if (n_seg > 1) {
        if (int rc = M.get(d_roll, 2 * roll_cells * 4)) return rc;
        int32_t *roll = d_roll.as<int32_t>();
        const int32_t *prev = ck;
        int g = 0;
        for (int l = 1; l <= seg[n_seg - 1]; ++l) {
            int32_t *dst = l == seg[g + 1] ? ck + ck_off[++g] : roll + (l & 1) * roll_cells;
            forward(prev, dst, l);
            prev = dst;
        }
        DG_HIP(hipGetLastError());
        DG_HIP(hipStreamSynchronize(s));                                    // the rolling states go before the segment buffers come
        M.drop(d_roll);
    }
    // ---- the segments, last first, down to the one that holds the first het level ----
    if (int rc = M.get(d_seg, seg_cells * 4)) return rc;
    if (nrec) {
        if (int rc = M.get(d_back, 2 * level_cells * 4)) return rc;
        if (int rc = M.get(d_sback, 2 * level_cells * 4)) return rc;
    }
    int32_t *back = d_back.as<int32_t>(), *sback = d_sback.as<int32_t>();
    std::vector<const int32_t *> Fp((size_t)L, nullptr);
    int t = nh - 1;                                                         // index of the next het level on the way down
    for (int g = n_seg - 1; g >= 0; --g) {
        const int a = seg[g], e = seg[g + 1];
        if (e <= h_first && g < n_seg - 1) break;                           // nothing is read out below the first het level
        Fp[a] = ck + ck_off[g];
        int64_t at = 0;
        for (int l = a + 1; l < e; ++l) {
            int32_t *dst = d_seg.as<int32_t>() + at;
            at += lv[l].cells;
            forward(Fp[l - 1], dst, l);
            Fp[l] = dst;
        }
        if (e == L) {
            const int sink = nV - 1 - lv[L - 1].a0;
            DG_HIP(hipMemcpyAsync(d_V.p, Fp[L - 1] + ((int64_t)sink * lv[L - 1].k + sink) * B1 + budget, 4, hipMemcpyDeviceToDevice, s));
        }
        for (int l = e - 1; l >= a && l >= h_first; --l) {
            int32_t *cur = back + (l & 1) * level_cells, *scur = sback + (l & 1) * level_cells;
            if (l == L - 1) fill(cur, l, nV - 1 - lv[l].a0);
            else {
                const uint16_t *m = scores(l + 1);
                backward(back + ((l + 1) & 1) * level_cells, cur, l, m);
                if (l < h_last) { backward(sback + ((l + 1) & 1) * level_cells, scur, l, m); ++seeded; }
            }
            if (t < 0 || l != het[(size_t)t]) continue;
            if (t < nh - 1) {                                               // the record of (h_t, h_{t + 1})
                hipLaunchKernelGGL(ph_readout_kernel, dim3((unsigned)lv[l].k), dim3(JT_THREADS), 0, s, Fp[l], (const int32_t *)scur, lv[l].k, B1, lv[l].a0, cls, c0[(size_t)l], c1[(size_t)l],
                                   d_part.as<long long>());
                hipLaunchKernelGGL(ph_finish_kernel, dim3(1), dim3(JT_THREADS), 0, s, (const long long *)d_part.as<long long>(), lv[l].k, lv[l].a0, l, het[(size_t)t + 1],
                                   d_rec.as<dg_dp_phase_margin>() + t);
                ++readouts;
            }
            if (t > 0) hipLaunchKernelGGL(ph_seed_kernel, dim3(jt_blocks((int64_t)lv[l].k * B1, JT_X_BLOCKS), (unsigned)lv[l].k), dim3(JT_THREADS), 0, s, (const int32_t *)cur, scur, lv[l].k, B1,
                                          lv[l].a0, cls, c0[(size_t)l], c1[(size_t)l]);
            --t;
        }
        DG_HIP(hipGetLastError());
    }
    // the caller's arrays are written only if the call succeeds
    std::vector<dg_dp_phase_margin> recs((size_t)nrec);
    int32_t V = NEG_INF;
    if (nrec) DG_HIP(hipMemcpyAsync(recs.data(), d_rec.p, recs.size() * sizeof(dg_dp_phase_margin), hipMemcpyDeviceToHost, s));
    DG_HIP(hipMemcpyAsync(&V, d_V.p, 4, hipMemcpyDeviceToHost, s));
    DG_HIP(hipStreamSynchronize(s));
    for (int q = 0; q < nrec; ++q)
        if (std::max(recs[(size_t)q].cis_value, recs[(size_t)q].trans_value) > V) {
            set_error("%s: record %d (levels %d, %d): cis %d, trans %d exceed the sink's value %d at budget %d", FN, q, recs[(size_t)q].level_a, recs[(size_t)q].level_b,
                      recs[(size_t)q].cis_value, recs[(size_t)q].trans_value, V, budget);
            return DG_ERR_STATE;
        }
    S.ph_stats[0] = nh; S.ph_stats[1] = nrec; S.ph_stats[2] = seeded; S.ph_stats[3] = readouts; S.ph_stats[4] = n_seg; S.ph_stats[5] = M.peak;
    if (nrec) memcpy(records, recs.data(), recs.size() * sizeof(dg_dp_phase_margin));
    *n_records = nrec;
    *best_value = V;
    return DG_OK;
}

// ---- dg_dp_phase_margins_budgets: many called pairs, each at a budget of its own, from one pass at B1 = bmax + 1 (F, B and S mean "at most
// r": planes 0..b are the states of a call at budget b).  Between a het level e and the next one below it S depends only on its seed key
// (e, c0[e], c1[e]) and on B, not on the query, so the one S of ph_call becomes a pool of slots, one per live key; the host plans the slots
// before the first launch (phb_call) and the kernels below are ph_call's with one more grid dimension and the slot, classes and budget from a
// table that is uploaded once.  A slot is two rolling states of the widest level: state (slot, parity of the level).  Gathers as above: every
// word has one owner lane (a slot belongs to one key, a read-out to one query), no atomics, nothing depends on the order of workgroups.
//   * phb_backward_kernel: grid (x blocks, k, live slots of the level): jt_backward_kernel's recurrence on the slot slots[blockIdx.z];
//   * phb_seed_kernel: grid (x blocks, k, keys created at the level): ph_seed_kernel on the slot and classes of seeds[blockIdx.z];
//   * phb_readout_kernel: grid (k, read-outs of the level): ph_readout_kernel on the slot, classes and budget b of reads[blockIdx.y], with
//     U = max over r = 0..b of F[r] + S[b - r]; part = [read-outs][2][k] keys;
//   * phb_finish_kernel: one workgroup per read-out writes the record reads[blockIdx.x].rec.
struct PhbSeed { int32_t slot, c0, c1; };
struct PhbRead { int32_t slot, c0, c1, budget, rec, level_b; };

__global__ __launch_bounds__(JT_THREADS) void phb_backward_kernel(int32_t *__restrict__ pool, int64_t state_cells, int par, const int32_t *__restrict__ slots, int k, int kn, int B1,
                                                                  int a0, int b0n, uint32_t in_base, int T, const uint32_t *__restrict__ oo, const uint32_t *__restrict__ oe,
                                                                  const uint32_t *__restrict__ in_edge, const int32_t *__restrict__ in_dst, const uint16_t *__restrict__ sc) {
    const int64_t slot = slots[blockIdx.z];
    const int32_t *next = pool + (slot * 2 + (par ^ 1)) * state_cells;      // level l + 1
    int32_t *cur = pool + (slot * 2 + par) * state_cells;                   // level l
    const int i = (int)blockIdx.y;
    const uint32_t ou0 = oo[a0 + i], ou1 = oo[a0 + i + 1];
    const int n = k * B1;
    for (int x = (int)(blockIdx.x * JT_THREADS + threadIdx.x); x < n; x += (int)(gridDim.x * JT_THREADS)) {
        const int j = x / B1, r = x - j * B1;
        const uint32_t ov0 = oo[a0 + j], ov1 = oo[a0 + j + 1];
        int best = NEG_INF;
        for (uint32_t ou = ou0; ou < ou1; ++ou) {
            const uint32_t eu = oe[ou] - in_base;                           // rank among the in-edges of level l + 1
            if (eu >= (uint32_t)T) continue;
            const uint32_t pi = (uint32_t)(in_dst[in_base + eu] - b0n);
            const int r1 = r - (int)(in_edge[in_base + eu] >> 31);
            if (pi >= (uint32_t)kn || r1 < 0) continue;
            for (uint32_t ov = ov0; ov < ov1; ++ov) {
                const uint32_t ev = oe[ov] - in_base;
                if (ev >= (uint32_t)T) continue;
                const uint32_t pj = (uint32_t)(in_dst[in_base + ev] - b0n);
                const int r2 = r1 - (int)(in_edge[in_base + ev] >> 31);
                if (pj >= (uint32_t)kn || r2 < 0) continue;
                const int s = next[((int64_t)pi * kn + pj) * B1 + r2];
                if (s == NEG_INF) continue;
                const int d = sc ? (int)sc[(int64_t)eu * T + ev] : 0;
                best = max(best, s + d);
            }
        }
        cur[((int64_t)i * k + j) * B1 + r] = best;
    }
}

__global__ __launch_bounds__(JT_THREADS) void phb_seed_kernel(const int32_t *__restrict__ B, int32_t *__restrict__ pool, int64_t state_cells, int par,
                                                              const PhbSeed *__restrict__ seeds, int k, int B1, int b0, const int32_t *__restrict__ cls) {
    const PhbSeed sd = seeds[blockIdx.z];
    int32_t *S = pool + ((int64_t)sd.slot * 2 + par) * state_cells;
    const int i = (int)blockIdx.y;
    const bool row = (cls ? cls[b0 + i] : b0 + i) == sd.c0;                 // uniform per workgroup
    const int n = k * B1;
    for (int x = (int)(blockIdx.x * JT_THREADS + threadIdx.x); x < n; x += (int)(gridDim.x * JT_THREADS)) {
        const int j = x / B1;
        const int64_t at = (int64_t)i * n + x;                              // ((i * k + j) * B1 + r)
        int v = NEG_INF;
        if (row && (cls ? cls[b0 + j] : b0 + j) == sd.c1) v = B[at];
        S[at] = v;
    }
}

__global__ __launch_bounds__(JT_THREADS) void phb_readout_kernel(const int32_t *__restrict__ F, const int32_t *__restrict__ pool, int64_t state_cells, int par,
                                                                 const PhbRead *__restrict__ reads, int k, int B1, int b0, const int32_t *__restrict__ cls,
                                                                 long long *__restrict__ part_all) {
    __shared__ long long s_key[JT_THREADS / 64];
    const int t = (int)threadIdx.x, i = (int)blockIdx.x;
    const PhbRead rd = reads[blockIdx.y];
    const int32_t *S = pool + ((int64_t)rd.slot * 2 + par) * state_cells;
    long long *part = part_all + (int64_t)blockIdx.y * 2 * k;
    const int c0 = rd.c0, c1 = rd.c1, b = rd.budget;                        // b < B1
    const int ci = cls ? cls[b0 + i] : b0 + i;
    if (ci != c0 && ci != c1) {                                             // uniform: no cell of either order in this row
        if (t == 0) { part[i] = JT_NO_KEY; part[k + i] = JT_NO_KEY; }
        return;
    }
    const int cj_want = ci == c0 ? c1 : c0;                                 // c0 != c1: the level is het
    long long key = JT_NO_KEY;
    for (int j = t; j < k; j += JT_THREADS) {
        if ((cls ? cls[b0 + j] : b0 + j) != cj_want) continue;
        const int32_t *f = F + ((int64_t)i * k + j) * B1, *sv = S + ((int64_t)i * k + j) * B1;
        int best = NEG_INF;
        for (int r = 0; r <= b; ++r) {
            const int fv = f[r], bv = sv[b - r];
            if (fv != NEG_INF && bv != NEG_INF) best = max(best, fv + bv);
        }
        if (best != NEG_INF) key = max(key, jt_key(best, i, j));
    }
    for (int d = 32; d; d >>= 1) key = max(key, __shfl_xor(key, d));
    if ((t & 63) == 0) s_key[t >> 6] = key;
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < JT_THREADS / 64; ++w) key = max(key, s_key[w]);
        part[i] = ci == c0 ? key : JT_NO_KEY;
        part[k + i] = ci == c0 ? JT_NO_KEY : key;
    }
}

__global__ __launch_bounds__(JT_THREADS) void phb_finish_kernel(const long long *__restrict__ part_all, const PhbRead *__restrict__ reads, int k, int b0, int level_a,
                                                                dg_dp_phase_margin *__restrict__ rec) {
    __shared__ long long s_key[2][JT_THREADS / 64];
    const int t = (int)threadIdx.x;
    const PhbRead rd = reads[blockIdx.x];
    const long long *part = part_all + (int64_t)blockIdx.x * 2 * k;
    long long cis = JT_NO_KEY, trans = JT_NO_KEY;
    for (int i = t; i < k; i += JT_THREADS) { cis = max(cis, part[i]); trans = max(trans, part[k + i]); }
    for (int d = 32; d; d >>= 1) { cis = max(cis, __shfl_xor(cis, d)); trans = max(trans, __shfl_xor(trans, d)); }
    if ((t & 63) == 0) { s_key[0][t >> 6] = cis; s_key[1][t >> 6] = trans; }
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < JT_THREADS / 64; ++w) { cis = max(cis, s_key[0][w]); trans = max(trans, s_key[1][w]); }
        dg_dp_phase_margin r;
        r.level_a = level_a; r.level_b = rd.level_b;
        r.cis_value = r.trans_value = NEG_INF;
        r.cis_vertex1 = r.cis_vertex2 = r.trans_vertex1 = r.trans_vertex2 = -1;
        if (cis != JT_NO_KEY) {
            const uint32_t lo = (uint32_t)cis;
            r.cis_vertex1 = b0 + (JT_MAX_K - (int)((lo >> 15) & 0x7FFFu));
            r.cis_vertex2 = b0 + (JT_MAX_K - (int)(lo & 0x7FFFu));
            r.cis_value = (int)(cis >> 32);
        }
        if (trans != JT_NO_KEY) {
            const uint32_t lo = (uint32_t)trans;
            r.trans_vertex1 = b0 + (JT_MAX_K - (int)((lo >> 15) & 0x7FFFu));
            r.trans_vertex2 = b0 + (JT_MAX_K - (int)(lo & 0x7FFFu));
            r.trans_value = (int)(trans >> 32);
        }
        r.reserved[0] = 0; r.reserved[1] = 0;
        rec[rd.rec] = r;
    }
}

// ph_call's schedule once at the largest budget, with the slot pool in place of its one S.  The plan (het levels, keys, slots, the
// per-level launch tables) is a function of called, vertex_class and the graph, made and uploaded before the first launch: the level loop
// has the launches of ph_call's and nothing that waits for the device.
int phb_call(dg_ctx *c, const int32_t *called, const int32_t *budgets, int64_t n, const int32_t *vertex_class, dg_dp_phase_margin *records, int64_t *record_off,
             int32_t *best_values) {
    const char *FN = "dg_dp_phase_margins_budgets";
    DpState *Sp = c->dp;
    if (!Sp || !Sp->loaded) { set_error("%s: no graph loaded", FN); return DG_ERR_STATE; }
    DpState &S = *Sp;
    if (n < 1) { set_error("%s: n_called = %lld", FN, (long long)n); return DG_ERR_ARG; }
    if (!called || !budgets || !records || !record_off || !best_values) { set_error("%s: called, budgets, records, record_off and best_values are required", FN); return DG_ERR_ARG; }
    if (n > JT_MAX_QUERIES) { set_error("%s: %lld called pairs exceed %d per call", FN, (long long)n, JT_MAX_QUERIES); return DG_ERR_UNSUPPORTED; }
    int32_t budget = 0;                                                     // the pass runs at the largest budget
    for (int64_t q = 0; q < n; ++q) {
        if (budgets[q] < 0) { set_error("%s: query %lld: budget %d is negative", FN, (long long)q, budgets[q]); return DG_ERR_ARG; }
        budget = std::max(budget, budgets[q]);
    }
    if ((int64_t)budget + 1 > JT_MAX_PLANES) { set_error("%s: budget + 1 = %lld exceeds %d planes", FN, (long long)budget + 1, JT_MAX_PLANES); return DG_ERR_UNSUPPORTED; }
    const int L = S.L, nV = S.nV, B1 = budget + 1;
    if (L < 2 || (int)S.descs.size() < L) { set_error("%s: the loaded graph has %d levels", FN, L); return DG_ERR_STATE; }
    std::vector<JtLevel> lv((size_t)L);
    int kmax = 1;
    int64_t tmax = 0;
    for (int l = 0; l < L; ++l) {
        const LevelDesc &d = S.descs[(size_t)std::max(l, 1)];
        lv[l] = l ? JtLevel{d.b0, d.k2, d.in_base, d.T, d.delta_off >= 0, 0} : JtLevel{d.a0, d.k, 0u, 0, false, 0};
        lv[l].cells = (int64_t)lv[l].k * lv[l].k * B1;
        kmax = std::max(kmax, lv[l].k);
        if (lv[l].coloured) tmax = std::max<int64_t>(tmax, lv[l].T);
    }
    if (kmax > JT_MAX_K) { set_error("%s: widest level %d exceeds %d", FN, kmax, JT_MAX_K); return DG_ERR_UNSUPPORTED; }
    for (int64_t q = 0; q < n; ++q)
        for (int row = 0; row < 2; ++row)
            for (int l = 0; l < L; ++l) {
                const int32_t v = called[(q * 2 + row) * L + l];
                if ((uint32_t)(v - lv[l].a0) >= (uint32_t)lv[l].k) {
                    set_error("%s: query %lld row %d level %d: vertex %d is not in its level", FN, (long long)q, row, l, v);
                    return DG_ERR_ARG;
                }
            }
    // ---- the plan.  Per query: its het levels ascending with the called ordered classes there (het_*[het_off[q] ..)), its records' place.
    // q carries on h_0 <= l < h_last; its key there is (e, c0[e], c1[e]) with e its nearest het level above l.  The key of a query changes
    // only at its own het levels, so the levels below walk at_q: per level, the queries that are het there (ascending), and nothing else ----
    struct Key { int32_t e, c0, c1; bool operator<(const Key &o) const { return e != o.e ? e < o.e : c0 != o.c0 ? c0 < o.c0 : c1 < o.c1; } };
    std::vector<int64_t> roff((size_t)n + 1, 0), het_off((size_t)n + 1, 0), at_off((size_t)L + 1, 0);
    std::vector<int32_t> het_l, het_c0, het_c1;
    int h_first = L;                                                        // the smallest h_0 of a query with a record; L: nothing backward at all
    for (int64_t q = 0; q < n; ++q) {
        for (int l = 0; l < L; ++l) {
            const int32_t v0 = called[(q * 2) * L + l], v1 = called[(q * 2 + 1) * L + l];
            const int32_t a = vertex_class ? vertex_class[v0] : v0, b = vertex_class ? vertex_class[v1] : v1;
            if (a != b) { het_l.push_back(l); het_c0.push_back(a); het_c1.push_back(b); }
        }
        het_off[(size_t)q + 1] = (int64_t)het_l.size();
        const int64_t nh = het_off[(size_t)q + 1] - het_off[(size_t)q];
        roff[(size_t)q + 1] = roff[(size_t)q] + std::max<int64_t>(nh - 1, 0);
        if (nh < 2) continue;
        h_first = std::min(h_first, (int)het_l[(size_t)het_off[(size_t)q]]);
        for (int64_t x = het_off[(size_t)q]; x < het_off[(size_t)q + 1]; ++x) ++at_off[(size_t)het_l[(size_t)x] + 1];
    }
    const int64_t nrec = roff[(size_t)n];
    for (int l = 0; l < L; ++l) at_off[(size_t)l + 1] += at_off[(size_t)l];
    std::vector<int32_t> at_q((size_t)at_off[(size_t)L]);                   // the queries with a record that are het on l: at_q[at_off[l] .. at_off[l + 1])
    std::vector<int64_t> het_at((size_t)n);                                 // going down the levels: where in het_* the next het level of q stands
    {
        std::vector<int64_t> next(at_off.begin(), at_off.end() - 1);
        for (int64_t q = 0; q < n; ++q) {
            het_at[(size_t)q] = het_off[(size_t)q + 1] - 1;
            if (het_off[(size_t)q + 1] - het_off[(size_t)q] < 2) continue;
            for (int64_t x = het_off[(size_t)q]; x < het_off[(size_t)q + 1]; ++x) at_q[(size_t)next[(size_t)het_l[(size_t)x]]++] = (int32_t)q;
        }
    }
    // the levels from the top: the slots live on l, the read-outs at l, the keys seeded at l (live on l - 1, not on l)
    std::vector<int32_t> live_off((size_t)L + 1, 0), read_off((size_t)L + 1, 0), seed_off((size_t)L + 1, 0), live_tab;   // tables in descending level order: entry L - 1 - l
    std::vector<PhbRead> read_tab;
    std::vector<PhbSeed> seed_tab;
    int64_t keys_created = 0, slot_levels = 0, back_launches = 0, read_launches = 0, max_live = 0, max_part = 1;
    int n_slots = 0;
    {
        struct Held { int32_t slot, queries; };
        std::map<Key, Held> live;                                           // the keys live on the level at hand -> slot, and how many queries carry it
        std::vector<std::map<Key, Held>::iterator> freed;
        std::vector<Key> born;
        std::vector<int32_t> free_slots;                                    // kept descending: the smallest is taken first
        for (int l = L - 1; l >= 0; --l) {
            const size_t at = (size_t)(L - 1 - l);
            for (const auto &kv : live) live_tab.push_back(kv.second.slot);
            live_off[at + 1] = (int32_t)live_tab.size();
            const int64_t nl = (int64_t)live.size();
            if (nl) { slot_levels += nl; ++back_launches; max_live = std::max(max_live, nl); }
            freed.clear();
            born.clear();
            for (int64_t i = at_off[(size_t)l]; i < at_off[(size_t)l + 1]; ++i) {
                const int64_t q = at_q[(size_t)i], x = het_at[(size_t)q]--, t = x - het_off[(size_t)q];   // (het_l[x] == l)
                if (x + 1 < het_off[(size_t)q + 1]) {                       // q carries on l: its record of (l, e), and it leaves the key of e here
                    const int32_t e = het_l[(size_t)x + 1];
                    const auto it = live.find(Key{e, het_c0[(size_t)x + 1], het_c1[(size_t)x + 1]});
                    read_tab.push_back(PhbRead{it->second.slot, het_c0[(size_t)x], het_c1[(size_t)x], budgets[q], (int32_t)(roff[(size_t)q] + t), e});
                    if (--it->second.queries == 0) freed.push_back(it);
                }
                if (t > 0) born.push_back(Key{l, het_c0[(size_t)x], het_c1[(size_t)x]});   // and carries the key of l below
            }
            read_off[at + 1] = (int32_t)read_tab.size();
            const int64_t nr = read_off[at + 1] - read_off[at];
            if (nr) { ++read_launches; max_part = std::max(max_part, nr * 2 * lv[l].k); }
            for (const auto &it : freed) { free_slots.push_back(it->second.slot); live.erase(it); }
            std::sort(free_slots.begin(), free_slots.end(), std::greater<int32_t>());
            std::sort(born.begin(), born.end());
            for (size_t i = 0; i < born.size(); ++i) {
                if (i && !(born[i - 1] < born[i])) { ++live.find(born[i])->second.queries; continue; }
                int32_t slot;
                if (free_slots.empty()) slot = n_slots++;                   // a key seeded here may take a slot freed here
                else { slot = free_slots.back(); free_slots.pop_back(); }
                live.emplace(born[i], Held{slot, 1});
                seed_tab.push_back(PhbSeed{slot, born[i].c0, born[i].c1});
                ++keys_created;
            }
            seed_off[at + 1] = (int32_t)seed_tab.size();
        }
    }
    hipStream_t s = c->stream;
    // ---- segments [seg[g], seg[g + 1]) whose forward states fit joint_state_bytes (at least one level each) ----
    std::vector<int> seg{0};
    {
        int64_t in_seg = 0;
        for (int l = 0; l < L; ++l) {
            const int64_t bytes = 4 * lv[l].cells;
            if (l > seg.back() && in_seg + bytes > S.opt.joint_state_bytes) { seg.push_back(l); in_seg = 0; }
            in_seg += bytes;
        }
    }
    const int n_seg = (int)seg.size();
    seg.push_back(L);
    std::vector<int64_t> ck_off((size_t)n_seg + 1, 0);                     // F of every segment's first level, int32 units
    int64_t seg_cells = 1, roll_cells = 0, level_cells = 1;
    for (int g = 0; g < n_seg; ++g) {
        ck_off[g + 1] = ck_off[g] + lv[seg[g]].cells;
        int64_t sum = 0;
        for (int l = seg[g] + 1; l < seg[g + 1]; ++l) { sum += lv[l].cells; if (g + 1 < n_seg) roll_cells = std::max(roll_cells, lv[l].cells); }
        seg_cells = std::max(seg_cells, sum);
    }
    for (int l = 0; l < L; ++l) level_cells = std::max(level_cells, lv[l].cells);
    JtMem M;
    DevBuf d_cls, d_rec, d_V, d_part, d_live, d_reads, d_seeds, d_oo, d_ocur, d_oe, d_sc, d_ck, d_roll, d_seg, d_back, d_pool;
    if (vertex_class) if (int rc = M.get(d_cls, (int64_t)nV * 4)) return rc;
    if (int rc = M.get(d_rec, std::max<int64_t>(nrec, 1) * (int64_t)sizeof(dg_dp_phase_margin))) return rc;
    if (int rc = M.get(d_V, (int64_t)B1 * 4)) return rc;
    if (int rc = M.get(d_part, max_part * 8)) return rc;
    if (tmax) if (int rc = M.get(d_sc, tmax * tmax * 2)) return rc;
    if (int rc = M.get(d_ck, ck_off[n_seg] * 4)) return rc;
    if (vertex_class) DG_HIP(hipMemcpyAsync(d_cls.p, vertex_class, (size_t)nV * 4, hipMemcpyHostToDevice, s));
    const int32_t *cls = vertex_class ? (const int32_t *)d_cls.as<int32_t>() : nullptr;
    const LevelDesc *descs = S.d_descs.as<LevelDesc>();
    const uint32_t *in_off = S.d_in_off.as<uint32_t>(), *in_edge = S.d_in_edge.as<uint32_t>();
    const int32_t *in_dst = S.d_in_dst.as<int32_t>();
    uint16_t *sc = d_sc.as<uint16_t>();
    if (nrec) {                                                             // the launch tables, once; the in-edges grouped by source
        if (int rc = M.get(d_live, (int64_t)std::max<size_t>(live_tab.size(), 1) * 4)) return rc;
        if (int rc = M.get(d_reads, (int64_t)std::max<size_t>(read_tab.size(), 1) * (int64_t)sizeof(PhbRead))) return rc;
        if (int rc = M.get(d_seeds, (int64_t)std::max<size_t>(seed_tab.size(), 1) * (int64_t)sizeof(PhbSeed))) return rc;
        if (!live_tab.empty()) DG_HIP(hipMemcpyAsync(d_live.p, live_tab.data(), live_tab.size() * 4, hipMemcpyHostToDevice, s));
        if (!read_tab.empty()) DG_HIP(hipMemcpyAsync(d_reads.p, read_tab.data(), read_tab.size() * sizeof(PhbRead), hipMemcpyHostToDevice, s));
        if (!seed_tab.empty()) DG_HIP(hipMemcpyAsync(d_seeds.p, seed_tab.data(), seed_tab.size() * sizeof(PhbSeed), hipMemcpyHostToDevice, s));
        if (int rc = M.get(d_oo, ((int64_t)nV + 1) * 4)) return rc;
        if (int rc = M.get(d_ocur, (int64_t)nV * 4)) return rc;
        if (int rc = M.get(d_oe, S.n_edges * 4)) return rc;
        DG_HIP(hipMemsetAsync(d_ocur.p, 0, (size_t)nV * 4, s));
        hipLaunchKernelGGL(jt_out_count_kernel, dim3((unsigned)(L - 1)), dim3(JT_THREADS), 0, s, descs, L, nV, in_edge, d_ocur.as<uint32_t>());
        hipLaunchKernelGGL(jt_out_scan_kernel, dim3(1), dim3(1024), 0, s, d_ocur.as<uint32_t>(), d_oo.as<uint32_t>(), d_ocur.as<uint32_t>(), nV);
        hipLaunchKernelGGL(jt_out_fill_kernel, dim3((unsigned)(L - 1)), dim3(JT_THREADS), 0, s, descs, L, nV, in_edge, d_ocur.as<uint32_t>(), d_oe.as<uint32_t>(), (uint32_t)S.n_edges);
        DG_HIP(hipGetLastError());
    }
    auto scores = [&](int l) -> const uint16_t * {                          // the matrix of the transition into level l, in d_sc
        const int T = lv[l].T;
        if (!lv[l].coloured || T < 1) return nullptr;
        hipLaunchKernelGGL(jt_scores_kernel, dim3(jt_blocks(T, 64), (unsigned)std::min(T, 16384)), dim3(JT_THREADS), 0, s, T, lv[l].in_base, lv[l - 1].a0, in_edge, in_dst,
                           colour_csr(S), S.d_eflag.as<uint8_t>(), S.d_eself.as<uint16_t>(), sc);
        return sc;
    };
    auto fill = [&](int32_t *st, int l, int pos) {                          // level l: 0 on every plane of the cell (pos, pos)
        hipLaunchKernelGGL(jt_fill_kernel, dim3(jt_blocks(lv[l].cells, 65536)), dim3(JT_THREADS), 0, s, st, lv[l].cells, ((int64_t)pos * lv[l].k + pos) * B1, B1);
    };
    auto forward = [&](const int32_t *prev, int32_t *cur, int l) {
        const uint16_t *m = scores(l);
        hipLaunchKernelGGL(jt_forward_kernel, dim3(jt_blocks((int64_t)lv[l].k * B1, JT_X_BLOCKS), (unsigned)lv[l].k), dim3(JT_THREADS), 0, s, prev, cur, lv[l - 1].k, lv[l].k, B1,
                           lv[l].a0, lv[l].in_base, lv[l].T, in_off, in_edge, m);
    };
    // ---- pass 1: the state at every segment's first level ----
    int32_t *ck = d_ck.as<int32_t>();
    fill(ck, 0, 0);
    if (n_seg > 1) {
        if (int rc = M.get(d_roll, 2 * roll_cells * 4)) return rc;
        int32_t *roll = d_roll.as<int32_t>();
        const int32_t *prev = ck;
        int g = 0;
        for (int l = 1; l <= seg[n_seg - 1]; ++l) {
            int32_t *dst = l == seg[g + 1] ? ck + ck_off[++g] : roll + (l & 1) * roll_cells;
            forward(prev, dst, l);
            prev = dst;
        }
        DG_HIP(hipGetLastError());
        DG_HIP(hipStreamSynchronize(s));                                    // the rolling states go before the segment buffers come
        M.drop(d_roll);
    }
    // ---- the segments, last first, down to the one that holds the smallest first het level ----
    if (int rc = M.get(d_seg, seg_cells * 4)) return rc;
    if (nrec) {
        if (int rc = M.get(d_back, 2 * level_cells * 4)) return rc;
        if (int rc = M.get(d_pool, (int64_t)std::max(n_slots, 1) * 2 * level_cells * 4)) return rc;
    }
    int32_t *back = d_back.as<int32_t>(), *pool = d_pool.as<int32_t>();
    const int32_t *live_d = d_live.as<int32_t>();
    const PhbRead *reads_d = d_reads.as<PhbRead>();
    const PhbSeed *seeds_d = d_seeds.as<PhbSeed>();
    dg_dp_phase_margin *rec_d = d_rec.as<dg_dp_phase_margin>();
    std::vector<const int32_t *> Fp((size_t)L, nullptr);
    for (int g = n_seg - 1; g >= 0; --g) {
        const int a = seg[g], e = seg[g + 1];
        if (e <= h_first && g < n_seg - 1) break;                           // nothing is read out below the first het level
        Fp[a] = ck + ck_off[g];
        int64_t at = 0;
        for (int l = a + 1; l < e; ++l) {
            int32_t *dst = d_seg.as<int32_t>() + at;
            at += lv[l].cells;
            forward(Fp[l - 1], dst, l);
            Fp[l] = dst;
        }
        if (e == L) {                                                       // V_b for every budget: the sink's planes
            const int sink = nV - 1 - lv[L - 1].a0;
            DG_HIP(hipMemcpyAsync(d_V.p, Fp[L - 1] + ((int64_t)sink * lv[L - 1].k + sink) * B1, (size_t)B1 * 4, hipMemcpyDeviceToDevice, s));
        }
        for (int l = e - 1; l >= a && l >= h_first; --l) {
            const size_t lx = (size_t)(L - 1 - l);
            const int par = l & 1;
            int32_t *cur = back + par * level_cells;
            const unsigned xb = jt_blocks((int64_t)lv[l].k * B1, JT_X_BLOCKS);
            if (l == L - 1) fill(cur, l, nV - 1 - lv[l].a0);
            else {
                const uint16_t *m = scores(l + 1);
                hipLaunchKernelGGL(jt_backward_kernel, dim3(xb, (unsigned)lv[l].k), dim3(JT_THREADS), 0, s, (const int32_t *)(back + (par ^ 1) * level_cells), cur, lv[l].k, lv[l + 1].k, B1,
                                   lv[l].a0, lv[l + 1].a0, lv[l + 1].in_base, lv[l + 1].T, d_oo.as<uint32_t>(), d_oe.as<uint32_t>(), in_edge, in_dst, m);
                if (const int nl = live_off[lx + 1] - live_off[lx])         // every live slot down one level, on the same matrix
                    hipLaunchKernelGGL(phb_backward_kernel, dim3(xb, (unsigned)lv[l].k, (unsigned)nl), dim3(JT_THREADS), 0, s, pool, level_cells, par, live_d + live_off[lx], lv[l].k,
                                       lv[l + 1].k, B1, lv[l].a0, lv[l + 1].a0, lv[l + 1].in_base, lv[l + 1].T, d_oo.as<uint32_t>(), d_oe.as<uint32_t>(), in_edge, in_dst, m);
            }
            if (const int nr = read_off[lx + 1] - read_off[lx]) {           // before the seeds: a slot freed here may be seeded here
                hipLaunchKernelGGL(phb_readout_kernel, dim3((unsigned)lv[l].k, (unsigned)nr), dim3(JT_THREADS), 0, s, Fp[l], (const int32_t *)pool, level_cells, par,
                                   reads_d + read_off[lx], lv[l].k, B1, lv[l].a0, cls, d_part.as<long long>());
                hipLaunchKernelGGL(phb_finish_kernel, dim3((unsigned)nr), dim3(JT_THREADS), 0, s, (const long long *)d_part.as<long long>(), reads_d + read_off[lx], lv[l].k, lv[l].a0, l, rec_d);
            }
            if (const int ns = seed_off[lx + 1] - seed_off[lx])
                hipLaunchKernelGGL(phb_seed_kernel, dim3(xb, (unsigned)lv[l].k, (unsigned)ns), dim3(JT_THREADS), 0, s, (const int32_t *)cur, pool, level_cells, par, seeds_d + seed_off[lx],
                                   lv[l].k, B1, lv[l].a0, cls);
        }
        DG_HIP(hipGetLastError());
    }
    // the caller's arrays are written only if the call succeeds
    std::vector<dg_dp_phase_margin> recs((size_t)nrec);
    std::vector<int32_t> Vs((size_t)B1, NEG_INF);
    if (nrec) DG_HIP(hipMemcpyAsync(recs.data(), d_rec.p, recs.size() * sizeof(dg_dp_phase_margin), hipMemcpyDeviceToHost, s));
    DG_HIP(hipMemcpyAsync(Vs.data(), d_V.p, Vs.size() * 4, hipMemcpyDeviceToHost, s));
    DG_HIP(hipStreamSynchronize(s));
    for (int64_t q = 0; q < n; ++q)
        for (int64_t x = roff[(size_t)q]; x < roff[(size_t)q + 1]; ++x)
            if (std::max(recs[(size_t)x].cis_value, recs[(size_t)x].trans_value) > Vs[(size_t)budgets[q]]) {
                set_error("%s: query %lld record %lld (levels %d, %d): cis %d, trans %d exceed the sink's value %d at budget %d", FN, (long long)q, (long long)(x - roff[(size_t)q]),
                          recs[(size_t)x].level_a, recs[(size_t)x].level_b, recs[(size_t)x].cis_value, recs[(size_t)x].trans_value, Vs[(size_t)budgets[q]], budgets[q]);
                return DG_ERR_STATE;
            }
    const int64_t st[10] = {n, nrec, keys_created, slot_levels, back_launches, read_launches, max_live, nrec ? n_slots : 0, n_seg, M.peak};
    for (int x = 0; x < 10; ++x) S.phb_stats[x] = st[x];
    if (nrec) memcpy(records, recs.data(), recs.size() * sizeof(dg_dp_phase_margin));
    for (int64_t q = 0; q <= n; ++q) record_off[q] = roff[(size_t)q];
    for (int64_t q = 0; q < n; ++q) best_values[q] = Vs[(size_t)budgets[q]];
    return DG_OK;
}

// ---- dg_dp_recombination_margins: per transition l -> l + 1 and s = 0, 1, 2 the best pair of paths that takes a hop pair of weight
// sum s there, E[s] = max F_l[i][j][r] + d + B_{l+1}[i'][j'][b - s - r], with the hop pair that attains it (include/dipgenie_hip.h has the
// definition).  A key is two words, compared one after the other, larger = better:
//   word 0 = value << 32 | (JT_MAX_K - i)           value descending, then i ascending        (JT_NO_KEY: no hop pair)
//   word 1 = (JT_MAX_K - j) << 30 | (JT_MAX_K - i') << 15 | (JT_MAX_K - j')                    then j, i', j' ascending
// so the winner is a function of the set of candidates alone, not of the order lanes or workgroups meet them in.  F, B and d are symmetric
// in the two haplotypes: the tuple (j, i, j', i') is worth what (i, j, i', j') is and, where i > j, comes before it in the tie order, so
// the cells j >= i hold every winner and the lanes of j < i do nothing.
//   * rb_edges_kernel: grid (x blocks, k) as jt_backward_kernel: row i = blockIdx.y, the lanes stride over (j, r).  A lane loads
//     F_l[i][j][r] once, and only where that is reachable walks out(i) x out(j) with three running maxima of F + d + B_{l+1}[i'][j'][b - s - r],
//     one per s: inside a cell i and j are fixed, so a candidate is one signed 64-bit word value << 32 | (JT_MAX_K - i') << 15 | (JT_MAX_K - j')
//     and the update one maximum; the cell's winners are folded into the lane's two-word keys once per cell, and the workgroup reduces per s
//     (__shfl_xor, one LDS slot per wave) to part[s][i][blockIdx.x];
//   * rb_finish_kernel: workgroup s < 3 reduces part[s][.][.] to the words of the level's record that belong to s (workgroup 0 the
//     level too); the workgroups from 3 on answer called_out, one wave per query: the lanes search the in-edges of the two called
//     destinations for the called sources (the first such in-edge: parallel edges share weight and score), then stride over r.
__device__ __forceinline__ bool rb_better(long long a0, long long a1, long long b0, long long b1) { return a0 > b0 || (a0 == b0 && a1 > b1); }

// F = level l [k][k][B1], next = B of level l + 1 [kn][kn][B1]; a0 / b0n = first vertex of level l / l + 1, in_base / T = the in-edges of
// level l + 1, sc = their scores (null: all zero); oo / oe = the out-index; part = [3][k][gridDim.x][2]
__global__ __launch_bounds__(JT_THREADS) void rb_edges_kernel(const int32_t *__restrict__ F, const int32_t *__restrict__ next, int k, int kn, int B1, int a0, int b0n,
                                                              uint32_t in_base, int T, const uint32_t *__restrict__ oo, const uint32_t *__restrict__ oe,
                                                              const uint32_t *__restrict__ in_edge, const int32_t *__restrict__ in_dst, const uint16_t *__restrict__ sc,
                                                              long long *__restrict__ part) {
    __shared__ long long s_key[3][JT_THREADS / 64][2];
    const int t = (int)threadIdx.x, i = (int)blockIdx.y;
    const uint32_t ou0 = oo[a0 + i], ou1 = oo[a0 + i + 1];
    const int n = k * B1;
    long long a0k = JT_NO_KEY, a1k = JT_NO_KEY, a2k = JT_NO_KEY, b0k = 0, b1k = 0, b2k = 0;      // the lane's best key per s
    for (int x = (int)(blockIdx.x * JT_THREADS + threadIdx.x); x < n; x += (int)(gridDim.x * JT_THREADS)) {
        const int j = x / B1, r = x - j * B1;
        if (j < i) continue;
        const int f = F[((int64_t)i * k + j) * B1 + r];
        if (f == NEG_INF) continue;                                         // nothing of B is read for an unreachable cell
        const uint32_t ov0 = oo[a0 + j], ov1 = oo[a0 + j + 1];
        // inside one cell i and j are fixed: a candidate is value << 32 | (JT_MAX_K - i') << 15 | (JT_MAX_K - j'), one signed maximum per s
        long long c0 = JT_NO_KEY, c1 = JT_NO_KEY, c2 = JT_NO_KEY;
        for (uint32_t ou = ou0; ou < ou1; ++ou) {
            const uint32_t eu = oe[ou] - in_base;                           // rank among the in-edges of level l + 1
            if (eu >= (uint32_t)T) continue;
            const uint32_t pi = (uint32_t)(in_dst[in_base + eu] - b0n);
            const int w1 = (int)(in_edge[in_base + eu] >> 31);
            if (pi >= (uint32_t)kn || B1 - 1 - r - w1 < 0) continue;
            const uint32_t hi = (uint32_t)(JT_MAX_K - (int)pi) << 15;
            for (uint32_t ov = ov0; ov < ov1; ++ov) {
                const uint32_t ev = oe[ov] - in_base;
                if (ev >= (uint32_t)T) continue;
                const uint32_t pj = (uint32_t)(in_dst[in_base + ev] - b0n);
                const int w = w1 + (int)(in_edge[in_base + ev] >> 31);
                const int r2 = B1 - 1 - r - w;                              // what is left for B
                if (pj >= (uint32_t)kn || r2 < 0) continue;
                const int s = next[((int64_t)pi * kn + pj) * B1 + r2];
                if (s == NEG_INF) continue;
                const int v = f + s + (sc ? (int)sc[(int64_t)eu * T + ev] : 0);
                const long long cand = (long long)(((unsigned long long)(uint32_t)v << 32) | hi | (uint32_t)(JT_MAX_K - (int)pj));
                if (w == 0) c0 = max(c0, cand);
                else if (w == 1) c1 = max(c1, cand);
                else c2 = max(c2, cand);
            }
        }
        auto fold = [&](long long c, long long &a, long long &b) {           // the cell's winner of one s against the lane's
            if (c == JT_NO_KEY) return;
            const long long ca = (long long)(((unsigned long long)c & 0xFFFFFFFF00000000ull) | (uint32_t)(JT_MAX_K - i));
            const long long cb = ((long long)(JT_MAX_K - j) << 30) | (c & 0x3FFFFFFF);
            if (rb_better(ca, cb, a, b)) { a = ca; b = cb; }
        };
        fold(c0, a0k, b0k);
        fold(c1, a1k, b1k);
        fold(c2, a2k, b2k);
    }
    auto reduce = [&](int s, long long a, long long b) {                    // the wave's best key of bucket s into its LDS slot
        for (int d = 32; d; d >>= 1) {
            const long long oa = __shfl_xor(a, d), ob = __shfl_xor(b, d);
            if (rb_better(oa, ob, a, b)) { a = oa; b = ob; }
        }
        if ((t & 63) == 0) { s_key[s][t >> 6][0] = a; s_key[s][t >> 6][1] = b; }
    };
    reduce(0, a0k, b0k);
    reduce(1, a1k, b1k);
    reduce(2, a2k, b2k);
    __syncthreads();
    if (t < 3) {
        long long a = s_key[t][0][0], b = s_key[t][0][1];
        for (int w = 1; w < JT_THREADS / 64; ++w)
            if (rb_better(s_key[t][w][0], s_key[t][w][1], a, b)) { a = s_key[t][w][0]; b = s_key[t][w][1]; }
        long long *out = part + (((int64_t)t * k + i) * gridDim.x + blockIdx.x) * 2;
        out[0] = a; out[1] = b;
    }
}

// grid: 3 + ceil(n / 4) workgroups.  part = [3][k][nx][2] of rb_edges_kernel; rec = the record of level l; F, next, sc and the level's
// numbers as above; called = [n][2][L] (validated by the host); cout = [n][L - 1][2]
__global__ __launch_bounds__(JT_THREADS) void rb_finish_kernel(const long long *__restrict__ part, int k, int nx, int a0, int b0n, int l, dg_dp_recombination_margin *__restrict__ rec,
                                                               const int32_t *__restrict__ F, const int32_t *__restrict__ next, int kn, int B1, uint32_t in_base, int T,
                                                               const uint32_t *__restrict__ in_off, const uint32_t *__restrict__ in_edge, const uint16_t *__restrict__ sc,
                                                               const int32_t *__restrict__ called, int n, int L, int32_t *__restrict__ cout) {
    __shared__ long long s_key[JT_THREADS / 64][2];
    const int t = (int)threadIdx.x;
    if (blockIdx.x < 3) {                                                   // uniform per workgroup
        const int s = (int)blockIdx.x;
        const long long *p = part + (int64_t)s * k * nx * 2;
        long long a = JT_NO_KEY, b = 0;
        for (int64_t x = t; x < (int64_t)k * nx; x += JT_THREADS)
            if (rb_better(p[2 * x], p[2 * x + 1], a, b)) { a = p[2 * x]; b = p[2 * x + 1]; }
        for (int d = 32; d; d >>= 1) {
            const long long oa = __shfl_xor(a, d), ob = __shfl_xor(b, d);
            if (rb_better(oa, ob, a, b)) { a = oa; b = ob; }
        }
        if ((t & 63) == 0) { s_key[t >> 6][0] = a; s_key[t >> 6][1] = b; }
        __syncthreads();
        if (t == 0) {
            for (int w = 1; w < JT_THREADS / 64; ++w)
                if (rb_better(s_key[w][0], s_key[w][1], a, b)) { a = s_key[w][0]; b = s_key[w][1]; }
            if (s == 0) rec->level = l;
            if (a == JT_NO_KEY) { rec->value[s] = NEG_INF; rec->from1[s] = rec->from2[s] = rec->to1[s] = rec->to2[s] = -1; }
            else {
                rec->value[s] = (int)(a >> 32);
                rec->from1[s] = a0 + (JT_MAX_K - (int)(a & 0x7FFF));
                rec->from2[s] = a0 + (JT_MAX_K - (int)((b >> 30) & 0x7FFF));
                rec->to1[s] = b0n + (JT_MAX_K - (int)((b >> 15) & 0x7FFF));
                rec->to2[s] = b0n + (JT_MAX_K - (int)(b & 0x7FFF));
            }
        }
        return;
    }
    const int q = ((int)blockIdx.x - 3) * (JT_THREADS / 64) + (t >> 6), lane = t & 63;      // uniform per wave
    if (q >= n) return;
    uint32_t e[2];                                                          // the first in-edge of each called hop, UINT32_MAX: no edge
    int pos[2], posn[2];
    for (int h = 0; h < 2; ++h) {
        const int u = called[((int64_t)q * 2 + h) * L + l], v = called[((int64_t)q * 2 + h) * L + l + 1];
        pos[h] = u - a0; posn[h] = v - b0n;
        uint32_t at = UINT32_MAX;
        for (uint32_t x = in_off[v] + (uint32_t)lane; x < in_off[v + 1]; x += 64)
            if ((in_edge[x] & 0x7FFFFFFFu) == (uint32_t)pos[h] && x - in_base < (uint32_t)T) at = min(at, x);
        for (int d = 32; d; d >>= 1) at = min(at, (uint32_t)__shfl_xor((int)at, d));
        e[h] = at;
    }
    int s = -1, best = NEG_INF;
    if (e[0] != UINT32_MAX && e[1] != UINT32_MAX) {
        s = (int)(in_edge[e[0]] >> 31) + (int)(in_edge[e[1]] >> 31);
        const int d = sc ? (int)sc[(int64_t)(e[0] - in_base) * T + (e[1] - in_base)] : 0;
        const int32_t *f = F + ((int64_t)pos[0] * k + pos[1]) * B1, *b = next + ((int64_t)posn[0] * kn + posn[1]) * B1;
        for (int r = lane; r <= B1 - 1 - s; r += 64) {
            const int fv = f[r], bv = b[B1 - 1 - s - r];
            if (fv != NEG_INF && bv != NEG_INF) best = max(best, fv + d + bv);
        }
        for (int w = 32; w; w >>= 1) best = max(best, __shfl_xor(best, w));
    }
    if (lane == 0) {
        int32_t *out = cout + ((int64_t)q * (L - 1) + l) * 2;
        out[0] = s; out[1] = best;
    }
}

// jt_call's schedule (plan by joint_state_bytes, forward checkpoints of pass 1, the segments from the last to the first with F
// recomputed, B rolling in two states) with the two rb_* launches per level l < L - 1 in place of that call's combination, record and
// table launches.  B crosses a segment boundary in its rolling state as it does there.  B_0 is not formed: nothing reads it.
int rb_call(dg_ctx *c, int32_t budget, const int32_t *called, int64_t n, dg_dp_recombination_margin *records, int32_t *called_out, int32_t *best_value) {
    const char *FN = "dg_dp_recombination_margins";
    DpState *Sp = c->dp;
    if (!Sp || !Sp->loaded) { set_error("%s: no graph loaded", FN); return DG_ERR_STATE; }
    DpState &S = *Sp;
    if (!records || !best_value) { set_error("%s: records and best_value are required", FN); return DG_ERR_ARG; }
    if (n < 0 || (n > 0 && (!called || !called_out))) { set_error("%s: n_called = %lld needs called and called_out", FN, (long long)n); return DG_ERR_ARG; }
    if (budget < 0) { set_error("%s: budget %d is negative", FN, budget); return DG_ERR_ARG; }
    if (n > JT_MAX_QUERIES) { set_error("%s: %lld called pairs exceed %d per call", FN, (long long)n, JT_MAX_QUERIES); return DG_ERR_UNSUPPORTED; }
    if ((int64_t)budget + 1 > JT_MAX_PLANES) { set_error("%s: budget + 1 = %lld exceeds %d planes", FN, (long long)budget + 1, JT_MAX_PLANES); return DG_ERR_UNSUPPORTED; }
    const int L = S.L, nV = S.nV, B1 = budget + 1;
    if (L < 2 || (int)S.descs.size() < L) { set_error("%s: the loaded graph has %d levels", FN, L); return DG_ERR_STATE; }
    std::vector<JtLevel> lv((size_t)L);
    int kmax = 1;
    int64_t tmax = 0, part_keys = 1;
    for (int l = 0; l < L; ++l) {
        const LevelDesc &d = S.descs[(size_t)std::max(l, 1)];
        lv[l] = l ? JtLevel{d.b0, d.k2, d.in_base, d.T, d.delta_off >= 0, 0} : JtLevel{d.a0, d.k, 0u, 0, false, 0};
        lv[l].cells = (int64_t)lv[l].k * lv[l].k * B1;
        kmax = std::max(kmax, lv[l].k);
        if (lv[l].coloured) tmax = std::max<int64_t>(tmax, lv[l].T);
        if (l < L - 1) part_keys = std::max(part_keys, (int64_t)3 * lv[l].k * jt_blocks((int64_t)lv[l].k * B1, JT_X_BLOCKS));
    }
    if (kmax > JT_MAX_K) { set_error("%s: widest level %d exceeds %d", FN, kmax, JT_MAX_K); return DG_ERR_UNSUPPORTED; }
    for (int64_t q = 0; q < n; ++q)
        for (int row = 0; row < 2; ++row)
            for (int l = 0; l < L; ++l) {
                const int32_t v = called[(q * 2 + row) * L + l];
                if ((uint32_t)(v - lv[l].a0) >= (uint32_t)lv[l].k) {
                    set_error("%s: query %lld row %d level %d: vertex %d is not in its level", FN, (long long)q, row, l, v);
                    return DG_ERR_ARG;
                }
            }
    hipStream_t s = c->stream;
    // ---- the plan: segments [seg[g], seg[g + 1]) whose forward states fit joint_state_bytes (at least one level each) ----
    std::vector<int> seg{0};
    {
        int64_t in_seg = 0;
        for (int l = 0; l < L; ++l) {
            const int64_t bytes = 4 * lv[l].cells;
            if (l > seg.back() && in_seg + bytes > S.opt.joint_state_bytes) { seg.push_back(l); in_seg = 0; }
            in_seg += bytes;
        }
    }
    const int n_seg = (int)seg.size();
    seg.push_back(L);
    std::vector<int64_t> ck_off((size_t)n_seg + 1, 0);                     // F of every segment's first level, int32 units
    int64_t seg_cells = 1, roll_cells = 0, level_cells = 1;
    for (int g = 0; g < n_seg; ++g) {
        ck_off[g + 1] = ck_off[g] + lv[seg[g]].cells;
        int64_t sum = 0;
        for (int l = seg[g] + 1; l < seg[g + 1]; ++l) { sum += lv[l].cells; if (g + 1 < n_seg) roll_cells = std::max(roll_cells, lv[l].cells); }
        seg_cells = std::max(seg_cells, sum);
    }
    for (int l = 1; l < L; ++l) level_cells = std::max(level_cells, lv[l].cells);      // B of the levels 1 .. L - 1
    int64_t launches = 0, twice = 0, edge_launches = 0, finish_launches = 0;
    JtMem M;
    DevBuf d_called, d_rec, d_cout, d_V, d_part, d_oo, d_ocur, d_oe, d_sc, d_ck, d_roll, d_seg, d_back;
    if (n) if (int rc = M.get(d_called, n * 2 * L * 4)) return rc;
    if (n) if (int rc = M.get(d_cout, n * (L - 1) * 2 * 4)) return rc;
    if (int rc = M.get(d_rec, ((int64_t)L - 1) * (int64_t)sizeof(dg_dp_recombination_margin))) return rc;
    if (int rc = M.get(d_V, 4)) return rc;
    if (int rc = M.get(d_part, part_keys * 16)) return rc;
    if (int rc = M.get(d_oo, ((int64_t)nV + 1) * 4)) return rc;
    if (int rc = M.get(d_ocur, (int64_t)nV * 4)) return rc;
    if (int rc = M.get(d_oe, S.n_edges * 4)) return rc;
    if (tmax) if (int rc = M.get(d_sc, tmax * tmax * 2)) return rc;
    if (int rc = M.get(d_ck, ck_off[n_seg] * 4)) return rc;
    if (n) DG_HIP(hipMemcpyAsync(d_called.p, called, (size_t)(n * 2 * L) * 4, hipMemcpyHostToDevice, s));
    const LevelDesc *descs = S.d_descs.as<LevelDesc>();
    const uint32_t *in_off = S.d_in_off.as<uint32_t>(), *in_edge = S.d_in_edge.as<uint32_t>();
    const int32_t *in_dst = S.d_in_dst.as<int32_t>();
    uint16_t *sc = d_sc.as<uint16_t>();
    // the in-edges grouped by source
    DG_HIP(hipMemsetAsync(d_ocur.p, 0, (size_t)nV * 4, s));
    hipLaunchKernelGGL(jt_out_count_kernel, dim3((unsigned)(L - 1)), dim3(JT_THREADS), 0, s, descs, L, nV, in_edge, d_ocur.as<uint32_t>());
    hipLaunchKernelGGL(jt_out_scan_kernel, dim3(1), dim3(1024), 0, s, d_ocur.as<uint32_t>(), d_oo.as<uint32_t>(), d_ocur.as<uint32_t>(), nV);
    hipLaunchKernelGGL(jt_out_fill_kernel, dim3((unsigned)(L - 1)), dim3(JT_THREADS), 0, s, descs, L, nV, in_edge, d_ocur.as<uint32_t>(), d_oe.as<uint32_t>(), (uint32_t)S.n_edges);
    DG_HIP(hipGetLastError());
    launches += 3;
    auto scores = [&](int l) -> const uint16_t * {                          // the matrix of the transition into level l, in d_sc
        const int T = lv[l].T;
        if (!lv[l].coloured || T < 1) return nullptr;
        hipLaunchKernelGGL(jt_scores_kernel, dim3(jt_blocks(T, 64), (unsigned)std::min(T, 16384)), dim3(JT_THREADS), 0, s, T, lv[l].in_base, lv[l - 1].a0, in_edge, in_dst,
                           colour_csr(S), S.d_eflag.as<uint8_t>(), S.d_eself.as<uint16_t>(), sc);
        ++launches;
        return sc;
    };
    auto fill = [&](int32_t *st, int l, int pos) {                          // level l: 0 on every plane of the cell (pos, pos)
        hipLaunchKernelGGL(jt_fill_kernel, dim3(jt_blocks(lv[l].cells, 65536)), dim3(JT_THREADS), 0, s, st, lv[l].cells, ((int64_t)pos * lv[l].k + pos) * B1, B1);
        ++launches;
    };
    auto forward = [&](const int32_t *prev, int32_t *cur, int l) {
        const uint16_t *m = scores(l);
        hipLaunchKernelGGL(jt_forward_kernel, dim3(jt_blocks((int64_t)lv[l].k * B1, JT_X_BLOCKS), (unsigned)lv[l].k), dim3(JT_THREADS), 0, s, prev, cur, lv[l - 1].k, lv[l].k, B1,
                           lv[l].a0, lv[l].in_base, lv[l].T, in_off, in_edge, m);
        ++launches;
    };
    // ---- pass 1: the state at every segment's first level ----
    int32_t *ck = d_ck.as<int32_t>();
    fill(ck, 0, 0);
    if (n_seg > 1) {
        if (int rc = M.get(d_roll, 2 * roll_cells * 4)) return rc;
        int32_t *roll = d_roll.as<int32_t>();
        const int32_t *prev = ck;
        int g = 0;
        for (int l = 1; l <= seg[n_seg - 1]; ++l) {
            int32_t *dst;
            if (l == seg[g + 1]) dst = ck + ck_off[++g];
            else { dst = roll + (l & 1) * roll_cells; ++twice; }
            forward(prev, dst, l);
            prev = dst;
        }
        DG_HIP(hipGetLastError());
        DG_HIP(hipStreamSynchronize(s));                                    // the rolling states go before the segment buffers come
        M.drop(d_roll);
    }
    // ---- the segments, last first ----
    if (int rc = M.get(d_seg, seg_cells * 4)) return rc;
    if (int rc = M.get(d_back, 2 * level_cells * 4)) return rc;
    int32_t *back = d_back.as<int32_t>();
    std::vector<const int32_t *> Fp((size_t)L, nullptr);
    for (int g = n_seg - 1; g >= 0; --g) {
        const int a = seg[g], e = seg[g + 1];
        Fp[a] = ck + ck_off[g];
        int64_t at = 0;
        for (int l = a + 1; l < e; ++l) {
            int32_t *dst = d_seg.as<int32_t>() + at;
            at += lv[l].cells;
            forward(Fp[l - 1], dst, l);
            Fp[l] = dst;
        }
        for (int l = e - 1; l >= a; --l) {
            int32_t *cur = back + (l & 1) * level_cells;
            if (l == L - 1) {
                const int sink = nV - 1 - lv[l].a0;
                fill(cur, l, sink);
                DG_HIP(hipMemcpyAsync(d_V.p, Fp[l] + ((int64_t)sink * lv[l].k + sink) * B1 + budget, 4, hipMemcpyDeviceToDevice, s));
                continue;
            }
            const int32_t *next = back + ((l + 1) & 1) * level_cells;
            const uint16_t *m = scores(l + 1);
            const unsigned nx = jt_blocks((int64_t)lv[l].k * B1, JT_X_BLOCKS);
            hipLaunchKernelGGL(rb_edges_kernel, dim3(nx, (unsigned)lv[l].k), dim3(JT_THREADS), 0, s, Fp[l], next, lv[l].k, lv[l + 1].k, B1, lv[l].a0, lv[l + 1].a0, lv[l + 1].in_base,
                               lv[l + 1].T, (const uint32_t *)d_oo.as<uint32_t>(), (const uint32_t *)d_oe.as<uint32_t>(), in_edge, in_dst, m, d_part.as<long long>());
            hipLaunchKernelGGL(rb_finish_kernel, dim3(3 + (unsigned)((n + JT_THREADS / 64 - 1) / (JT_THREADS / 64))), dim3(JT_THREADS), 0, s, (const long long *)d_part.as<long long>(),
                               lv[l].k, (int)nx, lv[l].a0, lv[l + 1].a0, l, d_rec.as<dg_dp_recombination_margin>() + l, Fp[l], next, lv[l + 1].k, B1, lv[l + 1].in_base, lv[l + 1].T,
                               in_off, in_edge, m, (const int32_t *)d_called.as<int32_t>(), (int)n, L, d_cout.as<int32_t>());
            ++edge_launches; ++finish_launches; launches += 2;
            if (l > 0) {
                hipLaunchKernelGGL(jt_backward_kernel, dim3(nx, (unsigned)lv[l].k), dim3(JT_THREADS), 0, s, next, cur, lv[l].k, lv[l + 1].k, B1, lv[l].a0, lv[l + 1].a0,
                                   lv[l + 1].in_base, lv[l + 1].T, d_oo.as<uint32_t>(), d_oe.as<uint32_t>(), in_edge, in_dst, m);
                ++launches;
            }
        }
        DG_HIP(hipGetLastError());
    }
    // the caller's arrays are written only if the call succeeds
    std::vector<dg_dp_recombination_margin> recs((size_t)L - 1);
    std::vector<int32_t> couts((size_t)(n * (L - 1) * 2));
    int32_t V = NEG_INF;
    DG_HIP(hipMemcpyAsync(recs.data(), d_rec.p, recs.size() * sizeof(dg_dp_recombination_margin), hipMemcpyDeviceToHost, s));
    if (n) DG_HIP(hipMemcpyAsync(couts.data(), d_cout.p, couts.size() * 4, hipMemcpyDeviceToHost, s));
    DG_HIP(hipMemcpyAsync(&V, d_V.p, 4, hipMemcpyDeviceToHost, s));
    DG_HIP(hipStreamSynchronize(s));
    // the closing check: at every transition the best pair of paths takes some hop pair of it
    for (int l = 0; l < L - 1; ++l) {
        const dg_dp_recombination_margin &r = recs[(size_t)l];
        if (std::max(r.value[0], std::max(r.value[1], r.value[2])) != V) {
            set_error("%s: level %d: the values %d, %d, %d of its transition do not reach the sink's value %d at budget %d", FN, l, r.value[0], r.value[1], r.value[2], V, budget);
            return DG_ERR_STATE;
        }
    }
    S.rb_stats[0] = L - 1; S.rb_stats[1] = edge_launches; S.rb_stats[2] = finish_launches; S.rb_stats[3] = n_seg; S.rb_stats[4] = twice; S.rb_stats[5] = M.peak;
    S.rb_stats[6] = launches;
    memcpy(records, recs.data(), recs.size() * sizeof(dg_dp_recombination_margin));
    if (n) memcpy(called_out, couts.data(), couts.size() * 4);
    *best_value = V;
    return DG_OK;
}

// ---- dg_dp_recombination_margins_budgets: the records above for every listed budget from ONE pass at the largest, bmax.  Both states
// mean "at most r", so plane p of F_l and of B_{l+1} at bmax is plane p at any budget b <= bmax, and
// E^b_t[s] = max F_l[i][j][r] + d + B_{l+1}[i'][j'][b - s - r] over r <= b - s pairs planes of the one pass: only the pairing depends on b.
// The host sorts the distinct budgets bud[0 .. nd); the two kernels are the two above with one more dimension:
//   * rb_edges_budgets_kernel: grid (x blocks, k, nd).  Workgroup (x, i, d) is rb_edges_kernel's (x, i) at budget b = bud[d]: its lanes stride
//     over (j, r <= b), the state stride stays bmax + 1 and the B plane is b - w - r; part[d][s][i][x].  A row of budget b has k * (b + 1)
//     lanes, so only its first rbb_nx(k, b, gridDim.x) workgroups have any: the others return without a store and the finish kernel reads
//     only those (both call rbb_nx);
//   * rb_finish_budgets_kernel: workgroup 3 * d + s reduces part[d][s] to the words of record [d][l] that belong to s; the workgroups from
//     3 * nd on answer called_out, one wave per query, with the query's own budget in the r loop.
__device__ __forceinline__ int rbb_nx(int k, int b, int nx) { return min(nx, (k * (b + 1) + JT_THREADS - 1) / JT_THREADS); }

// as rb_edges_kernel; B1 = bmax + 1 = the stride of both states, bud = the distinct budgets, part = [gridDim.z][3][k][gridDim.x][2]
__global__ __launch_bounds__(JT_THREADS) void rb_edges_budgets_kernel(const int32_t *__restrict__ F, const int32_t *__restrict__ next, int k, int kn, int B1, const int32_t *__restrict__ bud,
                                                               int a0, int b0n, uint32_t in_base, int T, const uint32_t *__restrict__ oo, const uint32_t *__restrict__ oe,
                                                               const uint32_t *__restrict__ in_edge, const int32_t *__restrict__ in_dst, const uint16_t *__restrict__ sc,
                                                               long long *__restrict__ part) {
    __shared__ long long s_key[3][JT_THREADS / 64][2];
    const int t = (int)threadIdx.x, i = (int)blockIdx.y, bq = bud[blockIdx.z], b1 = bq + 1;
    const int nxd = rbb_nx(k, bq, (int)gridDim.x);
    if ((int)blockIdx.x >= nxd) return;                                     // uniform per workgroup: no lane of this budget's row is here
    const uint32_t ou0 = oo[a0 + i], ou1 = oo[a0 + i + 1];
    const int n = k * b1;
    long long a0k = JT_NO_KEY, a1k = JT_NO_KEY, a2k = JT_NO_KEY, b0k = 0, b1k = 0, b2k = 0;      // the lane's best key per s
    for (int x = (int)(blockIdx.x * JT_THREADS + threadIdx.x); x < n; x += nxd * JT_THREADS) {
        const int j = x / b1, r = x - j * b1;                               // r <= bq
        if (j < i) continue;
        const int f = F[((int64_t)i * k + j) * B1 + r];
        if (f == NEG_INF) continue;
        const uint32_t ov0 = oo[a0 + j], ov1 = oo[a0 + j + 1];
        long long c0 = JT_NO_KEY, c1 = JT_NO_KEY, c2 = JT_NO_KEY;
        for (uint32_t ou = ou0; ou < ou1; ++ou) {
            const uint32_t eu = oe[ou] - in_base;
            if (eu >= (uint32_t)T) continue;
            const uint32_t pi = (uint32_t)(in_dst[in_base + eu] - b0n);
            const int w1 = (int)(in_edge[in_base + eu] >> 31);
            if (pi >= (uint32_t)kn || bq - r - w1 < 0) continue;
            const uint32_t hi = (uint32_t)(JT_MAX_K - (int)pi) << 15;
            for (uint32_t ov = ov0; ov < ov1; ++ov) {
                const uint32_t ev = oe[ov] - in_base;
                if (ev >= (uint32_t)T) continue;
                const uint32_t pj = (uint32_t)(in_dst[in_base + ev] - b0n);
                const int w = w1 + (int)(in_edge[in_base + ev] >> 31);
                const int r2 = bq - r - w;                                  // what this budget leaves for B
                if (pj >= (uint32_t)kn || r2 < 0) continue;
                const int s = next[((int64_t)pi * kn + pj) * B1 + r2];
                if (s == NEG_INF) continue;
                const int v = f + s + (sc ? (int)sc[(int64_t)eu * T + ev] : 0);
                const long long cand = (long long)(((unsigned long long)(uint32_t)v << 32) | hi | (uint32_t)(JT_MAX_K - (int)pj));
                if (w == 0) c0 = max(c0, cand);
                else if (w == 1) c1 = max(c1, cand);
                else c2 = max(c2, cand);
            }
        }
        auto fold = [&](long long c, long long &a, long long &b) {
            if (c == JT_NO_KEY) return;
            const long long ca = (long long)(((unsigned long long)c & 0xFFFFFFFF00000000ull) | (uint32_t)(JT_MAX_K - i));
            const long long cb = ((long long)(JT_MAX_K - j) << 30) | (c & 0x3FFFFFFF);
            if (rb_better(ca, cb, a, b)) { a = ca; b = cb; }
        };
        fold(c0, a0k, b0k);
        fold(c1, a1k, b1k);
        fold(c2, a2k, b2k);
    }
    auto reduce = [&](int s, long long a, long long b) {
        for (int d = 32; d; d >>= 1) {
            const long long oa = __shfl_xor(a, d), ob = __shfl_xor(b, d);
            if (rb_better(oa, ob, a, b)) { a = oa; b = ob; }
        }
        if ((t & 63) == 0) { s_key[s][t >> 6][0] = a; s_key[s][t >> 6][1] = b; }
    };
    reduce(0, a0k, b0k);
    reduce(1, a1k, b1k);
    reduce(2, a2k, b2k);
    __syncthreads();
    if (t < 3) {
        long long a = s_key[t][0][0], b = s_key[t][0][1];
        for (int w = 1; w < JT_THREADS / 64; ++w)
            if (rb_better(s_key[t][w][0], s_key[t][w][1], a, b)) { a = s_key[t][w][0]; b = s_key[t][w][1]; }
        long long *out = part + ((((int64_t)blockIdx.z * 3 + t) * k + i) * gridDim.x + blockIdx.x) * 2;
        out[0] = a; out[1] = b;
    }
}

// grid: 3 * nd + ceil(n / 4) workgroups.  part = [nd][3][k][nx][2]; rec = the records [nd][L - 1]; qb = the queries' budgets [n]; the rest
// as rb_finish_kernel
__global__ __launch_bounds__(JT_THREADS) void rb_finish_budgets_kernel(const long long *__restrict__ part, int k, int nx, int nd, const int32_t *__restrict__ bud, int a0, int b0n, int l,
                                                                dg_dp_recombination_margin *__restrict__ rec, const int32_t *__restrict__ F, const int32_t *__restrict__ next, int kn,
                                                                int B1, uint32_t in_base, int T, const uint32_t *__restrict__ in_off, const uint32_t *__restrict__ in_edge,
                                                                const uint16_t *__restrict__ sc, const int32_t *__restrict__ called, const int32_t *__restrict__ qb, int n, int L,
                                                                int32_t *__restrict__ cout) {
    __shared__ long long s_key[JT_THREADS / 64][2];
    const int t = (int)threadIdx.x;
    if ((int)blockIdx.x < 3 * nd) {                                         // uniform per workgroup
        const int d = (int)blockIdx.x / 3, s = (int)blockIdx.x - 3 * d;
        const int nxd = rbb_nx(k, bud[d], nx);                              // the workgroups of this budget's rows that stored a key
        const long long *p = part + ((int64_t)d * 3 + s) * k * nx * 2;
        long long a = JT_NO_KEY, b = 0;
        for (int64_t x = t; x < (int64_t)k * nxd; x += JT_THREADS) {
            const int64_t at = (x / nxd) * nx + x % nxd;
            if (rb_better(p[2 * at], p[2 * at + 1], a, b)) { a = p[2 * at]; b = p[2 * at + 1]; }
        }
        for (int w = 32; w; w >>= 1) {
            const long long oa = __shfl_xor(a, w), ob = __shfl_xor(b, w);
            if (rb_better(oa, ob, a, b)) { a = oa; b = ob; }
        }
        if ((t & 63) == 0) { s_key[t >> 6][0] = a; s_key[t >> 6][1] = b; }
        __syncthreads();
        if (t == 0) {
            for (int w = 1; w < JT_THREADS / 64; ++w)
                if (rb_better(s_key[w][0], s_key[w][1], a, b)) { a = s_key[w][0]; b = s_key[w][1]; }
            dg_dp_recombination_margin *r = rec + (int64_t)d * (L - 1) + l;
            if (s == 0) r->level = l;
            if (a == JT_NO_KEY) { r->value[s] = NEG_INF; r->from1[s] = r->from2[s] = r->to1[s] = r->to2[s] = -1; }
            else {
                r->value[s] = (int)(a >> 32);
                r->from1[s] = a0 + (JT_MAX_K - (int)(a & 0x7FFF));
                r->from2[s] = a0 + (JT_MAX_K - (int)((b >> 30) & 0x7FFF));
                r->to1[s] = b0n + (JT_MAX_K - (int)((b >> 15) & 0x7FFF));
                r->to2[s] = b0n + (JT_MAX_K - (int)(b & 0x7FFF));
            }
        }
        return;
    }
    const int q = ((int)blockIdx.x - 3 * nd) * (JT_THREADS / 64) + (t >> 6), lane = t & 63;      // uniform per wave
    if (q >= n) return;
    const int bq = qb[q];
    uint32_t e[2];                                                          // the first in-edge of each called hop, UINT32_MAX: no edge
    int pos[2], posn[2];
    for (int h = 0; h < 2; ++h) {
        const int u = called[((int64_t)q * 2 + h) * L + l], v = called[((int64_t)q * 2 + h) * L + l + 1];
        pos[h] = u - a0; posn[h] = v - b0n;
        uint32_t at = UINT32_MAX;
        for (uint32_t x = in_off[v] + (uint32_t)lane; x < in_off[v + 1]; x += 64)
            if ((in_edge[x] & 0x7FFFFFFFu) == (uint32_t)pos[h] && x - in_base < (uint32_t)T) at = min(at, x);
        for (int d = 32; d; d >>= 1) at = min(at, (uint32_t)__shfl_xor((int)at, d));
        e[h] = at;
    }
    int s = -1, best = NEG_INF;
    if (e[0] != UINT32_MAX && e[1] != UINT32_MAX) {
        s = (int)(in_edge[e[0]] >> 31) + (int)(in_edge[e[1]] >> 31);
        const int d = sc ? (int)sc[(int64_t)(e[0] - in_base) * T + (e[1] - in_base)] : 0;
        const int32_t *f = F + ((int64_t)pos[0] * k + pos[1]) * B1, *b = next + ((int64_t)posn[0] * kn + posn[1]) * B1;
        for (int r = lane; r <= bq - s; r += 64) {
            const int fv = f[r], bv = b[bq - s - r];
            if (fv != NEG_INF && bv != NEG_INF) best = max(best, fv + d + bv);
        }
        for (int w = 32; w; w >>= 1) best = max(best, __shfl_xor(best, w));
    }
    if (lane == 0) {
        int32_t *out = cout + ((int64_t)q * (L - 1) + l) * 2;
        out[0] = s; out[1] = best;
    }
}

// rb_call's schedule run once at B1 = bmax + 1 with the two rb_*_budgets launches per level: as many launches as rb_call(bmax) issues.
int rbb_call(dg_ctx *c, const int32_t *budgets, int64_t n, const int32_t *called, dg_dp_recombination_margin *records, int32_t *called_out, int32_t *best_values) {
    const char *FN = "dg_dp_recombination_margins_budgets";
    DpState *Sp = c->dp;
    if (!Sp || !Sp->loaded) { set_error("%s: no graph loaded", FN); return DG_ERR_STATE; }
    DpState &S = *Sp;
    if (n < 1) { set_error("%s: n = %lld", FN, (long long)n); return DG_ERR_ARG; }
    if (!budgets || !records || !best_values) { set_error("%s: budgets, records and best_values are required", FN); return DG_ERR_ARG; }
    if (called && !called_out) { set_error("%s: called needs called_out", FN); return DG_ERR_ARG; }
    if (n > JT_MAX_QUERIES) { set_error("%s: %lld queries exceed %d per call", FN, (long long)n, JT_MAX_QUERIES); return DG_ERR_UNSUPPORTED; }
    int32_t budget = 0;                                                     // the pass runs at the largest budget
    for (int64_t q = 0; q < n; ++q) {
        if (budgets[q] < 0) { set_error("%s: query %lld: budget %d is negative", FN, (long long)q, budgets[q]); return DG_ERR_ARG; }
        budget = std::max(budget, budgets[q]);
    }
    if ((int64_t)budget + 1 > JT_MAX_PLANES) { set_error("%s: budget + 1 = %lld exceeds %d planes", FN, (long long)budget + 1, JT_MAX_PLANES); return DG_ERR_UNSUPPORTED; }
    std::vector<int32_t> bud(budgets, budgets + n);                        // the distinct budgets, ascending
    std::sort(bud.begin(), bud.end());
    bud.erase(std::unique(bud.begin(), bud.end()), bud.end());
    const int nd = (int)bud.size();
    const int L = S.L, nV = S.nV, B1 = budget + 1;
    if (L < 2 || (int)S.descs.size() < L) { set_error("%s: the loaded graph has %d levels", FN, L); return DG_ERR_STATE; }
    std::vector<JtLevel> lv((size_t)L);
    int kmax = 1;
    int64_t tmax = 0, part_keys = 1;
    for (int l = 0; l < L; ++l) {
        const LevelDesc &d = S.descs[(size_t)std::max(l, 1)];
        lv[l] = l ? JtLevel{d.b0, d.k2, d.in_base, d.T, d.delta_off >= 0, 0} : JtLevel{d.a0, d.k, 0u, 0, false, 0};
        lv[l].cells = (int64_t)lv[l].k * lv[l].k * B1;
        kmax = std::max(kmax, lv[l].k);
        if (lv[l].coloured) tmax = std::max<int64_t>(tmax, lv[l].T);
        if (l < L - 1) part_keys = std::max(part_keys, (int64_t)nd * 3 * lv[l].k * jt_blocks((int64_t)lv[l].k * B1, JT_X_BLOCKS));
    }
    if (kmax > JT_MAX_K) { set_error("%s: widest level %d exceeds %d", FN, kmax, JT_MAX_K); return DG_ERR_UNSUPPORTED; }
    if (called)
        for (int64_t q = 0; q < n; ++q)
            for (int row = 0; row < 2; ++row)
                for (int l = 0; l < L; ++l) {
                    const int32_t v = called[(q * 2 + row) * L + l];
                    if ((uint32_t)(v - lv[l].a0) >= (uint32_t)lv[l].k) {
                        set_error("%s: query %lld row %d level %d: vertex %d is not in its level", FN, (long long)q, row, l, v);
                        return DG_ERR_ARG;
                    }
                }
    const int64_t nc = called ? n : 0;                                      // the queries the finish kernel answers
    hipStream_t s = c->stream;
    // ---- the plan: segments [seg[g], seg[g + 1]) whose forward states fit joint_state_bytes (at least one level each) ----
    std::vector<int> seg{0};
    {
        int64_t in_seg = 0;
        for (int l = 0; l < L; ++l) {
            const int64_t bytes = 4 * lv[l].cells;
            if (l > seg.back() && in_seg + bytes > S.opt.joint_state_bytes) { seg.push_back(l); in_seg = 0; }
            in_seg += bytes;
        }
    }
    const int n_seg = (int)seg.size();
    seg.push_back(L);
    std::vector<int64_t> ck_off((size_t)n_seg + 1, 0);                     // F of every segment's first level, int32 units
    int64_t seg_cells = 1, roll_cells = 0, level_cells = 1;
    for (int g = 0; g < n_seg; ++g) {
        ck_off[g + 1] = ck_off[g] + lv[seg[g]].cells;
        int64_t sum = 0;
        for (int l = seg[g] + 1; l < seg[g + 1]; ++l) { sum += lv[l].cells; if (g + 1 < n_seg) roll_cells = std::max(roll_cells, lv[l].cells); }
        seg_cells = std::max(seg_cells, sum);
    }
    for (int l = 1; l < L; ++l) level_cells = std::max(level_cells, lv[l].cells);      // B of the levels 1 .. L - 1
    int64_t launches = 0, twice = 0, edge_launches = 0, finish_launches = 0;
    JtMem M;
    DevBuf d_called, d_qb, d_bud, d_rec, d_cout, d_V, d_part, d_oo, d_ocur, d_oe, d_sc, d_ck, d_roll, d_seg, d_back;
    const int64_t n_rec = (int64_t)nd * (L - 1);
    if (nc) if (int rc = M.get(d_called, nc * 2 * L * 4)) return rc;
    if (nc) if (int rc = M.get(d_cout, nc * (L - 1) * 2 * 4)) return rc;
    if (int rc = M.get(d_qb, n * 4)) return rc;
    if (int rc = M.get(d_bud, (int64_t)nd * 4)) return rc;
    if (int rc = M.get(d_rec, n_rec * (int64_t)sizeof(dg_dp_recombination_margin))) return rc;
    if (int rc = M.get(d_V, (int64_t)B1 * 4)) return rc;
    if (int rc = M.get(d_part, part_keys * 16)) return rc;
    if (int rc = M.get(d_oo, ((int64_t)nV + 1) * 4)) return rc;
    if (int rc = M.get(d_ocur, (int64_t)nV * 4)) return rc;
    if (int rc = M.get(d_oe, S.n_edges * 4)) return rc;
    if (tmax) if (int rc = M.get(d_sc, tmax * tmax * 2)) return rc;
    if (int rc = M.get(d_ck, ck_off[n_seg] * 4)) return rc;
    if (nc) DG_HIP(hipMemcpyAsync(d_called.p, called, (size_t)(nc * 2 * L) * 4, hipMemcpyHostToDevice, s));
    DG_HIP(hipMemcpyAsync(d_qb.p, budgets, (size_t)n * 4, hipMemcpyHostToDevice, s));
    DG_HIP(hipMemcpyAsync(d_bud.p, bud.data(), (size_t)nd * 4, hipMemcpyHostToDevice, s));      // (bud outlives the call's last synchronisation)
    const LevelDesc *descs = S.d_descs.as<LevelDesc>();
    const uint32_t *in_off = S.d_in_off.as<uint32_t>(), *in_edge = S.d_in_edge.as<uint32_t>();
    const int32_t *in_dst = S.d_in_dst.as<int32_t>();
    uint16_t *sc = d_sc.as<uint16_t>();
    // the in-edges grouped by source
    DG_HIP(hipMemsetAsync(d_ocur.p, 0, (size_t)nV * 4, s));
    hipLaunchKernelGGL(jt_out_count_kernel, dim3((unsigned)(L - 1)), dim3(JT_THREADS), 0, s, descs, L, nV, in_edge, d_ocur.as<uint32_t>());
    hipLaunchKernelGGL(jt_out_scan_kernel, dim3(1), dim3(1024), 0, s, d_ocur.as<uint32_t>(), d_oo.as<uint32_t>(), d_ocur.as<uint32_t>(), nV);
    hipLaunchKernelGGL(jt_out_fill_kernel, dim3((unsigned)(L - 1)), dim3(JT_THREADS), 0, s, descs, L, nV, in_edge, d_ocur.as<uint32_t>(), d_oe.as<uint32_t>(), (uint32_t)S.n_edges);
    DG_HIP(hipGetLastError());
    launches += 3;
    auto scores = [&](int l) -> const uint16_t * {                          // the matrix of the transition into level l, in d_sc
        const int T = lv[l].T;
        if (!lv[l].coloured || T < 1) return nullptr;
        hipLaunchKernelGGL(jt_scores_kernel, dim3(jt_blocks(T, 64), (unsigned)std::min(T, 16384)), dim3(JT_THREADS), 0, s, T, lv[l].in_base, lv[l - 1].a0, in_edge, in_dst,
                           colour_csr(S), S.d_eflag.as<uint8_t>(), S.d_eself.as<uint16_t>(), sc);
        ++launches;
        return sc;
    };
    auto fill = [&](int32_t *st, int l, int pos) {                          // level l: 0 on every plane of the cell (pos, pos)
        hipLaunchKernelGGL(jt_fill_kernel, dim3(jt_blocks(lv[l].cells, 65536)), dim3(JT_THREADS), 0, s, st, lv[l].cells, ((int64_t)pos * lv[l].k + pos) * B1, B1);
        ++launches;
    };
    auto forward = [&](const int32_t *prev, int32_t *cur, int l) {
        const uint16_t *m = scores(l);
        hipLaunchKernelGGL(jt_forward_kernel, dim3(jt_blocks((int64_t)lv[l].k * B1, JT_X_BLOCKS), (unsigned)lv[l].k), dim3(JT_THREADS), 0, s, prev, cur, lv[l - 1].k, lv[l].k, B1,
                           lv[l].a0, lv[l].in_base, lv[l].T, in_off, in_edge, m);
        ++launches;
    };
    // ---- pass 1: the state at every segment's first level ----
    int32_t *ck = d_ck.as<int32_t>();
    fill(ck, 0, 0);
    if (n_seg > 1) {
        if (int rc = M.get(d_roll, 2 * roll_cells * 4)) return rc;
        int32_t *roll = d_roll.as<int32_t>();
        const int32_t *prev = ck;
        int g = 0;
        for (int l = 1; l <= seg[n_seg - 1]; ++l) {
            int32_t *dst;
            if (l == seg[g + 1]) dst = ck + ck_off[++g];
            else { dst = roll + (l & 1) * roll_cells; ++twice; }
            forward(prev, dst, l);
            prev = dst;
        }
        DG_HIP(hipGetLastError());
        DG_HIP(hipStreamSynchronize(s));                                    // the rolling states go before the segment buffers come
        M.drop(d_roll);
    }
    // ---- the segments, last first ----
    if (int rc = M.get(d_seg, seg_cells * 4)) return rc;
    if (int rc = M.get(d_back, 2 * level_cells * 4)) return rc;
    int32_t *back = d_back.as<int32_t>();
    std::vector<const int32_t *> Fp((size_t)L, nullptr);
    for (int g = n_seg - 1; g >= 0; --g) {
        const int a = seg[g], e = seg[g + 1];
        Fp[a] = ck + ck_off[g];
        int64_t at = 0;
        for (int l = a + 1; l < e; ++l) {
            int32_t *dst = d_seg.as<int32_t>() + at;
            at += lv[l].cells;
            forward(Fp[l - 1], dst, l);
            Fp[l] = dst;
        }
        for (int l = e - 1; l >= a; --l) {
            int32_t *cur = back + (l & 1) * level_cells;
            if (l == L - 1) {
                const int sink = nV - 1 - lv[l].a0;
                fill(cur, l, sink);
                DG_HIP(hipMemcpyAsync(d_V.p, Fp[l] + ((int64_t)sink * lv[l].k + sink) * B1, (size_t)B1 * 4, hipMemcpyDeviceToDevice, s));      // V_b for every plane b
                continue;
            }
            const int32_t *next = back + ((l + 1) & 1) * level_cells;
            const uint16_t *m = scores(l + 1);
            const unsigned nx = jt_blocks((int64_t)lv[l].k * B1, JT_X_BLOCKS);
            hipLaunchKernelGGL(rb_edges_budgets_kernel, dim3(nx, (unsigned)lv[l].k, (unsigned)nd), dim3(JT_THREADS), 0, s, Fp[l], next, lv[l].k, lv[l + 1].k, B1,
                               (const int32_t *)d_bud.as<int32_t>(), lv[l].a0, lv[l + 1].a0, lv[l + 1].in_base, lv[l + 1].T, (const uint32_t *)d_oo.as<uint32_t>(),
                               (const uint32_t *)d_oe.as<uint32_t>(), in_edge, in_dst, m, d_part.as<long long>());
            hipLaunchKernelGGL(rb_finish_budgets_kernel, dim3(3 * (unsigned)nd + (unsigned)((nc + JT_THREADS / 64 - 1) / (JT_THREADS / 64))), dim3(JT_THREADS), 0, s,
                               (const long long *)d_part.as<long long>(), lv[l].k, (int)nx, nd, (const int32_t *)d_bud.as<int32_t>(), lv[l].a0, lv[l + 1].a0, l,
                               d_rec.as<dg_dp_recombination_margin>(), Fp[l], next, lv[l + 1].k, B1, lv[l + 1].in_base, lv[l + 1].T, in_off, in_edge, m,
                               (const int32_t *)d_called.as<int32_t>(), (const int32_t *)d_qb.as<int32_t>(), (int)nc, L, d_cout.as<int32_t>());
            ++edge_launches; ++finish_launches; launches += 2;
            if (l > 0) {
                hipLaunchKernelGGL(jt_backward_kernel, dim3(nx, (unsigned)lv[l].k), dim3(JT_THREADS), 0, s, next, cur, lv[l].k, lv[l + 1].k, B1, lv[l].a0, lv[l + 1].a0,
                                   lv[l + 1].in_base, lv[l + 1].T, d_oo.as<uint32_t>(), d_oe.as<uint32_t>(), in_edge, in_dst, m);
                ++launches;
            }
        }
        DG_HIP(hipGetLastError());
    }
    // the caller's arrays are written only if the call succeeds
    std::vector<dg_dp_recombination_margin> recs((size_t)n_rec);
    std::vector<int32_t> couts((size_t)(nc * (L - 1) * 2));
    std::vector<int32_t> Vs((size_t)B1, NEG_INF);
    DG_HIP(hipMemcpyAsync(recs.data(), d_rec.p, recs.size() * sizeof(dg_dp_recombination_margin), hipMemcpyDeviceToHost, s));
    if (nc) DG_HIP(hipMemcpyAsync(couts.data(), d_cout.p, couts.size() * 4, hipMemcpyDeviceToHost, s));
    DG_HIP(hipMemcpyAsync(Vs.data(), d_V.p, (size_t)B1 * 4, hipMemcpyDeviceToHost, s));
    DG_HIP(hipStreamSynchronize(s));
    // the closing check, per distinct budget: at every transition the best pair of paths within it takes some hop pair
    for (int d = 0; d < nd; ++d)
        for (int l = 0; l < L - 1; ++l) {
            const dg_dp_recombination_margin &r = recs[(size_t)d * (L - 1) + l];
            const int32_t V = Vs[(size_t)bud[d]];
            if (std::max(r.value[0], std::max(r.value[1], r.value[2])) != V) {
                set_error("%s: level %d: the values %d, %d, %d of its transition do not reach the sink's value %d at budget %d", FN, l, r.value[0], r.value[1], r.value[2], V, bud[d]);
                return DG_ERR_STATE;
            }
        }
    const int64_t st[9] = {n, nd, L - 1, edge_launches, finish_launches, n_seg, twice, M.peak, launches};
    for (int x = 0; x < 9; ++x) S.rbb_stats[x] = st[x];
    for (int64_t q = 0; q < n; ++q) {                                       // queries of one budget share one set of records
        const int d = (int)(std::lower_bound(bud.begin(), bud.end(), budgets[q]) - bud.begin());
        memcpy(records + q * (L - 1), recs.data() + (size_t)d * (L - 1), (size_t)(L - 1) * sizeof(dg_dp_recombination_margin));
        best_values[q] = Vs[(size_t)budgets[q]];
    }
    if (nc) memcpy(called_out, couts.data(), couts.size() * 4);
    return DG_OK;
}

}  // namespace

int dp_recombination_margins(dg_ctx *c, int32_t budget, const int32_t *called, int64_t n, dg_dp_recombination_margin *records, int32_t *called_out, int32_t *best_value) {
    return rb_call(c, budget, called, n, records, called_out, best_value);
}

int dp_recombination_margins_budgets(dg_ctx *c, const int32_t *budgets, int64_t n, const int32_t *called, dg_dp_recombination_margin *records, int32_t *called_out,
                                     int32_t *best_values) {
    return rbb_call(c, budgets, n, called, records, called_out, best_values);
}

int dp_recombination_budget_stats(dg_ctx *c, int64_t *out, int n) {
    if (!out || n < 9) { set_error("dg_dp_get_recombination_budget_stats: out needs 9 words"); return DG_ERR_ARG; }
    if (!c->dp) { set_error("dg_dp_get_recombination_budget_stats: no graph loaded"); return DG_ERR_STATE; }
    for (int q = 0; q < 9; ++q) out[q] = c->dp->rbb_stats[q];
    return DG_OK;
}

int dp_recombination_stats(dg_ctx *c, int64_t *out, int n) {
    if (!out || n < 7) { set_error("dg_dp_get_recombination_stats: out needs 7 words"); return DG_ERR_ARG; }
    if (!c->dp) { set_error("dg_dp_get_recombination_stats: no graph loaded"); return DG_ERR_STATE; }
    for (int q = 0; q < 7; ++q) out[q] = c->dp->rb_stats[q];
    return DG_OK;
}

int dp_phase_margins(dg_ctx *c, const int32_t *called, int32_t budget, const int32_t *vertex_class, dg_dp_phase_margin *records, int64_t *n_records, int32_t *best_value) {
    return ph_call(c, called, budget, vertex_class, records, n_records, best_value);
}

int dp_phase_stats(dg_ctx *c, int64_t *out, int n) {
    if (!out || n < 6) { set_error("dg_dp_get_phase_stats: out needs 6 words"); return DG_ERR_ARG; }
    if (!c->dp) { set_error("dg_dp_get_phase_stats: no graph loaded"); return DG_ERR_STATE; }
    for (int q = 0; q < 6; ++q) out[q] = c->dp->ph_stats[q];
    return DG_OK;
}

int dp_phase_margins_budgets(dg_ctx *c, const int32_t *called, const int32_t *budgets, int64_t n, const int32_t *vertex_class, dg_dp_phase_margin *records, int64_t *record_off,
                             int32_t *best_values) {
    return phb_call(c, called, budgets, n, vertex_class, records, record_off, best_values);
}

int dp_phase_budget_stats(dg_ctx *c, int64_t *out, int n) {
    if (!out || n < 10) { set_error("dg_dp_get_phase_budget_stats: out needs 10 words"); return DG_ERR_ARG; }
    if (!c->dp) { set_error("dg_dp_get_phase_budget_stats: no graph loaded"); return DG_ERR_STATE; }
    for (int q = 0; q < 10; ++q) out[q] = c->dp->phb_stats[q];
    return DG_OK;
}

int dp_genotype_margins(dg_ctx *c, bool pinned, const dg_dp_pin *pins, int64_t n_pins, const int32_t *called, int64_t n, int32_t budget, const int32_t *vertex_class,
                        dg_dp_genotype_margin *levels, int32_t *vertex_values, int32_t *best_value) {
    return jt_call(c, pinned ? "dg_dp_genotype_margins_pinned" : "dg_dp_genotype_margins", pinned ? pins : nullptr, pinned ? n_pins : 0, called, n, budget, vertex_class, levels, vertex_values, best_value, nullptr);
}

int dp_genotype_margins_budgets(dg_ctx *c, const dg_dp_pin *pins, int64_t n_pins, const int32_t *called, const int32_t *budgets, int64_t n, const int32_t *vertex_class,
                                dg_dp_genotype_margin *levels, int32_t *best_values) {
    const JtBudgets mb{budgets, best_values};
    return jt_call(c, "dg_dp_genotype_margins_budgets", n_pins != 0 ? pins : nullptr, n_pins, called, n, 0, vertex_class, levels, nullptr, nullptr, nullptr, &mb);
}

int dp_genotype_table(dg_ctx *c, bool pinned, const dg_dp_pin *pins, int64_t n_pins, int32_t budget, const int32_t *vertex_class, const int32_t *called, int64_t n,
                      dg_dp_genotype_margin *levels, int64_t *level_off, dg_dp_genotype_entry **entries, int64_t *n_entries, int32_t *best_value) {
    const JtTable tab{level_off, entries, n_entries};
    return jt_call(c, pinned ? "dg_dp_genotype_table_pinned" : "dg_dp_genotype_table", pinned ? pins : nullptr, pinned ? n_pins : 0, called, n, budget, vertex_class, levels, nullptr, best_value, &tab);
}

int dp_genotype_stats(dg_ctx *c, int64_t *out, int n) {
    if (!out || n < 4) { set_error("dg_dp_get_genotype_stats: out needs 4 words"); return DG_ERR_ARG; }
    if (!c->dp) { set_error("dg_dp_get_genotype_stats: no graph loaded"); return DG_ERR_STATE; }
    for (int q = 0; q < (n >= 8 ? 8 : n >= 6 ? 6 : 4); ++q) out[q] = c->dp->jt_stats[q];
    return DG_OK;
}

}  // namespace dgi

extern "C" int dg_dp_genotype_margins(dg_ctx *c, const int32_t *called, int64_t n_called, int32_t budget, const int32_t *vertex_class, dg_dp_genotype_margin *levels,
                                      int32_t *vertex_values, int32_t *best_value) {
    if (int rc = dgi::bind(c)) return rc;
    return dgi::dp_genotype_margins(c, false, nullptr, 0, called, n_called, budget, vertex_class, levels, vertex_values, best_value);
}

extern "C" int dg_dp_genotype_table(dg_ctx *c, int32_t budget, const int32_t *vertex_class, const int32_t *called, int64_t n_called, dg_dp_genotype_margin *levels,
                                    int64_t *level_off, dg_dp_genotype_entry **entries, int64_t *n_entries, int32_t *best_value) {
    if (int rc = dgi::bind(c)) return rc;
    return dgi::dp_genotype_table(c, false, nullptr, 0, budget, vertex_class, called, n_called, levels, level_off, entries, n_entries, best_value);
}

extern "C" int dg_dp_genotype_margins_pinned(dg_ctx *c, const dg_dp_pin *pins, int64_t n_pins, const int32_t *called, int64_t n_called, int32_t budget,
                                             const int32_t *vertex_class, dg_dp_genotype_margin *levels, int32_t *vertex_values, int32_t *best_value) {
    if (int rc = dgi::bind(c)) return rc;
    return dgi::dp_genotype_margins(c, true, pins, n_pins, called, n_called, budget, vertex_class, levels, vertex_values, best_value);
}

extern "C" int dg_dp_genotype_table_pinned(dg_ctx *c, const dg_dp_pin *pins, int64_t n_pins, int32_t budget, const int32_t *vertex_class, const int32_t *called,
                                           int64_t n_called, dg_dp_genotype_margin *levels, int64_t *level_off, dg_dp_genotype_entry **entries,
                                           int64_t *n_entries, int32_t *best_value) {
    if (int rc = dgi::bind(c)) return rc;
    return dgi::dp_genotype_table(c, true, pins, n_pins, budget, vertex_class, called, n_called, levels, level_off, entries, n_entries, best_value);
}

extern "C" int dg_dp_genotype_margins_budgets(dg_ctx *c, const dg_dp_pin *pins, int64_t n_pins, const int32_t *called, const int32_t *budgets, int64_t n_called,
                                              const int32_t *vertex_class, dg_dp_genotype_margin *levels, int32_t *best_values) {
    if (int rc = dgi::bind(c)) return rc;
    return dgi::dp_genotype_margins_budgets(c, pins, n_pins, called, budgets, n_called, vertex_class, levels, best_values);
}

extern "C" int dg_dp_get_genotype_stats(dg_ctx *c, int64_t *out, int n) {
    if (int rc = dgi::bind(c)) return rc;
    return dgi::dp_genotype_stats(c, out, n);
}

extern "C" int dg_dp_phase_margins(dg_ctx *c, const int32_t *called, int32_t budget, const int32_t *vertex_class, dg_dp_phase_margin *records, int64_t *n_records,
                                   int32_t *best_value) {
    if (int rc = dgi::bind(c)) return rc;
    return dgi::dp_phase_margins(c, called, budget, vertex_class, records, n_records, best_value);
}

extern "C" int dg_dp_get_phase_stats(dg_ctx *c, int64_t *out, int n) {
    if (int rc = dgi::bind(c)) return rc;
    return dgi::dp_phase_stats(c, out, n);
}

extern "C" int dg_dp_phase_margins_budgets(dg_ctx *c, const int32_t *called, const int32_t *budgets, int64_t n_called, const int32_t *vertex_class, dg_dp_phase_margin *records,
                                           int64_t *record_off, int32_t *best_values) {
    if (int rc = dgi::bind(c)) return rc;
    return dgi::dp_phase_margins_budgets(c, called, budgets, n_called, vertex_class, records, record_off, best_values);
}

extern "C" int dg_dp_get_phase_budget_stats(dg_ctx *c, int64_t *out, int n) {
    if (int rc = dgi::bind(c)) return rc;
    return dgi::dp_phase_budget_stats(c, out, n);
}

extern "C" int dg_dp_recombination_margins(dg_ctx *c, int32_t budget, const int32_t *called, int64_t n_called, dg_dp_recombination_margin *records, int32_t *called_out,
                                           int32_t *best_value) {
    if (int rc = dgi::bind(c)) return rc;
    return dgi::dp_recombination_margins(c, budget, called, n_called, records, called_out, best_value);
}

extern "C" int dg_dp_get_recombination_stats(dg_ctx *c, int64_t *out, int n) {
    if (int rc = dgi::bind(c)) return rc;
    return dgi::dp_recombination_stats(c, out, n);
}

extern "C" int dg_dp_recombination_margins_budgets(dg_ctx *c, const int32_t *budgets, int64_t n, const int32_t *called, dg_dp_recombination_margin *records, int32_t *called_out,
                                                   int32_t *best_values) {
    if (int rc = dgi::bind(c)) return rc;
    return dgi::dp_recombination_margins_budgets(c, budgets, n, called, records, called_out, best_values);
}

extern "C" int dg_dp_get_recombination_budget_stats(dg_ctx *c, int64_t *out, int n) {
    if (int rc = dgi::bind(c)) return rc;
    return dgi::dp_recombination_budget_stats(c, out, n);
}

// dg_dp_run_pinned: per-level cell constraints on the run's own DP.  The sweep kernels are not touched: a source cell counts as
// unreachable where its value is NEG_INF (relax_select, dg_dp_sweep.hip:238, which sweep_task and the cooperative tasks share;
// the generic dp_sweep_kernel, :135; the pair kernel, :515), so a level is constrained by storing exactly that value over its cells that
// are not allowed, between the launch that writes the level and the next one (dg_dp_run.hip issues both on the run's stream).  The mask
// only stores: it loads no state and leaves the back-pointer lattice alone -- a cleared cell is never a winner of the level after
// it, so no chain walk arrives there.
// dg_dp_genotype_margins_pinned / dg_dp_genotype_table_pinned constrain the joint pass (dg_dp_joint.hip) the same way: its recurrences
// skip a NEG_INF source cell too, its states are [i][j][r], and jt_pin_mask_kernel below is the mask for that layout.
#include <algorithm>

#include "dg_dp.hpp"

namespace dgi {

// One wave per (row i, block of 64 columns j); pins = the level's own slice of the sorted pin list, vertices as positions inside the
// level (-1: any).  Every lane decides "allowed" once for its cell, then stores over the planes: a wave writes one 256-byte row
// per plane.  state = the level's slab [i][r][j] (64-bit offsets: a slab may exceed 2^31 bytes where SweepLaunch::small_state is false).
__global__ __launch_bounds__(256) void dp_pin_mask_kernel(const dg_dp_pin *__restrict__ pins, int n, int32_t *__restrict__ state, int k, int RP) {
    const int i = (int)blockIdx.y, j = ((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6)) * 64 + (int)(threadIdx.x & 63);
    if (j >= k) return;
    bool any_req = false, req = false, forbid = false;
    for (int q = 0; q < n; ++q) {                                       // (the same address in every lane: scalar loads)
        const dg_dp_pin p = pins[q];
        const bool m = (p.vertex1 < 0 || p.vertex1 == i) && (p.vertex2 < 0 || p.vertex2 == j);
        if (p.kind == 0) { any_req = true; req |= m; } else forbid |= m;
    }
    if ((!any_req || req) && !forbid) return;
    int32_t *cell = state + (int64_t)i * RP * k + j;
    for (int r = 0; r < RP; ++r) cell[(int64_t)r * k] = NEG_INF;
}

// The same for a state of the joint pass (dg_dp_joint.hip), int32 [i][j][r], r fastest: the planes of a cell are contiguous, so the
// lanes stride over the flattened (j, r) of row i = blockIdx.y and a wave's stores are 256 consecutive bytes; "allowed" is decided once
// per j (the pins' addresses are the same in every lane: scalar loads).  A row has k * B1 <= 32767 * 4096 < 2^27 words, so the position
// inside the row is an int; the row's own offset is 64-bit (a state may exceed 2^31 words).  Stores only: no state is loaded.
__global__ __launch_bounds__(256) void jt_pin_mask_kernel(const dg_dp_pin *__restrict__ pins, int n, int32_t *__restrict__ state, int k, int B1) {
    const int i = (int)blockIdx.y;
    if (i >= k) return;
    const int n_row = k * B1;
    int32_t *row = state + (int64_t)i * k * B1;
    int seen = -1;
    bool clear = false;
    for (int x = (int)(blockIdx.x * 256 + threadIdx.x); x < n_row; x += (int)(gridDim.x * 256)) {
        const int j = x / B1;
        if (j != seen) {
            seen = j;
            bool any_req = false, req = false, forbid = false;
            for (int q = 0; q < n; ++q) {
                const dg_dp_pin p = pins[q];
                const bool m = (p.vertex1 < 0 || p.vertex1 == i) && (p.vertex2 < 0 || p.vertex2 == j);
                if (p.kind == 0) { any_req = true; req |= m; } else forbid |= m;
            }
            clear = (any_req && !req) || forbid;
        }
        if (clear) row[x] = NEG_INF;
    }
}

int pins_prepare(const char *FN, const DpState &S, const dg_dp_pin *pins, int64_t n, PinSet &P, DevBuf &buf) {
    if (n < 0 || n > 65536) { set_error("%s: n_pins = %lld outside 0..65536", FN, (long long)n); return DG_ERR_ARG; }
    if (n > 0 && !pins) { set_error("%s: null pins with n_pins = %lld", FN, (long long)n); return DG_ERR_ARG; }
    const int L = S.L;
    P.off.assign((size_t)L + 1, 0);
    for (int64_t q = 0; q < n; ++q) {
        const dg_dp_pin &p = pins[q];
        if (p.level < 1 || p.level > L - 2) { set_error("%s: pin %lld: level %d outside 1..%d", FN, (long long)q, p.level, L - 2); return DG_ERR_ARG; }
        const LevelDesc &d = S.descs[p.level];
        for (int h = 0; h < 2; ++h) {
            const int v = h ? p.vertex2 : p.vertex1;
            if (v != -1 && (v < d.b0 || v >= d.b0 + d.k2)) {
                set_error("%s: pin %lld: vertex%d %d is neither -1 nor inside level %d (%d..%d)", FN, (long long)q, h + 1, v, p.level, d.b0, d.b0 + d.k2 - 1);
                return DG_ERR_ARG;
            }
        }
        if (p.kind != 0 && p.kind != 1) { set_error("%s: pin %lld: kind %d is neither 0 (require) nor 1 (forbid)", FN, (long long)q, p.kind); return DG_ERR_ARG; }
        ++P.off[(size_t)p.level + 1];
    }
    for (int l = 0; l < L; ++l) P.off[(size_t)l + 1] += P.off[(size_t)l];
    // counting sort by level; the device copy holds positions inside the level
    std::vector<dg_dp_pin> sorted((size_t)n);
    std::vector<int32_t> next(P.off.begin(), P.off.end() - 1);
    for (int64_t q = 0; q < n; ++q) {
        dg_dp_pin p = pins[q];
        const int b0 = S.descs[p.level].b0;
        if (p.vertex1 >= 0) p.vertex1 -= b0;
        if (p.vertex2 >= 0) p.vertex2 -= b0;
        sorted[(size_t)next[(size_t)p.level]++] = p;
    }
    if (int rc = buf.ensure(sizeof(dg_dp_pin) * (size_t)n)) return rc;
    DG_HIP(hipMemcpy(buf.p, sorted.data(), sizeof(dg_dp_pin) * (size_t)n, hipMemcpyHostToDevice));   // once per call
    P.d_pins = buf.as<dg_dp_pin>();
    return DG_OK;
}

void pins_launch_mask(const DpState &S, PinSet &P, int level, int32_t *state, hipStream_t s) {
    const int k = S.descs[level].k2;
    const dim3 grid((unsigned)(((k + 63) / 64 + 3) / 4), (unsigned)k);                      // (k <= MAX_K = 32768 rows)
    hipLaunchKernelGGL(dp_pin_mask_kernel, grid, dim3(256), 0, s, P.d_pins + P.off[(size_t)level], P.off[(size_t)level + 1] - P.off[(size_t)level], state, k, S.RP);
    ++P.n_mask;
}

void pins_launch_joint_mask(PinSet &P, int level, int32_t *state, int k, int planes, hipStream_t s) {
    const int64_t n_row = (int64_t)k * planes;
    const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>((n_row + 255) / 256, 4096)), (unsigned)k);      // (k <= 32767 rows)
    hipLaunchKernelGGL(jt_pin_mask_kernel, grid, dim3(256), 0, s, P.d_pins + P.off[(size_t)level], P.off[(size_t)level + 1] - P.off[(size_t)level], state, k, planes);
    ++P.n_mask;
}

}  // namespace dgi

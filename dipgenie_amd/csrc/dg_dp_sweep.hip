// Level sweep of the diploid DP (approximator.cpp:627-701), edge-pair form.  State layout [i][r][j] (j fastest).
//
// The work of one transition is the T x T grid of in-edge pairs (e_u, e_v) -- exactly the index space of the delta
// matrix.  One wave owns one task = (destination row i2, column group g, chunk of RC recombination counts): a group is
// a run of <= 64 consecutive in-edges e_v that covers whole destination columns (host-built), so lane <-> e_v and
// every destination cell's candidates sit in adjacent lanes.  The wave walks the row's in-edges e_u (wave-uniform),
// and per step every lane does one delta load (coalesced along e_v) and RC value loads (coalesced along the source
// column j) -- no per-lane inner loop, so a vertex with in-degree 24 costs 24 steps instead of 24 x 24.  Each lane
// keeps, per recombination count, the best candidate as the pair (value, ord) with ord built from the in-edge ranks so
// that a plain lexicographic max IS the reference's take-if order (value desc, pred_i asc, pred_j asc,
// approximator.cpp:657-659).  A log-step segmented max over lanes of equal destination column finishes the cell; the
// segment head stores the value and the back-pointer.
#include <algorithm>
#include <cmath>
#include <type_traits>

#include "dg_dp.hpp"

namespace dgi {

// state slot of a level: the two slots are ping-pong buffers
#define DG_SLOT(LEVEL) ((LEVEL) & 1)

constexpr unsigned long long DIGEST_PRED_MUL = 0x9E3779B97F4A7C15ULL;   // oracle_dp.cpp: weight of the predecessor term

// narrow form: ord = (255 - eu) << 8 | (255 - ev) is never 0 for a real candidate, and the stored back-pointer is
// simply ~ord (an untouched best keeps ord 0 -> 0xFFFF = unreachable)
// non-temporal 16-bit store as inline asm: with the builtin on one side of a branch and a plain store on the other the
// optimiser merges the two into ONE plain store (the !nontemporal hint is dropped)
__device__ __forceinline__ void store_bp_nt(uint16_t *p, uint32_t v) { asm volatile("global_store_short %0, %1, off nt" ::"v"(p), "v"(v) : "memory"); }
__device__ __forceinline__ uint32_t ord_rank(int eu, int ev) { return ((uint32_t)(BP_MAX_RANK - eu) << 8) | (uint32_t)(BP_MAX_RANK - ev); }

// digest of one reachable cell: the oracle's definition (oracle_dp.cpp), o = its r-major cell index
__device__ __forceinline__ unsigned long long digest_term(int value, unsigned long long o, uint32_t pred_i, uint32_t pred_j) {
    return (unsigned long long)(uint32_t)(value + 1) * (o + 1) +
           DIGEST_PRED_MUL * ((((unsigned long long)pred_i << 15) | pred_j) + 1ULL) * (o + 1);
}

// neighbour exchange by one lane as DPP wave shifts (a few cycles) instead of ds_bpermute (an LDS crossbar round trip):
// most column groups need exactly one step of the segmented max (columns with at most two in-edges)
__device__ __forceinline__ int lane_down1(int x) { return __builtin_amdgcn_update_dpp(x, x, 0x130 /* wave_shl:1: lane i <- lane i + 1 */, 0xF, 0xF, false); }
__device__ __forceinline__ int lane_up1(int x) { return __builtin_amdgcn_update_dpp(x, x, 0x138 /* wave_shr:1: lane i <- lane i - 1 */, 0xF, 0xF, false); }

// What a task needs before its stores, as leading scalar kernel arguments: the command processor preloads the first 16
// dwords of scalar arguments into SGPRs (-mllvm -amdgpu-kernarg-preload-count; by-value structs stop the preload), so
// neither load round waits for a load of the kernel-argument segment (a cold miss on every CU at every launch: 0.3-0.4 us
// per level when the first round had to wait for it).  Plain launches preload everything below; cooperative launches
// spend five of the sixteen dwords on the heavy-row list and read {dm, pad_bytes, dT, buf_bytes} the ordinary way.
struct LevelHead {
    const uint4 *rowrec_l;              // rowrec + b0
    const uint2 *slots_l;               // slots + slot_first
    const uint32_t *rowx_l;             // rowx + rowx_off
    const int32_t *cur;                 // padded start of the source level's state buffer
    const uint16_t *dm;                 // delta matrix biased by -in_base * dT (entry of in-edge pair (e_u, e_v): dm[e_u * dT + dcol]); the zero slot if dT = 0
    int rowx_stride, RP, k, pad_bytes, dT;
    uint32_t buf_bytes;
};

__device__ __forceinline__ __amdgpu_buffer_rsrc_t state_rsrc(const int32_t *padded_base, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc((void *)padded_base, 0, bytes, 0x00020000);
}

// per-level launch of the fast form: grid = (ceil(nblocks/4), nchunk, k2 [+ 4 per heavy row]), one task per wave (a 3-D
// grid: splitting a combined index would cost a runtime integer division -- ~40 instructions of a 380-instruction task)
// workgroup 0 of a launch tells the L2 prefetcher which level is running
__device__ __forceinline__ void publish_level(int *progress, int lvl) {
    if ((blockIdx.x | blockIdx.y | blockIdx.z) == 0 && threadIdx.x == 0) __hip_atomic_store(progress, lvl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ uint32_t ord_word(int i, int j, int wu, int wv) {
    return ((uint32_t)(0x7FFF - i) << 17) | ((uint32_t)(0x7FFF - j) << 2) | ((uint32_t)wu << 1) | (uint32_t)wv;
}
__device__ __forceinline__ uint32_t bp_from_ord(uint32_t o) {
    const uint32_t i = 0x7FFFu - (o >> 17), j = 0x7FFFu - ((o >> 2) & 0x7FFFu);
    return i | (j << 15) | (((o >> 1) & 1u) << 30) | ((o & 1u) << 31);
}
// ---------------------------------------------------------------------------------------------
// generic form: group offsets read at run time; any in-degree, any level size, wide back-pointers
// ---------------------------------------------------------------------------------------------
template <int RC, bool DIGEST>
__device__ __forceinline__ void sweep_level_pairs(const SweepArgs &A, int lvl, int wave_id, int n_waves) {
    const LevelDesc d = A.descs[lvl];
    const int RP = A.RP;
    const int32_t *__restrict__ cur = (const int32_t *)(A.ring + (size_t)(DG_SLOT(lvl - 1) ^ A.flip) * A.slot_bytes + A.pad_bytes);
    int32_t *__restrict__ nxt = (int32_t *)(A.ring + (size_t)(DG_SLOT(lvl) ^ A.flip) * A.slot_bytes + A.pad_bytes);
    const int lane = threadIdx.x & 63;
    const int nchunk = (RP + RC - 1) / RC;
    const int64_t ntask = (int64_t)d.k2 * d.ngroups * nchunk;
    const bool has_delta = d.delta_off >= 0;
    const uint16_t *dm = has_delta ? A.delta + d.delta_off : A.delta_zero;   // (A.delta is biased by the resident delta window)
    const int dT = has_delta ? d.T : 0, dmask = has_delta ? -1 : 0;
    const uint32_t *gb = A.grp_begin + d.grp_first;
    unsigned long long dsum = 0;
    for (int64_t task = wave_id; task < ntask; task += n_waves) {
        const int g = (int)(task % d.ngroups);
        const int64_t rest = task / d.ngroups;
        const int rc = (int)(rest % nchunk), i2 = (int)(rest / nchunk);
        const int r0 = rc * RC;
        const uint32_t gbeg = gb[g], gend = gb[g + 1];
        const uint32_t eu0 = A.in_off[d.b0 + i2], eu1 = A.in_off[d.b0 + i2 + 1];
        int bval[RC];
        uint32_t bord[RC];
#pragma unroll
        for (int q = 0; q < RC; ++q) { bval[q] = NEG_INF; bord[q] = 0; }
        int j2 = -1 - lane;                                             // inactive lanes: unique negative ids
        // a group wider than 64 is one giant column (host guarantee): lanes accumulate over its chunks
        for (uint32_t cb = gbeg; cb < gend; cb += 64) {
            const uint32_t ev = cb + lane;
            const bool act = ev < gend;
            int j = 0, wv = 0, evr = 0;
            if (act) {
                const uint32_t pv = A.in_edge[ev];
                j = (int)(pv & 0x7FFFFFFFu); wv = (int)(pv >> 31);
                const int cv = A.in_dst[ev];
                j2 = cv - d.b0;
                if (!d.bp_wide) evr = (int)(ev - A.in_off[cv]);            // rank inside the column's in-edge list
            }
            const int dcol = (int)(ev - d.in_base) & dmask;
            for (uint32_t eu = eu0; eu < eu1; ++eu) {
                const uint32_t pu = A.in_edge[eu];
                const int i = (int)(pu & 0x7FFFFFFFu), wu = (int)(pu >> 31);
                if (act) {
                    const int w = wu + wv;
                    const int dl = (int)dm[(int64_t)(eu - d.in_base) * dT + dcol];
                    const uint32_t ord = d.bp_wide ? ord_word(i, j, wu, wv) : ord_rank((int)(eu - eu0), evr);
                    // rows r = r2 - w; the buffers carry front/tail padding so r = -1, -2 (and r2 >= RP in a
                    // ragged last chunk) are legal reads that the select discards: RC loads back to back
                    const int32_t *base = cur + ((int64_t)i * RP + (r0 - w)) * d.k + j;
                    int vals[RC];
#pragma unroll
                    for (int q = 0; q < RC; ++q) vals[q] = base[q * d.k];
#pragma unroll
                    for (int q = 0; q < RC; ++q) {
                        const int cand = vals[q] + dl;
                        const bool ok = (r0 + q < RP) & (r0 + q - w >= 0) & (vals[q] != NEG_INF);       // :633, :646-647
                        const bool take = ok & ((cand > bval[q]) | ((cand == bval[q]) & (ord > bord[q])));   // :657-659
                        bval[q] = take ? cand : bval[q];
                        bord[q] = take ? ord : bord[q];
                    }
                }
            }
        }
        // segmented max over lanes with equal destination column (lanes of a column are adjacent)
        const int span = (int)min(gend - gbeg, 64u);
        for (int s = 1; s < span; s <<= 1) {
            const int oj2 = __shfl_down(j2, s);
            const bool same = (lane + s < 64) & (oj2 == j2);
#pragma unroll
            for (int q = 0; q < RC; ++q) {
                const int ov = __shfl_down(bval[q], s);
                const uint32_t oo = (uint32_t)__shfl_down((int)bord[q], s);
                const bool take = same & ((ov > bval[q]) | ((ov == bval[q]) & (oo > bord[q])));
                bval[q] = take ? ov : bval[q];
                bord[q] = take ? oo : bord[q];
            }
        }
        const int pj2 = __shfl_up(j2, 1);
        const bool head = (j2 >= 0) & ((lane == 0) | (pj2 != j2));
        if (head) {
#pragma unroll
            for (int q = 0; q < RC; ++q) {
                const int r2 = r0 + q;
                if (r2 < RP) {
                    const int64_t idx = ((int64_t)i2 * RP + r2) * d.k2 + j2;
                    nxt[idx] = bval[q];
                    if (A.bp) {
                        if (d.bp_wide) __builtin_nontemporal_store((uint32_t)(bval[q] == NEG_INF ? BP_NONE : bp_from_ord(bord[q])), (uint32_t *)(A.bp + d.bp_off + 2 * idx));
                        else __builtin_nontemporal_store((uint16_t)~bord[q], &A.bp[d.bp_off + idx]);
                    }
                    if (DIGEST && bval[q] != NEG_INF) {
                        const unsigned long long o = ((unsigned long long)r2 * d.k2 + i2) * d.k2 + j2;   // oracle's r-major index
                        uint32_t pi, pj;
                        if (d.bp_wide) { const uint32_t h = bp_from_ord(bord[q]); pi = h & 0x7FFFu; pj = (h >> 15) & 0x7FFFu; }
                        else {
                            const uint32_t ru = BP_MAX_RANK - (bord[q] >> 8), rv = BP_MAX_RANK - (bord[q] & 0xFFu);
                            pi = A.in_edge[eu0 + ru] & 0x7FFFFFFFu;
                            pj = A.in_edge[A.in_off[d.b0 + j2] + rv] & 0x7FFFFFFFu;
                        }
                        dsum += digest_term(bval[q], o, pi, pj);
                    }
                }
            }
        }
        // destination columns without any in-edge are unreachable: nobody owns them, clear them here
        if (g == 0 && d.ndead > 0) {
            for (int t = lane; t < d.ndead * RC; t += 64) {
                const int q = t % RC, c = A.dead_cols[d.dead_first + t / RC];
                if (r0 + q < RP) {
                    const int64_t idx = ((int64_t)i2 * RP + r0 + q) * d.k2 + c;
                    nxt[idx] = NEG_INF;
                    if (A.bp) {
                        if (d.bp_wide) __builtin_nontemporal_store((uint32_t)(BP_NONE), (uint32_t *)(A.bp + d.bp_off + 2 * idx));
                        else __builtin_nontemporal_store((uint16_t)0xFFFFu, &A.bp[d.bp_off + idx]);
                    }
                }
            }
        }
    }
    if (DIGEST && dsum) atomicAdd(&A.digest[lvl], dsum);
}

template <int RC, bool DIGEST>
__global__ __launch_bounds__(256) void dp_sweep_kernel(SweepArgs A, int lvl) {
    sweep_level_pairs<RC, DIGEST>(A, lvl, (int)(blockIdx.x * 4 + (threadIdx.x >> 6)), (int)(gridDim.x * 4));
}

__global__ void dp_init_kernel(int32_t *cur, int RP) {   // level 0: k = 1, every r starts at 0 (:534-535)
    const int r = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (r < RP) cur[r] = 0;
}

// ---------------------------------------------------------------------------------------------
// Fast form of the same sweep.  A level's kernel starts with cold caches (kernel boundary), so its
// duration is a chain of dependent memory round trips (~0.5-1 us each) -- the fast form cuts the chain to
//   kernel arguments (LevelDesc by value)  ->  {row record, slot record, row in-edge words}  ->  {delta, RC values}  ->  stores
// * slot table: every column group is padded to exactly 64 records {j | wv<<15 | j2<<16, ev_local |
//   rank<<20 | steps<<28}, so a lane finds its in-edge without reading group offsets;
// * row record {first in-edge, in-degree, in-edge 0, in-edge 1} serves 97 % of the rows in one load;
// * rows with more in-edges read them, one per lane, from the level's row in-edge matrix (LevelDesc::rowx_*) whose
//   address needs no record -- the same load round -- and broadcast them with readlane; only levels without a matrix
//   (in-degree > 64, or beyond the matrix budget) fetch the list from in_edge[] after the row record, one round later;
// * the row's in-edges are processed U per step so U sets of RC loads are in flight;
// * the segmented max runs only ceil(log2(max column in-degree of the group)) steps.
// GENERAL variant (levels tagged fast_ok == 2): a column with in-degree > 64 (more than 64 haplotypes recombining into
// one vertex) spans several slot blocks that one wave walks in turn, and rows of any in-degree fetch their in-edges 64
// at a time.  Only sizes beyond the 3-D grid or 2^20 in-edges per level fall back to the generic kernel above.
// COOP: 0 = every row; 1 = rows with more than COOP_MIN in-edges return (they are done by the cooperative region of
// the same launch); 2 = cooperative: the four waves of the workgroup walk a quarter of the row's in-edges each, wave 0
// merges the partial bests through LDS and finishes the task.
// ---------------------------------------------------------------------------------------------

template <int RC>
__device__ __forceinline__ void relax_select(const int (&vals)[RC], int dl, uint32_t ord, int r0, int w, int RP,
                                             int (&bval)[RC], uint32_t (&bord)[RC]) {
#pragma unroll
    for (int q = 0; q < RC; ++q) {
        const int cand = vals[q] + dl;
        const bool ok = (r0 + q < RP) & (r0 + q - w >= 0) & (vals[q] != NEG_INF);                   // :633, :646-647
        const bool take = ok & ((cand > bval[q]) | ((cand == bval[q]) & (ord > bord[q])));           // :657-659
        bval[q] = take ? cand : bval[q];
        bord[q] = take ? ord : bord[q];
    }
}

__device__ __forceinline__ void merge_best(int ov, uint32_t oo, bool same, int &bv, uint32_t &bo) {
    const bool take = same & ((ov > bv) | ((ov == bv) & (oo > bo)));
    bv = take ? ov : bv;
    bo = take ? oo : bo;
}

// Measurement build only (-DDG_SWEEP_PROBE, tools/probe build; never in the product library): one wave per destination row
// stamps the 100 MHz real-time counter at the task's phase boundaries.
#ifdef DG_SWEEP_PROBE
#define DG_PROBE_BEGIN unsigned long long pq[6] = {0, 0, 0, 0, 0, 0}; \
    const bool probe_on = A.probe != nullptr && blockIdx.x == 0 && blockIdx.y == 0 && (threadIdx.x >> 6) == 0 && (int)blockIdx.z < d.k2;
#define DG_PROBE(q) do { if (probe_on) { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); pq[q] = __builtin_amdgcn_s_memrealtime(); } } while (0)
#define DG_PROBE_END do { if (probe_on && (threadIdx.x & 63) == 0) { \
        atomicMin(&A.probe[(size_t)lvl * 8 + 0], pq[0]); atomicMax(&A.probe[(size_t)lvl * 8 + 1], pq[5]); \
        if ((int)blockIdx.z == d.k2 / 2) for (int q = 0; q < 6; ++q) A.probe[(size_t)lvl * 8 + 2 + q] = pq[q]; } } while (0)
#else
#define DG_PROBE_BEGIN
#define DG_PROBE(q) do { } while (0)
#define DG_PROBE_END do { } while (0)
#endif

template <int RC, bool DIGEST, bool GENERAL, int COOP>
__device__ __forceinline__ void sweep_task(const LevelHead &H, const FastArgs &A, const LevelDesc &d, __amdgpu_buffer_rsrc_t cur_rsrc,
                                           int32_t *__restrict__ nxt, int i2, int g, int r0, int lvl, int part = 0, uint2 *ex = nullptr) {
    const int lane = threadIdx.x & 63;
    const int RP = H.RP;
    DG_PROBE_BEGIN
    DG_PROBE(0);
    // first load round: every address below comes from kernel arguments and the block index alone
    const uint4 rr = H.rowrec_l[i2];                                    // {eu0, du, pu0, pu1}
    uint2 sl = H.slots_l[g * 64 + lane];
    const bool rowx = !GENERAL && H.rowx_stride > 0;
    uint32_t mypu = 0;                                                  // in-edge words of the row, one per lane
    if (rowx && lane < H.rowx_stride) mypu = H.rowx_l[i2 * H.rowx_stride + lane];
    // steps field: 0..6 = log2 steps of the segmented max; 15 = first block of a giant column (in-degree > 64: its
    // in-edges fill several consecutive blocks, all walked by THIS wave); 14 = continuation block (nothing to do)
    int steps = __builtin_amdgcn_readfirstlane((int)(sl.y >> 28));
    const int j2 = (sl.x != 0xFFFFFFFFu) ? (int)((sl.x >> 16) & 0x7FFFu) : -1 - lane;
    int nblk = 1;
    if (GENERAL) {
        if (steps == 14) return;                                        // (workgroup-uniform in the cooperative region: same g)
        if (steps == 15) {
            const int col = __builtin_amdgcn_readfirstlane(j2);
            nblk = ((int)H.rowrec_l[col].y + 63) >> 6;
            steps = 6;
        }
    }
    const uint16_t *dm = H.dm;
    const int dT = H.dT;
    const bool has_delta = dT != 0;
    const int du = (int)rr.y;
    if (COOP == 1 && du > COOP_MIN) return;
    DG_PROBE(1);
    const int t_lo = COOP == 2 ? (du * part) >> 2 : 0, t_hi = COOP == 2 ? (du * (part + 1)) >> 2 : du;   // this wave's share of the row's in-edges
    int bval[RC];
    uint32_t bord[RC];
#pragma unroll
    for (int q = 0; q < RC; ++q) { bval[q] = NEG_INF; bord[q] = 0; }
    const int64_t erow0 = (int64_t)rr.x * dT;                           // (dm is biased by the level's first in-edge)
    const int rowbytes = H.k * 4;
    bool act = false;
    // Source rows are r = r2 - w.  Byte offsets are relative to the padded buffer start (the resource), so rows
    // r = -1, -2 land in the front padding and r2 >= RP (ragged last chunk) in the tail padding; the select
    // discards what is out of range, which lets every load be issued unconditionally, back to back.
    for (int blk = 0; blk < (GENERAL ? nblk : 1); ++blk) {
        if (GENERAL && blk > 0) sl = H.slots_l[(g + blk) * 64 + lane];
        const bool actb = sl.x != 0xFFFFFFFFu;
        act |= actb;
        const int j = (int)(sl.x & 0x7FFFu), wv = (int)((sl.x >> 15) & 1u);
        const int dcol = has_delta ? (int)(sl.y & 0x000FFFFFu) : 0;
        const int evr = (int)((sl.y >> 20) & 0xFFu);                   // rank of this lane's in-edge inside its column's list
        if (du <= 2) {
            // 97 % of the rows: both in-edges came with the row record, no loop, no extra load
            if (actb && du > 0) {
                const int ia = (int)(rr.z & 0x7FFFu), wa = (int)(rr.z >> 31) + wv;    // (bit 16: flag for the chain walk)
                const int ib = (int)(rr.w & 0x7FFFu), wb = (int)(rr.w >> 31) + wv;
                const int offa = ((ia * RP + (r0 - wa)) * H.k + j) * 4 + H.pad_bytes;
                const int offb = ((ib * RP + (r0 - wb)) * H.k + j) * 4 + H.pad_bytes;
                int va[RC], vb[RC];
                const int dla = (int)dm[erow0 + dcol];
                int dlb = 0;
#pragma unroll
                for (int q = 0; q < RC; ++q)
                    va[q] = __builtin_amdgcn_raw_buffer_load_b32(cur_rsrc, offa + q * rowbytes, 0, 0);
                if (du == 2) {
                    dlb = (int)dm[erow0 + dT + dcol];
#pragma unroll
                    for (int q = 0; q < RC; ++q)
                        vb[q] = __builtin_amdgcn_raw_buffer_load_b32(cur_rsrc, offb + q * rowbytes, 0, 0);
                }
                relax_select<RC>(va, dla, ord_rank(0, evr), r0, wa, RP, bval, bord);
                if (du == 2) relax_select<RC>(vb, dlb, ord_rank(1, evr), r0, wb, RP, bval, bord);
            }
        } else {
            // heavy rows (recombination fan-in): U in-edges per step -- all their loads (U deltas + U*RC values) go out
            // back to back, then the selects run; (value, ord) max is associative and commutative, so the order inside
            // a step is irrelevant.  Small RC leaves registers for a deep step: in-degree 23 takes 2 steps at RC = 1.
            constexpr int U = GENERAL ? (RC >= 4 ? 2 : 4) : (RC >= 8 ? 2 : (RC >= 4 ? 4 : 8));
            // lean variant: one trip (in-degree <= 64, lane t of mypu = in-edge t); general: 64 in-edges per trip
            for (int c0 = GENERAL ? t_lo : 0; c0 < t_hi; c0 += GENERAL ? 64 : (1 << 30)) {
                const int tb = GENERAL ? c0 : t_lo, te = GENERAL ? min(c0 + 64, t_hi) : t_hi;
                if (!rowx) { mypu = 0; if (c0 + lane < te) mypu = A.in_edge[rr.x + c0 + lane]; }
                for (int t = tb; t < te; t += U) {
                    // the in-edge words live in SGPRs only until the load offset is formed; the select needs just their
                    // weight bits, kept in one mask (a deep step would otherwise hold U scalars and spill)
                    uint32_t wmask = 0;
                    if (actb) {
                        int vals[U][RC], dl[U];
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            if (t + u < te) {                                 // wave-uniform
                                const uint32_t p = (uint32_t)__builtin_amdgcn_readlane((int)mypu, t + u - c0);
                                wmask |= (p >> 31) << u;
                                const int iu = (int)(p & 0x7FFFFFFFu), w = (int)(p >> 31) + wv;
                                const int off = ((iu * RP + (r0 - w)) * H.k + j) * 4 + H.pad_bytes;
                                dl[u] = (int)dm[erow0 + (int64_t)(t + u) * dT + dcol];
#pragma unroll
                                for (int q = 0; q < RC; ++q)
                                    vals[u][q] = __builtin_amdgcn_raw_buffer_load_b32(cur_rsrc, off + q * rowbytes, 0, 0);
                            }
                        }
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            if (t + u < te) {
                                const int wu = (int)((wmask >> u) & 1u);
                                relax_select<RC>(vals[u], dl[u], ord_rank(t + u, evr), r0, wu + wv, RP, bval, bord);
                            }
                        }
                    }
                }
            }
        }
    }
    DG_PROBE(2);
    if (COOP == 2) {                                                    // partial bests of waves 1..3 -> wave 0
        if (part > 0) {
#pragma unroll
            for (int q = 0; q < RC; ++q) ex[((part - 1) * RC + q) * 64 + lane] = make_uint2((uint32_t)bval[q], bord[q]);
        }
        __syncthreads();
        if (part > 0) return;
#pragma unroll
        for (int p = 0; p < 3; ++p) {
#pragma unroll
            for (int q = 0; q < RC; ++q) {
                const uint2 o = ex[(p * RC + q) * 64 + lane];
                merge_best((int)o.x, o.y, true, bval[q], bord[q]);
            }
        }
    }
    // segmented max over lanes with equal destination column (lanes of a column are adjacent)
    if (steps > 0) {                                                    // first step: distance 1, DPP
        const int oj2 = lane_down1(j2);
        const bool same = (lane + 1 < 64) & (oj2 == j2);
#pragma unroll
        for (int q = 0; q < RC; ++q) merge_best(lane_down1(bval[q]), (uint32_t)lane_down1((int)bord[q]), same, bval[q], bord[q]);
    }
    for (int st = 1, sh = 2; st < steps; ++st, sh <<= 1) {
        const int oj2 = __shfl_down(j2, sh);
        const bool same = (lane + sh < 64) & (oj2 == j2);
#pragma unroll
        for (int q = 0; q < RC; ++q) merge_best(__shfl_down(bval[q], sh), (uint32_t)__shfl_down((int)bord[q], sh), same, bval[q], bord[q]);
    }
    const int pj2 = lane_up1(j2);
    const bool head = act & ((lane == 0) | (pj2 != j2));
    unsigned long long dsum = 0;
    DG_PROBE(3);
    if (head) {
#pragma unroll
        for (int q = 0; q < RC; ++q) {
            const int r2 = r0 + q;
            if (r2 < RP) {
                const int idx = (i2 * RP + r2) * d.k2 + j2;            // fast form: a state buffer is < 2 GB, 32-bit indices
                nxt[idx] = bval[q];                                    // (plain store: write-through costs +5 %, non-temporal +4.4 % on MHC-24)
                if (A.bp) { if (d.bp_nt) store_bp_nt(&A.bp[d.bp_off + idx], ~bord[q]); else A.bp[d.bp_off + idx] = (uint16_t)~bord[q]; }
                if (DIGEST && bval[q] != NEG_INF) {                    // (parity runs only: the extra loads are off the product path)
                    const unsigned long long o = ((unsigned long long)r2 * d.k2 + i2) * d.k2 + j2;   // oracle's r-major index
                    const uint32_t ru = BP_MAX_RANK - (bord[q] >> 8), rv = BP_MAX_RANK - (bord[q] & 0xFFu);
                    const uint32_t pi = A.in_edge[rr.x + ru] & 0x7FFFFFFFu;
                    const uint32_t pj = A.in_edge[H.rowrec_l[j2].x + rv] & 0x7FFFFFFFu;
                    dsum += digest_term(bval[q], o, pi, pj);
                }
            }
        }
    }
    if (g == 0 && d.ndead > 0) {                                        // columns nobody owns: unreachable
        for (int t = lane; t < d.ndead * RC; t += 64) {
            const int q = t % RC, c = A.dead_cols[d.dead_first + t / RC];
            if (r0 + q < RP) {
                const int64_t idx = ((int64_t)i2 * RP + r0 + q) * d.k2 + c;
                nxt[idx] = NEG_INF;
                if (A.bp) { if (d.bp_nt) store_bp_nt(&A.bp[d.bp_off + idx], 0xFFFFu); else A.bp[d.bp_off + idx] = (uint16_t)0xFFFFu; }
            }
        }
    }
    if (DIGEST && dsum) atomicAdd(&A.digest[lvl], dsum);
#ifdef DG_SWEEP_PROBE
    if (probe_on) pq[4] = __builtin_amdgcn_s_memrealtime();
    DG_PROBE(5);
    DG_PROBE_END;
#endif
}

#ifndef DG_PLAIN_WG
#define DG_PLAIN_WG 256
#endif
#define DG_PLAIN_GW ((DG_PLAIN_WG / 64) < 4 ? (DG_PLAIN_WG / 64) : 4)        // column blocks per workgroup
#define DG_PLAIN_CH ((DG_PLAIN_WG / 64) / DG_PLAIN_GW)                      // r chunks per workgroup
template <int RC, bool DIGEST, bool GENERAL>
__global__ __launch_bounds__(DG_PLAIN_WG) void dp_sweep_fast_kernel(const uint4 *rowrec_l, const uint2 *slots_l, const uint32_t *rowx_l, const int32_t *cur, const uint16_t *dm,
                                                            int rowx_stride, int nblocks, int rp_k, int pad_bytes, int dT, uint32_t buf_bytes,   // 16 dwords: preloaded
                                                            FastArgs A, LevelDesc d, int lvl) {
    const LevelHead H{rowrec_l, slots_l, rowx_l, cur, dm, rowx_stride, rp_k & 0x1FFF, rp_k >> 13, pad_bytes, dT, buf_bytes};
    publish_level(A.progress, lvl);
    const int wv = (int)(threadIdx.x >> 6);
    const int g = (int)blockIdx.x * DG_PLAIN_GW + (wv % DG_PLAIN_GW);    // always launched with DG_PLAIN_WG threads (reading blockDim would be a kernel-argument load)
    const int r0 = ((int)blockIdx.y * DG_PLAIN_CH + wv / DG_PLAIN_GW) * RC;
    if (g >= nblocks || r0 >= (rp_k & 0x1FFF)) return;                  // wave-uniform; no block barrier below
    int32_t *nxt = (int32_t *)(A.ring + (size_t)(DG_SLOT(lvl) ^ A.flip) * A.slot_bytes + A.pad_bytes);
    sweep_task<RC, DIGEST, GENERAL, 0>(H, A, d, state_rsrc(cur, buf_bytes), nxt, (int)blockIdx.z, g, r0, lvl);
}

// the same with a cooperative region: workgroup z < 4 n_heavy = slot block 4 x + (z & 3) of heavy row z >> 2, its four waves
// walk a quarter of the row's in-edges each.  The region is dispatched FIRST: its tasks (load round + LDS merge) are the
// longest of the launch, and started last they were the launch's tail (-3.6 % on the MHC-24 sweep against z >= k2).
template <int RC, bool DIGEST, bool GENERAL>
__global__ __launch_bounds__(256) void dp_sweep_coop_kernel(const uint4 *rowrec_l, const uint2 *slots_l, const uint32_t *rowx_l, const int32_t *cur,
                                                            int rowx_stride, int nblocks, int n_heavy, int rp_k, unsigned long long heavy_lo,
                                                            unsigned long long heavy_hi,                                                  // 16 dwords: preloaded
                                                            FastArgs A, LevelDesc d, int lvl, const uint16_t *dm, int dT, const int32_t *__restrict__ heavy_rows) {
    const LevelHead H{rowrec_l, slots_l, rowx_l, cur, dm, rowx_stride, rp_k & 0x1FFF, rp_k >> 13, A.pad_bytes, dT, A.buf_bytes};
    publish_level(A.progress, lvl);
    int32_t *nxt = (int32_t *)(A.ring + (size_t)(DG_SLOT(lvl) ^ A.flip) * A.slot_bytes + A.pad_bytes);
    const int r0 = (int)blockIdx.y * RC;                                // chunks of a row are neighbours in dispatch order: they share its delta row
    const int zc = 4 * n_heavy;
    if ((int)blockIdx.z < zc) {
        __shared__ uint2 ex[3 * RC * 64];
        const int hz = (int)blockIdx.z;
        const int g = (int)blockIdx.x * 4 + (hz & 3);
        if (g >= nblocks) return;                                       // workgroup-uniform: nobody is left at the barrier
        const int h = hz >> 2;
        int i2;                                                         // the first heavy rows ride in the kernel arguments (16 bits each): no dependent load
        if (h < 4) i2 = (int)((heavy_lo >> (16 * h)) & 0xFFFFu);
        else if (h < HEAVY_INLINE) i2 = (int)((heavy_hi >> (16 * (h - 4))) & 0xFFFFu);
        else i2 = heavy_rows[d.heavy_first + h];
        sweep_task<RC, DIGEST, GENERAL, 2>(H, A, d, state_rsrc(cur, A.buf_bytes), nxt, i2, g, r0, lvl, (int)(threadIdx.x >> 6), ex);
        return;
    }
    const int g = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (g >= nblocks) return;                                           // wave-uniform; no block barrier below
    sweep_task<RC, DIGEST, GENERAL, 1>(H, A, d, state_rsrc(cur, A.buf_bytes), nxt, (int)blockIdx.z - zc, g, r0, lvl);
}

// ---------------------------------------------------------------------------------------------
// Level pair: destination levels (l - 1, l) as ONE composed transition from level l - 2 (tables: dg_dp_pairs.hip).  The task shape
// is the plain fast kernel's -- one wave per (destination row, slot block, chunk of RC planes), the leading scalars preloaded,
// two load rounds: {composed row records, composed slot records}, then {both score deltas, RC values} per composed row in-edge.
// Each lane keeps per plane (value, ord, mid): ord = (255 - ru2) << 24 | (255 - rv2) << 16 | (255 - ru1) << 8 | (255 - rv1) makes the
// plain lexicographic max the reference's order over both levels; mid = middle row << 16 | middle column << 8 | w2u + w2v (in the wide
// layout: middle row << 13 | middle column << 3 | w2u + w2v, 10-bit positions: PairLayout in dg_dp.hpp) rides along with the winner, so the head lane addresses the middle cell without another load.  The state of level l - 1 is never
// written.  The head stores value and back-pointer of its cell of level l, and the back-pointer ru1 << 8 | rv1 of the middle cell
// it won through: cells that share a middle cell store the same word, middle cells nobody wins through stay unwritten (the walk
// reaches a middle cell only from a winner).
// ---------------------------------------------------------------------------------------------
template <int RC>
__device__ __forceinline__ void relax_pair(const int (&vals)[RC], int dl, uint32_t ord, uint32_t mid, int r0, int w, int RP,
                                           int (&bval)[RC], uint32_t (&bord)[RC], uint32_t (&bmid)[RC]) {
#pragma unroll
    for (int q = 0; q < RC; ++q) {
        const int cand = vals[q] + dl;
        const bool ok = (r0 + q < RP) & (r0 + q - w >= 0) & (vals[q] != NEG_INF);
        const bool take = ok & ((cand > bval[q]) | ((cand == bval[q]) & (ord > bord[q])));
        bval[q] = take ? cand : bval[q];
        bord[q] = take ? ord : bord[q];
        bmid[q] = take ? mid : bmid[q];
    }
}
__device__ __forceinline__ void merge_best_pair(int ov, uint32_t oo, uint32_t om, bool same, int &bv, uint32_t &bo, uint32_t &bm) {
    const bool take = same & ((ov > bv) | ((ov == bv) & (oo > bo)));
    bv = take ? ov : bv;
    bo = take ? oo : bo;
    bm = take ? om : bm;
}

// What a pair task needs before its stores (the pair kernels' leading scalars, as LevelHead is the fast kernels').
struct PairHead {
    const uint4 *pslots_l;              // the pair's composed slot records
    const int32_t *cur;                 // padded start of the state buffer of level l - 2
    const uint16_t *dm1, *dm2;          // score deltas of levels l - 1 and l (the zero slot where dT = 0)
    int RP, k0, pad_bytes, dT1, dT2;
    uint32_t buf_bytes;
};

// One wave's task of a pair launch: destination row i2, slot block g, planes r0 .. r0 + RC - 1.  recs: the row's records.
// COOP: 0 = every row from its PAIR_MAX_INDEG light records (dp_sweep_pair_kernel); 1 = the same, big rows return (they are done by the
// cooperative region of the same launch); 2 = cooperative, recs = the big row's PAIR_BIG_MAX_INDEG records: wave `part` of the workgroup
// walks a quarter of the composed row in-edges -- at most PAIR_MAX_INDEG, one gather step, the depth of a light row --, waves 1..3 park
// (value, ord, mid) per plane in LDS, wave 0 merges them and finishes the task.  No wave leaves before the barrier.
// digest: null, or (DIGEST) the per-level accumulators.  WIDE: the records' layout (PairLayout: 10-bit positions for levels up to
// PAIR_WIDE_MAX_WIDTH wide); it changes the shifts and masks of the decode and of the mid word, nothing else.
template <int RC, bool DIGEST, int COOP, bool WIDE>
__device__ __forceinline__ void pair_task(const PairHead &H, const uint2 *recs, int32_t *__restrict__ nxt, uint16_t *__restrict__ bp1, uint16_t *__restrict__ bp2, int kk, int nt,
                                          int i2, int g, int r0, int lvl, unsigned long long *digest, int part = 0, uint4 *ex = nullptr) {
    typedef PairLayout<WIDE> Y;
    const int lane = threadIdx.x & 63;
    const int RP = H.RP, k0 = H.k0, pad_bytes = H.pad_bytes, dT1 = H.dT1, dT2 = H.dT2;
    const uint16_t *dm1 = H.dm1, *dm2 = H.dm2;
    constexpr int NREC = COOP == 2 ? PAIR_BIG_MAX_INDEG : PAIR_MAX_INDEG, RU1_SHIFT = COOP == 2 ? 27 : 25, RANK_MASK = COOP == 2 ? 31 : 7;
    // first load round: addresses from kernel arguments and the block index alone
    const uint2 rec = recs[lane & (NREC - 1)];                          // composed row in-edge t in lanes t, t + NREC, ...
    const uint4 sl = H.pslots_l[g * 64 + lane];
    const __amdgpu_buffer_rsrc_t cur_rsrc = state_rsrc(H.cur, H.buf_bytes);
    const int du = __builtin_amdgcn_readfirstlane((int)(rec.x >> Y::DEG)) & (COOP == 2 ? 0x3F : 0xF);
    if (COOP == 1 && du > PAIR_MAX_INDEG) return;                       // (wave-uniform; no block barrier in the light region)
    const int t_lo = COOP == 2 ? (du * part) >> 2 : 0, t_hi = COOP == 2 ? (du * (part + 1)) >> 2 : du;   // this wave's share of the composed row in-edges
    const int steps = __builtin_amdgcn_readfirstlane((int)(sl.z >> 16)) & 0xF;
    const bool act = sl.x != 0xFFFFFFFFu;
    const int j = (int)(sl.x & Y::POS), wv = (int)((sl.x >> Y::W1) & 1u) + (int)((sl.x >> Y::W2) & 1u);
    const uint32_t lanemid = (((sl.x >> Y::MID) & Y::MID_MASK) << Y::MID_COL) | ((sl.x >> Y::W2) & 1u);
    const int j2 = act ? (int)((sl.z >> 20) & Y::COL_MASK) : -1 - lane;
    const int c2 = dT2 ? (int)(sl.y & 0xFFFFu) : 0, c1 = dT1 ? (int)(sl.y >> 16) : 0;
    const uint32_t ordc = ((uint32_t)(BP_MAX_RANK - (int)(sl.z & 0xFFu)) << 16) | (uint32_t)(BP_MAX_RANK - (int)((sl.z >> 8) & 0xFFu));
    int bval[RC];
    uint32_t bord[RC], bmid[RC];
#pragma unroll
    for (int q = 0; q < RC; ++q) { bval[q] = NEG_INF; bord[q] = 0; bmid[q] = 0; }
    const int rowbytes = k0 * 4;
    // Source rows are r = r2 - w, w <= 4: rows -1 .. -4 land in the front padding (4 * max_k cells when pairs exist), a ragged last
    // chunk in the tail padding; the select discards both, so every load is issued unconditionally.
    constexpr int U = COOP == 2 ? PAIR_MAX_INDEG : (RC >= 4 ? 4 : 8);
    for (int t = t_lo; t < t_hi; t += U) {
        if (act) {
            int vals[U][RC], dl[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (t + u < t_hi) {                                         // wave-uniform
                    const uint32_t px = (uint32_t)__builtin_amdgcn_readlane((int)rec.x, t + u), py = (uint32_t)__builtin_amdgcn_readlane((int)rec.y, t + u);
                    const int iu = (int)(px & Y::POS), w = (int)((px >> Y::W1) & 1u) + (int)((px >> Y::W2) & 1u) + wv;
                    const int off = ((iu * RP + (r0 - w)) * k0 + j) * 4 + pad_bytes;
                    dl[u] = (int)dm2[(int)(py & 0x7FFu) * dT2 + c2] + (int)dm1[(int)((py >> 11) & 0x7FFu) * dT1 + c1];
#pragma unroll
                    for (int q = 0; q < RC; ++q) vals[u][q] = __builtin_amdgcn_raw_buffer_load_b32(cur_rsrc, off + q * rowbytes, 0, 0);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (t + u < t_hi) {
                    const uint32_t px = (uint32_t)__builtin_amdgcn_readlane((int)rec.x, t + u), py = (uint32_t)__builtin_amdgcn_readlane((int)rec.y, t + u);
                    const int w = (int)((px >> Y::W1) & 1u) + (int)((px >> Y::W2) & 1u) + wv;
                    const uint32_t ord = ((uint32_t)(BP_MAX_RANK - (int)((py >> 22) & RANK_MASK)) << 24) | ((uint32_t)(BP_MAX_RANK - (int)((py >> RU1_SHIFT) & RANK_MASK)) << 8) | ordc;
                    const uint32_t mid = ((((px >> Y::MID) & Y::MID_MASK) << Y::MID_ROW) | ((px >> Y::W2) & 1u)) + lanemid;
                    relax_pair<RC>(vals[u], dl[u], ord, mid, r0, w, RP, bval, bord, bmid);
                }
            }
        }
    }
    if (COOP == 2) {                                                    // partial bests of waves 1..3 -> wave 0
        if (part > 0) {
#pragma unroll
            for (int q = 0; q < RC; ++q) ex[((part - 1) * RC + q) * 64 + lane] = make_uint4((uint32_t)bval[q], bord[q], bmid[q], 0u);
        }
        __syncthreads();
        if (part > 0) return;
#pragma unroll
        for (int p = 0; p < 3; ++p) {
#pragma unroll
            for (int q = 0; q < RC; ++q) {
                const uint4 o = ex[(p * RC + q) * 64 + lane];
                merge_best_pair((int)o.x, o.y, o.z, true, bval[q], bord[q], bmid[q]);
            }
        }
    }
    // segmented max over lanes with equal destination column (lanes of a column are adjacent)
    if (steps > 0) {
        const int oj2 = lane_down1(j2);
        const bool same = (lane + 1 < 64) & (oj2 == j2);
#pragma unroll
        for (int q = 0; q < RC; ++q) merge_best_pair(lane_down1(bval[q]), (uint32_t)lane_down1((int)bord[q]), (uint32_t)lane_down1((int)bmid[q]), same, bval[q], bord[q], bmid[q]);
    }
    for (int st = 1, sh = 2; st < steps; ++st, sh <<= 1) {
        const int oj2 = __shfl_down(j2, sh);
        const bool same = (lane + sh < 64) & (oj2 == j2);
#pragma unroll
        for (int q = 0; q < RC; ++q)
            merge_best_pair(__shfl_down(bval[q], sh), (uint32_t)__shfl_down((int)bord[q], sh), (uint32_t)__shfl_down((int)bmid[q], sh), same, bval[q], bord[q], bmid[q]);
    }
    const int pj2 = lane_up1(j2);
    const bool head = act & ((lane == 0) | (pj2 != j2));
    unsigned long long dsum = 0;
    if (head) {
        const int k1 = kk & (int)Y::COL_MASK, k2 = kk >> Y::KK;
#pragma unroll
        for (int q = 0; q < RC; ++q) {
            const int r2 = r0 + q;
            if (r2 < RP) {
                const int idx = (i2 * RP + r2) * k2 + j2;
                nxt[idx] = bval[q];
                if (bp2) {
                    const uint32_t b2 = ~(bord[q] >> 16);                   // ru2 << 8 | rv2; an untouched best keeps ord 0 -> 0xFFFF = unreachable
                    if (nt) store_bp_nt(&bp2[idx], b2); else bp2[idx] = (uint16_t)b2;
                    if (bord[q]) {                                          // reachable: mark the middle cell it came through (row r2 - w2u - w2v >= 0)
                        const uint32_t m = bmid[q];
                        bp1[((int)(m >> Y::MID_ROW) * RP + r2 - (int)(m & Y::MID_W)) * k1 + (int)((m >> Y::MID_COL) & Y::MID_MASK)] = (uint16_t)~bord[q];
                    }
                }
                if (DIGEST && bval[q] != NEG_INF) {
                    const unsigned long long o = ((unsigned long long)r2 * k2 + i2) * k2 + j2;   // oracle's r-major index
                    dsum += digest_term(bval[q], o, bmid[q] >> Y::MID_ROW, (bmid[q] >> Y::MID_COL) & Y::MID_MASK);
                }
            }
        }
    }
    if (DIGEST && dsum) atomicAdd(&digest[lvl], dsum);
}

// DG: empty -- the kernels the product runs, dp_sweep_pair_kernel<RC> -- or one trailing unsigned long long *digest (parity runs, options
// digest + pair_digest): the head lane then also adds the oracle's term of every reachable cell of level l -- its predecessor is the
// middle cell in bmid -- to digest[lvl]; level l - 1 is never materialised and keeps the 0 of the run's memset.
// WIDE: the record layout (PairLayout).  The tracer prints the instantiations as dp_sweep_pair_kernel<RC, false> and <RC, true>; the pair
// profile calls them dp_sweep_pair_kernel<RC> and dp_sweep_pair_wide_kernel<RC>.  The narrow instantiations are, instruction for
// instruction, what dp_sweep_pair_kernel<RC> was before the wide layout existed (a body shared through an inlined function instead
// made the compiler order their scalar instructions differently).
template <int RC, bool WIDE, typename... DG>
__global__ __launch_bounds__(256) void dp_sweep_pair_kernel(const uint2 *prow_l, const uint4 *pslots_l, const int32_t *cur, const uint16_t *dm1, const uint16_t *dm2,
                                                            int nblocks, int rp_k, int pad_bytes, int dT1, int dT2, uint32_t buf_bytes,   // 16 dwords: preloaded
                                                            int32_t *__restrict__ nxt, uint16_t *__restrict__ bp1, uint16_t *__restrict__ bp2, int kk, int nt, int *progress, int lvl,
                                                            DG... digest) {
    constexpr bool DIGEST = sizeof...(DG) != 0;
    publish_level(progress, lvl);
    const int g = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6), r0 = (int)blockIdx.y * RC, i2 = (int)blockIdx.z;
    if (g >= nblocks) return;                                           // wave-uniform; no block barrier below
    const PairHead H{pslots_l, cur, dm1, dm2, rp_k & 0x1FFF, rp_k >> 13, pad_bytes, dT1, dT2, buf_bytes};
    unsigned long long *const acc[] = {nullptr, digest...};
    pair_task<RC, DIGEST, 0, WIDE>(H, prow_l + i2 * PAIR_MAX_INDEG, nxt, bp1, bp2, kk, nt, i2, g, r0, lvl, acc[sizeof...(DG)]);
}

// The same for a fan-in pair: the later level holds n_big big rows (composed in-degree 9..32).  Workgroup z < 4 n_big = slot block
// 4 x + (z & 3) of big row z >> 2, its four waves a quarter of the row's records each; the region is dispatched first, as in
// dp_sweep_coop_kernel.  The rows beyond run the light task; a big row returns from it at once.  The first PAIR_BIG_INLINE big rows
// ride in a preloaded scalar (8 bits each; of a wide pair the first PAIR_WIDE_BIG_INLINE, 16 bits each), later ones come from the pair's
// list.  In the pair profile: dp_sweep_pair_coop_kernel<RC> (narrow) and dp_sweep_pair_coop_wide_kernel<RC>.
template <int RC, bool WIDE, typename... DG>
__global__ __launch_bounds__(256) void dp_sweep_pair_coop_kernel(const uint2 *prow_l, const uint4 *pslots_l, const uint2 *pbig_l, const int32_t *cur, const uint16_t *dm2,
                                                                 unsigned long long big_in, int nblocks, int n_big, int rp_k, int dT2,   // 16 dwords: preloaded
                                                                 const uint16_t *dm1, int dT1, int pad_bytes, uint32_t buf_bytes, const int32_t *__restrict__ big_rows,
                                                                 int32_t *__restrict__ nxt, uint16_t *__restrict__ bp1, uint16_t *__restrict__ bp2, int kk, int nt, int *progress, int lvl,
                                                                 DG... digest) {
    constexpr bool DIGEST = sizeof...(DG) != 0;
    publish_level(progress, lvl);
    const PairHead H{pslots_l, cur, dm1, dm2, rp_k & 0x1FFF, rp_k >> 13, pad_bytes, dT1, dT2, buf_bytes};
    unsigned long long *const acc[] = {nullptr, digest...};
    const int r0 = (int)blockIdx.y * RC;
    const int zc = 4 * n_big;
    if ((int)blockIdx.z < zc) {
        __shared__ uint4 ex[3 * RC * 64];
        const int hz = (int)blockIdx.z;
        const int g = (int)blockIdx.x * 4 + (hz & 3);
        if (g >= nblocks) return;                                       // workgroup-uniform: nobody is left at the barrier
        const int h = hz >> 2;
        const int i2 = WIDE ? (h < PAIR_WIDE_BIG_INLINE ? (int)((big_in >> (16 * h)) & 0xFFFFu) : big_rows[h])
                            : (h < PAIR_BIG_INLINE ? (int)((big_in >> (8 * h)) & 0xFFu) : big_rows[h]);
        pair_task<RC, DIGEST, 2, WIDE>(H, pbig_l + h * PAIR_BIG_MAX_INDEG, nxt, bp1, bp2, kk, nt, i2, g, r0, lvl, acc[sizeof...(DG)], (int)(threadIdx.x >> 6), ex);
        return;
    }
    const int g = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6), i2 = (int)blockIdx.z - zc;
    if (g >= nblocks) return;                                           // wave-uniform; no block barrier below
    pair_task<RC, DIGEST, 1, WIDE>(H, prow_l + i2 * PAIR_MAX_INDEG, nxt, bp1, bp2, kk, nt, i2, g, r0, lvl, acc[sizeof...(DG)]);
}

// Sweep look-ahead: streams the graph tables (row records, slot records, in-edges, score deltas) of a batch of upcoming
// levels through the memory-side Infinity Cache.  Every table byte is read exactly once per pass, so without this each
// level's two dependent load rounds go all the way to HBM; the batch is a few MB, read at full chip bandwidth.
constexpr int WARM_RANGES = 5;
struct WarmRanges { const char *p[WARM_RANGES]; long long n16[WARM_RANGES]; };   // start (16-byte aligned down) and length in 16-byte units
__global__ __launch_bounds__(256) void dp_warm_tables_kernel(WarmRanges W) {
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x, nth = (long long)gridDim.x * blockDim.x;
#pragma unroll
    for (int q = 0; q < WARM_RANGES; ++q) {
        const uint4 *p = (const uint4 *)W.p[q];
        for (long long i = tid; i < W.n16[q]; i += nth) { uint4 v = p[i]; asm volatile("" ::"v"(v.x), "v"(v.y), "v"(v.z), "v"(v.w)); }
    }
}

// L2 table prefetcher.  The look-ahead above gets a level's tables as far as the memory-side Infinity Cache; the two load
// rounds of a task then cost an Infinity-Cache round trip each.  The L2 is per XCD, so this kernel -- PF_WORKGROUPS one-wave
// workgroups on a side stream, two per XCD by round-robin dispatch -- reads one word of every 128-byte line of the next
// levels' tables (row records, slot records, in-edges, row matrices, score deltas) on EVERY XCD, l2_prefetch levels ahead of
// the level the sweep publishes (workgroup 0 of every sweep launch stores its level).
// Measured on MHC-24 (sweep, ms): off 589; publishing alone 595; 8 / 16 / 64 workgroups 584.5 / 581.9 / 622-627 (64 pollers
// on the published word cost more than the prefetch gives: poll-only 638); 3 / 6 / 12 levels ahead 585.6 / 584.5 / 588.9.
// (A per-level prefetch LAUNCH in the chain made the traced sweep kernels 9 % shorter, 5.26 -> 4.79 us -- most of that was
// the extra launch absorbing the kernel boundary, not the cache.)
// Hints only: nothing waits for it; it leaves when the host marks the range done, when a newer range's sequence number
// appears, or after 0.3 ms without progress.
constexpr int PF_WORKGROUPS = 16, PF_FAR_WORKGROUPS = 16;
constexpr unsigned long long PF_IDLE_TICKS = 30000;      // 0.3 ms
struct PfCtl { int seq, stop, levels_done, probe, probe_ok, pad_[27]; int level; int pad2_[31]; };      // level: a line of its own

__global__ void dp_pf_ctl_kernel(PfCtl *c, int seq, int level, int stop) {
    __hip_atomic_store(&c->level, level, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&c->stop, stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&c->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}

// Does the side stream run beside the sweep's stream?  HIP maps streams onto a handful of hardware queues; a prefetcher that
// shares the sweep's queue would sit in front of the levels it is waiting for until it gives up.  Probed once per state: a
// kernel on the side stream waits up to ~2 ms (100 MHz counter) for a word that a kernel issued AFTER it on the sweep's
// stream sets -- it sees it only if the two really run concurrently.
__global__ void dp_pf_probe_wait_kernel(PfCtl *c, int token) {
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    int ok = 0;
    while (__builtin_amdgcn_s_memrealtime() - t0 < 200000ULL) {
        if (__hip_atomic_load(&c->probe, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == token) { ok = 1; break; }
        __builtin_amdgcn_s_sleep(16);
    }
    c->probe_ok = ok;
}
__global__ void dp_pf_probe_set_kernel(PfCtl *c, int token) { __hip_atomic_store(&c->probe, token, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(64) void dp_l2_prefetch_kernel(const LevelDesc *__restrict__ descs, FastArgs F, PfCtl *ctl, int seq, int lb, int le, int ahead_near, int delta_resident, int far,
                                                            const int32_t *__restrict__ pair_at, const PairDesc *__restrict__ pairs, const uint2 *__restrict__ prow, const uint4 *__restrict__ pslots, const uint2 *__restrict__ pbig) {
    __shared__ int dump[64];
    // a load whose data nobody wants: straight into an LDS dump word per lane (no destination register, nothing to wait for)
#define DG_DROP_LOAD(PTR) __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(PTR), (__attribute__((address_space(3))) void *)dump, 4, 0, 0)
    // blocks [0, PF_WORKGROUPS): the L2 role (every XCD reads every line of the level `ahead_near` levels down);
    // blocks beyond (far > 0): the Infinity-Cache role -- each line once chip-wide, `far` levels down (what the periodic
    // look-ahead launches in the level chain did)
    const bool far_role = (int)blockIdx.x >= PF_WORKGROUPS;
    const int lane = (int)threadIdx.x;
    const int slot = far_role ? (int)blockIdx.x - PF_WORKGROUPS : (int)(blockIdx.x >> 3), nslot = far_role ? (int)gridDim.x - PF_WORKGROUPS : PF_WORKGROUPS >> 3;
    const int ahead = far_role ? far : ahead_near, behind = far_role ? far - 64 : 0;      // the far role stays within [far - 64, far] levels of the sweep
    int last = INT32_MIN, done = 0;
    unsigned long long t_last = __builtin_amdgcn_s_memrealtime();
    int *level_word = &ctl->level;
    auto lines = [&](const char *base, long long bytes) {               // this workgroup's share of the 128-byte lines of [base, base + bytes)
        if (bytes <= 0) return;
        const uintptr_t a = (uintptr_t)base & ~(uintptr_t)127;
        const int n = (int)(((uintptr_t)base + (uintptr_t)bytes - a + 127) >> 7);
        for (int t = slot * 64 + lane; t < n; t += nslot * 64) DG_DROP_LOAD((const char *)a + ((size_t)t << 7));
    };
    int polls = 0;
    for (int lp = lb; lp < le;) {
        // one word is polled (the line the sweep's workgroup 0 stores to: every poll competes with that store); the range's
        // sequence number and stop flag, in another line, every 32nd time
        if ((polls++ & 31) == 0 &&
            (__hip_atomic_load(&ctl->seq, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) != seq || __hip_atomic_load(&ctl->stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) break;
        const int lv = __builtin_amdgcn_readfirstlane(__hip_atomic_load(level_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        // Leaves after PF_IDLE_TICKS (100 MHz) without progress.  HIP maps streams and graph launches onto a few hardware queues;
        // if this kernel ever lands in front of the sweep in one queue, the sweep cannot start until it is gone (seen with
        // GPU_MAX_HW_QUEUES=8: every range waited out the former 10^5-poll limit, a 6.5x slower sweep).  0.3 ms per range bounds
        // that case at well under 1 % of a pass; a longer legitimate gap (the capturing pass) merely ends the prefetching of the range.
        const unsigned long long now = __builtin_amdgcn_s_memrealtime();
        if (lv != last) { last = lv; t_last = now; } else if (now - t_last > PF_IDLE_TICKS) break;
        if (lp <= lv + behind) lp = lv + behind + 1;                    // overtaken (L2 role: level lv is running)
        if (lp >= le) break;
        if (lp - lv > ahead) { __builtin_amdgcn_s_sleep(48); continue; }
        const LevelDesc &d = descs[lp];
        const int k2 = __builtin_amdgcn_readfirstlane(d.k2), T = __builtin_amdgcn_readfirstlane(d.T);
        // "paired with" word of the level (null: this range launches no pairs): the earlier level of a pair has no launch of its own, the
        // later one reads the composed tables and both levels' score deltas.  (A pair that straddles the edge of a hipGraph batch or of a
        // lattice chunk runs as two single launches whose own tables are then not prefetched: one pair per 1,000 levels, hints only.)
        const int pa = pair_at ? __builtin_amdgcn_readfirstlane(pair_at[lp]) : -1;
        if (pa == -2) { ++lp; ++done; continue; }
        if (pa >= 0) {
            const PairDesc &p = pairs[pa];
            lines((const char *)(prow + p.row_first), 8LL * PAIR_MAX_INDEG * k2);
            lines((const char *)(pslots + p.slot_first), 1024LL * p.nblocks);
            lines((const char *)(pbig + (long long)PAIR_BIG_MAX_INDEG * p.big_first), 8LL * PAIR_BIG_MAX_INDEG * p.n_big);
            if (delta_resident) {
                const LevelDesc &d1 = descs[lp - 1];
                if (d.delta_off >= 0 && (long long)T * T <= (128 << 10)) lines((const char *)(F.delta + d.delta_off), 2LL * T * T);
                if (d1.delta_off >= 0 && (long long)d1.T * d1.T <= (128 << 10)) lines((const char *)(F.delta + d1.delta_off), 2LL * d1.T * d1.T);
            }
            ++lp; ++done;
            continue;
        }
        lines((const char *)(F.rowrec + d.b0), 16LL * k2);
        lines((const char *)(F.slots + d.slot_first), 512LL * d.nblocks);
        lines((const char *)(F.in_edge + d.in_base), 4LL * T);
        if (d.rowx_stride > 0) lines((const char *)(F.rowx + d.rowx_off), 4LL * k2 * d.rowx_stride);
        if (delta_resident && d.delta_off >= 0 && (long long)T * T <= (128 << 10)) lines((const char *)(F.delta + d.delta_off), 2LL * T * T);
        ++lp; ++done;
    }
    if (lane == 0 && blockIdx.x == 0) atomicAdd(&ctl->levels_done, done);
#undef DG_DROP_LOAD
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// THE table of recombination-chunk sizes (RC), ascending; dispatch (launch_variant), per-level choice (choose_rc), the run's all-planes chunk
// (sweep_prepare) and the variants' indices and names (SweepVariant) walk it, and no RC is written anywhere else.  Every entry is an instantiation of
// the fast kernel.  RC_COOP: of the cooperative kernel too, and a candidate of choose_rc's cooperative pass; RC_PART: a candidate of choose_rc while
// below the run's all-planes chunk; RC_ALL: an all-planes chunk (the first that holds R + 1 planes is the run's rc_sel), instantiated for the generic kernel too.
enum : unsigned { RC_COOP = 1, RC_PART = 2, RC_ALL = 4, RC_ANY = 7 };
constexpr struct SweepRc { int rc; unsigned is; } SWEEP_RCS[] = {
    {1, RC_COOP | RC_PART}, {2, RC_COOP | RC_PART}, {3, RC_COOP | RC_PART}, {4, RC_COOP | RC_PART}, {5, RC_PART}, {6, RC_PART},
    {8, RC_PART | RC_ALL}, {10, RC_PART}, {11, RC_PART}, {16, RC_PART}, {19, RC_ALL}, {33, RC_ALL}};
constexpr int N_SWEEP_RCS = (int)(sizeof SWEEP_RCS / sizeof SWEEP_RCS[0]);
constexpr bool sweep_rcs_ascend(int q = 1) { return q >= N_SWEEP_RCS || (SWEEP_RCS[q - 1].rc < SWEEP_RCS[q].rc && sweep_rcs_ascend(q + 1)); }
static_assert(SWEEP_RCS[0].rc >= 1 && sweep_rcs_ascend() && (SWEEP_RCS[N_SWEEP_RCS - 1].is & RC_ALL), "ascending (choose_rc's ties go to the larger RC), and the largest chunk is an all-planes one");

// variants in the launch profile's order: the generic kernel, then per table entry lean, lean cooperative, general, general cooperative
int SweepVariant::count() { return 1 + 4 * N_SWEEP_RCS; }
SweepVariant SweepVariant::at(int index) { return index == 0 ? SweepVariant{0, false, false} : SweepVariant{SWEEP_RCS[(index - 1) / 4].rc, ((index - 1) & 2) != 0, ((index - 1) & 1) != 0}; }
int SweepVariant::index() const {
    for (int q = 0; q < N_SWEEP_RCS; ++q) if (SWEEP_RCS[q].rc == rc) return 1 + 4 * q + (general ? 2 : 0) + (coop ? 1 : 0);
    return 0;
}
bool SweepVariant::exists() const {
    if (rc == 0) return !general && !coop;
    for (const SweepRc &e : SWEEP_RCS) if (e.rc == rc) return !coop || (e.is & RC_COOP);
    return false;
}
std::string SweepVariant::name() const {
    return rc == 0 ? "dp_sweep_kernel" : std::string("dp_sweep_") + (coop ? "coop" : "fast") + "_kernel<" + std::to_string(rc) + (general ? ",general>" : ",lean>");
}

// The run-time (rc, digest, general) as template arguments: calls f(RC, DIGEST, GENERAL), each a std::integral_constant, for the table entry rc if it
// carries a mark of WANT (f is instantiated for those entries only).  A chunk size that is not among them cannot be launched: false, nothing called.
template <unsigned WANT, int Q = 0, class F>
static bool launch_variant(int rc, bool digest, bool general, F &f) {
    if constexpr (Q < N_SWEEP_RCS) {
        if constexpr ((SWEEP_RCS[Q].is & WANT) != 0) if (rc == SWEEP_RCS[Q].rc) {
            constexpr std::integral_constant<int, SWEEP_RCS[Q].rc> RC{};
            if (digest) { if (general) f(RC, std::true_type{}, std::true_type{}); else f(RC, std::true_type{}, std::false_type{}); }
            else { if (general) f(RC, std::false_type{}, std::true_type{}); else f(RC, std::false_type{}, std::false_type{}); }
            return true;
        }
        return launch_variant<WANT, Q + 1>(rc, digest, general, f);
    }
    return false;
}

void sweep_prepare(const DpState &S, SweepLaunch &X) {
    for (const SweepRc &e : SWEEP_RCS) if ((e.is & RC_ALL) && (X.rc_sel = e.rc) >= S.RP) break;
    X.digest = S.opt.want_digest != 0; X.rp_active = S.RP;
    X.small_state = S.state_alloc_bytes < ((size_t)1 << 31);            // 32-bit buffer offsets inside a slot
    SweepArgs &A = X.A;
    A.descs = S.d_descs.as<LevelDesc>(); A.in_off = S.d_in_off.as<uint32_t>(); A.in_edge = S.d_in_edge.as<uint32_t>();
    A.grp_begin = S.d_grp.as<uint32_t>(); A.in_dst = S.d_in_dst.as<int32_t>(); A.dead_cols = S.d_dead.as<int32_t>();
    A.delta = A.delta_zero = S.d_delta.as<uint16_t>();
    A.ring = S.d_ring.as<char>(); A.slot_bytes = S.state_alloc_bytes; A.pad_bytes = 4 * (size_t)S.pad_front;
    A.bp = nullptr; A.digest = S.d_digest.as<unsigned long long>(); A.RP = S.RP; A.flip = 0;
    FastArgs &F = X.F;
    F.rowrec = S.d_rowrec.as<uint4>(); F.slots = S.d_slots.as<uint2>(); F.in_edge = A.in_edge; F.rowx = S.d_rowx.as<uint32_t>(); F.dead_cols = A.dead_cols;
    F.delta = F.delta_zero = A.delta; F.bp = nullptr; F.digest = A.digest; F.RP = S.RP;
    F.ring = S.d_ring.as<char>(); F.slot_bytes = (uint32_t)S.state_alloc_bytes; F.flip = 0;
#ifdef DG_SWEEP_PROBE
    F.probe = S.d_probe.as<unsigned long long>();
#endif
    F.progress = A.progress = &S.d_pfctl.as<PfCtl>()->level;
    F.pad_bytes = (int)(4 * S.pad_front);
    F.buf_bytes = (uint32_t)std::min<size_t>(S.state_alloc_bytes, 0x7FFFFFFFu);
}

void sweep_init_state(const DpState &S, hipStream_t s) {
    hipLaunchKernelGGL(dp_init_kernel, dim3((unsigned)((S.RP + 255) / 256)), dim3(256), 0, s, S.d_ring.as<int32_t>() + S.pad_front, S.RP);
}

// A lone wave retires ~1 instruction per 4-8 cycles, so an RC-fold unrolled task is the level's critical path: while
// the chip has idle wave slots, give each wave fewer recombination counts.  Cost model fitted on MHC-24 (R = 18) and
// the 100-walk chr22-style panel (R = 32):
//   T(RC) = max(1, W / cap) * (t0 + dmax * RC * tg) + W * tw,   W = tasks * ceil(RP / RC) waves.
// First factor: rounds of resident waves; second: a wave's dependent chain (the row with the largest in-degree walks
// dmax in-edges with RC gathers each); last: per-wave issue overhead.  Cooperative variant (RC <= 4): rows above
// COOP_MIN in-edges are walked by four waves, so the chain is a quarter (at least COOP_MIN) while four extra
// workgroup slots per heavy row are launched.
static void choose_rc(const DpState &S, const SweepLaunch &X, const LevelDesc &d, int l, int &rc, bool &coop) {
    const int rc_sel = rc = X.rc_sel;
    coop = false;
    if (S.opt.adaptive_rc == 0) return;
    const bool coop_ok = S.opt.use_coop && d.n_heavy > 0 && d.k2 + 4 * d.n_heavy <= 65535;
    const double dmax = (double)std::max(1, S.level_dmax[l]);
    double best = 1e300;
    for (int pass = (coop_ok && S.opt.use_coop == 2) ? 1 : 0; pass < (coop_ok ? 2 : 1); ++pass) {     // coop = 2 (tests): whenever possible
        for (const SweepRc &e : SWEEP_RCS) {                                   // the partial chunks below rc_sel, then rc_sel itself
            if (e.rc != rc_sel && !((e.is & RC_PART) && e.rc < rc_sel)) continue;
            if (pass == 1 && !(e.is & RC_COOP)) continue;
            if (S.opt.test_force_rc && e.rc != S.opt.test_force_rc) continue;  // tests: this entry or, where it is no candidate, plain rc_sel
            const double rows = pass ? (double)d.k2 + 4.0 * d.n_heavy : (double)d.k2;
            const double chain = pass ? std::max((double)COOP_MIN, std::ceil(dmax / 4.0)) + 1.0 : dmax;
            const double W = rows * d.nblocks * ((X.rp_active + e.rc - 1) / e.rc);
            const double T = std::max(1.0, W / (double)S.opt.rc_cap) * ((double)S.opt.rc_t0_ns + chain * e.rc * (double)S.opt.rc_tg_ps * 1e-3) + W * (double)S.opt.rc_tw_ps * 1e-3;
            if (T <= best) { best = T; rc = e.rc; coop = pass == 1; }      // ties: the larger RC (fewer waves)
        }
    }
}

int sweep_launch_level(const DpState &S, SweepLaunch &X, int l, hipStream_t s) {
    LevelDesc d = S.descs[l];                                           // the copy that goes to the kernel
    // small and mid-sized levels end sooner with write-back back-pointer stores (3.6 vs 4.2 us per level on MHC_4; threshold
    // 16 K / 64 K / 256 K / 1 M / 4 M cells: MHC-24 sweep 580 / 575 / 574 / 579 / 586 ms), big ones with non-temporal ones that
    // keep the once-written lattice out of the L2
    d.bp_nt = (int64_t)d.k2 * d.k2 * S.RP >= S.opt.bp_nt_min_cells ? 1 : 0;
    SweepVariant v{0, false, false};
    bool launched;                                                      // false: the table holds no such kernel, nothing was launched
    if (d.fast_ok && X.small_state && S.RP <= 65535 && S.opt.use_fast) {
        choose_rc(S, X, d, l, v.rc, v.coop);
        v.general = d.fast_ok == 2;
        const int nch = (X.rp_active + v.rc - 1) / v.rc;          // (rp_active < RP: re-sweep of a segment whose path stays below that plane, dg_dp_run.hip)
        const dim3 grid((unsigned)((d.nblocks + 3) / 4), (unsigned)nch, (unsigned)(d.k2 + (v.coop ? 4 * d.n_heavy : 0)));
        const dim3 pgrid((unsigned)((d.nblocks + DG_PLAIN_GW - 1) / DG_PLAIN_GW), (unsigned)((nch + DG_PLAIN_CH - 1) / DG_PLAIN_CH), grid.z);
        const int32_t *hv = S.d_heavy.as<int32_t>();
        FastArgs F = X.F;
        F.flip = X.flip;
        const uint4 *rowrec_l = F.rowrec + d.b0;
        const uint2 *slots_l = F.slots + d.slot_first;
        const uint32_t *rowx_l = F.rowx + d.rowx_off;
        const int32_t *cur = (const int32_t *)(F.ring + (size_t)(DG_SLOT(l - 1) ^ X.flip) * F.slot_bytes);
        const int dT = d.delta_off >= 0 ? d.T : 0;
        const uint16_t *dm = dT ? F.delta + d.delta_off - (int64_t)d.in_base * dT : F.delta_zero;   // (F.delta is biased by the resident delta window)
        const int rp_k = S.RP | (d.k << 13);
        unsigned long long hlo = 0, hhi = 0;
        for (int q = 0; q < 4; ++q) { hlo |= (unsigned long long)(uint16_t)d.heavy_in[q] << (16 * q); hhi |= (unsigned long long)(uint16_t)d.heavy_in[4 + q] << (16 * q); }
        auto fast = [&](auto RC, auto DG, auto GEN) { hipLaunchKernelGGL((dp_sweep_fast_kernel<RC.value, DG.value, GEN.value>), pgrid, dim3(DG_PLAIN_WG), 0, s, rowrec_l, slots_l, rowx_l, cur, dm, d.rowx_stride, d.nblocks, rp_k, F.pad_bytes, dT, F.buf_bytes, F, d, l); };
        auto cooperative = [&](auto RC, auto DG, auto GEN) { hipLaunchKernelGGL((dp_sweep_coop_kernel<RC.value, DG.value, GEN.value>), grid, dim3(256), 0, s, rowrec_l, slots_l, rowx_l, cur, d.rowx_stride, d.nblocks, d.n_heavy, rp_k, hlo, hhi, F, d, l, dm, dT, hv); };
        launched = v.coop ? launch_variant<RC_COOP>(v.rc, X.digest, v.general, cooperative) : launch_variant<RC_ANY>(v.rc, X.digest, v.general, fast);
    } else {
        const int nchunk = (S.RP + X.rc_sel - 1) / X.rc_sel;
        const int64_t ntask = (int64_t)d.k2 * d.ngroups * nchunk;
        const unsigned grid = (unsigned)std::min<int64_t>((ntask + 3) / 4, S.opt.max_blocks);
        SweepArgs A = X.A;
        A.flip = X.flip;
        auto generic = [&](auto RC, auto DG, auto) { hipLaunchKernelGGL((dp_sweep_kernel<RC.value, DG.value>), dim3(grid), dim3(256), 0, s, A, l); };
        launched = launch_variant<RC_ALL>(X.rc_sel, X.digest, false, generic);
    }
    if (!launched) { set_error("sweep of level %d: no %s kernel is instantiated for chunks of %d recombination counts", l, v.coop ? "cooperative" : v.rc ? "fast" : "generic", v.rc ? v.rc : X.rc_sel); return DG_ERR_STATE; }
    X.hist.n[(size_t)v.index()]++;
    return DG_OK;
}

// the pair's chunk size by choose_rc's cost model: the wave's chain is the largest composed in-degree -- of a fan-in pair the largest among
// the light rows or a quarter of the largest big row's, plus the LDS merge, and every big row adds four rows of workgroups.  Wide pairs
// take the same model and constants: measured on MHC-24 it puts all but a handful at chunks of 4, the best single setting (DESIGN s3.3).
static int choose_pair_rc(const DpState &S, const PairDesc &p) {
    for (int q = 0; q < N_PAIR_RCS; ++q) if (S.opt.test_force_pair_rc == PAIR_RCS[q]) return q;     // tests: this chunk size for every pair
    for (int q = 0; q < N_PAIR_RCS; ++q) if (p.wide && S.opt.pair_wide_rc == PAIR_RCS[q]) return q;  // measurement: ... for every wide pair
    int best_q = 0;
    double best = 1e300;
    const double rows = (double)p.k2 + 4.0 * p.n_big;
    const double chain = p.n_big ? std::max((double)p.dmax_light, std::ceil(p.dmax / 4.0) + 1.0) : (double)p.dmax;
    for (int q = 0; q < N_PAIR_RCS; ++q) {
        const int rc = PAIR_RCS[q];
        const double W = rows * p.nblocks * ((S.RP + rc - 1) / rc);
        const double T = std::max(1.0, W / (double)S.opt.rc_cap) * ((double)S.opt.rc_t0_ns + chain * rc * (double)S.opt.rc_tg_ps * 1e-3) + W * (double)S.opt.rc_tw_ps * 1e-3;
        if (T <= best) { best = T; best_q = q; }
    }
    return best_q;
}
std::string pair_variant_name(int q) {
    static const char *const kernels[] = {"dp_sweep_pair_kernel<", "dp_sweep_pair_coop_kernel<", "dp_sweep_pair_wide_kernel<", "dp_sweep_pair_coop_wide_kernel<"};
    return std::string(kernels[q / N_PAIR_RCS]) + std::to_string(PAIR_RCS[q % N_PAIR_RCS]) + ">";
}

// f(RC, DIGEST), each a std::integral_constant, for the run-time chunk index q and digest flag
template <int Q = 0, class F>
static void launch_pair_rc(int q, bool digest, F &f) {
    if constexpr (Q < N_PAIR_RCS) {
        if (q != Q) return launch_pair_rc<Q + 1>(q, digest, f);
        constexpr std::integral_constant<int, PAIR_RCS[Q]> RC{};
        if (digest) f(RC, std::true_type{}); else f(RC, std::false_type{});
    }
}

// Levels l - 1 and l in one launch.  Level l - 2 is read from its slot; level l goes into the slot level l - 1 would have taken (the
// two-slot ring cannot take it where level l - 2 lies), which flips the slot parity of every level from here on (SweepLaunch::flip).
int sweep_launch_pair(const DpState &S, SweepLaunch &X, int l, hipStream_t s) {
    const PairDesc &p = S.pairs[(size_t)S.pair_at[l]];
    const LevelDesc &d2 = S.descs[l], &d1 = S.descs[l - 1];
    const FastArgs &F = X.F;
    const int q = choose_pair_rc(S, p), rc = PAIR_RCS[q];
    const int nch = (S.RP + rc - 1) / rc;
    const dim3 grid((unsigned)((p.nblocks + 3) / 4), (unsigned)nch, (unsigned)(p.k2 + 4 * p.n_big));
    const int32_t *cur = (const int32_t *)(F.ring + (size_t)(DG_SLOT(l - 2) ^ X.flip) * F.slot_bytes);
    int32_t *nxt = (int32_t *)(F.ring + (size_t)(DG_SLOT(l - 1) ^ X.flip) * F.slot_bytes + F.pad_bytes);
    const int dT1 = d1.delta_off >= 0 ? d1.T : 0, dT2 = d2.delta_off >= 0 ? d2.T : 0;
    const uint16_t *dm1 = dT1 ? F.delta + d1.delta_off : F.delta_zero, *dm2 = dT2 ? F.delta + d2.delta_off : F.delta_zero;
    const int nt = (int64_t)d2.k2 * d2.k2 * S.RP >= S.opt.bp_nt_min_cells ? 1 : 0;
    const uint2 *prow_l = S.d_prow.as<uint2>() + p.row_first;
    const uint4 *pslots_l = S.d_pslots.as<uint4>() + p.slot_first;
    const int rp_k = S.RP | (p.k0 << 13), kk = p.k1 | (p.k2 << (p.wide ? PairLayout<true>::KK : PairLayout<false>::KK)), nblocks = p.nblocks, n_big = p.n_big, pad_bytes = F.pad_bytes;
    const uint32_t buf_bytes = F.buf_bytes;
    uint16_t *bp1 = F.bp ? F.bp + d1.bp_off : nullptr, *bp2 = F.bp ? F.bp + d2.bp_off : nullptr;
    int *progress = F.progress;
    unsigned long long *digest = F.digest;                              // (passed to the digest form only: the product's kernels take no such argument)
    if (p.n_big == 0) {
        auto light = [&](auto RC, auto DG) {
            if constexpr (DG.value) hipLaunchKernelGGL((dp_sweep_pair_kernel<RC.value, false, unsigned long long *>), grid, dim3(256), 0, s, prow_l, pslots_l, cur, dm1, dm2, nblocks, rp_k, pad_bytes, dT1, dT2, buf_bytes, nxt, bp1, bp2, kk, nt, progress, l, digest);
            else hipLaunchKernelGGL((dp_sweep_pair_kernel<RC.value, false>), grid, dim3(256), 0, s, prow_l, pslots_l, cur, dm1, dm2, nblocks, rp_k, pad_bytes, dT1, dT2, buf_bytes, nxt, bp1, bp2, kk, nt, progress, l);
        };
        auto light_wide = [&](auto RC, auto DG) {
            if constexpr (DG.value) hipLaunchKernelGGL((dp_sweep_pair_kernel<RC.value, true, unsigned long long *>), grid, dim3(256), 0, s, prow_l, pslots_l, cur, dm1, dm2, nblocks, rp_k, pad_bytes, dT1, dT2, buf_bytes, nxt, bp1, bp2, kk, nt, progress, l, digest);
            else hipLaunchKernelGGL((dp_sweep_pair_kernel<RC.value, true>), grid, dim3(256), 0, s, prow_l, pslots_l, cur, dm1, dm2, nblocks, rp_k, pad_bytes, dT1, dT2, buf_bytes, nxt, bp1, bp2, kk, nt, progress, l);
        };
        if (p.wide) launch_pair_rc(q, X.digest, light_wide); else launch_pair_rc(q, X.digest, light);
    } else {
        const uint2 *pbig_l = S.d_pbig.as<uint2>() + (size_t)PAIR_BIG_MAX_INDEG * (size_t)p.big_first;
        const int32_t *big_rows = S.d_pbig_rows.as<int32_t>() + p.big_first;
        unsigned long long big_in = 0;
        if (p.wide) for (int h = 0; h < PAIR_WIDE_BIG_INLINE; ++h) big_in |= (unsigned long long)p.big_in[h] << (16 * h);
        else for (int h = 0; h < PAIR_BIG_INLINE; ++h) big_in |= (unsigned long long)p.big_in[h] << (8 * h);
        auto fanin = [&](auto RC, auto DG) {
            if constexpr (DG.value) hipLaunchKernelGGL((dp_sweep_pair_coop_kernel<RC.value, false, unsigned long long *>), grid, dim3(256), 0, s, prow_l, pslots_l, pbig_l, cur, dm2, big_in, nblocks, n_big, rp_k, dT2, dm1, dT1, pad_bytes, buf_bytes, big_rows, nxt, bp1, bp2, kk, nt, progress, l, digest);
            else hipLaunchKernelGGL((dp_sweep_pair_coop_kernel<RC.value, false>), grid, dim3(256), 0, s, prow_l, pslots_l, pbig_l, cur, dm2, big_in, nblocks, n_big, rp_k, dT2, dm1, dT1, pad_bytes, buf_bytes, big_rows, nxt, bp1, bp2, kk, nt, progress, l);
        };
        auto fanin_wide = [&](auto RC, auto DG) {
            if constexpr (DG.value) hipLaunchKernelGGL((dp_sweep_pair_coop_kernel<RC.value, true, unsigned long long *>), grid, dim3(256), 0, s, prow_l, pslots_l, pbig_l, cur, dm2, big_in, nblocks, n_big, rp_k, dT2, dm1, dT1, pad_bytes, buf_bytes, big_rows, nxt, bp1, bp2, kk, nt, progress, l, digest);
            else hipLaunchKernelGGL((dp_sweep_pair_coop_kernel<RC.value, true>), grid, dim3(256), 0, s, prow_l, pslots_l, pbig_l, cur, dm2, big_in, nblocks, n_big, rp_k, dT2, dm1, dT1, pad_bytes, buf_bytes, big_rows, nxt, bp1, bp2, kk, nt, progress, l);
        };
        if (p.wide) launch_pair_rc(q, X.digest, fanin_wide); else launch_pair_rc(q, X.digest, fanin);
    }
    X.flip ^= 1;
    X.pair_hist.n[q + (p.n_big ? N_PAIR_RCS : 0) + (p.wide ? PAIR_HIST_WIDE : 0)]++;
    return DG_OK;
}

void sweep_warm_tables(const DpState &S, const SweepLaunch &X, int q0, int q1, hipStream_t s) {   // graph tables of destination levels [q0, q1) -> Infinity Cache
    const LevelDesc &da = S.descs[q0], &db = S.descs[q1 - 1];
    const FastArgs &F = X.F;
    WarmRanges W{};
    auto put = [&](int q, const void *base, int64_t b0, int64_t b1) {       // byte range [b0, b1) behind base
        const uintptr_t a = ((uintptr_t)base + (uintptr_t)b0) & ~(uintptr_t)15, e = ((uintptr_t)base + (uintptr_t)b1) & ~(uintptr_t)15;
        W.p[q] = (const char *)a; W.n16[q] = e > a ? (long long)((e - a) >> 4) : 0;
    };
    put(0, F.rowrec, 16 * (int64_t)da.b0, 16 * ((int64_t)db.b0 + db.k2));
    put(1, F.slots, 8 * da.slot_first, 8 * (db.slot_first + (int64_t)db.nblocks * 64));
    put(2, F.in_edge, 4 * (int64_t)da.in_base, 4 * ((int64_t)db.in_base + db.T));
    int64_t d0 = -1, d1 = -1, x0 = -1, x1 = -1;
    for (int q = q0; q < q1; ++q) {
        const LevelDesc &dq = S.descs[q];
        if (dq.rowx_stride > 0) {                                           // (matrices are laid out in level order)
            if (x0 < 0) x0 = dq.rowx_off;
            x1 = dq.rowx_off + (int64_t)dq.k2 * dq.rowx_stride;
        }
        if (dq.delta_off < 0 || S.level_win[q] != S.cur_win) continue;
        const int64_t e = dq.delta_off + (int64_t)dq.T * dq.T;
        d0 = d0 < 0 ? dq.delta_off : std::min(d0, dq.delta_off);
        d1 = std::max(d1, e);
    }
    if (d0 >= 0) put(3, F.delta, 2 * d0, 2 * d1);
    if (x0 >= 0) put(4, F.rowx, 4 * x0, 4 * x1);
    long long tot = 0;
    for (int q = 0; q < WARM_RANGES; ++q) tot += W.n16[q];
    if (tot <= 0) return;
    const unsigned grid = (unsigned)std::min<long long>((tot + 255) / 256, 2048);
    hipLaunchKernelGGL(dp_warm_tables_kernel, dim3(grid), dim3(256), 0, s, W);
}

// L2 prefetcher of the sweep range [lb, le): control words set in stream order on s, the prefetcher itself on the side stream
int sweep_prefetch_begin(DpState &S, const SweepLaunch &X, int lb, int le, bool delta_resident, hipStream_t s) {
    S.pf_active = false;
    if (S.opt.l2_prefetch <= 0 || !X.small_state || !S.opt.use_fast || le - lb < 64) return DG_OK;
    if (!S.pf_stream && hipStreamCreateWithFlags(&S.pf_stream, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); S.pf_stream = nullptr; S.opt.l2_prefetch = 0; return DG_OK; }
    if (!S.pf_ev && hipEventCreateWithFlags(&S.pf_ev, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); S.pf_ev = nullptr; S.opt.l2_prefetch = 0; return DG_OK; }
    // One DP state per DEVICE (option side_stream: -1 = this rule, 0 / 1 = the caller decides): a second instance's sweep could share a
    // hardware queue with THIS state's prefetcher and would then wait behind it for a whole range (three concurrent instances on
    // one GPU: 78 -> 52 G cells/s before this rule).
    if (!S.side_stream_ok()) return DG_OK;
    if (!S.pf_tested) {
        S.pf_tested = 1;
        DG_HIP(hipStreamSynchronize(s));
        hipLaunchKernelGGL(dp_pf_probe_wait_kernel, dim3(1), dim3(1), 0, S.pf_stream, S.d_pfctl.as<PfCtl>(), 0x5EED);
        hipLaunchKernelGGL(dp_pf_probe_set_kernel, dim3(1), dim3(1), 0, s, S.d_pfctl.as<PfCtl>(), 0x5EED);
        PfCtl h;
        if (hipStreamSynchronize(S.pf_stream) != hipSuccess || hipStreamSynchronize(s) != hipSuccess ||
            hipMemcpy(&h, S.d_pfctl.p, sizeof h, hipMemcpyDeviceToHost) != hipSuccess || !h.probe_ok) {
            (void)hipGetLastError();
            if (getenv("DG_DEBUG")) fprintf(stderr, "[dipgenie_hip] L2 prefetcher off: its stream does not run beside the sweep's\n");
            S.opt.l2_prefetch = 0;
            return DG_OK;
        }
    }
    const int seq = ++S.pf_seq;
    hipLaunchKernelGGL(dp_pf_ctl_kernel, dim3(1), dim3(1), 0, s, S.d_pfctl.as<PfCtl>(), seq, lb - 1, 0);
    DG_HIP(hipEventRecord(S.pf_ev, s));
    DG_HIP(hipStreamWaitEvent(S.pf_stream, S.pf_ev, 0));
    const int far = (int)S.opt.pf_far;
    hipLaunchKernelGGL(dp_l2_prefetch_kernel, dim3(PF_WORKGROUPS + (far > 0 ? PF_FAR_WORKGROUPS : 0)), dim3(64), 0, S.pf_stream, S.d_descs.as<LevelDesc>(), X.F,
                       S.d_pfctl.as<PfCtl>(), seq, lb, le, (int)S.opt.l2_prefetch, delta_resident ? 1 : 0, far,
                       X.pairs_ok ? S.d_pair_at.as<int32_t>() : (const int32_t *)nullptr, S.d_pairs.as<PairDesc>(), S.d_prow.as<uint2>(), S.d_pslots.as<uint4>(), S.d_pbig.as<uint2>());
    S.pf_active = true;
    return DG_OK;
}
void sweep_prefetch_end(DpState &S, int le, hipStream_t s) {
    if (S.pf_stream && S.opt.l2_prefetch > 0) hipLaunchKernelGGL(dp_pf_ctl_kernel, dim3(1), dim3(1), 0, s, S.d_pfctl.as<PfCtl>(), S.pf_seq, le, 1);
}
void sweep_prefetch_free(DpState &S) {
    if (S.pf_stream) { (void)hipStreamSynchronize(S.pf_stream); (void)hipStreamDestroy(S.pf_stream); S.pf_stream = nullptr; }
    if (S.pf_ev) { (void)hipEventDestroy(S.pf_ev); S.pf_ev = nullptr; }
}

}  // namespace dgi

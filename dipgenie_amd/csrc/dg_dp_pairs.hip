// Level pairs of the diploid DP sweep: which adjacent levels run as ONE composed launch, and the tables of those launches.
//
// A level costs about as much in kernel boundary as in work, so two adjacent levels (l - 1, l) whose vertices
// have few in-edges are composed at load time into one transition from level l - 2: a cell (i2, j2, r2) of level l takes the
// maximum over composed row in-edges (eu2, eu1) and composed column in-edges (ev2, ev1) of
//     state[l - 2][src(eu1)][src(ev1)][r2 - w] + delta_{l-1}(eu1, ev1) + delta_l(eu2, ev2),     w = the four weight bits.
// That is exact: the maximum over the middle cell's candidates distributes over the sum, and the reference's tie order -- level
// l by (ru2 asc, rv2 asc), then inside the winning middle cell by (ru1 asc, rv1 asc) -- is the lexicographic order of the word
// (255 - ru2) << 24 | (255 - rv2) << 16 | (255 - ru1) << 8 | (255 - rv1) that the kernel maximises beside the value.
//
//   composed row records   PAIR_MAX_INDEG per vertex of level l, uint2:
//                          x = source position | w1u << 15 | middle position << 16 | w2u << 24 | composed in-degree << 25
//                          y = delta row of level l | delta row of level l - 1 << 11 | ru2 << 22 | ru1 << 25
//   composed slot records  64 per block (a run of whole destination columns), uint4, all ones in x = padding:
//                          x = source position | w1v << 15 | middle position << 16 | w2v << 24
//                          y = delta column of level l | delta column of level l - 1 << 16
//                          z = rv2 | rv1 << 8 | steps of the segmented max << 16 | destination column << 20
//
// Eligible: both levels on the lean fast form without a dead column, both narrower than 256, at most 2,047 in-edges each, every
// vertex of level l with a composed in-degree of at most PAIR_MAX_INDEG, score deltas resident in one window.  Pairs are chosen
// greedily left to right and are disjoint.  Built on the host from the in-CSR that the loader has just put on the device (read back:
// two copies), so the in-edge order is the loader's by construction.
#include <algorithm>
#include <cstdlib>

#include "dg_dp.hpp"

namespace dgi {

int dp_build_pairs(dg_ctx *c, const dg_dp_graph *g, DpState &S) {
    S.pairs.clear(); S.pair_at.clear();
    S.d_pairs.release(); S.d_pair_at.release(); S.d_prow.release(); S.d_pslots.release();
    const int L = S.L, nV = S.nV;
    // a graph of L levels holds at most (L - 1) / 2 pairs: below pair_min nothing is even indexed
    if (!S.opt.pair_levels || (int64_t)(L - 1) / 2 < std::max<int64_t>(S.opt.pair_min, 1) || (int)S.dwin_t.size() != 2 || S.RP > 0x1FFF) return DG_OK;
    const double t0 = wall_s();
    // the loader's in-CSR (in-edges of every vertex by source position, then adjacency order; word = position | weight << 31)
    std::vector<uint32_t> in_off((size_t)nV + 1, 0), in_edge((size_t)g->out_off[nV]);
    DG_HIP(hipMemcpyAsync(in_off.data(), S.d_in_off.p, 4 * in_off.size(), hipMemcpyDeviceToHost, c->stream));
    if (!in_edge.empty()) DG_HIP(hipMemcpyAsync(in_edge.data(), S.d_in_edge.p, 4 * in_edge.size(), hipMemcpyDeviceToHost, c->stream));
    DG_HIP(hipStreamSynchronize(c->stream));
    auto indeg = [&](int v) { return (int)(in_off[v + 1] - in_off[v]); };
    auto level_ok = [&](int l) {
        const LevelDesc &d = S.descs[l];
        return d.fast_ok == 1 && d.ndead == 0 && d.k2 <= PAIR_MAX_WIDTH && d.T <= PAIR_MAX_T && !d.bp_wide;
    };
    auto composed = [&](int v, int a0m) {                              // composed in-degree of vertex v of the later level
        int n = 0;
        for (uint32_t e = in_off[v]; e < in_off[v + 1]; ++e) n += indeg(a0m + (int)(in_edge[e] & 0x7FFFu));
        return n;
    };
    std::vector<int32_t> at((size_t)L, -1);
    std::vector<PairDesc> pairs;
    for (int l = 2; l < L; ++l) {
        if (!level_ok(l - 1) || !level_ok(l)) continue;
        const LevelDesc &d = S.descs[l];
        bool ok = true;
        int dmax = 0;
        for (int v = d.b0; v < d.b0 + d.k2 && ok; ++v) { const int n = composed(v, d.a0); dmax = std::max(dmax, n); ok = n >= 1 && n <= PAIR_MAX_INDEG; }
        if (!ok) continue;
        PairDesc p{};
        p.l = l; p.k0 = S.descs[l - 1].k; p.k1 = d.k; p.k2 = d.k2; p.dmax = dmax;
        at[l] = (int32_t)pairs.size(); at[l - 1] = -2;
        pairs.push_back(p);
        ++l;                                                            // disjoint: the next pair starts after this one
    }
    if ((int64_t)pairs.size() < std::max<int64_t>(S.opt.pair_min, 1)) return DG_OK;
    std::vector<uint32_t> prow, pslots;
    std::vector<uint32_t> col;                                          // slot records of one destination column
    for (PairDesc &p : pairs) {
        const LevelDesc &d2 = S.descs[p.l], &d1 = S.descs[p.l - 1];
        p.row_first = (int64_t)(prow.size() / 2);
        p.slot_first = (int64_t)(pslots.size() / 4);
        size_t blk0 = pslots.size();                                    // start of the open block
        uint32_t used = 0, maxdv = 1;
        auto close_block = [&]() {
            if (used == 0) return;
            uint32_t steps = 0;
            while ((1u << steps) < maxdv) ++steps;
            for (uint32_t q = used; q < 64; ++q) { pslots.push_back(0xFFFFFFFFu); pslots.push_back(0); pslots.push_back(0); pslots.push_back(0); }
            for (uint32_t q = 0; q < 64; ++q) pslots[blk0 + 4 * q + 2] |= steps << 16;
            blk0 = pslots.size(); used = 0; maxdv = 1;
        };
        for (int c2 = 0; c2 < d2.k2; ++c2) {
            const int v = d2.b0 + c2;
            const uint32_t n = (uint32_t)composed(v, d2.a0);
            uint32_t t = 0;
            col.clear();
            for (uint32_t e2 = in_off[v]; e2 < in_off[v + 1]; ++e2) {
                const uint32_t m = in_edge[e2] & 0x7FFFu, w2 = in_edge[e2] >> 31, r2 = e2 - in_off[v];
                const int mv = d2.a0 + (int)m;
                for (uint32_t e1 = in_off[mv]; e1 < in_off[mv + 1]; ++e1, ++t) {
                    const uint32_t src = in_edge[e1] & 0x7FFFu, w1 = in_edge[e1] >> 31, r1 = e1 - in_off[mv];
                    const uint32_t i2 = e2 - d2.in_base, i1 = e1 - d1.in_base;          // delta row / column of either level
                    prow.push_back(src | (w1 << 15) | (m << 16) | (w2 << 24) | (n << 25));
                    prow.push_back(i2 | (i1 << 11) | (r2 << 22) | (r1 << 25));
                    col.push_back(src | (w1 << 15) | (m << 16) | (w2 << 24));
                    col.push_back(i2 | (i1 << 16));
                    col.push_back(r2 | (r1 << 8) | ((uint32_t)c2 << 20));
                    col.push_back(0);
                }
            }
            for (; t < (uint32_t)PAIR_MAX_INDEG; ++t) { prow.push_back(n << 25); prow.push_back(0); }
            if (used + n > 64) close_block();
            pslots.insert(pslots.end(), col.begin(), col.end());
            used += n; maxdv = std::max(maxdv, n);
        }
        close_block();
        p.nblocks = (int32_t)((int64_t)(pslots.size() / 4) - p.slot_first) / 64;
    }
    auto up = [&](DevBuf &b, const void *src, size_t bytes) -> int {
        if (int rc = b.ensure(bytes + 16)) return rc;
        DG_HIP(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, c->stream));
        return DG_OK;
    };
    if (int rc = up(S.d_pairs, pairs.data(), sizeof(PairDesc) * pairs.size())) return rc;
    if (int rc = up(S.d_pair_at, at.data(), 4 * at.size())) return rc;
    if (int rc = up(S.d_prow, prow.data(), 4 * prow.size())) return rc;
    if (int rc = up(S.d_pslots, pslots.data(), 4 * pslots.size())) return rc;
    DG_HIP(hipStreamSynchronize(c->stream));                            // the staging vectors die here
    if (getenv("DG_DEBUG"))
        fprintf(stderr, "[dipgenie_hip] load: %zu level pairs (%.1f %% of the launches), composed tables %.1f MB, built in %.3f s\n", pairs.size(),
                100.0 * (double)pairs.size() / std::max(1, L - 1), 4e-6 * (double)(prow.size() + pslots.size()), wall_s() - t0);
    S.pairs.swap(pairs); S.pair_at.swap(at);
    return DG_OK;
}

}  // namespace dgi

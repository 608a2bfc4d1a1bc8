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
//                          (a big row: composed in-degree PAIR_ROW_BIG, nothing else)
//   big row records        PAIR_BIG_MAX_INDEG per big row (composed in-degree 9..32), in the order of the pair's big-row list, uint2:
//                          x as above (the composed in-degree takes 6 bits),  y = ... | ru2 << 22 | ru1 << 27 (5-bit ranks)
//   composed slot records  64 per block (a run of whole destination columns), uint4, all ones in x = padding:
//                          x = source position | w1v << 15 | middle position << 16 | w2v << 24
//                          y = delta column of level l | delta column of level l - 1 << 16
//                          z = rv2 | rv1 << 8 | steps of the segmented max << 16 | destination column << 20
//
// Wide pairs (PairLayout<true> in dg_dp.hpp): the same records with 10-bit positions -- x = source | w1 << 10 | middle << 11 | w2 << 21 |
// composed in-degree << 22, the destination column of slot z 10 bits wide -- for pairs in which one of the three levels holds 256..1,023
// vertices; the first PAIR_WIDE_BIG_INLINE big rows ride in the kernel arguments, 16 bits each.
//
// Eligible: both levels on the lean fast form without a dead column, at most 2,047 in-edges each, every vertex of level l with a
// composed in-degree of at most PAIR_MAX_INDEG, score deltas resident in one window.  Pairs are chosen greedily left to right and
// are disjoint.  The widths, by rule:
//   narrow rule   levels l - 1 and l at most PAIR_MAX_WIDTH (255) wide; the source level l - 2 up to 32,767 (15-bit source positions);
//   wide rule     (options pair_wide, pair_wide_min, pair_wide_fanin) levels l - 1 and l at most PAIR_WIDE_MAX_WIDTH (1,023) wide.  A pair
//                 takes the wide layout exactly when one of its three levels exceeds 255, and then the source level too is at most
//                 1,023 wide -- except that a source beyond 1,023 over two narrow levels keeps the narrow layout.
// Fan-in pairs (options pair_fanin, pair_fanin_min): either rule with a composed in-degree of at most PAIR_BIG_MAX_INDEG, the vertices
// above PAIR_MAX_INDEG listed as the pair's big rows.  The greedy choice under a wider rule pairs other levels than the one under a
// narrower rule, so a wider choice is taken as a whole: with big rows only where it holds at least pair_fanin_min pairs with a big
// row, with wide levels only where it holds at least pair_wide_min pairs in the wide layout.  On every other graph the pairs are
// those of the narrow rule without big rows.
// Built on the host from the in-CSR that the loader has just put on the device (read back: two copies), so the in-edge order is the
// loader's by construction; the tables are filled by up to 16 threads.
#include <sched.h>

#include <algorithm>
#include <cstdlib>
#include <memory>

#include "dg_dp.hpp"

namespace dgi {

// CPUs this process may use: its affinity mask and its cgroup's quota, not the machine's core count
static int cpu_share() {
    int64_t n = (int64_t)std::max(1u, std::thread::hardware_concurrency());
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof set, &set) == 0) n = std::min<int64_t>(n, std::max(1, CPU_COUNT(&set)));
    if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
        long long quota = 0, period = 0;
        if (fscanf(f, "%lld %lld", &quota, &period) == 2 && quota > 0 && period > 0) n = std::min<int64_t>(n, (quota + period - 1) / period);   // ("max": no quota)
        fclose(f);
    }
    return (int)std::max<int64_t>(n, 1);
}

// f(b0, b1) over [0, n) in blocks that nt threads (this one among them) take from a counter
template <class F>
static void parallel_blocks(int64_t n, int64_t block, int nt, F f) {
    std::atomic<int64_t> next{0};
    auto work = [&]() {
        for (;;) {
            const int64_t b = next.fetch_add(block);
            if (b >= n) return;
            f(b, std::min(n, b + block));
        }
    };
    std::vector<std::thread> th;
    for (int t = 1; t < nt && (int64_t)t * block < n; ++t) th.emplace_back(work);
    work();
    for (std::thread &t : th) t.join();
}

int dp_build_pairs(dg_ctx *c, const dg_dp_graph *g, DpState &S) {
    S.pairs.clear(); S.pair_at.clear();
    S.d_pairs.release(); S.d_pair_at.release(); S.d_prow.release(); S.d_pslots.release(); S.d_pbig.release(); S.d_pbig_rows.release();
    const int L = S.L, nV = S.nV;
    // a graph of L levels holds at most (L - 1) / 2 pairs: below pair_min nothing is even indexed
    if (!S.opt.pair_levels || (int64_t)(L - 1) / 2 < std::max<int64_t>(S.opt.pair_min, 1) || (int)S.dwin_t.size() != 2 || S.RP > 0x1FFF) return DG_OK;
    const double t0 = wall_s();
    // the loader's in-CSR (in-edges of every vertex by source position, then adjacency order; word = position | weight << 31)
    std::vector<uint32_t> in_off((size_t)nV + 1, 0), in_edge((size_t)g->out_off[nV]);
    DG_HIP(hipMemcpyAsync(in_off.data(), S.d_in_off.p, 4 * in_off.size(), hipMemcpyDeviceToHost, c->stream));
    if (!in_edge.empty()) DG_HIP(hipMemcpyAsync(in_edge.data(), S.d_in_edge.p, 4 * in_edge.size(), hipMemcpyDeviceToHost, c->stream));
    DG_HIP(hipStreamSynchronize(c->stream));
    const int nt = (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)16, S.opt.host_threads, (int64_t)cpu_share()}));
    auto indeg = [&](int v) { return (int)(in_off[v + 1] - in_off[v]); };
    // the widest level any rule in use takes: the wide form's cap when it is on (its own rule below decides per pair)
    const int wide_cap = (int)std::min<int64_t>(S.opt.pair_wide_max_width, PAIR_WIDE_MAX_WIDTH), any_cap = S.opt.pair_wide ? std::max(wide_cap, PAIR_MAX_WIDTH) : PAIR_MAX_WIDTH;
    auto level_ok = [&](int l) {
        const LevelDesc &d = S.descs[l];
        return d.fast_ok == 1 && d.ndead == 0 && d.k2 <= any_cap && d.T <= PAIR_MAX_T && !d.bp_wide;
    };
    // composed in-degree of every vertex of a level l that could be the later level of a pair (lean levels: at most 64 * 64), and per level
    // what the choice needs: smallest, largest, largest among the light rows, rows above PAIR_MAX_INDEG; cmin = 0: not eligible
    struct LevelSum { int32_t cmin, cmax, cmax_light, n_big; };
    std::vector<uint16_t> comp((size_t)nV, 0);
    std::vector<LevelSum> sum((size_t)L, LevelSum{0, 0, 0, 0});
    parallel_blocks(std::max(L - 2, 0), 512, nt, [&](int64_t q0, int64_t q1) {
        for (int l = (int)q0 + 2; l < (int)q1 + 2; ++l) {
            if (!level_ok(l - 1) || !level_ok(l)) continue;
            const LevelDesc &d = S.descs[l];
            LevelSum s{1 << 30, 0, 0, 0};
            for (int v = d.b0; v < d.b0 + d.k2; ++v) {
                int n = 0;
                for (uint32_t e = in_off[v]; e < in_off[v + 1]; ++e) n += indeg(d.a0 + (int)(in_edge[e] & 0x7FFFu));
                comp[(size_t)v] = (uint16_t)n;
                s.cmin = std::min(s.cmin, n); s.cmax = std::max(s.cmax, n);
                if (n > PAIR_MAX_INDEG) ++s.n_big; else s.cmax_light = std::max(s.cmax_light, n);
            }
            sum[(size_t)l] = s;
        }
    });
    const int max_big = (int)std::min<int64_t>(S.opt.pair_fanin_max_big, PAIR_MAX_WIDTH), max_indeg = (int)std::min<int64_t>(S.opt.pair_fanin_max_indeg, PAIR_BIG_MAX_INDEG);
    // greedy from the left, disjoint; fanin: big rows allowed; wide: levels up to wide_cap allowed.  A pair takes the wide layout exactly
    // when one of its three levels exceeds PAIR_MAX_WIDTH -- but a source beyond wide_cap over two narrow levels keeps the narrow one, whose
    // source positions have 15 bits.  Returns the number of pairs that have a big row; n_wide: of those in the wide layout.
    auto choose = [&](bool fanin, bool wide, std::vector<PairDesc> &pairs, std::vector<int32_t> &at, int64_t &n_wide) {
        int64_t n_fanin = 0;
        n_wide = 0;
        pairs.clear(); at.assign((size_t)L, -1);
        for (int l = 2; l < L; ++l) {
            const LevelSum &s = sum[(size_t)l];
            if (s.cmin < 1) continue;
            const LevelDesc &d = S.descs[l];
            const int k0 = S.descs[l - 1].k;
            const bool wide_level = d.k > PAIR_MAX_WIDTH || d.k2 > PAIR_MAX_WIDTH, wide_layout = wide_level || (wide && k0 > PAIR_MAX_WIDTH && k0 <= wide_cap);
            if (wide_level && !(wide && k0 <= wide_cap && d.k <= wide_cap && d.k2 <= wide_cap)) continue;
            if (s.cmax > PAIR_MAX_INDEG && !(fanin && s.cmax <= max_indeg && s.n_big <= max_big && !(wide_layout && !S.opt.pair_wide_fanin))) continue;
            PairDesc p{};
            p.l = l; p.k0 = k0; p.k1 = d.k; p.k2 = d.k2; p.dmax = s.cmax; p.n_big = s.n_big; p.dmax_light = s.cmax_light; p.wide = wide_layout;
            n_fanin += s.n_big > 0; n_wide += wide_layout;
            at[(size_t)l] = (int32_t)pairs.size(); at[(size_t)l - 1] = -2;
            pairs.push_back(p);
            ++l;                                                        // disjoint: the next pair starts after this one
        }
        return n_fanin;
    };
    std::vector<int32_t> at;
    std::vector<PairDesc> pairs;
    // the rule's choice with or without wide levels: the fan-in choice as a whole where it holds enough pairs with a big row, else the light one
    int64_t n_fanin = 0, n_wide = 0;
    auto choose_fanin = [&](bool wide, std::vector<PairDesc> &pairs, std::vector<int32_t> &at, int64_t &n_fanin, int64_t &n_wide) {
        n_fanin = choose(false, wide, pairs, at, n_wide);
        if (!S.opt.pair_fanin) return;
        std::vector<int32_t> at_f;
        std::vector<PairDesc> pairs_f;
        int64_t nw = 0;
        const int64_t nf = choose(true, wide, pairs_f, at_f, nw);
        if (nf >= std::max<int64_t>(S.opt.pair_fanin_min, 1)) { pairs.swap(pairs_f); at.swap(at_f); n_fanin = nf; n_wide = nw; }
    };
    choose_fanin(false, pairs, at, n_fanin, n_wide);
    // wide pairs take levels the choice above pairs otherwise: the wider choice as a whole, where it holds enough pairs in the wide layout
    if (S.opt.pair_wide) {
        std::vector<int32_t> at_w;
        std::vector<PairDesc> pairs_w;
        int64_t nf = 0, nw = 0;
        choose_fanin(true, pairs_w, at_w, nf, nw);
        if (nw >= std::max<int64_t>(S.opt.pair_wide_min, 1)) { pairs.swap(pairs_w); at.swap(at_w); n_fanin = nf; n_wide = nw; }
    }
    if ((int64_t)pairs.size() < std::max<int64_t>(S.opt.pair_min, 1)) return DG_OK;
    // slot blocks of every pair (a column never straddles a block), then the pairs' places in the tables
    const int64_t NP = (int64_t)pairs.size();
    parallel_blocks(NP, 256, nt, [&](int64_t q0, int64_t q1) {
        for (int64_t q = q0; q < q1; ++q) {
            PairDesc &p = pairs[(size_t)q];
            const LevelDesc &d2 = S.descs[p.l];
            uint32_t used = 0;
            int32_t nb = 1;
            for (int v = d2.b0; v < d2.b0 + d2.k2; ++v) {
                const uint32_t n = comp[(size_t)v];
                if (used + n > 64) { ++nb; used = 0; }
                used += n;
            }
            p.nblocks = nb;
        }
    });
    int64_t n_rows = 0, n_blocks = 0, n_big = 0;
    for (PairDesc &p : pairs) {
        p.row_first = n_rows * PAIR_MAX_INDEG; p.slot_first = n_blocks * 64; p.big_first = n_big;
        n_rows += p.k2; n_blocks += p.nblocks; n_big += p.n_big;
    }
    const size_t prow_words = 2 * (size_t)PAIR_MAX_INDEG * (size_t)n_rows, pslot_words = 4 * 64 * (size_t)n_blocks, pbig_words = 2 * (size_t)PAIR_BIG_MAX_INDEG * (size_t)n_big;
    // (not value-initialised: the threads below write every word)
    std::unique_ptr<uint32_t[]> prow(new uint32_t[prow_words + 1]), pslots(new uint32_t[pslot_words + 1]), pbig(new uint32_t[pbig_words + 1]);
    std::unique_ptr<int32_t[]> big_rows(new int32_t[(size_t)n_big + 1]);
    parallel_blocks(NP, 64, nt, [&](int64_t q0, int64_t q1) {
        for (int64_t q = q0; q < q1; ++q) {
            PairDesc &p = pairs[(size_t)q];
            const LevelDesc &d2 = S.descs[p.l], &d1 = S.descs[p.l - 1];
            uint32_t *const pr = prow.get() + 2 * p.row_first, *const pb = pbig.get() + 2 * (size_t)PAIR_BIG_MAX_INDEG * (size_t)p.big_first;
            uint32_t *blk = pslots.get() + 4 * p.slot_first;                // the open block
            int32_t *const br = big_rows.get() + p.big_first;
            uint32_t used = 0, maxdv = 1, h = 0;
            typedef PairLayout<false> Y0;
            typedef PairLayout<true> Y1;
            const uint32_t W1 = p.wide ? Y1::W1 : Y0::W1, MID = p.wide ? Y1::MID : Y0::MID, W2 = p.wide ? Y1::W2 : Y0::W2, DEG = p.wide ? Y1::DEG : Y0::DEG;
            auto close_block = [&]() {
                uint32_t steps = 0;
                while ((1u << steps) < maxdv) ++steps;
                for (uint32_t s = used; s < 64; ++s) { blk[4 * s] = 0xFFFFFFFFu; blk[4 * s + 1] = 0; blk[4 * s + 2] = 0; blk[4 * s + 3] = 0; }
                for (uint32_t s = 0; s < 64; ++s) blk[4 * s + 2] |= steps << 16;
                blk += 4 * 64; used = 0; maxdv = 1;
            };
            for (int c2 = 0; c2 < d2.k2; ++c2) {
                const int v = d2.b0 + c2;
                const uint32_t n = comp[(size_t)v];
                const bool big = n > (uint32_t)PAIR_MAX_INDEG;
                if (used + n > 64) close_block();
                uint32_t *const light = pr + 2 * (size_t)PAIR_MAX_INDEG * (size_t)c2;
                uint32_t *const rec = big ? pb + 2 * (size_t)PAIR_BIG_MAX_INDEG * h : light;
                const uint32_t cap = big ? PAIR_BIG_MAX_INDEG : PAIR_MAX_INDEG, ru1_shift = big ? 27 : 25;
                uint32_t t = 0;
                for (uint32_t e2 = in_off[v]; e2 < in_off[v + 1]; ++e2) {
                    const uint32_t m = in_edge[e2] & 0x7FFFu, w2 = in_edge[e2] >> 31, r2 = e2 - in_off[v];
                    const int mv = d2.a0 + (int)m;
                    for (uint32_t e1 = in_off[mv]; e1 < in_off[mv + 1]; ++e1, ++t) {
                        const uint32_t src = in_edge[e1] & 0x7FFFu, w1 = in_edge[e1] >> 31, r1 = e1 - in_off[mv];
                        const uint32_t i2 = e2 - d2.in_base, i1 = e1 - d1.in_base;          // delta row / column of either level
                        rec[2 * t] = src | (w1 << W1) | (m << MID) | (w2 << W2) | (n << DEG);
                        rec[2 * t + 1] = i2 | (i1 << 11) | (r2 << 22) | (r1 << ru1_shift);
                        uint32_t *const sl = blk + 4 * (used + t);
                        sl[0] = src | (w1 << W1) | (m << MID) | (w2 << W2);
                        sl[1] = i2 | (i1 << 16);
                        sl[2] = r2 | (r1 << 8) | ((uint32_t)c2 << 20);
                        sl[3] = 0;
                    }
                }
                for (; t < cap; ++t) { rec[2 * t] = n << DEG; rec[2 * t + 1] = 0; }
                if (big) {
                    for (t = 0; t < (uint32_t)PAIR_MAX_INDEG; ++t) { light[2 * t] = PAIR_ROW_BIG << DEG; light[2 * t + 1] = 0; }
                    br[h] = c2;
                    if (h < (uint32_t)PAIR_BIG_INLINE) p.big_in[h] = (uint16_t)c2;
                    ++h;
                }
                used += n; maxdv = std::max(maxdv, n);
            }
            close_block();
        }
    });
    auto up = [&](DevBuf &b, const void *src, size_t bytes) -> int {
        if (int rc = b.ensure(bytes + 16)) return rc;
        if (bytes) DG_HIP(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, c->stream));
        return DG_OK;
    };
    if (int rc = up(S.d_pairs, pairs.data(), sizeof(PairDesc) * pairs.size())) return rc;
    if (int rc = up(S.d_pair_at, at.data(), 4 * at.size())) return rc;
    if (int rc = up(S.d_prow, prow.get(), 4 * prow_words)) return rc;
    if (int rc = up(S.d_pslots, pslots.get(), 4 * pslot_words)) return rc;
    if (int rc = up(S.d_pbig, pbig.get(), 4 * pbig_words)) return rc;
    if (int rc = up(S.d_pbig_rows, big_rows.get(), 4 * (size_t)n_big)) return rc;
    DG_HIP(hipStreamSynchronize(c->stream));                            // the staging buffers die here
    if (getenv("DG_DEBUG"))
        fprintf(stderr, "[dipgenie_hip] load: %zu level pairs (%.1f %% of the launches), %lld of them with big rows (%lld big rows), %lld in the wide layout, composed tables %.1f MB, built in %.3f s by %d threads\n",
                pairs.size(), 100.0 * (double)pairs.size() / std::max(1, L - 1), (long long)n_fanin, (long long)n_big, (long long)n_wide, 4e-6 * (double)(prow_words + pslot_words + pbig_words), wall_s() - t0, nt);
    S.pairs.swap(pairs); S.pair_at.swap(at);
    return DG_OK;
}

}  // namespace dgi

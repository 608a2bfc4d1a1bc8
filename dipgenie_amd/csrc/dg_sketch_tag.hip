// libdipgenie_hip.so -- read tagging: every read's distinct minimizer hashes joined against two hash lists (gfx950).
//
// dg_sketch_tag_reads answers, per read, how many of its distinct minimizer hashes S lie only in A, only in B, or in both
// (dg_read_tag, include/dipgenie_hip.h).  The minimizers come from the tile kernel of dg_sketch.hip (sparse form, every
// emission, compacted: a read's emissions are contiguous, from the base of its first tile to the base of the tile after its
// last).  Three steps:
//   dictionary   A and B with labels 1 / 2 -> radix sort by hash + reduce-by-key (OR of the labels: 3 = both), rocPRIM; the
//                distinct hashes go into an open-addressed table in device memory: power-of-two capacity >= 2 x distinct, slot =
//                low bits of the hash, linear probing.  A slot is occupied iff its LABEL is non-zero, so every 64-bit key is legal.
//   first route  one wave per read, lanes take emissions.  A per-wave LDS set of emission indices (slot holds index + 1, 0 =
//                empty, claimed with a CAS; equality is decided on the hash the index points to) keeps one of equal hashes; every
//                kept emission probes the table; the four counts are ballots, lane 0 writes the 16-byte record with one store.
//   second route a read with more emissions than the LDS set takes (tag_lds_entries) is appended to a list instead; those reads'
//                segments are sorted (rocPRIM segmented radix sort into d_hash2) and the same probe-and-count runs on the sorted run,
//                an entry counting iff it differs from its predecessor.
// LDS: TAG_LDS_DEFAULT = 1024 emissions -> 2048 slots x 4 B = 8 KB per wave, 32 KB per 256-thread workgroup (5 workgroups per CU of 160 KB).
#include <algorithm>
#include <cstring>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "dg_sketch.hpp"

namespace dgi {

constexpr int TAG_LDS_DEFAULT = 1024;   // emissions of one read on the first route (the LDS set holds twice as many slots)
constexpr int TAG_MIN_SLOTS = 64;
#define TAG_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)

struct TagTable { const uint64_t *key; const uint32_t *lab; uint64_t mask; };      // slots = mask + 1; lab 0 = empty, 1 only A, 2 only B, 3 both
struct TagLong { uint32_t *n; int64_t *read; uint32_t *beg, *end; uint32_t cap; }; // reads of the second route: read id, its segment of the emissions

struct LabelOr { __host__ __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a | b; } };

__global__ void tag_fill_labels_kernel(uint32_t *__restrict__ lab, int64_t n_a, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) lab[i] = i < n_a ? 1u : 2u;
}

// one thread per distinct hash: claims the first empty slot from its home slot on (the label is the occupancy), then writes the key.
// The table is read by later kernels only.
__global__ void tag_table_insert_kernel(const uint64_t *__restrict__ ukey, const uint32_t *__restrict__ ulab, int64_t n, uint64_t *__restrict__ tkey,
                                        uint32_t *__restrict__ tlab, uint64_t mask) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t key = ukey[i];
    const uint32_t lab = ulab[i];                                      // 1 .. 3
    for (uint64_t s = key & mask;; s = (s + 1) & mask)                 // (ends: the table has more slots than keys)
        if (atomicCAS(&tlab[s], 0u, lab) == 0u) { tkey[s] = key; return; }
}

// label of key H: 0 = in neither list.  Ends at the first empty slot (the host keeps at least one).
__device__ __forceinline__ uint32_t tag_probe(const TagTable &tb, uint64_t H) {
    for (uint64_t s = H & tb.mask;; s = (s + 1) & tb.mask) {
        const uint32_t lab = tb.lab[s];
        if (lab == 0u) return 0u;
        if (tb.key[s] == H) return lab;
    }
}

// counts of one chunk of up to 64 emissions: keep = this lane's emission is the one kept of its hash
__device__ __forceinline__ void tag_count(const TagTable &tb, bool keep, uint64_t H, int &c_n, int &c_a, int &c_b, int &c_ab) {
    const uint32_t lab = keep ? tag_probe(tb, H) : 0u;
    c_n += __popcll(__ballot(keep));
    c_a += __popcll(__ballot(lab == 1u));
    c_b += __popcll(__ballot(lab == 2u));
    c_ab += __popcll(__ballot(lab == 3u));
}

__device__ __forceinline__ void tag_store(dg_read_tag *out, int64_t r, int c_n, int c_a, int c_b, int c_ab) {
    *reinterpret_cast<int4 *>(out + r) = make_int4(c_n, c_a, c_b, c_ab);   // one 16-byte vector store
}

// first route.  first[r].tiles = first tile of read r (entry n_reads: all tiles), tile_base[t] = first emission of tile t.
__global__ __launch_bounds__(256) void tag_reads_kernel(const uint64_t *__restrict__ hash, const SeqCount *__restrict__ first, const int64_t *__restrict__ tile_base,
                                                        int64_t n_reads, int limit, int set_slots, TagTable tb, dg_read_tag *__restrict__ out, TagLong ll) {
    extern __shared__ uint32_t tag_lds[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint32_t *set = tag_lds + (size_t)wave * set_slots;
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < n_reads; r += (int64_t)gridDim.x * 4) {
        const int64_t beg = tile_base[first[r].tiles], end = tile_base[first[r + 1].tiles];
        const int64_t n64 = end - beg;
        if (n64 > limit) {                                             // second route: the record is written by tag_sorted_kernel
            if (lane == 0) {
                const uint32_t at = atomicAdd(ll.n, 1u);
                if (at < ll.cap) { ll.read[at] = r; ll.beg[at] = (uint32_t)beg; ll.end[at] = (uint32_t)end; }
            }
            continue;
        }
        const int n = (int)n64;
        int slots = TAG_MIN_SLOTS;
        while (slots < 2 * n) slots <<= 1;                             // <= set_slots: n <= limit
        const uint32_t smask = (uint32_t)slots - 1u;
        for (int q = lane; q < slots; q += 64) set[q] = 0u;
        TAG_WAVE_SYNC();
        const uint64_t *h = hash + beg;
        int c_n = 0, c_a = 0, c_b = 0, c_ab = 0;
        for (int j0 = 0; j0 < n; j0 += 64) {
            const int j = j0 + lane;
            bool keep = false;
            uint64_t H = 0;
            if (j < n) {
                H = h[j];
                for (uint32_t s = (uint32_t)H & smask;; s = (s + 1u) & smask) {   // (ends: at most n < slots entries)
                    const uint32_t old = atomicCAS(&set[s], 0u, (uint32_t)j + 1u);
                    if (old == 0u) { keep = true; break; }
                    if (h[old - 1u] == H) break;                       // an equal hash holds the slot: this one is a repeat
                }
            }
            tag_count(tb, keep, H, c_n, c_a, c_b, c_ab);
        }
        if (lane == 0) tag_store(out, r, c_n, c_a, c_b, c_ab);
        TAG_WAVE_SYNC();                                               // the set is cleared for the next read after the last probe of this one
    }
}

// second route: one wave per listed read, on its sorted segment
__global__ __launch_bounds__(256) void tag_sorted_kernel(const uint64_t *__restrict__ sorted, uint32_t n_long, TagLong ll, TagTable tb, dg_read_tag *__restrict__ out) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (uint32_t i = blockIdx.x * 4u + (uint32_t)wave; i < n_long; i += gridDim.x * 4u) {
        const uint64_t *h = sorted + ll.beg[i];
        const uint32_t n = ll.end[i] - ll.beg[i];
        int c_n = 0, c_a = 0, c_b = 0, c_ab = 0;
        for (uint32_t j0 = 0; j0 < n; j0 += 64u) {
            const uint32_t j = j0 + (uint32_t)lane;
            bool keep = false;
            uint64_t H = 0;
            if (j < n) { H = h[j]; keep = j == 0u || h[j - 1u] != H; }
            tag_count(tb, keep, H, c_n, c_a, c_b, c_ab);
        }
        if (lane == 0) tag_store(out, ll.read[i], c_n, c_a, c_b, c_ab);
    }
}

// A and B (host) go up, A first (as the reads, outside the timed part)
static int tag_upload_lists(dg_ctx *c, SketchState &S, const uint64_t *hash_a, int64_t n_a, const uint64_t *hash_b, int64_t n_b) {
    if (n_a + n_b == 0) return DG_OK;
    if (int rc = S.d_tag_key.ensure(8 * (size_t)(n_a + n_b))) return rc;
    if (n_a) DG_HIP(hipMemcpyAsync(S.d_tag_key.p, hash_a, 8 * (size_t)n_a, hipMemcpyHostToDevice, c->stream));
    if (n_b) DG_HIP(hipMemcpyAsync(S.d_tag_key.as<uint64_t>() + n_a, hash_b, 8 * (size_t)n_b, hipMemcpyHostToDevice, c->stream));
    return DG_OK;
}

// the uploaded lists -> the table; the stats are set once it stands
static int tag_build_table(dg_ctx *c, SketchState &S, int64_t n_a, int64_t n_b, TagTable *tb) {
    hipStream_t s = c->stream;
    const int64_t n = n_a + n_b;
    unsigned long long nd = 0;
    if (n > 0) {
        if (int rc = S.d_tag_lab.ensure(4 * (size_t)n)) return rc;
        if (int rc = S.d_tag_key2.ensure(8 * (size_t)n)) return rc;
        if (int rc = S.d_tag_lab2.ensure(4 * (size_t)n)) return rc;
        if (int rc = S.d_tag_ukey.ensure(8 * (size_t)n)) return rc;
        if (int rc = S.d_tag_ulab.ensure(4 * (size_t)n)) return rc;
        if (int rc = S.d_n.ensure(8)) return rc;
        hipLaunchKernelGGL(tag_fill_labels_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, S.d_tag_lab.as<uint32_t>(), n_a, n);
        size_t tb1 = 0, tb2 = 0;
        DG_HIP(rocprim::radix_sort_pairs(nullptr, tb1, S.d_tag_key.as<uint64_t>(), S.d_tag_key2.as<uint64_t>(), S.d_tag_lab.as<uint32_t>(), S.d_tag_lab2.as<uint32_t>(), (size_t)n, 0, 64, s));
        DG_HIP(rocprim::reduce_by_key(nullptr, tb2, S.d_tag_key2.as<uint64_t>(), S.d_tag_lab2.as<uint32_t>(), (size_t)n, S.d_tag_ukey.as<uint64_t>(), S.d_tag_ulab.as<uint32_t>(),
                                      S.d_n.as<unsigned long long>(), LabelOr(), rocprim::equal_to<uint64_t>(), s));
        if (int rc = S.d_tmp.ensure(std::max(tb1, tb2))) return rc;
        DG_HIP(rocprim::radix_sort_pairs(S.d_tmp.p, tb1, S.d_tag_key.as<uint64_t>(), S.d_tag_key2.as<uint64_t>(), S.d_tag_lab.as<uint32_t>(), S.d_tag_lab2.as<uint32_t>(), (size_t)n, 0, 64, s));
        DG_HIP(rocprim::reduce_by_key(S.d_tmp.p, tb2, S.d_tag_key2.as<uint64_t>(), S.d_tag_lab2.as<uint32_t>(), (size_t)n, S.d_tag_ukey.as<uint64_t>(), S.d_tag_ulab.as<uint32_t>(),
                                      S.d_n.as<unsigned long long>(), LabelOr(), rocprim::equal_to<uint64_t>(), s));
        DG_HIP(hipMemcpyAsync(&nd, S.d_n.p, 8, hipMemcpyDeviceToHost, s));
        DG_HIP(hipStreamSynchronize(s));
    }
    uint64_t slots = 1;
    if (S.opt.tag_table_bits > 0) {
        slots = 1ULL << S.opt.tag_table_bits;
        if (slots < nd + 1) { set_error("dg_sketch_tag_reads: tag_table_bits %lld leaves no empty slot for %llu distinct hashes", (long long)S.opt.tag_table_bits, nd); return DG_ERR_ARG; }
    } else while (slots < 2 * nd) slots <<= 1;
    if (int rc = S.d_tag_tkey.ensure(8 * (size_t)slots)) return rc;
    if (int rc = S.d_tag_tlab.ensure(4 * (size_t)slots)) return rc;
    DG_HIP(hipMemsetAsync(S.d_tag_tlab.p, 0, 4 * (size_t)slots, s));
    if (nd) hipLaunchKernelGGL(tag_table_insert_kernel, dim3((unsigned)((nd + 255) / 256)), dim3(256), 0, s, S.d_tag_ukey.as<uint64_t>(), S.d_tag_ulab.as<uint32_t>(), (int64_t)nd,
                               S.d_tag_tkey.as<uint64_t>(), S.d_tag_tlab.as<uint32_t>(), slots - 1);
    DG_HIP(hipGetLastError());
    *tb = TagTable{S.d_tag_tkey.as<uint64_t>(), S.d_tag_tlab.as<uint32_t>(), slots - 1};
    S.stat_tag_distinct = (int64_t)nd; S.stat_tag_slots = (int64_t)slots;
    return DG_OK;
}

}  // namespace dgi

using namespace dgi;

extern "C" int dg_sketch_tag_reads(dg_ctx *c, const char *bases, const int64_t *read_off, int64_t n_reads, int k, int w, const uint64_t *hash_a, int64_t n_a,
                                   const uint64_t *hash_b, int64_t n_b, dg_read_tag *out) {
    if (int rc = bind(c)) return rc;
    if (int rc = sketch_check_kw(k, w)) return rc;
    if (n_reads < 0 || n_a < 0 || n_b < 0 || (n_reads > 0 && (!read_off || !out)) || (n_a > 0 && !hash_a) || (n_b > 0 && !hash_b)) {
        set_error("dg_sketch_tag_reads: bad arguments");
        return DG_ERR_ARG;
    }
    const int64_t nb = n_reads ? read_off[n_reads] : 0;
    if (nb > 0 && !bases) { set_error("dg_sketch_tag_reads: null bases"); return DG_ERR_ARG; }
    SketchState &S = sketch_state(c);
    hipStream_t s = c->stream;
    if (int rc = sketch_events(S)) return rc;
    S.stat_tag_long = 0; S.stat_tag_distinct = 0; S.stat_tag_slots = 0;
    // the table first: a tag_table_bits too small for the lists is an argument error, found before anything else is done
    if (int rc = tag_upload_lists(c, S, hash_a, n_a, hash_b, n_b)) return rc;
    DG_HIP(hipEventRecord(S.ev[0], s));
    TagTable tb;
    if (int rc = tag_build_table(c, S, n_a, n_b, &tb)) return rc;
    DG_HIP(hipEventRecord(S.ev[1], s));
    float dict_ms = 0;
    DG_HIP(hipEventSynchronize(S.ev[1]));
    DG_HIP(hipEventElapsedTime(&dict_ms, S.ev[0], S.ev[1]));
    S.timing = dg_sketch_timing{0.f, dict_ms, dict_ms, 0};
    if (n_reads == 0) return DG_OK;

    if (int rc = S.d_bases.ensure((size_t)nb + 16)) return rc;
    if (nb) DG_HIP(hipMemcpyAsync(S.d_bases.p, bases, (size_t)nb, hipMemcpyHostToDevice, s));
    if (int rc = S.d_off.ensure(8 * (size_t)(n_reads + 1))) return rc;
    DG_HIP(hipMemcpyAsync(S.d_off.p, read_off, 8 * (size_t)(n_reads + 1), hipMemcpyHostToDevice, s));
    // tile pass: every emission with its read id, compacted
    DG_HIP(hipEventRecord(S.ev[0], s));
    int64_t nt = 0, n_win = 0, n_emit = 0;
    if (int rc = sketch_prepare_tiles(c, S.d_off.as<int64_t>(), n_reads, k, w, &nt, &n_win)) return rc;
    if (int rc = sketch_launch_tiles_reads(c, S.d_bases.as<char>(), nt, n_win, k, w, 0)) return rc;
    if (int rc = sketch_compact_tiles(c, nt, &n_emit)) return rc;
    DG_HIP(hipEventRecord(S.ev[1], s));
    if (n_emit > 0) {
        const int limit = S.opt.tag_lds_entries > 0 ? (int)S.opt.tag_lds_entries : TAG_LDS_DEFAULT;
        int set_slots = TAG_MIN_SLOTS;
        while (set_slots < 2 * limit) set_slots <<= 1;
        if (int rc = S.d_tag_out.ensure(sizeof(dg_read_tag) * (size_t)n_reads)) return rc;
        // (a read of more than `limit` emissions has at least two of them: at most n_emit / 2 + 1 entries, and never more than n_reads)
        const uint32_t long_cap = (uint32_t)std::min<int64_t>(std::min<int64_t>(n_reads, n_emit / 2 + 1), (int64_t)UINT32_MAX);
        if (int rc = S.d_tag_long.ensure(16 + 16 * (size_t)long_cap)) return rc;
        char *lp = S.d_tag_long.as<char>();
        TagLong ll{(uint32_t *)lp, (int64_t *)(lp + 16), (uint32_t *)(lp + 16 + 8 * (size_t)long_cap), (uint32_t *)(lp + 16 + 12 * (size_t)long_cap), long_cap};
        DG_HIP(hipMemsetAsync(ll.n, 0, 16, s));
        const unsigned grid = (unsigned)std::min<int64_t>((n_reads + 3) / 4, 8192);
        hipLaunchKernelGGL(tag_reads_kernel, dim3(grid), dim3(256), 4 * sizeof(uint32_t) * (size_t)set_slots, s, S.d_hash.as<uint64_t>(), S.d_seq_tile0.as<SeqCount>(),
                           S.d_tile_base.as<int64_t>(), n_reads, limit, set_slots, tb, S.d_tag_out.as<dg_read_tag>(), ll);
        DG_HIP(hipGetLastError());
        uint32_t n_long = 0;
        DG_HIP(hipMemcpyAsync(&n_long, ll.n, 4, hipMemcpyDeviceToHost, s));
        DG_HIP(hipStreamSynchronize(s));
        if (n_long > 0) {
            if (n_emit > (int64_t)UINT32_MAX || n_long > long_cap) { set_error("dg_sketch_tag_reads: %lld emissions exceed what the sorted route indexes (2^32)", (long long)n_emit); return DG_ERR_UNSUPPORTED; }
            if (int rc = S.d_hash2.ensure(8 * (size_t)n_emit)) return rc;
            size_t tbs = 0;
            DG_HIP(rocprim::segmented_radix_sort_keys(nullptr, tbs, S.d_hash.as<uint64_t>(), S.d_hash2.as<uint64_t>(), (unsigned)n_emit, n_long, ll.beg, ll.end, 0, 64, s));
            if (int rc = S.d_tmp.ensure(tbs)) return rc;
            DG_HIP(rocprim::segmented_radix_sort_keys(S.d_tmp.p, tbs, S.d_hash.as<uint64_t>(), S.d_hash2.as<uint64_t>(), (unsigned)n_emit, n_long, ll.beg, ll.end, 0, 64, s));
            hipLaunchKernelGGL(tag_sorted_kernel, dim3(std::min<unsigned>((n_long + 3) / 4, 8192u)), dim3(256), 0, s, S.d_hash2.as<uint64_t>(), n_long, ll, tb, S.d_tag_out.as<dg_read_tag>());
            DG_HIP(hipGetLastError());
        }
        S.stat_tag_long = n_long;
    }
    DG_HIP(hipEventRecord(S.ev[2], s));
    if (n_emit > 0) DG_HIP(hipMemcpyAsync(out, S.d_tag_out.p, sizeof(dg_read_tag) * (size_t)n_reads, hipMemcpyDeviceToHost, s));
    DG_HIP(hipStreamSynchronize(s));
    if (n_emit == 0) memset(out, 0, sizeof(dg_read_tag) * (size_t)n_reads);   // no read has a window, or none emitted anything
    float tile_ms = 0, tag_ms = 0;
    DG_HIP(hipEventElapsedTime(&tile_ms, S.ev[0], S.ev[1]));
    DG_HIP(hipEventElapsedTime(&tag_ms, S.ev[1], S.ev[2]));
    S.timing = dg_sketch_timing{tile_ms, dict_ms + tag_ms, tile_ms + dict_ms + tag_ms, n_emit};
    return DG_OK;
}

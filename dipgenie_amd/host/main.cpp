// DipGenie drop-in CLI for the diploid hot path on MI355X.
//
// Same command line as the reference (/root/reference/src/main.cpp:39-111): -t -p -R -g -r -o -k -w
// -T -d are honoured; -a -q -N -m -P -H -l -c are accepted and ignored exactly as the reference's DP
// path ignores them. The two device loops go through libdipgenie_hip.so; there is no
// CPU fallback: without a usable gfx950 device the program exits with an error.
#include <algorithm>
#include <sys/resource.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <iostream>
#include <string>
#include <thread>
#include <vector>

#include "pipeline.hpp"

// The device context is created on a side thread while the main thread reads the GFA and the reads (HIP start-up is
// ~0.3 s, the two overlap); the first backend call joins it.
struct LazyCtx {
    std::thread th;
    dg_ctx *ctx = nullptr;
    std::string err;
    bool joined = false;
    void start(int device, int k, int w) {
        th = std::thread([this, device, k, w] {
            const double tc0 = dg::now_s();
            ctx = dg_create(device);
            if (!ctx) { err = dg_last_error(); return; }
            const double tc1 = dg::now_s();
            // first launch from the sketch module loads its code object and makes the first device allocations (~10 ms):
            // paid here, beside the GFA parse, instead of in front of the first haplotype
            const std::string warm(256, 'A');
            uint64_t *h = nullptr; int64_t *p = nullptr; int64_t n = 0;
            if (k >= 1 && k <= 255 && w >= 1 && dg_sketch_haplotype(ctx, warm.data(), (int64_t)warm.size(), k, w, &h, &p, &n) == DG_OK) { dg_free(h); dg_free(p); }
            if (getenv("DG_DEBUG")) fprintf(stderr, "[dg::main] side thread: dg_create %.3f s, first sketch call %.3f s\n", tc1 - tc0, dg::now_s() - tc1);
        });
    }
    dg_ctx *get() {
        if (!joined) { th.join(); joined = true; }
        return ctx;
    }
    // the reference's error exits (exit(1) in read_gfa on a reverse-strand walk step, solver.cpp:116-119) run the static destructors while
    // the side thread may still be creating the context: a joinable std::thread there would end the process with SIGABRT instead of code 1
    ~LazyCtx() { if (th.joinable()) th.join(); }
};
static LazyCtx g_lazy;

// DG_DEBUG timeline: seconds since the kernel started this process (exec, dynamic linking and the HIP library's static
// initialisers all run before main)
static double since_exec_s() {
    FILE *f = fopen("/proc/self/stat", "r");
    if (!f) return -1;
    char buf[1024];
    const size_t n = fread(buf, 1, sizeof buf - 1, f);
    fclose(f);
    buf[n] = 0;
    const char *q = strrchr(buf, ')');                      // field 22 (starttime, clock ticks since boot) = 20th after the ')'
    if (!q) return -1;
    unsigned long long start = 0;
    int field = 3;                                          // q + 2 = field 3 (state)
    for (q += 2; *q && field < 22; ++q) if (*q == ' ') ++field;
    if (sscanf(q, "%llu", &start) != 1) return -1;
    struct timespec ts;
    clock_gettime(CLOCK_BOOTTIME, &ts);
    return ts.tv_sec + 1e-9 * ts.tv_nsec - (double)start / (double)sysconf(_SC_CLK_TCK);
}
static const char *b_last_error() { return g_lazy.joined && !g_lazy.ctx ? g_lazy.err.c_str() : dg_last_error(); }

static int b_sketch_reads(void *c, const char *b, const int64_t *off, int64_t n, int k, int w, uint64_t **h, int32_t **cnt, int64_t *nd) {
    dg_ctx *x = ((LazyCtx *)c)->get();
    return x ? dg_sketch_reads(x, b, off, n, k, w, h, cnt, nd) : DG_ERR_NO_DEVICE;
}
static int b_sketch_hap(void *c, const char *s, int64_t len, int k, int w, uint64_t **h, int64_t **p, int64_t *n) {
    dg_ctx *x = ((LazyCtx *)c)->get();
    return x ? dg_sketch_haplotype(x, s, len, k, w, h, p, n) : DG_ERR_NO_DEVICE;
}
static bool g_wide_levels = false;                          // --wide-levels
static int apply_dp_options(dg_ctx *x) {
    // DG_DP_OPTIONS="key=value,key=value": dg_dp_set_option tuning knobs for profiling and for the segmented-lattice tests (none needed
    // in normal use).  Honoured with a notice on stderr; the fault-injection keys (test_*) are refused here -- they exist for the
    // library's own tests, which set them through the C ABI.
    if (const char *o = getenv("DG_DP_OPTIONS")) {
        std::string all(o);
        if (!all.empty()) fprintf(stderr, "[dg::main] DG_DP_OPTIONS honoured: %s\n", all.c_str());
        for (size_t a = 0; a < all.size();) {
            size_t b = all.find(',', a);
            if (b == std::string::npos) b = all.size();
            const std::string kv = all.substr(a, b - a);
            const size_t eq = kv.find('=');
            if (eq != std::string::npos) {
                const std::string key = kv.substr(0, eq);
                if (key.rfind("test_", 0) == 0) { fprintf(stderr, "[E::main] DG_DP_OPTIONS: '%s' is a fault-injection key, refused\n", key.c_str()); return DG_ERR_ARG; }
                if (dg_dp_set_option(x, key.c_str(), atoll(kv.c_str() + eq + 1)) != DG_OK) return DG_ERR_ARG;
            }
            a = b + 1;
        }
    }
    return DG_OK;
}
static int b_dp(void *c, const dg_dp_graph *g, dg_dp_result *r) {
    dg_ctx *x = ((LazyCtx *)c)->get();
    if (!x) return DG_ERR_NO_DEVICE;
    if (int rc = apply_dp_options(x)) return rc;
    return dg_dp_solve_diploid(x, g, r);
}
// --budgets: the graph loaded once, every listed budget read out of one sweep
static int b_dp_load(void *c, const dg_dp_graph *g) {
    dg_ctx *x = ((LazyCtx *)c)->get();
    if (!x) return DG_ERR_NO_DEVICE;
    if (int rc = apply_dp_options(x)) return rc;
    if (g_wide_levels && dg_dp_set_option(x, "partner_wide", 1) != DG_OK) return DG_ERR_ARG;   // --wide-levels (the --site-margins run goes through here)
    return dg_dp_load_graph(x, g);
}
static int b_dp_budgets(void *c, const int32_t *budgets, int32_t n, dg_dp_result *r) {
    dg_ctx *x = ((LazyCtx *)c)->get();
    return x ? dg_dp_run_budgets(x, budgets, n, r) : DG_ERR_NO_DEVICE;
}
static int b_dp_pinned(void *c, const dg_dp_pin *pins, int64_t n_pins, const int32_t *budgets, int32_t n, dg_dp_result *r) {
    dg_ctx *x = ((LazyCtx *)c)->get();
    return x ? dg_dp_run_pinned(x, pins, n_pins, budgets, n, r) : DG_ERR_NO_DEVICE;
}
static int b_dp_pin_stats(void *c, int64_t *out, int n) {
    dg_ctx *x = ((LazyCtx *)c)->get();
    return x ? dg_dp_get_pin_stats(x, out, n) : DG_ERR_NO_DEVICE;
}
static int b_dp_call_margins(void *c, int32_t budget, const int32_t *cls, dg_dp_call_margin *levels, int32_t *paths) {
    dg_ctx *x = ((LazyCtx *)c)->get();
    return x ? dg_dp_call_margins(x, budget, cls, levels, paths) : DG_ERR_NO_DEVICE;
}
static int b_dp_answer_paths(void *c, int32_t budget, int32_t *paths) {
    dg_ctx *x = ((LazyCtx *)c)->get();
    return x ? dg_dp_get_answer_paths(x, budget, paths) : DG_ERR_NO_DEVICE;
}
static int b_dp_genotype_margins(void *c, const int32_t *called, int64_t n, int32_t budget, const int32_t *cls, dg_dp_genotype_margin *levels, int32_t *vv, int32_t *best) {
    dg_ctx *x = ((LazyCtx *)c)->get();
    return x ? dg_dp_genotype_margins(x, called, n, budget, cls, levels, vv, best) : DG_ERR_NO_DEVICE;
}
static int b_dp_genotype_table(void *c, int32_t budget, const int32_t *cls, const int32_t *called, int64_t n, dg_dp_genotype_margin *levels, int64_t *level_off,
                               dg_dp_genotype_entry **entries, int64_t *n_entries, int32_t *best) {
    dg_ctx *x = ((LazyCtx *)c)->get();
    return x ? dg_dp_genotype_table(x, budget, cls, called, n, levels, level_off, entries, n_entries, best) : DG_ERR_NO_DEVICE;
}
static int b_dp_genotype_margins_pinned(void *c, const dg_dp_pin *pins, int64_t n_pins, const int32_t *called, int64_t n, int32_t budget, const int32_t *cls,
                                        dg_dp_genotype_margin *levels, int32_t *vv, int32_t *best) {
    dg_ctx *x = ((LazyCtx *)c)->get();
    return x ? dg_dp_genotype_margins_pinned(x, pins, n_pins, called, n, budget, cls, levels, vv, best) : DG_ERR_NO_DEVICE;
}
static int b_dp_genotype_table_pinned(void *c, const dg_dp_pin *pins, int64_t n_pins, int32_t budget, const int32_t *cls, const int32_t *called, int64_t n,
                                      dg_dp_genotype_margin *levels, int64_t *level_off, dg_dp_genotype_entry **entries, int64_t *n_entries, int32_t *best) {
    dg_ctx *x = ((LazyCtx *)c)->get();
    return x ? dg_dp_genotype_table_pinned(x, pins, n_pins, budget, cls, called, n, levels, level_off, entries, n_entries, best) : DG_ERR_NO_DEVICE;
}
static int b_dp_genotype_margins_budgets(void *c, const dg_dp_pin *pins, int64_t n_pins, const int32_t *called, const int32_t *budgets, int64_t n, const int32_t *cls,
                                         dg_dp_genotype_margin *levels, int32_t *best) {
    dg_ctx *x = ((LazyCtx *)c)->get();
    return x ? dg_dp_genotype_margins_budgets(x, pins, n_pins, called, budgets, n, cls, levels, best) : DG_ERR_NO_DEVICE;
}
static int b_dp_genotype_stats(void *c, int64_t *out, int n) {
    dg_ctx *x = ((LazyCtx *)c)->get();
    return x ? dg_dp_get_genotype_stats(x, out, n) : DG_ERR_NO_DEVICE;
}
static int b_dp_phase_margins(void *c, const int32_t *called, int32_t budget, const int32_t *cls, dg_dp_phase_margin *records, int64_t *n_records, int32_t *best) {
    dg_ctx *x = ((LazyCtx *)c)->get();
    return x ? dg_dp_phase_margins(x, called, budget, cls, records, n_records, best) : DG_ERR_NO_DEVICE;
}
static int b_dp_phase_stats(void *c, int64_t *out, int n) {
    dg_ctx *x = ((LazyCtx *)c)->get();
    return x ? dg_dp_get_phase_stats(x, out, n) : DG_ERR_NO_DEVICE;
}
static int b_dp_phase_margins_budgets(void *c, const int32_t *called, const int32_t *budgets, int64_t n, const int32_t *cls, dg_dp_phase_margin *records, int64_t *record_off,
                                      int32_t *best) {
    dg_ctx *x = ((LazyCtx *)c)->get();
    return x ? dg_dp_phase_margins_budgets(x, called, budgets, n, cls, records, record_off, best) : DG_ERR_NO_DEVICE;
}
static int b_dp_phase_budget_stats(void *c, int64_t *out, int n) {
    dg_ctx *x = ((LazyCtx *)c)->get();
    return x ? dg_dp_get_phase_budget_stats(x, out, n) : DG_ERR_NO_DEVICE;
}
static int b_dp_recombination_margins(void *c, int32_t budget, const int32_t *called, int64_t n, dg_dp_recombination_margin *records, int32_t *called_out, int32_t *best) {
    dg_ctx *x = ((LazyCtx *)c)->get();
    return x ? dg_dp_recombination_margins(x, budget, called, n, records, called_out, best) : DG_ERR_NO_DEVICE;
}
static int b_dp_recombination_stats(void *c, int64_t *out, int n) {
    dg_ctx *x = ((LazyCtx *)c)->get();
    return x ? dg_dp_get_recombination_stats(x, out, n) : DG_ERR_NO_DEVICE;
}
static int b_dp_recombination_margins_budgets(void *c, const int32_t *budgets, int64_t n, const int32_t *called, dg_dp_recombination_margin *records, int32_t *called_out, int32_t *best) {
    dg_ctx *x = ((LazyCtx *)c)->get();
    return x ? dg_dp_recombination_margins_budgets(x, budgets, n, called, records, called_out, best) : DG_ERR_NO_DEVICE;
}
static int b_dp_recombination_budget_stats(void *c, int64_t *out, int n) {
    dg_ctx *x = ((LazyCtx *)c)->get();
    return x ? dg_dp_get_recombination_budget_stats(x, out, n) : DG_ERR_NO_DEVICE;
}
static int b_dp_score_paths(void *c, const int32_t *paths, int64_t n, dg_dp_pair_score *out) {
    dg_ctx *x = ((LazyCtx *)c)->get();
    return x ? dg_dp_score_paths(x, paths, n, out) : DG_ERR_NO_DEVICE;
}
static int b_dp_answer_objectives(void *c, const int32_t *budgets, int32_t n, dg_dp_pair_objective *out) {
    dg_ctx *x = ((LazyCtx *)c)->get();
    return x ? dg_dp_answer_objectives(x, budgets, n, out) : DG_ERR_NO_DEVICE;
}
static int b_tag_reads(void *c, const char *b, const int64_t *off, int64_t n, int k, int w, const uint64_t *ha, int64_t na, const uint64_t *hb, int64_t nb, dg_read_tag *out) {
    dg_ctx *x = ((LazyCtx *)c)->get();
    return x ? dg_sketch_tag_reads(x, b, off, n, k, w, ha, na, hb, nb, out) : DG_ERR_NO_DEVICE;
}
static int b_hap(void *c, const dg_hap_graph *g, int32_t *dp, int32_t *bv, int32_t *br) {
    dg_ctx *x = ((LazyCtx *)c)->get();
    return x ? dg_dp_solve_haploid(x, g, dp, bv, br) : DG_ERR_NO_DEVICE;
}
static int b_anchor_begin(void *c, int32_t nh, int32_t nv, const int32_t *top, int k, int w) {
    dg_ctx *x = ((LazyCtx *)c)->get();
    return x ? dg_anchor_begin(x, nh, nv, top, k, w) : DG_ERR_NO_DEVICE;
}
static int b_anchor_add(void *c, int32_t h, const char *s, int64_t len, const int32_t *sv, const int64_t *ss, int64_t ns, int64_t *n) {
    dg_ctx *x = ((LazyCtx *)c)->get();
    return x ? dg_anchor_add_haplotype(x, h, s, len, sv, ss, ns, n) : DG_ERR_NO_DEVICE;
}
static int b_anchor_finish(void *c, const uint64_t *sp, int64_t n, float thr, dg_anchor_result *out) {
    dg_ctx *x = ((LazyCtx *)c)->get();
    return x ? dg_anchor_finish(x, sp, n, thr, out) : DG_ERR_NO_DEVICE;
}
static void b_hint(void *c, int64_t est_cells) {   // overlap the lattice reservation (2 B/cell) with the host stages
    dg_ctx *x = ((LazyCtx *)c)->get();
    const double bytes = 2.0 * (double)est_cells;     // a low estimate is harmless: the rest is mapped before the sweep starts
    if (x && bytes >= 4e9) dg_dp_prealloc(x, bytes > 8e18 ? 0 : (int64_t)bytes);   // small lattices allocate instantly anyway
}

// ---- --gpus N: minimizer scoring sharded over N devices inside this one process (BASELINE configs[3]) ----
// One host thread per device.  Haplotype h is sketched on device h mod N (index_kmers is independent per haplotype, solver.cpp:470-473);
// the reads are scored by dg_shard_score_reads (contiguous blocks, RCCL all-reduce of the dictionary hit vector, hash-range exchange,
// per-owner merge: dipgenie_amd/csrc/dg_shard.hip); spectrum and sketches are handed to the host pipeline exactly as the Python
// driver hands them in (Pipeline::inj_*), and everything from the anchor join on -- fit, graph, DP, FASTA -- runs on the first device.
struct ShardInfo { int gpus = 0, transport = 0; int64_t n_dict = 0, dict_hits = 0; double ms_sketch = 0, ms_exchange = 0, wall_s = 0; };
static int run_sharded(dg::Pipeline &p, int n_gpus, int transport, const std::vector<int> &devices, ShardInfo &info, std::string &err) {
    const double t0 = dg::now_s();
    p.sum = dg::Summary();
    // contexts + RCCL communicator (HIP start-up, librccl, ncclCommInitAll: ~1.3 s) on a thread of their own beside the GFA and the reads
    dg_shard *sh = nullptr;
    std::string sh_err, reads_err;
    int reads_rc = 0;
    std::thread sh_thread([&] { sh = dg_shard_create(n_gpus, devices.empty() ? nullptr : devices.data(), transport); if (!sh) sh_err = dg_last_error(); });
    std::thread reads_thread([&] { reads_rc = p.load_reads(reads_err); });
    const int grc = p.load_graph(err);
    reads_thread.join();
    sh_thread.join();
    if (!sh) { err = sh_err; return -2; }                                // no gfx950 device / no librccl: no fallback
    if (grc || reads_rc) { if (!grc) err = reads_err; dg_shard_destroy(sh); return -1; }
    const double t1 = dg::now_s();
    p.inj_hap.assign(p.num_walks, {});
    std::vector<std::string> terr((size_t)n_gpus);
    std::vector<std::thread> th;
    for (int r = 0; r < n_gpus; ++r)
        th.emplace_back([&, r] {
            dg_ctx *c = dg_shard_ctx(sh, r);
            for (uint32_t h = (uint32_t)r; h < p.num_walks; h += (uint32_t)n_gpus) {
                const std::string seq = p.haplotype_sequence(h);
                uint64_t *hh = nullptr; int64_t *pp = nullptr; int64_t n = 0;
                if (dg_sketch_haplotype(c, seq.data(), (int64_t)seq.size(), p.opt.k, p.opt.w, &hh, &pp, &n) != DG_OK) { terr[r] = dg_last_error(); return; }
                p.inj_hap[h].hash.assign(hh, hh + n); p.inj_hap[h].pos.assign(pp, pp + n); p.inj_hap[h].set = true;
                dg_free(hh); dg_free(pp);
            }
        });
    for (auto &t : th) t.join();
    for (auto &e : terr) if (!e.empty()) { err = "haplotype sketch: " + e; dg_shard_destroy(sh); return -1; }
    std::vector<uint64_t> hap_hash;
    for (auto &hs : p.inj_hap) hap_hash.insert(hap_hash.end(), hs.hash.begin(), hs.hash.end());
    std::vector<int64_t> off(p.reads.size() + 1, 0);
    for (size_t r = 0; r < p.reads.size(); ++r) off[r + 1] = off[r] + (int64_t)p.reads[r].second.size();
    std::string bases;
    bases.reserve((size_t)off.back());
    for (auto &rd : p.reads) bases += rd.second;
    const int64_t n_reads = (int64_t)p.reads.size();
    p.reads.clear(); p.reads.shrink_to_fit();
    const double t2 = dg::now_s();
    uint64_t *sph = nullptr; int32_t *spc = nullptr; int64_t nsp = 0;
    std::vector<int64_t> hist(4096, 0);
    if (dg_shard_score_reads(sh, bases.data(), off.data(), n_reads, p.opt.k, p.opt.w, hap_hash.data(), (int64_t)hap_hash.size(), &sph, &spc, &nsp, hist.data(), (int)hist.size(),
                             &info.n_dict, &info.dict_hits, &info.ms_sketch, &info.ms_exchange) != DG_OK) { err = dg_last_error(); dg_shard_destroy(sh); return -1; }
    p.inj_sp_hash.assign(sph, sph + nsp); p.inj_sp_count.assign(spc, spc + nsp); p.inj_hist = hist; p.spectrum_injected = true;
    dg_free(sph); dg_free(spc);
    const double t3 = dg::now_s();
    if (!p.opt.quiet) fprintf(stderr, "[dg::shard] %d ranks (%s): haplotype sketches %.3f s, read scoring %.3f s (slowest rank: sketch %.2f ms, exchange + merge %.2f ms); dictionary %lld, hit by reads %lld\n",
                              n_gpus, transport == 0 ? "RCCL" : "host-staged", t2 - t1, t3 - t2, info.ms_sketch, info.ms_exchange, (long long)info.n_dict, (long long)info.dict_hits);
    p.sum.stage_s.emplace_back("sharded: contexts + communicator (beside GFA + reads)", t1 - t0);
    p.sum.stage_s.emplace_back("sharded: haplotype sketches", t2 - t1);
    p.sum.stage_s.emplace_back("sharded: read scoring", t3 - t2);
    g_lazy.ctx = dg_shard_ctx(sh, 0); g_lazy.joined = true;              // the rest of the pipeline: the first device's context
    info.gpus = n_gpus; info.transport = transport;
    const int rc = p.run_loaded(err);
    info.wall_s = dg::now_s() - t0;
    return rc;                                                           // (the shard object lives until the process exits: its first context is in use)
}

static void usage(FILE *fp, const dg::Options &o) {   // main.cpp:90-110
    fprintf(fp, "Usage: PHI -g <target.gfa> -r <reads.fa> -o <haplotype.fasta> \n");
    fprintf(fp, "Options:\n");
    fprintf(fp, "    -a bool      DP approximation mode\n");
    fprintf(fp, "    -k INT       K-mer size [%d]\n", o.k);
    fprintf(fp, "    -w INT       Minimizer window size [%d]\n", o.w);
    fprintf(fp, "    -R INT       Recombination limit [%d]\n", o.R);
    fprintf(fp, "    -p INT       Ploidy (default diploid i.e -p2, use -p1 for haploid) [%d]\n", o.ploidy);
    fprintf(fp, "    -T FLOAT     Threshold for minimizer filtering [%.3f]\n", o.threshold);
    fprintf(fp, "    -t INT       Threads [%d]\n", o.threads);
    fprintf(fp, "    -g INT       GFA file [%s]\n", o.gfa_file.c_str());
    fprintf(fp, "    -r INT       Read [%s]\n", o.reads_file.c_str());
    fprintf(fp, "    -o INT       Output haplotype [%s]\n", o.hap_file.c_str());
    fprintf(fp, "    -d bool      Debug mode [%d]\n", (int)o.debug);
    fprintf(fp, "    -G INT       (MI355X build) HIP device ordinal [0]\n");
    fprintf(fp, "    --budgets all|a,b,c   (MI355X build, -p2) also answer these recombination limits below -R from the same DP pass: <haplotype.fasta>.R<r>\n");
    fprintf(fp, "    --budget-table FILE   (MI355X build) with --budgets: one line r, DP value, r1, r2, len1, len2 per listed limit\n");
    fprintf(fp, "    --site-margins FILE   (MI355X build, -p2) per level and haplotype of the answer at -R: called vertex, best other allele, margin (TSV)\n");
    fprintf(fp, "    --wide-levels         (MI355X build) with --site-margins: lift its limit of 16384 cells (widest level x (R + 1)) by keeping the level state in device memory (then: widest level <= 32767, <= 16777216 cells)\n");
    fprintf(fp, "    --genotype-margins FILE   (MI355X build, -p2) per level: the genotype of the answer at -R against the best other genotype, both haplotypes free, and the margin (TSV)\n");
    fprintf(fp, "    --budget-genotype-margins FILE   (MI355X build, -p2, with --budgets) the rows of --genotype-margins for the answer at every listed limit that has one, each against the best other genotype within that limit, behind a first column r; one joint pass serves all limits (TSV)\n");
    fprintf(fp, "    --genotype-table FILE     (MI355X build, -p2) per level one row for every genotype a pair of paths within -R passes through: its best cell, value, distance to the DP value, whether the answer has it (TSV)\n");
    fprintf(fp, "    --phase-margins FILE      (MI355X build, -p2) per pair of neighbouring het levels of the answer at -R: the best pair of paths that keeps the answer's phase between them (cis) against the best that switches it (trans), and the margin (TSV)\n");
    fprintf(fp, "    --budget-phase-margins FILE   (MI355X build, -p2, with --budgets) the rows of --phase-margins for the answer at every listed limit that has one, each within that limit, behind a first column r; one joint pass serves all limits (TSV)\n");
    fprintf(fp, "    --recombination-margins FILE   (MI355X build, -p2) per transition level -> level + 1: the two hops of the answer at -R, the crossovers they spend there, and the best pair of paths within -R that spends 0, 1 or 2 there; the best other number against the answer's is the margin of the breakpoint, or of its absence (TSV)\n");
    fprintf(fp, "    --budget-recombination-margins FILE   (MI355X build, -p2, with --budgets) the rows of --recombination-margins for the answer at every listed limit that has one, each within that limit, behind a first column r; one joint pass serves all limits (TSV)\n");
    fprintf(fp, "    --objective-table FILE   (MI355X build, -p2) per limit of --budgets (without it: -R): r, DP value, objective, hom_shared, hom_single, het_single, het_both (TSV)\n");
    fprintf(fp, "    --tag-reads FILE      (MI355X build, -p2) per read: its minimizers found only in haplotype 1 / only in haplotype 2 / in both of the answer at -R, and the haplotype they support (TSV)\n");
    fprintf(fp, "    --pins FILE           (MI355X build, -p2) run the DP under cell constraints: rows level, vertex1, vertex2 [, require|forbid|require-ordered|forbid-ordered], tab-separated, . = any vertex, ids as --genotype-table prints them\n");
    fprintf(fp, "    --pinned-genotype-margins FILE   (MI355X build, -p2, with --pins) --genotype-margins of the DP under the pins: the genotype of the pinned answer at -R against the best other genotype that satisfies them\n");
    fprintf(fp, "    --pinned-genotype-table FILE     (MI355X build, -p2, with --pins) --genotype-table of the DP under the pins: every genotype a pair of paths that satisfies them passes through\n");
    fprintf(fp, "    --gpus INT   (MI355X build) shard the minimizer scoring over INT devices (RCCL); the DP runs on the first [1]\n");
}

int main(int argc, char **argv) {
    // kernel arguments in device memory (the default of this ROCm stack; in host memory every level launch of the sweep
    // costs 1.9 us more: 929 vs 666 ms on MHC-24) -- pinned before the HIP runtime starts
    setenv("HIP_FORCE_DEV_KERNARG", "1", 0);
    const bool dbg_tl = getenv("DG_DEBUG") != nullptr;
    if (dbg_tl) fprintf(stderr, "[dg::main] main() entered %.3f s after exec\n", since_exec_s());
    dg::Pipeline p;
    int device = 0, help = 0;
    std::string json;
    for (int i = 1; i < argc; ++i)
        if (!strcmp(argv[i], "--version")) { fprintf(stderr, "PHI version: 1.0 (dipgenie-mi355x)\n"); return 0; }
    // long options of this build, taken out of argv before the reference's getopt string sees it:
    //   --gpus N, --shard-transport rccl|host (host: tests on a one-GPU box), --shard-devices a,b,c (default 0 .. N-1; host transport: -G for every rank)
    int n_gpus = 1, shard_transport = -1;
    std::vector<int> shard_devices;
    std::string budgets_arg;
    bool have_budgets = false, have_site_margins = false, have_objective_table = false, have_tag_reads = false, have_genotype_margins = false, have_genotype_table = false, have_pins = false;
    bool have_pinned_margins = false, have_pinned_table = false, have_budget_margins = false, have_phase_margins = false, have_budget_phase = false, have_recombination = false, have_budget_recombination = false;
    {
        int w = 1;
        for (int i = 1; i < argc; ++i) {
            auto val = [&](const char *name) -> const char * {
                const size_t n = strlen(name);
                if (!strncmp(argv[i], name, n) && argv[i][n] == '=') return argv[i] + n + 1;
                if (!strcmp(argv[i], name) && i + 1 < argc) return argv[++i];
                return nullptr;
            };
            if (!strncmp(argv[i], "--gpus", 6)) { const char *v = val("--gpus"); if (v) { n_gpus = atoi(v); continue; } }
            if (!strncmp(argv[i], "--shard-transport", 17)) { const char *v = val("--shard-transport"); if (v) { shard_transport = !strcmp(v, "host") ? 1 : 0; continue; } }
            if (!strncmp(argv[i], "--shard-devices", 15)) { const char *v = val("--shard-devices"); if (v) { for (const char *q = v; *q;) { shard_devices.push_back(atoi(q)); q = strchr(q, ','); if (!q) break; ++q; } continue; } }
            if (!strncmp(argv[i], "--budgets", 9) && (argv[i][9] == 0 || argv[i][9] == '=')) { const char *v = val("--budgets"); if (v) { budgets_arg = v; have_budgets = true; continue; } }
            if (!strncmp(argv[i], "--site-margins", 14) && (argv[i][14] == 0 || argv[i][14] == '=')) {
                have_site_margins = true;                              // (a missing value is an empty file name: refused below)
                const char *v = val("--site-margins");
                p.opt.site_margins = v ? v : "";
                continue;
            }
            if (!strncmp(argv[i], "--genotype-margins", 18) && (argv[i][18] == 0 || argv[i][18] == '=')) {
                have_genotype_margins = true;                          // (a missing value is an empty file name: refused below)
                const char *v = val("--genotype-margins");
                p.opt.genotype_margins = v ? v : "";
                continue;
            }
            if (!strncmp(argv[i], "--budget-genotype-margins", 25) && (argv[i][25] == 0 || argv[i][25] == '=')) {
                have_budget_margins = true;                            // (a missing value is an empty file name: refused below)
                const char *v = val("--budget-genotype-margins");
                p.opt.budget_genotype_margins = v ? v : "";
                continue;
            }
            if (!strncmp(argv[i], "--budget-phase-margins", 22) && (argv[i][22] == 0 || argv[i][22] == '=')) {
                have_budget_phase = true;                              // (a missing value is an empty file name: refused below)
                const char *v = val("--budget-phase-margins");
                p.opt.budget_phase_margins = v ? v : "";
                continue;
            }
            if (!strncmp(argv[i], "--budget-recombination-margins", 30) && (argv[i][30] == 0 || argv[i][30] == '=')) {
                have_budget_recombination = true;                      // (a missing value is an empty file name: refused below)
                const char *v = val("--budget-recombination-margins");
                p.opt.budget_recombination_margins = v ? v : "";
                continue;
            }
            if (!strncmp(argv[i], "--recombination-margins", 23) && (argv[i][23] == 0 || argv[i][23] == '=')) {
                have_recombination = true;                             // (a missing value is an empty file name: refused below)
                const char *v = val("--recombination-margins");
                p.opt.recombination_margins = v ? v : "";
                continue;
            }
            if (!strncmp(argv[i], "--phase-margins", 15) && (argv[i][15] == 0 || argv[i][15] == '=')) {
                have_phase_margins = true;                             // (a missing value is an empty file name: refused below)
                const char *v = val("--phase-margins");
                p.opt.phase_margins = v ? v : "";
                continue;
            }
            if (!strncmp(argv[i], "--genotype-table", 16) && (argv[i][16] == 0 || argv[i][16] == '=')) {
                have_genotype_table = true;                            // (a missing value is an empty file name: refused below)
                const char *v = val("--genotype-table");
                p.opt.genotype_table = v ? v : "";
                continue;
            }
            if (!strncmp(argv[i], "--pins", 6) && (argv[i][6] == 0 || argv[i][6] == '=')) {
                have_pins = true;                                      // (a missing value is an empty file name: refused below)
                const char *v = val("--pins");
                p.opt.pins_file = v ? v : "";
                continue;
            }
            if (!strncmp(argv[i], "--pinned-genotype-margins", 25) && (argv[i][25] == 0 || argv[i][25] == '=')) {
                have_pinned_margins = true;                            // (a missing value is an empty file name: refused below)
                const char *v = val("--pinned-genotype-margins");
                p.opt.pinned_genotype_margins = v ? v : "";
                continue;
            }
            if (!strncmp(argv[i], "--pinned-genotype-table", 23) && (argv[i][23] == 0 || argv[i][23] == '=')) {
                have_pinned_table = true;                              // (a missing value is an empty file name: refused below)
                const char *v = val("--pinned-genotype-table");
                p.opt.pinned_genotype_table = v ? v : "";
                continue;
            }
            if (!strcmp(argv[i], "--wide-levels")) { p.opt.wide_levels = true; continue; }
            if (!strncmp(argv[i], "--objective-table", 17) && (argv[i][17] == 0 || argv[i][17] == '=')) {
                have_objective_table = true;                           // (a missing value is an empty file name: refused below)
                const char *v = val("--objective-table");
                p.opt.objective_table = v ? v : "";
                continue;
            }
            if (!strncmp(argv[i], "--tag-reads", 11) && (argv[i][11] == 0 || argv[i][11] == '=')) {
                have_tag_reads = true;                                 // (a missing value is an empty file name: refused below)
                const char *v = val("--tag-reads");
                p.opt.tag_reads = v ? v : "";
                continue;
            }
            if (!strncmp(argv[i], "--budget-table", 14)) { const char *v = val("--budget-table"); if (v) { p.opt.budget_table = v; continue; } }
            argv[w++] = argv[i];
        }
        argc = w;
    }
    int c;
    // reference option string: "x:p:d:c:l:s:m:R:P:a:q:T:H:N:m:h:k:w:t:g:r:o:DSc" (main.cpp:39); -G -J -D -A -X are ours
    while ((c = getopt(argc, argv, "x:p:d:c:l:s:m:R:P:a:q:T:H:N:h:k:w:t:g:r:o:G:J:D:A:X")) >= 0) {
        switch (c) {
        case 'w': p.opt.w = atoi(optarg); break;
        case 'k': p.opt.k = atoi(optarg); break;
        case 'p': p.opt.ploidy = atoi(optarg); break;
        case 't': p.opt.threads = atoi(optarg); break;
        case 'g': p.opt.gfa_file = optarg; break;
        case 'R': p.opt.R = atoi(optarg); break;
        case 'T': p.opt.threshold = (float)atof(optarg); break;
        case 'r': p.opt.reads_file = optarg; break;
        case 'o': p.opt.hap_file = optarg; break;
        case 'd': p.opt.debug = atoi(optarg); break;
        case 'h': help = 1; break;
        case 'G': device = atoi(optarg); break;
        case 'J': json = optarg; break;
        case 'D': p.opt.dump_prefix = optarg; break;
        case 'A': p.opt.anchor_dump = optarg; break;
        case 'X': p.opt.dump_only = true; break;
        default: break;   // parsed-but-unused on this path
        }
    }
    if (argc < 2 || p.opt.gfa_file.empty() || p.opt.reads_file.empty() || p.opt.hap_file.empty() || help) {
        usage(stderr, p.opt);
        return 1;
    }
    const double t0 = dg::now_s();
    const bool sharded = n_gpus > 1 || shard_transport >= 0;
    if (n_gpus < 1 || n_gpus > 64) { fprintf(stderr, "[E::main] --gpus must be 1 .. 64\n"); return 1; }
    if (sharded && p.opt.ploidy != 2) { fprintf(stderr, "[E::main] --gpus shards the diploid path (-p2)\n"); return 1; }
    // --budget-genotype-margins FILE: checked here, before any device is asked for; it describes the answers of --budgets on the unconstrained DP
    if (have_budget_margins) {
        if (p.opt.ploidy != 2) { fprintf(stderr, "[E::main] --budget-genotype-margins describes the genotypes of the diploid route (-p2)\n"); return 1; }
        if (!have_budgets) { fprintf(stderr, "[E::main] --budget-genotype-margins needs --budgets\n"); return 1; }
        if (p.opt.budget_genotype_margins.empty()) { fprintf(stderr, "[E::main] --budget-genotype-margins needs a file name\n"); return 1; }
        if (sharded) { fprintf(stderr, "[E::main] --budget-genotype-margins does not go with --gpus / --shard-transport\n"); return 1; }
        if (have_pins) { fprintf(stderr, "[E::main] --budget-genotype-margins does not go with --pins: it describes the unconstrained DP\n"); return 1; }
    }
    // --budget-phase-margins FILE: the same
    if (have_budget_phase) {
        if (p.opt.ploidy != 2) { fprintf(stderr, "[E::main] --budget-phase-margins describes the phase of the diploid route (-p2)\n"); return 1; }
        if (!have_budgets) { fprintf(stderr, "[E::main] --budget-phase-margins needs --budgets\n"); return 1; }
        if (p.opt.budget_phase_margins.empty()) { fprintf(stderr, "[E::main] --budget-phase-margins needs a file name\n"); return 1; }
        if (sharded) { fprintf(stderr, "[E::main] --budget-phase-margins does not go with --gpus / --shard-transport\n"); return 1; }
        if (have_pins) { fprintf(stderr, "[E::main] --budget-phase-margins does not go with --pins: it describes the unconstrained DP\n"); return 1; }
    }
    // --budget-recombination-margins FILE: as --budget-phase-margins
    if (have_budget_recombination) {
        if (p.opt.ploidy != 2) { fprintf(stderr, "[E::main] --budget-recombination-margins describes the crossovers of the diploid route (-p2)\n"); return 1; }
        if (!have_budgets) { fprintf(stderr, "[E::main] --budget-recombination-margins needs --budgets\n"); return 1; }
        if (p.opt.budget_recombination_margins.empty()) { fprintf(stderr, "[E::main] --budget-recombination-margins needs a file name\n"); return 1; }
        if (sharded) { fprintf(stderr, "[E::main] --budget-recombination-margins does not go with --gpus / --shard-transport\n"); return 1; }
        if (have_pins) { fprintf(stderr, "[E::main] --budget-recombination-margins does not go with --pins: it describes the unconstrained DP\n"); return 1; }
    }
    // --budgets all|a,b,c: checked here, before any device is asked for
    if (!p.opt.budget_table.empty() && !have_budgets) { fprintf(stderr, "[E::main] --budget-table needs --budgets\n"); return 1; }
    if (have_budgets) {
        if (p.opt.ploidy != 2) { fprintf(stderr, "[E::main] --budgets answers the diploid route (-p2); the haploid route (-p1) already evaluates every r\n"); return 1; }
        if (p.opt.R < 0) { fprintf(stderr, "[E::main] --budgets needs -R >= 0\n"); return 1; }
        if (budgets_arg == "all") for (int r = 0; r <= p.opt.R; ++r) p.opt.budgets.push_back(r);
        else {
            for (size_t a = 0; a <= budgets_arg.size();) {
                size_t b = budgets_arg.find(',', a);
                if (b == std::string::npos) b = budgets_arg.size();
                const std::string item = budgets_arg.substr(a, b - a);
                if (item.empty() || item.size() > 9 || item.find_first_not_of("0123456789") != std::string::npos) {
                    fprintf(stderr, "[E::main] --budgets: '%s' is not a recombination limit (all, or non-negative integers separated by commas)\n", item.c_str()); return 1;
                }
                const int r = atoi(item.c_str());
                if (r > p.opt.R) { fprintf(stderr, "[E::main] --budgets: %d is above -R %d (one pass answers the limits 0..R)\n", r, p.opt.R); return 1; }
                if (std::find(p.opt.budgets.begin(), p.opt.budgets.end(), r) == p.opt.budgets.end()) p.opt.budgets.push_back(r);
                a = b + 1;
            }
        }
        // one device call takes 256 called pairs: a longer list is refused here, not after the DP run
        if (have_budget_phase && p.opt.budgets.size() > 256) {
            fprintf(stderr, "[E::main] --budget-phase-margins: --budgets lists %zu limits; one call answers 256 at the most\n", p.opt.budgets.size()); return 1;
        }
        if (have_budget_recombination && p.opt.budgets.size() > 256) {
            fprintf(stderr, "[E::main] --budget-recombination-margins: --budgets lists %zu limits; one call answers 256 at the most\n", p.opt.budgets.size()); return 1;
        }
    }
    // --site-margins FILE: checked here too, before any device is asked for
    if (have_site_margins) {
        if (p.opt.ploidy != 2) { fprintf(stderr, "[E::main] --site-margins describes the two haplotypes of the diploid route (-p2)\n"); return 1; }
        if (p.opt.site_margins.empty()) { fprintf(stderr, "[E::main] --site-margins needs a file name\n"); return 1; }
    }
    if (p.opt.wide_levels && !have_site_margins) { fprintf(stderr, "[E::main] --wide-levels goes with --site-margins: it lifts the cell limit of that option alone\n"); return 1; }
    // --genotype-margins FILE: the same
    if (have_genotype_margins) {
        if (p.opt.ploidy != 2) { fprintf(stderr, "[E::main] --genotype-margins describes the genotype of the diploid route (-p2)\n"); return 1; }
        if (p.opt.genotype_margins.empty()) { fprintf(stderr, "[E::main] --genotype-margins needs a file name\n"); return 1; }
        if (sharded) { fprintf(stderr, "[E::main] --genotype-margins does not go with --gpus / --shard-transport\n"); return 1; }
    }
    // --genotype-table FILE: the same
    if (have_genotype_table) {
        if (p.opt.ploidy != 2) { fprintf(stderr, "[E::main] --genotype-table lists the genotypes of the diploid route (-p2)\n"); return 1; }
        if (p.opt.genotype_table.empty()) { fprintf(stderr, "[E::main] --genotype-table needs a file name\n"); return 1; }
        if (sharded) { fprintf(stderr, "[E::main] --genotype-table does not go with --gpus / --shard-transport\n"); return 1; }
    }
    // --phase-margins FILE: the same; it describes the unconstrained DP (the library has no pinned form of the call)
    if (have_phase_margins) {
        if (p.opt.ploidy != 2) { fprintf(stderr, "[E::main] --phase-margins describes the phase of the diploid route (-p2)\n"); return 1; }
        if (p.opt.phase_margins.empty()) { fprintf(stderr, "[E::main] --phase-margins needs a file name\n"); return 1; }
        if (sharded) { fprintf(stderr, "[E::main] --phase-margins does not go with --gpus / --shard-transport\n"); return 1; }
        if (have_pins) { fprintf(stderr, "[E::main] --phase-margins does not go with --pins: it describes the unconstrained DP\n"); return 1; }
    }
    // --recombination-margins FILE: the same; it too describes the unconstrained DP
    if (have_recombination) {
        if (p.opt.ploidy != 2) { fprintf(stderr, "[E::main] --recombination-margins describes the crossovers of the diploid route (-p2)\n"); return 1; }
        if (p.opt.recombination_margins.empty()) { fprintf(stderr, "[E::main] --recombination-margins needs a file name\n"); return 1; }
        if (sharded) { fprintf(stderr, "[E::main] --recombination-margins does not go with --gpus / --shard-transport\n"); return 1; }
        if (have_pins) { fprintf(stderr, "[E::main] --recombination-margins does not go with --pins: it describes the unconstrained DP\n"); return 1; }
    }
    // --objective-table FILE: the same
    if (have_objective_table) {
        if (p.opt.ploidy != 2) { fprintf(stderr, "[E::main] --objective-table describes the pairs of paths of the diploid route (-p2)\n"); return 1; }
        if (p.opt.objective_table.empty()) { fprintf(stderr, "[E::main] --objective-table needs a file name\n"); return 1; }
    }
    // --tag-reads FILE: the same
    if (have_tag_reads) {
        if (p.opt.ploidy != 2) { fprintf(stderr, "[E::main] --tag-reads tags the reads by the two haplotypes of the diploid route (-p2)\n"); return 1; }
        if (p.opt.tag_reads.empty()) { fprintf(stderr, "[E::main] --tag-reads needs a file name\n"); return 1; }
        if (sharded) { fprintf(stderr, "[E::main] --tag-reads does not go with --gpus / --shard-transport: the sharded path drops the reads once they are scored\n"); return 1; }
    }
    // --pinned-genotype-margins FILE, --pinned-genotype-table FILE: the joint pass on the DP that --pins constrains; checked here too
    if (have_pinned_margins || have_pinned_table) {
        const char *which = have_pinned_margins ? "--pinned-genotype-margins" : "--pinned-genotype-table";
        if (!have_pins) { fprintf(stderr, "[E::main] --pinned-genotype-margins / --pinned-genotype-table describe the DP under --pins: they need it\n"); return 1; }
        if (p.opt.ploidy != 2) { fprintf(stderr, "[E::main] %s describes the genotypes of the diploid route (-p2)\n", which); return 1; }
        if (have_pinned_margins && p.opt.pinned_genotype_margins.empty()) { fprintf(stderr, "[E::main] --pinned-genotype-margins needs a file name\n"); return 1; }
        if (have_pinned_table && p.opt.pinned_genotype_table.empty()) { fprintf(stderr, "[E::main] --pinned-genotype-table needs a file name\n"); return 1; }
        if (sharded) { fprintf(stderr, "[E::main] %s does not go with --gpus / --shard-transport\n", which); return 1; }
    }
    // --pins FILE: the same; the margin and table options describe the unconstrained DP, the sharded path has no pinned run
    if (have_pins) {
        if (p.opt.ploidy != 2) { fprintf(stderr, "[E::main] --pins constrains the pair of paths of the diploid route (-p2)\n"); return 1; }
        if (p.opt.pins_file.empty()) { fprintf(stderr, "[E::main] --pins needs a file name\n"); return 1; }
        if (have_site_margins || have_genotype_margins || have_genotype_table) {
            fprintf(stderr, "[E::main] --pins does not go with --site-margins / --genotype-margins / --genotype-table: they describe the unconstrained DP\n"); return 1;
        }
        if (sharded) { fprintf(stderr, "[E::main] --pins does not go with --gpus / --shard-transport\n"); return 1; }
        const std::string e = dg::read_pins_file(p.opt.pins_file, p.opt.pin_rows);   // a malformed row: exit status 2, before any device is asked for
        if (!e.empty()) { fprintf(stderr, "[E::main] %s\n", e.c_str()); return 2; }
    }
    g_wide_levels = p.opt.wide_levels;
    if (!sharded) g_lazy.start(device, p.opt.k, p.opt.w);
    p.be.ctx = &g_lazy;
    p.be.sketch_reads = b_sketch_reads;
    p.be.sketch_haplotype = b_sketch_hap;
    p.be.dp_solve_diploid = b_dp;
    p.be.dp_load_graph = b_dp_load;
    p.be.dp_run_budgets = b_dp_budgets;
    p.be.dp_call_margins = b_dp_call_margins;
    p.be.dp_answer_objectives = b_dp_answer_objectives;
    p.be.tag_reads = b_tag_reads;
    p.be.dp_answer_paths = b_dp_answer_paths;
    p.be.dp_genotype_margins = b_dp_genotype_margins;
    p.be.dp_genotype_stats = b_dp_genotype_stats;
    p.be.dp_genotype_table = b_dp_genotype_table;
    p.be.dp_genotype_margins_budgets = b_dp_genotype_margins_budgets;
    p.be.dp_genotype_margins_pinned = b_dp_genotype_margins_pinned;
    p.be.dp_genotype_table_pinned = b_dp_genotype_table_pinned;
    p.be.dp_phase_margins = b_dp_phase_margins;
    p.be.dp_phase_stats = b_dp_phase_stats;
    p.be.dp_phase_margins_budgets = b_dp_phase_margins_budgets;
    p.be.dp_phase_budget_stats = b_dp_phase_budget_stats;
    p.be.dp_recombination_margins = b_dp_recombination_margins;
    p.be.dp_recombination_stats = b_dp_recombination_stats;
    p.be.dp_score_paths = b_dp_score_paths;
    p.be.dp_recombination_margins_budgets = b_dp_recombination_margins_budgets;
    p.be.dp_recombination_budget_stats = b_dp_recombination_budget_stats;
    p.be.dp_run_pinned = b_dp_pinned;
    p.be.dp_pin_stats = b_dp_pin_stats;
    p.be.free_buf = dg_free;
    p.be.hint_dp_soon = b_hint;
    p.be.dp_solve_haploid = b_hap;
    if (const char *hm = getenv("DG_HAPLOID")) p.opt.haploid_mode = !strcmp(hm, "host") ? 1 : (!strcmp(hm, "device") ? 2 : 0);   // default: by graph shape
    p.be.anchor_begin = b_anchor_begin;
    p.be.anchor_add_haplotype = b_anchor_add;
    p.be.anchor_finish = b_anchor_finish;
    if (getenv("DG_HOST_ANCHORS")) p.opt.host_anchors = true;
    p.opt.leak_at_exit = !getenv("DG_CLEAN_EXIT");   // A/B and parity runs: the host join / filter / sort
    p.be.last_error = b_last_error;
    std::string err;
    if (dbg_tl) fprintf(stderr, "[dg::main] run() starts %.3f s after main\n", dg::now_s() - t0);
    ShardInfo shard;
    int rc;
    if (sharded) {
        if (shard_transport < 0) shard_transport = 0;
        if (shard_devices.empty() && shard_transport == 1) shard_devices.assign((size_t)n_gpus, device);   // host-staged: every rank on -G
        if (!shard_devices.empty() && (int)shard_devices.size() != n_gpus) { fprintf(stderr, "[E::main] --shard-devices needs %d entries\n", n_gpus); return 1; }
        rc = run_sharded(p, n_gpus, shard_transport, shard_devices, shard, err);
        if (rc == -2) { fprintf(stderr, "[E::main] %s\n", err.c_str()); return 2; }
    } else rc = p.run(err);
    if (dbg_tl) {
        fprintf(stderr, "[dg::main] run() returned %.3f s after main", dg::now_s() - t0);
        for (auto &st : p.sum.stage_s) if (st.first == "total") fprintf(stderr, " (its own total: %.3f s)", st.second);
        fputc('\n', stderr);
    }
    dg_ctx *ctx = g_lazy.get();
    if (!ctx) { fprintf(stderr, "[E::main] %s\n", g_lazy.err.c_str()); return 2; }   // no gfx950 device: no CPU fallback
    if (rc != 0 && err == "dump_only") { std::cout.flush(); fflush(nullptr); _exit(0); }   // -X: stop after the dump(s)
    if (rc != 0 && p.sum.pins.bad_rows) { fprintf(stderr, "[E::main] %s\n", err.c_str()); dg_destroy(ctx); return 2; }   // --pins: a level or a vertex the graph does not have
    if (rc != 0) { fprintf(stderr, "[E::main] %s\n", err.c_str()); dg_destroy(ctx); return 1; }
    dg_dp_timing tm;
    const bool have_tm = p.opt.ploidy == 2 && dg_dp_get_timing(ctx, &tm) == DG_OK;
    if (have_tm)
        fprintf(stderr, "[dg::dp] delta %.3f ms, forward %.3f ms (%lld launches), traceback %.3f ms; %.3f G cells, %.3f G relaxations\n",
                tm.delta_ms, tm.forward_ms, (long long)tm.n_forward_launches, tm.traceback_ms, p.sum.cells / 1e9, p.sum.relaxations / 1e9);
    if (!json.empty()) {
        FILE *f = fopen(json.c_str(), "w");
        if (f) {
            fprintf(f, "{\"dp_value\": %d, \"s_het\": %d, \"r1\": %d, \"r2\": %d, \"obj\": %d, \"len1\": %lld, \"len2\": %lld, "
                       "\"spectrum\": %lld, \"n_levels\": %lld, \"n_vertices\": %lld, \"cells\": %llu, \"relaxations\": %llu, "
                       "\"gpus\": %d, \"shard_transport\": \"%s\", \"dictionary\": %lld, \"dictionary_hits\": %lld, \"shard_sketch_ms\": %.3f, \"shard_exchange_ms\": %.3f, "
                       "\"best_r_haploid\": %d, \"fit_nll\": %.17g, \"dp_segments\": %d, \"dp_chunks\": %d, \"dp_forward_ms\": %.3f, \"dp_traceback_ms\": %.3f, \"dp_forward_launches\": %lld, \"dp_edge_pairs\": %llu, \"dp_colour_entries\": %llu, \"stages\": {",
                    p.sum.dp_value, p.sum.s_het, p.sum.r1, p.sum.r2, p.sum.obj, (long long)p.sum.len1, (long long)p.sum.len2,
                    (long long)p.sum.spectrum, (long long)p.sum.n_levels, (long long)p.sum.n_vertices,
                    (unsigned long long)p.sum.cells, (unsigned long long)p.sum.relaxations, sharded ? shard.gpus : 1, !sharded ? "none" : (shard.transport ? "host" : "rccl"),
                    (long long)shard.n_dict, (long long)shard.dict_hits, shard.ms_sketch, shard.ms_exchange, p.sum.best_r_haploid, p.sum.fit.nll,
                    have_tm ? tm.n_segments : 0, have_tm ? tm.n_chunks : 0, have_tm ? tm.forward_ms : 0.f, have_tm ? tm.traceback_ms : 0.f,
                    have_tm ? (long long)tm.n_forward_launches : 0LL, have_tm ? (unsigned long long)tm.edge_pairs : 0ULL, have_tm ? (unsigned long long)tm.colour_entries : 0ULL);
            for (size_t i = 0; i < p.sum.stage_s.size(); ++i)
                fprintf(f, "%s\"%s\": %.6f", i ? ", " : "", p.sum.stage_s[i].first.c_str(), p.sum.stage_s[i].second);
            fprintf(f, "}");
            if (have_budgets) {                                         // one entry per listed limit; null fields: unreachable
                fprintf(f, ", \"budgets\": [");
                for (size_t i = 0; i < p.sum.budget_rows.size(); ++i) {
                    const dg::BudgetRow &b = p.sum.budget_rows[i];
                    if (b.reachable) fprintf(f, "%s{\"r\": %d, \"dp_value\": %d, \"r1\": %d, \"r2\": %d, \"len1\": %lld, \"len2\": %lld}", i ? ", " : "", b.r, b.dp_value, b.r1, b.r2, (long long)b.len1, (long long)b.len2);
                    else fprintf(f, "%s{\"r\": %d, \"dp_value\": null, \"r1\": null, \"r2\": null, \"len1\": null, \"len2\": null}", i ? ", " : "", b.r);
                }
                fprintf(f, "]");
            }
            if (p.sum.site_margins.set) {                               // per haplotype, over the levels 1 .. L - 2; min_positive_margin null: none is positive
                const dg::SiteMargins &sm = p.sum.site_margins;
                fprintf(f, ", \"site_margins\": {\"haplotypes\": [");
                for (int h = 0; h < 2; ++h) {
                    fprintf(f, "%s{\"with_alternative\": %lld, \"margin0\": %lld, \"min_positive_margin\": ", h ? ", " : "", (long long)sm.with_alternative[h], (long long)sm.margin0[h]);
                    if (sm.min_positive_margin[h] >= 0) fprintf(f, "%d}", sm.min_positive_margin[h]); else fprintf(f, "null}");
                }
                fprintf(f, "], \"wall_s\": %.6f}", sm.wall_s);
            }
            for (int pinned = 0; pinned < 2; ++pinned) {                // the unpinned objects, then (with --pins) the same fields of the DP under the pins
                const dg::GenotypeMargins &gm = pinned ? p.sum.pinned_genotype_margins : p.sum.genotype_margins;
                if (gm.set) {                                           // over the levels 1 .. L - 2; min_positive_margin null: none is positive
                    fprintf(f, ", \"%sgenotype_margins\": {\"with_alternative\": %lld, \"margin0\": %lld, \"min_positive_margin\": ", pinned ? "pinned_" : "", (long long)gm.with_alternative, (long long)gm.margin0);
                    if (gm.min_positive_margin >= 0) fprintf(f, "%d", gm.min_positive_margin); else fprintf(f, "null");
                    fprintf(f, ", \"segments\": %lld, \"wall_s\": %.6f}", (long long)gm.segments, gm.wall_s);
                }
                const dg::GenotypeTable &gt = pinned ? p.sum.pinned_genotype_table : p.sum.genotype_table;
                if (gt.set) {                                           // a recount of FILE: its rows, levels with >= 2 rows, levels with >= 2 rows of delta 0, most rows of a level
                    fprintf(f, ", \"%sgenotype_table\": {\"entries\": %lld, \"levels_with_choice\": %lld, \"co_optimal_levels\": %lld, \"max_per_level\": %lld, \"wall_s\": %.6f}", pinned ? "pinned_" : "",
                            (long long)gt.entries, (long long)gt.levels_with_choice, (long long)gt.co_optimal_levels, (long long)gt.max_per_level, gt.wall_s);
                }
            }
            if (p.sum.budget_genotype_margins.set) {                    // per listed limit with an answer the fields of genotype_margins; one device call
                const dg::BudgetGenotypeMargins &bm = p.sum.budget_genotype_margins;
                fprintf(f, ", \"budget_genotype_margins\": {\"budgets\": [");
                for (size_t i = 0; i < bm.rows.size(); ++i) {
                    fprintf(f, "%s{\"r\": %d, \"with_alternative\": %lld, \"margin0\": %lld, \"min_positive_margin\": ", i ? ", " : "", bm.rows[i].r, (long long)bm.rows[i].with_alternative, (long long)bm.rows[i].margin0);
                    if (bm.rows[i].min_positive_margin >= 0) fprintf(f, "%d}", bm.rows[i].min_positive_margin); else fprintf(f, "null}");
                }
                fprintf(f, "], \"segments\": %lld, \"wall_s\": %.6f}", (long long)bm.segments, bm.wall_s);
            }
            if (p.sum.phase_margins.set) {                              // a recount of FILE: with_alternative = rows with a reachable trans; min_positive_margin null: none is positive
                const dg::PhaseMargins &pm = p.sum.phase_margins;
                fprintf(f, ", \"phase_margins\": {\"het_levels\": %lld, \"records\": %lld, \"with_alternative\": %lld, \"margin0\": %lld, \"min_positive_margin\": ", (long long)pm.het_levels,
                        (long long)pm.records, (long long)pm.with_alternative, (long long)pm.margin0);
                if (pm.min_positive_margin >= 0) fprintf(f, "%d", pm.min_positive_margin); else fprintf(f, "null");
                fprintf(f, ", \"segments\": %lld, \"wall_s\": %.6f}", (long long)pm.segments, pm.wall_s);
            }
            if (p.sum.recombination_margins.set) {                      // a recount of FILE: breakpoints = rows with s_called > 0; min_positive_breakpoint_margin null: none is positive
                const dg::RecombinationMargins &rm = p.sum.recombination_margins;
                fprintf(f, ", \"recombination_margins\": {\"transitions\": %lld, \"called_recombinations\": %lld, \"breakpoints_margin0\": %lld, \"min_positive_breakpoint_margin\": ",
                        (long long)rm.transitions, (long long)rm.called_recombinations, (long long)rm.breakpoints_margin0);
                if (rm.min_positive_breakpoint_margin >= 0) fprintf(f, "%d", rm.min_positive_breakpoint_margin); else fprintf(f, "null");
                fprintf(f, ", \"co_optimal_elsewhere\": %lld, \"segments\": %lld, \"wall_s\": %.6f}", (long long)rm.co_optimal_elsewhere, (long long)rm.segments, rm.wall_s);
            }
            if (p.sum.budget_recombination_margins.set) {               // per listed limit with an answer the counts of recombination_margins; one device call
                const dg::BudgetRecombinationMargins &br = p.sum.budget_recombination_margins;
                fprintf(f, ", \"budget_recombination_margins\": {\"budgets\": [");
                for (size_t i = 0; i < br.rows.size(); ++i) {
                    const dg::RecombinationMargins &rm = br.rows[i].counts;
                    fprintf(f, "%s{\"r\": %d, \"transitions\": %lld, \"called_recombinations\": %lld, \"breakpoints_margin0\": %lld, \"min_positive_breakpoint_margin\": ", i ? ", " : "", br.rows[i].r,
                            (long long)rm.transitions, (long long)rm.called_recombinations, (long long)rm.breakpoints_margin0);
                    if (rm.min_positive_breakpoint_margin >= 0) fprintf(f, "%d", rm.min_positive_breakpoint_margin); else fprintf(f, "null");
                    fprintf(f, ", \"co_optimal_elsewhere\": %lld}", (long long)rm.co_optimal_elsewhere);
                }
                fprintf(f, "], \"segments\": %lld, \"wall_s\": %.6f}", (long long)br.segments, br.wall_s);
            }
            if (p.sum.budget_phase_margins.set) {                       // per listed limit with an answer the fields of phase_margins; one device call
                const dg::BudgetPhaseMargins &bp = p.sum.budget_phase_margins;
                fprintf(f, ", \"budget_phase_margins\": {\"budgets\": [");
                for (size_t i = 0; i < bp.rows.size(); ++i) {
                    const dg::BudgetPhaseMargins::Row &row = bp.rows[i];
                    fprintf(f, "%s{\"r\": %d, \"het_levels\": %lld, \"records\": %lld, \"with_alternative\": %lld, \"margin0\": %lld, \"min_positive_margin\": ", i ? ", " : "", row.r,
                            (long long)row.het_levels, (long long)row.records, (long long)row.with_alternative, (long long)row.margin0);
                    if (row.min_positive_margin >= 0) fprintf(f, "%d}", row.min_positive_margin); else fprintf(f, "null}");
                }
                fprintf(f, "], \"seed_keys\": %lld, \"slot_levels\": %lld, \"segments\": %lld, \"wall_s\": %.6f}", (long long)bp.seed_keys, (long long)bp.slot_levels, (long long)bp.segments,
                        bp.wall_s);
            }
            if (have_objective_table) {                                 // one entry per row of the table; null fields: unreachable
                fprintf(f, ", \"objectives\": [");
                for (size_t i = 0; i < p.sum.objective_rows.size(); ++i) {
                    const dg::ObjectiveRow &o = p.sum.objective_rows[i];
                    if (o.reachable) fprintf(f, "%s{\"r\": %d, \"dp_value\": %d, \"objective\": %d, \"hom_shared\": %d, \"hom_single\": %d, \"het_single\": %d, \"het_both\": %d}", i ? ", " : "", o.r, o.dp_value,
                                         o.rec.hom_shared + o.rec.het_single, o.rec.hom_shared, o.rec.hom_single, o.rec.het_single, o.rec.het_both);
                    else fprintf(f, "%s{\"r\": %d, \"dp_value\": null, \"objective\": null, \"hom_shared\": null, \"hom_single\": null, \"het_single\": null, \"het_both\": null}", i ? ", " : "", o.r);
                }
                fprintf(f, "]");
            }
            if (p.sum.pins.set) {                                       // the file's rows, the run's pins and pinned levels, pairs it ran as two launches, the answer at -R passes only allowed cells
                const dg::PinSummary &ps = p.sum.pins;
                fprintf(f, ", \"pins\": {\"rows\": %lld, \"pins\": %lld, \"levels\": %lld, \"pairs_as_singles\": %lld, \"satisfied\": %s}", (long long)ps.rows, (long long)ps.pins, (long long)ps.levels,
                        (long long)ps.pairs_as_singles, ps.satisfied ? "true" : "false");
            }
            if (p.sum.read_tags.set) {                                  // hap1 + hap2 + tie + no_evidence = reads
                const dg::ReadTags &rt = p.sum.read_tags;
                fprintf(f, ", \"read_tags\": {\"reads\": %lld, \"hap1\": %lld, \"hap2\": %lld, \"tie\": %lld, \"no_evidence\": %lld}", (long long)rt.reads, (long long)rt.hap1, (long long)rt.hap2,
                        (long long)rt.tie, (long long)rt.no_evidence);
            }
            fprintf(f, "}\n");
            fclose(f);
        }
    }
    fprintf(stderr, "[M::main] Real time: %.3f sec\n", dg::now_s() - t0);
    if (dbg_tl) {
        struct rusage ru;
        getrusage(RUSAGE_SELF, &ru);
        fprintf(stderr, "[dg::main] leaving %.3f s after exec; peak RSS %.2f GB, %ld minor page faults, user %.2f s, system %.2f s\n", since_exec_s(),
                ru.ru_maxrss / 1048576.0, ru.ru_minflt, ru.ru_utime.tv_sec + 1e-6 * ru.ru_utime.tv_usec, ru.ru_stime.tv_sec + 1e-6 * ru.ru_stime.tv_usec);
        if (FILE *f = fopen("/proc/self/smaps_rollup", "r")) {      // what the resident set is made of right now
            char line[256];
            while (fgets(line, sizeof line, f))
                if (!strncmp(line, "Rss:", 4) || !strncmp(line, "AnonHugePages:", 14) || !strncmp(line, "Anonymous:", 10) || !strncmp(line, "Shared_Clean:", 13) ||
                    !strncmp(line, "Private_Clean:", 14) || !strncmp(line, "Pss_File:", 9) || !strncmp(line, "Pss_Shmem:", 10))
                    fprintf(stderr, "[dg::main] smaps_rollup %s", line);
            fclose(f);
        }
    }
    // Everything is written and closed.  Tearing down tens of GB of device chunks and host vectors one by one costs
    // ~0.4 s that the operating system does for free at exit; DG_CLEAN_EXIT=1 keeps the orderly path (leak checkers).
    if (!getenv("DG_CLEAN_EXIT")) {
        std::cout.flush();
        fflush(nullptr);
        _exit(0);
    }
    const double td0 = dg::now_s();
    dg_destroy(ctx);
    if (dbg_tl) fprintf(stderr, "[dg::main] dg_destroy %.3f s\n", dg::now_s() - td0);
    if (getenv("DG_CLEAN_EXIT_FAST")) { std::cout.flush(); fflush(nullptr); _exit(0); }   // (measurement: device side released, host side left to the OS)
    return 0;
}

"""ctypes bindings of include/dipgenie_hip.h (libdipgenie_hip.so).  No fallbacks, no oracle imports."""
import contextlib
import ctypes as C
import os
import struct

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DG_LIB") or os.path.join(_HERE, "csrc", "libdipgenie_hip.so")   # DG_LIB: A/B runs of two builds (tools/)

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: build it with `make -C dipgenie_amd/csrc` (or __graft_entry__.build()). "
        "dipgenie_amd has no CPU fallback."
    )
# One HIP runtime per process: PyTorch ships its own libamdhip64 / libhsa-runtime64 (ROCm 7.0) under the same sonames as
# the system's (ROCm 7.2) that libdipgenie_hip.so is linked against, and the dynamic loader binds a soname to whichever
# copy came first.  Loaded after this library, torch would get the system copy and then finds "No HIP GPUs"; loaded before
# it, both share torch's copy (what bench.py, dist_sketch.py and the GPU tests need).  So where torch is installed it goes first.
try:
    import torch  # noqa: F401
except ImportError:
    pass
lib = C.CDLL(LIB_PATH)


class DpGraph(C.Structure):
    _fields_ = [
        ("n_vertices", C.c_int32), ("n_levels", C.c_int32), ("R", C.c_int32),
        ("level_off", C.c_void_p), ("out_off", C.c_void_p), ("out_dst", C.c_void_p), ("out_w", C.c_void_p),
        ("hom_off", C.c_void_p), ("het_off", C.c_void_p), ("hom_col", C.c_void_p), ("het_col", C.c_void_p),
    ]


class DpResult(C.Structure):
    _fields_ = [
        ("value", C.c_int32), ("s_het", C.c_int32), ("n_p1", C.c_int32), ("n_p2", C.c_int32),
        ("p1_from", C.c_void_p), ("p1_to", C.c_void_p), ("p2_from", C.c_void_p), ("p2_to", C.c_void_p),
        ("cap", C.c_int32), ("cells", C.c_uint64), ("relaxations", C.c_uint64),
    ]


class DpTiming(C.Structure):
    _fields_ = [
        ("delta_ms", C.c_float), ("forward_ms", C.c_float), ("traceback_ms", C.c_float), ("total_ms", C.c_float),
        ("n_forward_launches", C.c_int64), ("edge_pairs", C.c_uint64), ("colour_entries", C.c_uint64),
        ("state_bytes", C.c_uint64), ("bp_bytes", C.c_uint64), ("delta_bytes", C.c_uint64), ("n_segments", C.c_int32), ("n_chunks", C.c_int32),
    ]


# dg_dp_pair_score as a numpy record: what Context.dp_score_paths returns
PAIR_SCORE = np.dtype([("value", np.int32), ("s_het", np.int32), ("r1", np.int32), ("r2", np.int32)])

# dg_dp_partner as a numpy record: what Context.dp_best_partners returns
PARTNER = np.dtype([("value", np.int32), ("s_het", np.int32), ("r1", np.int32), ("r2", np.int32)])

# dg_dp_level_margin as a numpy record: one per (query, level) of Context.dp_partner_marginals
LEVEL_MARGIN = np.dtype([("best_vertex", np.int32), ("best_value", np.int32), ("second_vertex", np.int32), ("second_value", np.int32)])

# dg_dp_call_margin as a numpy record: one per (haplotype, level) of Context.dp_call_margins
CALL_MARGIN = np.dtype([("vertex", np.int32), ("value", np.int32), ("alt_vertex", np.int32), ("alt_value", np.int32)])

# dg_dp_genotype_margin as a numpy record: one per (query, level) of Context.dp_genotype_margins
GENOTYPE_MARGIN = np.dtype([("vertex1", np.int32), ("vertex2", np.int32), ("value", np.int32), ("alt_vertex1", np.int32), ("alt_vertex2", np.int32),
                            ("alt_value", np.int32), ("reserved", np.int32, (2,))])

# dg_dp_genotype_entry as a numpy record: one per (level, genotype) of Context.dp_genotype_table
GENOTYPE_ENTRY = np.dtype([("class1", np.int32), ("class2", np.int32), ("vertex1", np.int32), ("vertex2", np.int32), ("value", np.int32), ("reserved", np.int32)])

# dg_dp_phase_margin as a numpy record: one per pair of neighbouring het levels of Context.dp_phase_margins
PHASE_MARGIN = np.dtype([("level_a", np.int32), ("level_b", np.int32), ("cis_value", np.int32), ("cis_vertex1", np.int32), ("cis_vertex2", np.int32),
                         ("trans_value", np.int32), ("trans_vertex1", np.int32), ("trans_vertex2", np.int32), ("reserved", np.int32, (2,))])

# dg_dp_recombination_margin as a numpy record: one per transition of Context.dp_recombination_margins
RECOMBINATION_MARGIN = np.dtype([("level", np.int32), ("value", np.int32, (3,)), ("from1", np.int32, (3,)), ("from2", np.int32, (3,)), ("to1", np.int32, (3,)),
                                 ("to2", np.int32, (3,))])

# dg_dp_pair_objective as a numpy record: what Context.dp_objective_paths and Context.dp_answer_objectives return
PAIR_OBJECTIVE = np.dtype([("hom_shared", np.int32), ("hom_single", np.int32), ("het_single", np.int32), ("het_both", np.int32)])


class SketchTiming(C.Structure):
    _fields_ = [("kernel_ms", C.c_float), ("sort_ms", C.c_float), ("total_ms", C.c_float), ("n_emitted", C.c_int64)]


class ReadTag(C.Structure):
    """dg_read_tag: one row of what Context.sketch_tag_reads returns (columns in this order)"""
    _fields_ = [("n_min", C.c_int32), ("only_a", C.c_int32), ("only_b", C.c_int32), ("both", C.c_int32)]


# every symbol include/dipgenie_hip.h declares
SYMBOLS = [
    "dg_create", "dg_destroy", "dg_last_error", "dg_set_stream", "dg_synchronize", "dg_device_info",
    "dg_dp_prealloc", "dg_dp_load_graph", "dg_dp_run", "dg_dp_get_timing", "dg_dp_solve_diploid", "dg_dp_get_level_digest",
    "dg_dp_set_option", "dg_dp_get_launch_profile", "dg_sketch_reads", "dg_sketch_haplotype", "dg_hash_kmers", "dg_free",
    "dg_sketch_get_timing", "dg_sketch_reads_dev", "dg_sketch_count_dictionary_dev", "dg_sketch_merge_runs_dev",
    "dg_sketch_partition_dev", "dg_sketch_rank_dictionary_dev", "dg_sketch_histogram_dev",
    "dg_anchor_begin", "dg_anchor_add_haplotype", "dg_anchor_finish", "dg_dp_solve_haploid", "dg_dp_get_table_digest", "dg_hip_versions", "dg_anchor_add_haplotype_sketched",
    "dg_sketch_set_option", "dg_sketch_get_stat", "dg_sketch_count_rank_dictionary_dev",
    "dg_shard_create", "dg_shard_destroy", "dg_shard_n_ranks", "dg_shard_ctx", "dg_shard_score_reads",
    "dg_dp_run_budgets", "dg_dp_get_budget_values", "dg_dp_score_paths", "dg_dp_best_partners", "dg_dp_partner_marginals",
    "dg_dp_get_option", "dg_sketch_get_option", "dg_dp_list_sweep_variants", "dg_dp_get_answer_paths", "dg_dp_call_margins",
    "dg_dp_objective_paths", "dg_dp_answer_objectives", "dg_dp_get_partner_route", "dg_dp_get_pair_profile", "dg_dp_list_pair_variants",
    "dg_sketch_tag_reads", "dg_dp_genotype_margins", "dg_dp_get_genotype_stats", "dg_dp_genotype_table",
    "dg_dp_run_pinned", "dg_dp_get_pin_stats", "dg_dp_genotype_margins_pinned", "dg_dp_genotype_table_pinned",
    "dg_dp_genotype_margins_budgets", "dg_dp_phase_margins", "dg_dp_get_phase_stats", "dg_dp_phase_margins_budgets", "dg_dp_get_phase_budget_stats",
    "dg_dp_recombination_margins", "dg_dp_get_recombination_stats", "dg_dp_recombination_margins_budgets", "dg_dp_get_recombination_budget_stats",
]

lib.dg_create.restype = C.c_void_p
lib.dg_create.argtypes = [C.c_int]
lib.dg_destroy.argtypes = [C.c_void_p]
lib.dg_destroy.restype = None
lib.dg_last_error.restype = C.c_char_p
lib.dg_set_stream.argtypes = [C.c_void_p, C.c_void_p]
lib.dg_synchronize.argtypes = [C.c_void_p]
lib.dg_device_info.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int64)]
lib.dg_dp_prealloc.argtypes = [C.c_void_p, C.c_int64]
lib.dg_dp_load_graph.argtypes = [C.c_void_p, C.POINTER(DpGraph)]
lib.dg_dp_run.argtypes = [C.c_void_p, C.POINTER(DpResult)]
lib.dg_dp_run_budgets.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(DpResult)]
lib.dg_dp_get_budget_values.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
lib.dg_dp_run_pinned.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.POINTER(DpResult)]
lib.dg_dp_get_pin_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
lib.dg_dp_score_paths.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
lib.dg_dp_best_partners.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
lib.dg_dp_partner_marginals.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
lib.dg_dp_get_answer_paths.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
lib.dg_dp_call_margins.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
lib.dg_dp_get_partner_route.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
lib.dg_dp_genotype_margins.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]
lib.dg_dp_genotype_table.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                     C.POINTER(C.c_int32)]
lib.dg_dp_get_genotype_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
lib.dg_dp_genotype_margins_pinned.argtypes = [C.c_void_p, C.c_void_p, C.c_int64] + lib.dg_dp_genotype_margins.argtypes[1:]
lib.dg_dp_genotype_margins_budgets.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
lib.dg_dp_phase_margins.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
lib.dg_dp_get_phase_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
lib.dg_dp_phase_margins_budgets.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
lib.dg_dp_get_phase_budget_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
lib.dg_dp_recombination_margins.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]
lib.dg_dp_get_recombination_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
lib.dg_dp_recombination_margins_budgets.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
lib.dg_dp_get_recombination_budget_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
lib.dg_dp_genotype_table_pinned.argtypes = [C.c_void_p, C.c_void_p, C.c_int64] + lib.dg_dp_genotype_table.argtypes[1:]
lib.dg_dp_objective_paths.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
lib.dg_dp_answer_objectives.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
lib.dg_dp_get_timing.argtypes = [C.c_void_p, C.POINTER(DpTiming)]
lib.dg_dp_solve_diploid.argtypes = [C.c_void_p, C.POINTER(DpGraph), C.POINTER(DpResult)]
lib.dg_dp_get_level_digest.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
lib.dg_dp_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
lib.dg_dp_get_option.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int64)]
lib.dg_dp_get_launch_profile.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
lib.dg_dp_list_sweep_variants.argtypes = [C.c_char_p, C.c_int]
lib.dg_dp_get_pair_profile.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
lib.dg_dp_list_pair_variants.argtypes = [C.c_char_p, C.c_int]
lib.dg_dp_get_table_digest.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
lib.dg_sketch_reads.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, C.c_int, C.c_int,
                                C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
lib.dg_sketch_haplotype.argtypes = [C.c_void_p, C.c_char_p, C.c_int64, C.c_int, C.c_int,
                                    C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
lib.dg_hash_kmers.argtypes = [C.c_void_p, C.c_char_p, C.c_int64, C.c_int, C.c_void_p]
lib.dg_free.argtypes = [C.c_void_p]
lib.dg_free.restype = None
lib.dg_sketch_get_timing.argtypes = [C.c_void_p, C.POINTER(SketchTiming)]
lib.dg_sketch_reads_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int,
                                    C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
lib.dg_sketch_count_dictionary_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
lib.dg_sketch_merge_runs_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                         C.c_int64, C.POINTER(C.c_int64)]
lib.dg_sketch_partition_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
lib.dg_sketch_rank_dictionary_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
lib.dg_sketch_histogram_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
lib.dg_sketch_count_rank_dictionary_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
lib.dg_sketch_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
lib.dg_sketch_get_option.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int64)]
lib.dg_sketch_get_stat.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int64)]
lib.dg_sketch_tag_reads.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]


class HapGraph(C.Structure):
    _fields_ = [("n_vertices", C.c_int32), ("R", C.c_int32), ("out_off", C.c_void_p), ("out_dst", C.c_void_p), ("out_w", C.c_void_p), ("n_colours", C.c_void_p)]


lib.dg_dp_solve_haploid.argtypes = [C.c_void_p, C.POINTER(HapGraph), C.c_void_p, C.c_void_p, C.c_void_p]


class AnchorResult(C.Structure):
    _fields_ = [("n_occ", C.c_int64), ("n_vtx", C.c_int64), ("occ_id", C.c_void_p), ("occ_hap", C.c_void_p), ("occ_off", C.c_void_p),
                ("occ_len", C.c_void_p), ("vpool", C.c_void_p), ("n_candidates", C.c_int64), ("n_unstable_groups", C.c_int64)]


lib.dg_anchor_begin.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int, C.c_int]
lib.dg_anchor_add_haplotype.argtypes = [C.c_void_p, C.c_int32, C.c_char_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
lib.dg_anchor_add_haplotype_sketched.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64]
lib.dg_anchor_finish.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.POINTER(AnchorResult)]


lib.dg_hip_versions.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int)]


def hip_versions():
    """(HIP version the library was built against, HIP runtime it is bound to in this process), as "major.minor.patch" strings"""
    a, b = C.c_int(), C.c_int()
    if lib.dg_hip_versions(C.byref(a), C.byref(b)) != 0:
        raise DgError(lib.dg_last_error().decode())
    fmt = lambda v: f"{v // 10000000}.{v // 100000 % 100}.{v % 100000}"
    return fmt(a.value), fmt(b.value)


class DgError(RuntimeError):
    pass


def _check(rc, what):
    if rc != 0:
        raise DgError(f"{what} failed (rc={rc}): {lib.dg_last_error().decode()}")


class DpGraphArrays:
    """Levelized DP graph in the dg_dp_graph layout (numpy arrays); loads the host pipeline's .dpg dump."""

    NAMES = ["level_off", "out_off", "out_dst", "out_w", "hom_off", "hom_col", "het_off", "het_col"]
    DTYPES = [np.int32, np.int64, np.int32, np.uint8, np.int64, np.int32, np.int64, np.int32]

    def __init__(self, R, **arrays):
        self.R = int(R)
        for n, dt in zip(self.NAMES, self.DTYPES):
            setattr(self, n, np.ascontiguousarray(arrays[n], dtype=dt))

    @classmethod
    def load(cls, path):
        with open(path, "rb") as f:
            if f.read(8) != b"DGDP0001":
                raise ValueError("not a .dpg file")
            (R,) = struct.unpack("<i", f.read(4))
            arrs = {}
            for n, dt in zip(cls.NAMES, cls.DTYPES):
                (cnt,) = struct.unpack("<Q", f.read(8))
                arrs[n] = np.frombuffer(f.read(cnt * np.dtype(dt).itemsize), dtype=dt).copy()
        return cls(R, **arrs)

    def save(self, path):
        with open(path, "wb") as f:
            f.write(b"DGDP0001")
            f.write(struct.pack("<i", self.R))
            for n in self.NAMES:
                a = getattr(self, n)
                f.write(struct.pack("<Q", a.size))
                f.write(a.tobytes())

    @property
    def n_vertices(self):
        return self.out_off.size - 1

    @property
    def n_levels(self):
        return self.level_off.size - 1

    def as_struct(self, struct_cls=DpGraph):
        g = struct_cls()
        g.n_vertices, g.n_levels, g.R = self.n_vertices, self.n_levels, self.R
        for n in self.NAMES:
            a = getattr(self, n)
            # keep a non-NULL pointer even for empty colour arrays
            setattr(g, n, a.ctypes.data if a.size else np.zeros(1, a.dtype).ctypes.data)
        return g


class DpOutcome:
    def __init__(self, res, p1, p2):
        self.value, self.s_het = res.value, res.s_het
        self.cells, self.relaxations = res.cells, res.relaxations
        self.p1, self.p2 = p1, p2  # lists of (from, to)

    def key(self):
        return (self.value, self.s_het, tuple(self.p1), tuple(self.p2))


def make_result(cap):
    bufs = [np.zeros(cap, np.int32) for _ in range(4)]
    res = DpResult()
    res.p1_from, res.p1_to, res.p2_from, res.p2_to = (b.ctypes.data for b in bufs)
    res.cap = cap
    return res, bufs


def outcome_from(res, bufs):
    p1 = [(int(bufs[0][i]), int(bufs[1][i])) for i in range(res.n_p1)]
    p2 = [(int(bufs[2][i]), int(bufs[3][i])) for i in range(res.n_p2)]
    return DpOutcome(res, p1, p2)


PIN_REQUIRE, PIN_FORBID = 0, 1


def _pin_rows(pins):
    """pins as int32 [n, 4]: from an array or an iterable of (level, vertex1, vertex2, kind)"""
    return np.ascontiguousarray(np.asarray(list(pins) if not isinstance(pins, np.ndarray) else pins, np.int32).reshape(-1, 4))


def genotype_pins(level, v1, v2, kind=PIN_REQUIRE):
    """the pins of an unordered genotype: cell (v1, v2) of `level` in both orders (one pin where v1 == v2), as rows
    (level, vertex1, vertex2, kind) for Context.dp_run_pinned"""
    rows = [(int(level), int(v1), int(v2), int(kind))]
    if int(v1) != int(v2):
        rows.append((int(level), int(v2), int(v1), int(kind)))
    return rows


@contextlib.contextmanager
def _options(get, set_, kv):
    saved = []
    try:
        for key, value in kv.items():
            old = get(key)
            set_(key, value)
            saved.append((key, old))
        yield
    finally:
        for key, old in reversed(saved):
            set_(key, old)


class Context:
    """One dg_ctx (one HIP device + stream)."""

    def __init__(self, device=0):
        self.h = lib.dg_create(device)
        if not self.h:
            raise DgError(f"dg_create({device}) failed: {lib.dg_last_error().decode()}")

    def close(self):
        if self.h:
            lib.dg_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_ptr):
        _check(lib.dg_set_stream(self.h, C.c_void_p(stream_ptr)), "dg_set_stream")

    def device_info(self):
        name = C.create_string_buffer(256)
        ncu, hbm = C.c_int(), C.c_int64()
        _check(lib.dg_device_info(self.h, name, 256, C.byref(ncu), C.byref(hbm)), "dg_device_info")
        return name.value.decode(), ncu.value, hbm.value

    # ---- DP ----
    def dp_set_option(self, key, value):
        _check(lib.dg_dp_set_option(self.h, key.encode(), int(value)), "dg_dp_set_option")

    def dp_get_option(self, key):
        v = C.c_int64(0)
        _check(lib.dg_dp_get_option(self.h, key.encode(), C.byref(v)), "dg_dp_get_option")
        return v.value

    def dp_options(self, **kv):
        """with ctx.dp_options(fast=0, ...): the given DP options for the body, then the values they had before"""
        return _options(self.dp_get_option, self.dp_set_option, kv)

    def dp_prealloc(self, nbytes=0):
        """start reserving back-pointer lattice chunks in the background (nbytes <= 0: 60 % of the free HBM)"""
        _check(lib.dg_dp_prealloc(self.h, int(nbytes)), "dg_dp_prealloc")

    def dp_load_graph(self, g):
        self._g = g
        st = g.as_struct()
        _check(lib.dg_dp_load_graph(self.h, C.byref(st)), "dg_dp_load_graph")

    def dp_run(self):
        res, bufs = make_result(self._g.R + 8)
        _check(lib.dg_dp_run(self.h, C.byref(res)), "dg_dp_run")
        return outcome_from(res, bufs)

    def dp_run_budgets(self, budgets):
        """one sweep of the loaded graph, then the read-out of every listed budget (0..R, distinct, any order): a DpOutcome per
        entry, equal to what a graph loaded with R = budget gives; an unreachable budget has value NEG_INF and empty paths"""
        budgets = [int(b) for b in budgets]
        arr = (DpResult * max(len(budgets), 1))()
        keep = []
        for q, b in enumerate(budgets):
            res, bufs = make_result(max(b, 0) + 8)
            arr[q] = res
            keep.append(bufs)
        want = np.asarray(budgets, np.int32)
        _check(lib.dg_dp_run_budgets(self.h, want.ctypes.data if want.size else None, len(budgets), arr), "dg_dp_run_budgets")
        return [outcome_from(arr[q], keep[q]) for q in range(len(budgets))]

    def dp_run_pinned(self, pins, budgets=None):
        """dp_run_budgets on the DP in which some cells are unreachable.  pins: int32 [n, 4] or an iterable of (level, vertex1,
        vertex2, kind): the pin matches cell (i, j) of its level -- i the vertex of haplotype 1, j of haplotype 2, ordered -- if
        vertex1 is -1 or i and vertex2 is -1 or j; kind 0 (PIN_REQUIRE): the level's cell must match one of its require-pins, 1
        (PIN_FORBID): it must match none of its forbid-pins.  budgets defaults to [R].  Returns a DpOutcome per budget; a
        constraint set nothing satisfies within a budget has value NEG_INF and empty paths.  The call is the last run for
        dp_budget_values, dp_answer_paths, dp_answer_objectives, dp_timing and the profiles; dp_call_margins refuses it."""
        p = _pin_rows(pins)
        budgets = [self._g.R] if budgets is None else [int(b) for b in budgets]
        arr = (DpResult * max(len(budgets), 1))()
        keep = []
        for q, b in enumerate(budgets):
            res, bufs = make_result(max(b, 0) + 8)
            arr[q] = res
            keep.append(bufs)
        want = np.asarray(budgets, np.int32)
        _check(lib.dg_dp_run_pinned(self.h, p.ctypes.data if p.size else None, p.shape[0], want.ctypes.data if want.size else None, len(budgets), arr),
               "dg_dp_run_pinned")
        return [outcome_from(arr[q], keep[q]) for q in range(len(budgets))]

    def dp_pin_stats(self):
        """of the last dp_run_pinned with pins on this context: dict(pins, levels, mask_launches, pairs_as_singles, batches_plain)"""
        out = np.zeros(5, np.int64)
        _check(lib.dg_dp_get_pin_stats(self.h, out.ctypes.data, 5), "dg_dp_get_pin_stats")
        return dict(zip(("pins", "levels", "mask_launches", "pairs_as_singles", "batches_plain"), out.tolist()))

    def dp_budget_values(self):
        """the sink's value on planes 0..R of the last dp_run / dp_run_budgets (int32[R + 1], NEG_INF where unreachable)"""
        out = np.zeros(self._g.R + 1, np.int32)
        _check(lib.dg_dp_get_budget_values(self.h, out.ctypes.data, out.size), "dg_dp_get_budget_values")
        return out

    def dp_score_paths(self, paths):
        """paths: int32 [n, 2, n_levels], the vertex id of both paths of n pairs at every level of the loaded graph (source first,
        sink last).  Returns a PAIR_SCORE record array of n entries (fields value, s_het, r1, r2); a vertex outside its level or a
        hop without an edge raises DgError naming the first offending pair, path and level.  Leaves the last run's answers alone."""
        p = np.ascontiguousarray(paths, np.int32)
        g = getattr(self, "_g", None)                      # (no graph loaded: the library answers DG_ERR_STATE)
        if p.ndim != 3 or p.shape[1] != 2 or (g is not None and p.shape[2] != g.n_levels):
            raise ValueError(f"paths must have shape [n, 2, n_levels], got {p.shape}")
        out = np.zeros(p.shape[0], PAIR_SCORE)
        _check(lib.dg_dp_score_paths(self.h, p.ctypes.data if p.size else None, p.shape[0], out.ctypes.data if out.size else None), "dg_dp_score_paths")
        return out

    def dp_best_partners(self, given, budgets, want_paths=True):
        """given: int32 [n, n_levels], one source -> sink path of the loaded graph per query; budgets: int [n], each >= 0.  Returns
        (records, partners): a PARTNER record array of n entries (value, s_het, r1, r2) and the best partner of every given path
        within its budget, int32 [n, n_levels] (None with want_paths=False).  value = NEG_INF: no path fits the budget, the row is
        all -1.  A bad given path raises DgError naming the first (query, level).  Leaves the last run's answers alone."""
        p = np.ascontiguousarray(given, np.int32)
        b = np.ascontiguousarray(budgets, np.int32)
        g = getattr(self, "_g", None)                      # (no graph loaded: the library answers DG_ERR_STATE)
        if p.ndim != 2 or (g is not None and p.shape[1] != g.n_levels):
            raise ValueError(f"given must have shape [n, n_levels], got {p.shape}")
        if b.shape != (p.shape[0],):
            raise ValueError(f"budgets must have shape [{p.shape[0]}], got {b.shape}")
        out = np.zeros(p.shape[0], PARTNER)
        partners = np.zeros(p.shape, np.int32) if want_paths else None
        _check(lib.dg_dp_best_partners(self.h, p.ctypes.data if p.size else None, p.shape[0], b.ctypes.data if b.size else None,
                                       partners.ctypes.data if want_paths and partners.size else None, out.ctypes.data if out.size else None), "dg_dp_best_partners")
        return out, partners

    def dp_partner_marginals(self, given, budgets, want_vertices=False):
        """given, budgets: as for dp_best_partners.  Returns (levels, vertex_values): a LEVEL_MARGIN record array [n, n_levels]
        (best_vertex, best_value, second_vertex, second_value: the vertex of the level that the best partner within the budget
        passes through -- the smallest id among equals --, what that partner is worth, and the same for the best partner that goes
        through another vertex of the level; -1 and NEG_INF where there is none) and, with want_vertices=True, int32
        [n, n_vertices]: the value of the best partner through every vertex, NEG_INF where no path within the budget passes
        (None otherwise).  best_value - second_value is the margin of the call at that level.  A query whose budget nothing fits
        is all -1 / NEG_INF.  A bad given path raises DgError naming the first (query, level).  Leaves the last run's answers alone."""
        p = np.ascontiguousarray(given, np.int32)
        b = np.ascontiguousarray(budgets, np.int32)
        g = getattr(self, "_g", None)                      # (no graph loaded: the library answers DG_ERR_STATE)
        if p.ndim != 2 or (g is not None and p.shape[1] != g.n_levels):
            raise ValueError(f"given must have shape [n, n_levels], got {p.shape}")
        if b.shape != (p.shape[0],):
            raise ValueError(f"budgets must have shape [{p.shape[0]}], got {b.shape}")
        levels = np.zeros(p.shape, LEVEL_MARGIN)
        values = np.zeros((p.shape[0], g.n_vertices if g is not None else 0), np.int32) if want_vertices else None
        _check(lib.dg_dp_partner_marginals(self.h, p.ctypes.data if p.size else None, p.shape[0], b.ctypes.data if b.size else None,
                                           levels.ctypes.data if levels.size else None, values.ctypes.data if want_vertices and values.size else None),
               "dg_dp_partner_marginals")
        return levels, values

    def dp_answer_paths(self, budget):
        """the pair of paths the last dp_run / dp_run_budgets walked for `budget` (one the run read out): int32 [2, n_levels], row 0
        the path of DpOutcome.p1, row 1 that of p2 -- rows that dp_score_paths, dp_best_partners and dp_partner_marginals take.  Both
        rows are all -1 where no pair fits the budget.  Leaves the run's answers alone."""
        g = getattr(self, "_g", None)                      # (no graph loaded: the library answers DG_ERR_STATE)
        paths = np.zeros((2, g.n_levels if g is not None else 1), np.int32)
        _check(lib.dg_dp_get_answer_paths(self.h, int(budget), paths.ctypes.data), "dg_dp_get_answer_paths")
        return paths

    def dp_call_margins(self, budget, vertex_class=None, want_paths=False):
        """Per haplotype of the last run's answer at `budget` and per level: a CALL_MARGIN record array [2, n_levels] (vertex: the
        called vertex; value: what the best partner through it is worth with the other haplotype fixed, the run's value at the
        budget; alt_vertex, alt_value: the same for the best vertex of another class, -1 and NEG_INF where there is none) and, with
        want_paths=True, what dp_answer_paths returns (None otherwise).  vertex_class: int32 [n_vertices], or None for "every vertex
        is its own class".  value - alt_value is the margin of the call.  Leaves the run's answers alone."""
        g = getattr(self, "_g", None)                      # (no graph loaded: the library answers DG_ERR_STATE)
        n_levels = g.n_levels if g is not None else 1
        cls = None
        if vertex_class is not None:
            cls = np.ascontiguousarray(vertex_class, np.int32)
            if g is not None and cls.shape != (g.n_vertices,):
                raise ValueError(f"vertex_class must have shape [{g.n_vertices}], got {cls.shape}")
        levels = np.zeros((2, n_levels), CALL_MARGIN)
        paths = np.zeros((2, n_levels), np.int32) if want_paths else None
        _check(lib.dg_dp_call_margins(self.h, int(budget), cls.ctypes.data if cls is not None else None, levels.ctypes.data,
                                      paths.ctypes.data if want_paths else None), "dg_dp_call_margins")
        return levels, paths

    def dp_partner_route(self):
        """(route, cells) of the last dp_best_partners / dp_partner_marginals / dp_call_margins on this context that got as far as
        a launch: route 1 = level state in LDS, 2 = in device memory (option partner_wide), 0 = no such call yet; cells = that call's
        widest level x (largest budget + 1)."""
        route, cells = C.c_int32(0), C.c_int64(0)
        _check(lib.dg_dp_get_partner_route(self.h, C.byref(route), C.byref(cells)), "dg_dp_get_partner_route")
        return route.value, cells.value

    def dp_genotype_margins(self, called, budget, vertex_class=None, want_vertices=False):
        """Genotype margins with both haplotypes free.  called: int32 [n, 2, n_levels] (or [2, n_levels] for n = 1), per query one
        cell per level, every id inside its level -- the two rows of dp_answer_paths are such a query; budget >= 0, independent of the
        graph's R; vertex_class: int32 [n_vertices], or None for "every vertex is its own class".  Returns (levels, best_value) or,
        with want_vertices=True, (levels, best_value, vertex_values): a GENOTYPE_MARGIN record array [n, n_levels] (vertex1, vertex2:
        the called cell; value: the best value of any pair of paths through it within the budget; alt_vertex1 <= alt_vertex2,
        alt_value: the same for the best cell of another genotype, -1, -1 and NEG_INF where there is none), the best value of any pair
        within the budget, and int32 [n_vertices]: the best value of any pair with one path through the vertex.  value - alt_value
        is the margin of the called genotype at that level, negative where the called cell is not optimal.  An id outside its
        level raises DgError naming the first (query, row, level).  Leaves the last run's answers alone."""
        return self._genotype_margins(None, called, budget, vertex_class, want_vertices)

    def dp_genotype_margins_pinned(self, pins, called, budget, vertex_class=None, want_vertices=False):
        """dp_genotype_margins on the DP that the pins constrain (pins as for dp_run_pinned): value is the best value of any ordered
        pair of paths through the ordered called cell that satisfies the pins, best_value what dp_run_pinned(pins) gives for the
        budget.  Pins are ordered, so the through-values need not be symmetric: the alternative (alt_vertex1 <= alt_vertex2) is worth
        the better of its two orders, vertex_values the best of the ordered row.  A pin set nothing satisfies within the budget is
        NEG_INF / -1 everywhere.  No pins: dp_genotype_margins.  Leaves the last run's answers, pins and statistics alone."""
        return self._genotype_margins(_pin_rows(pins), called, budget, vertex_class, want_vertices)

    def _genotype_margins(self, pins, called, budget, vertex_class, want_vertices):
        p = np.ascontiguousarray(called, np.int32)
        if p.ndim == 2:
            p = p[None]
        g = getattr(self, "_g", None)                      # (no graph loaded: the library answers DG_ERR_STATE)
        if p.ndim != 3 or p.shape[1] != 2 or (g is not None and p.shape[2] != g.n_levels):
            raise ValueError(f"called must have shape [n, 2, n_levels], got {p.shape}")
        cls = None
        if vertex_class is not None:
            cls = np.ascontiguousarray(vertex_class, np.int32)
            if g is not None and cls.shape != (g.n_vertices,):
                raise ValueError(f"vertex_class must have shape [{g.n_vertices}], got {cls.shape}")
        levels = np.zeros((p.shape[0], p.shape[2]), GENOTYPE_MARGIN)
        values = np.zeros(g.n_vertices if g is not None else 1, np.int32) if want_vertices else None
        best = C.c_int32(0)
        args = (p.ctypes.data if p.size else None, p.shape[0], int(budget), cls.ctypes.data if cls is not None else None,
                levels.ctypes.data if levels.size else None, values.ctypes.data if want_vertices else None, C.byref(best))
        if pins is None:
            _check(lib.dg_dp_genotype_margins(self.h, *args), "dg_dp_genotype_margins")
        else:
            _check(lib.dg_dp_genotype_margins_pinned(self.h, pins.ctypes.data if pins.size else None, pins.shape[0], *args), "dg_dp_genotype_margins_pinned")
        return (levels, best.value, values) if want_vertices else (levels, best.value)

    def dp_genotype_margins_budgets(self, called, budgets, vertex_class=None, pins=None):
        """dp_genotype_margins with one budget per query, from one joint pass at the largest of them.  called: int32 [n, 2, n_levels],
        or [2, n_levels] with a scalar budget; budgets: n integers >= 0, in any order, repeats allowed; vertex_class as for
        dp_genotype_margins; pins as for dp_run_pinned (None or empty: the unpinned DP).  Returns (levels, best_values): the
        GENOTYPE_MARGIN records [n, n_levels], query q exactly what dp_genotype_margins(called[q], budgets[q], vertex_class) -- with
        pins dp_genotype_margins_pinned -- answers, and int32 [n]: the best value of any pair within budgets[q].  A budget that no
        pair fits gives NEG_INF / -1 records for its query only.  At most 256 queries.  Leaves the last run's answers alone."""
        p = np.ascontiguousarray(called, np.int32)
        if p.ndim == 2 and np.ndim(budgets) == 0:
            p, budgets = p[None], [budgets]
        b = np.ascontiguousarray(budgets, np.int32)          # (a scalar with [n, 2, n_levels] comes out as [1]: refused below unless n = 1)
        g = getattr(self, "_g", None)                      # (no graph loaded: the library answers DG_ERR_STATE)
        if p.ndim != 3 or p.shape[1] != 2 or (g is not None and p.shape[2] != g.n_levels):
            raise ValueError(f"called must have shape [n, 2, n_levels], got {p.shape}")
        if b.shape != (p.shape[0],):
            raise ValueError(f"budgets must have shape [{p.shape[0]}], got {b.shape}")
        cls = None
        if vertex_class is not None:
            cls = np.ascontiguousarray(vertex_class, np.int32)
            if g is not None and cls.shape != (g.n_vertices,):
                raise ValueError(f"vertex_class must have shape [{g.n_vertices}], got {cls.shape}")
        pins = _pin_rows(pins) if pins is not None else None
        levels = np.zeros((p.shape[0], p.shape[2]), GENOTYPE_MARGIN)
        best = np.zeros(p.shape[0], np.int32)
        _check(lib.dg_dp_genotype_margins_budgets(self.h, pins.ctypes.data if pins is not None and pins.size else None, pins.shape[0] if pins is not None else 0,
                                                  p.ctypes.data if p.size else None, b.ctypes.data if b.size else None, p.shape[0], cls.ctypes.data if cls is not None else None,
                                                  levels.ctypes.data if levels.size else None, best.ctypes.data if best.size else None), "dg_dp_genotype_margins_budgets")
        return levels, best

    def dp_genotype_table(self, budget, vertex_class=None, called=None):
        """The genotype table: per level and genotype (the unordered pair of its cell's classes) the best value of any pair of paths
        through a cell of that genotype, and that cell.  budget, vertex_class as for dp_genotype_margins.  Returns (level_off,
        entries, best_value): int64 [n_levels + 1], a GENOTYPE_ENTRY record array (class1 <= class2, vertex1 <= vertex2, value) whose
        slice level_off[l] : level_off[l + 1] lists level l in ascending (class1, class2), genotypes without a reachable cell left
        out, and the best value of any pair within the budget.  With called (as for dp_genotype_margins, at most 256 queries) a
        fourth element follows: the GENOTYPE_MARGIN records dp_genotype_margins answers for it, from the same pass.  Leaves the last
        run's answers alone."""
        return self._genotype_table(None, budget, vertex_class, called)

    def dp_genotype_table_pinned(self, pins, budget, vertex_class=None, called=None):
        """dp_genotype_table on the DP that the pins constrain (pins as for dp_run_pinned): an entry is the best value of any pair of
        paths that satisfies the pins through a cell of the genotype in either order (vertex1 <= vertex2), the records are those of
        dp_genotype_margins_pinned.  A pin set nothing satisfies within the budget is the empty table.  No pins: dp_genotype_table.
        Leaves the last run's answers, pins and statistics alone."""
        return self._genotype_table(_pin_rows(pins), budget, vertex_class, called)

    def _genotype_table(self, pins, budget, vertex_class, called):
        g = getattr(self, "_g", None)                      # (no graph loaded: the library answers DG_ERR_STATE)
        p = levels = None
        if called is not None:
            p = np.ascontiguousarray(called, np.int32)
            if p.ndim == 2:
                p = p[None]
            if p.ndim != 3 or p.shape[1] != 2 or (g is not None and p.shape[2] != g.n_levels):
                raise ValueError(f"called must have shape [n, 2, n_levels], got {p.shape}")
            levels = np.zeros((p.shape[0], p.shape[2]), GENOTYPE_MARGIN)
        cls = None
        if vertex_class is not None:
            cls = np.ascontiguousarray(vertex_class, np.int32)
            if g is not None and cls.shape != (g.n_vertices,):
                raise ValueError(f"vertex_class must have shape [{g.n_vertices}], got {cls.shape}")
        off = np.zeros((g.n_levels if g is not None else 0) + 1, np.int64)
        ptr, n, best = C.c_void_p(None), C.c_int64(0), C.c_int32(0)
        args = (int(budget), cls.ctypes.data if cls is not None else None, p.ctypes.data if p is not None and p.size else None,
                p.shape[0] if p is not None else 0, levels.ctypes.data if levels is not None and levels.size else None, off.ctypes.data,
                C.byref(ptr), C.byref(n), C.byref(best))
        if pins is None:
            _check(lib.dg_dp_genotype_table(self.h, *args), "dg_dp_genotype_table")
        else:
            _check(lib.dg_dp_genotype_table_pinned(self.h, pins.ctypes.data if pins.size else None, pins.shape[0], *args), "dg_dp_genotype_table_pinned")
        try:
            entries = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_int32)), (n.value * 6,)).view(GENOTYPE_ENTRY).copy() if n.value else np.zeros(0, GENOTYPE_ENTRY)
        finally:
            lib.dg_free(ptr)
        return (off, entries, best.value) if called is None else (off, entries, best.value, levels)

    def dp_genotype_stats(self):
        """of the last dp_genotype_margins / dp_genotype_table on this context: dict(n_segments, levels_twice, peak_bytes, launches,
        entries, staging_copies); the last two are 0 after dp_genotype_margins"""
        out = np.zeros(6, np.int64)
        _check(lib.dg_dp_get_genotype_stats(self.h, out.ctypes.data, 6), "dg_dp_get_genotype_stats")
        return dict(zip(("n_segments", "levels_twice", "peak_bytes", "launches", "entries", "staging_copies"), out.tolist()))

    def dp_genotype_pin_stats(self):
        """of the last dp_genotype_margins(_pinned) / dp_genotype_table(_pinned) on this context: dict(pins, mask_launches), both 0
        after an unpinned call"""
        out = np.zeros(8, np.int64)
        _check(lib.dg_dp_get_genotype_stats(self.h, out.ctypes.data, 8), "dg_dp_get_genotype_stats")
        return dict(pins=int(out[6]), mask_launches=int(out[7]))

    def dp_phase_margins(self, called, budget, vertex_class=None):
        """Phase margins: cis against trans for every pair of neighbouring het levels of one called pair.  called: int32
        [2, n_levels], one cell per level, every id inside its level -- the two rows of dp_answer_paths are such a pair; budget >= 0;
        vertex_class as for dp_genotype_margins.  A level is het where the classes of its two called vertices differ.  Returns
        (records, best_value): a PHASE_MARGIN record array, one per pair of neighbouring het levels (level_a < level_b), ascending
        (empty with fewer than two het levels), and the best value of any pair within the budget.  cis_value: the best value of any
        ordered pair of paths within the budget that has the called ordered classes at both levels; trans_value: the same with the
        classes at level_a swapped; cis_vertex1/2, trans_vertex1/2: the cells of level_a that attain them; NEG_INF and -1 where there
        is none.  cis_value - trans_value is the phase margin of the two sites.  Leaves the last run's answers and what
        dp_genotype_stats reports alone."""
        p = np.ascontiguousarray(called, np.int32)
        g = getattr(self, "_g", None)                      # (no graph loaded: the library answers DG_ERR_STATE)
        if p.ndim != 2 or p.shape[0] != 2 or (g is not None and p.shape[1] != g.n_levels):
            raise ValueError(f"called must have shape [2, n_levels], got {p.shape}")
        cls = None
        if vertex_class is not None:
            cls = np.ascontiguousarray(vertex_class, np.int32)
            if g is not None and cls.shape != (g.n_vertices,):
                raise ValueError(f"vertex_class must have shape [{g.n_vertices}], got {cls.shape}")
        records = np.zeros(max(p.shape[1] - 1, 1), PHASE_MARGIN)
        n, best = C.c_int64(0), C.c_int32(0)
        _check(lib.dg_dp_phase_margins(self.h, p.ctypes.data if p.size else None, int(budget), cls.ctypes.data if cls is not None else None, records.ctypes.data,
                                       C.byref(n), C.byref(best)), "dg_dp_phase_margins")
        return records[:n.value].copy(), best.value

    def dp_phase_stats(self):
        """of the last dp_phase_margins on this context: dict(het_levels, records, seeded_launches, readout_launches, segments,
        peak_bytes)"""
        out = np.zeros(6, np.int64)
        _check(lib.dg_dp_get_phase_stats(self.h, out.ctypes.data, 6), "dg_dp_get_phase_stats")
        return dict(zip(("het_levels", "records", "seeded_launches", "readout_launches", "segments", "peak_bytes"), out.tolist()))

    def dp_phase_margins_budgets(self, called, budgets, vertex_class=None):
        """dp_phase_margins for many called pairs, each at a budget of its own, from one joint pass at the largest of them.  called:
        int32 [n, 2, n_levels]; budgets: n integers >= 0, in any order, repeats allowed; vertex_class as for dp_genotype_margins.
        Returns (records, best_values): a list of n PHASE_MARGIN record arrays, query q exactly what dp_phase_margins(called[q],
        budgets[q], vertex_class) answers (empty with fewer than two het levels), and int32 [n]: the best value of any pair within
        budgets[q].  Queries whose seeded states coincide -- the same ordered classes at the same het level -- share them on the
        device.  At most 256 queries.  Leaves the last run's answers and what dp_phase_stats / dp_genotype_stats report alone."""
        p = np.ascontiguousarray(called, np.int32)
        b = np.ascontiguousarray(budgets, np.int32)
        g = getattr(self, "_g", None)                      # (no graph loaded: the library answers DG_ERR_STATE)
        if p.ndim != 3 or p.shape[1] != 2 or (g is not None and p.shape[2] != g.n_levels):
            raise ValueError(f"called must have shape [n, 2, n_levels], got {p.shape}")
        if b.shape != (p.shape[0],):
            raise ValueError(f"budgets must have shape [{p.shape[0]}], got {b.shape}")
        cls = None
        if vertex_class is not None:
            cls = np.ascontiguousarray(vertex_class, np.int32)
            if g is not None and cls.shape != (g.n_vertices,):
                raise ValueError(f"vertex_class must have shape [{g.n_vertices}], got {cls.shape}")
        n = p.shape[0]
        records = np.zeros(max(n * max(p.shape[2] - 1, 0), 1), PHASE_MARGIN)
        off = np.zeros(n + 1, np.int64)
        best = np.zeros(n, np.int32)
        _check(lib.dg_dp_phase_margins_budgets(self.h, p.ctypes.data if p.size else None, b.ctypes.data if b.size else None, n, cls.ctypes.data if cls is not None else None,
                                               records.ctypes.data, off.ctypes.data, best.ctypes.data if best.size else None), "dg_dp_phase_margins_budgets")
        return [records[off[q]:off[q + 1]].copy() for q in range(n)], best

    PHASE_BUDGET_STATS = ("queries", "records", "seed_keys", "slot_levels", "backward_launches", "readout_launches", "max_live_slots", "slots_allocated", "segments", "peak_bytes")

    def dp_phase_budget_stats(self):
        """of the last dp_phase_margins_budgets on this context: dict(queries, records, seed_keys, slot_levels, backward_launches,
        readout_launches, max_live_slots, slots_allocated, segments, peak_bytes)"""
        out = np.zeros(10, np.int64)
        _check(lib.dg_dp_get_phase_budget_stats(self.h, out.ctypes.data, 10), "dg_dp_get_phase_budget_stats")
        return dict(zip(self.PHASE_BUDGET_STATS, out.tolist()))

    def dp_recombination_margins(self, budget, called=None):
        """Recombination margins: what a crossover at each transition is worth.  budget >= 0; called: None or int32 [n, 2, n_levels]
        (n <= 256), one cell per level and row, every id inside its level -- the two rows of dp_answer_paths are such a pair.  Returns
        (records, called_out, best_value): a RECOMBINATION_MARGIN record array, one per transition level -> level + 1: value[s] is the
        best value of any ordered pair of paths within the budget whose two hops of that transition weigh s together (s = 0, 1, 2),
        from1/from2 -> to1/to2 the hop pair that attains it (among equals the smallest positions, in that order), NEG_INF and -1
        where there is none; called_out: None without called, else int32 [n, n_levels - 1, 2] = (s_called, called_value): the weights
        of the two called hops summed (-1 if either is no edge) and the best value of any pair that takes exactly them (NEG_INF if
        none does); best_value: that of any pair within the budget, the largest of value[.] at every transition.  Leaves the last
        run's answers and what the other statistics report alone."""
        g = getattr(self, "_g", None)                      # (no graph loaded: the library answers DG_ERR_STATE)
        p = None
        if called is not None:
            p = np.ascontiguousarray(called, np.int32)
            if p.ndim != 3 or p.shape[1] != 2 or (g is not None and p.shape[2] != g.n_levels):
                raise ValueError(f"called must have shape [n, 2, n_levels], got {p.shape}")
        n = 0 if p is None else p.shape[0]
        n_levels = g.n_levels if g is not None else (p.shape[2] if p is not None else 2)
        records = np.zeros(max(n_levels - 1, 1), RECOMBINATION_MARGIN)
        out = np.zeros((n, max(n_levels - 1, 0), 2), np.int32)
        best = C.c_int32(0)
        _check(lib.dg_dp_recombination_margins(self.h, int(budget), p.ctypes.data if n and p.size else None, n, records.ctypes.data, out.ctypes.data if out.size else None,
                                               C.byref(best)), "dg_dp_recombination_margins")
        return records[:n_levels - 1], (out if called is not None else None), best.value

    RECOMBINATION_STATS = ("transitions", "edge_launches", "finish_launches", "segments", "levels_twice", "peak_bytes", "launches")

    def dp_recombination_stats(self):
        """of the last dp_recombination_margins on this context: dict(transitions, edge_launches, finish_launches, segments,
        levels_twice, peak_bytes, launches)"""
        out = np.zeros(7, np.int64)
        _check(lib.dg_dp_get_recombination_stats(self.h, out.ctypes.data, 7), "dg_dp_get_recombination_stats")
        return dict(zip(self.RECOMBINATION_STATS, out.tolist()))

    def dp_recombination_margins_budgets(self, budgets, called=None):
        """dp_recombination_margins for every listed budget from one joint pass at the largest of them.  budgets: n integers >= 0
        (1 <= n <= 256), in any order, repeats allowed; called: None or int32 [n, 2, n_levels], the pair of cells per level of query q.
        Returns (records, called_out, best_values): a RECOMBINATION_MARGIN record array [n, n_levels - 1], called_out int32
        [n, n_levels - 1, 2] (None without called) and int32 [n]; query q is exactly what dp_recombination_margins(budgets[q],
        called[q:q + 1]) answers, s_called and called_value at its own budget, best_values[q] the best value of any pair within
        budgets[q].  Queries of one budget share one set of records, computed once.  Leaves the last run's answers and what every
        other statistics call reports alone."""
        b = np.ascontiguousarray(budgets, np.int32).reshape(-1)
        n = b.shape[0]
        g = getattr(self, "_g", None)                      # (no graph loaded: the library answers DG_ERR_STATE)
        p = None
        if called is not None:
            p = np.ascontiguousarray(called, np.int32)
            if p.ndim != 3 or p.shape[0] != n or p.shape[1] != 2 or (g is not None and p.shape[2] != g.n_levels):
                raise ValueError(f"called must have shape [{n}, 2, n_levels], got {p.shape}")
        n_levels = g.n_levels if g is not None else (p.shape[2] if p is not None else 2)
        T = max(n_levels - 1, 0)
        records = np.zeros((max(n, 1), max(T, 1)), RECOMBINATION_MARGIN)
        out = np.zeros((max(n, 1), max(T, 1), 2), np.int32)
        best = np.zeros(max(n, 1), np.int32)
        _check(lib.dg_dp_recombination_margins_budgets(self.h, b.ctypes.data if n else None, n, p.ctypes.data if p is not None and p.size else None, records.ctypes.data,
                                                       out.ctypes.data, best.ctypes.data), "dg_dp_recombination_margins_budgets")
        return records[:n, :T], (out[:n, :T] if called is not None else None), best[:n]

    RECOMBINATION_BUDGET_STATS = ("queries", "distinct_budgets", "transitions", "edge_launches", "finish_launches", "segments", "levels_twice", "peak_bytes", "launches")

    def dp_recombination_budget_stats(self):
        """of the last dp_recombination_margins_budgets on this context: dict(queries, distinct_budgets, transitions, edge_launches,
        finish_launches, segments, levels_twice, peak_bytes, launches)"""
        out = np.zeros(9, np.int64)
        _check(lib.dg_dp_get_recombination_budget_stats(self.h, out.ctypes.data, 9), "dg_dp_get_recombination_budget_stats")
        return dict(zip(self.RECOMBINATION_BUDGET_STATS, out.tolist()))

    def dp_objective_paths(self, paths):
        """paths: int32 [n, 2, n_levels], as for dp_score_paths.  Returns a PAIR_OBJECTIVE record array of n entries: the hom colours
        both paths cover (hom_shared) and exactly one covers (hom_single), the het colours exactly one covers (het_single) and both
        cover (het_both), every colour counted once per path; the objective is hom_shared + het_single.  A vertex outside its
        level or a hop without an edge raises DgError naming the first offending pair, path and level.  Leaves the last run's
        answers alone."""
        p = np.ascontiguousarray(paths, np.int32)
        g = getattr(self, "_g", None)                      # (no graph loaded: the library answers DG_ERR_STATE)
        if p.ndim != 3 or p.shape[1] != 2 or (g is not None and p.shape[2] != g.n_levels):
            raise ValueError(f"paths must have shape [n, 2, n_levels], got {p.shape}")
        out = np.zeros(p.shape[0], PAIR_OBJECTIVE)
        _check(lib.dg_dp_objective_paths(self.h, p.ctypes.data if p.size else None, p.shape[0], out.ctypes.data if out.size else None), "dg_dp_objective_paths")
        return out

    def dp_answer_objectives(self, budgets):
        """the PAIR_OBJECTIVE records of the pairs of paths the last dp_run / dp_run_budgets walked for `budgets` (each one the run
        read out), without the paths leaving the device; all four fields are -1 where no pair fits the budget.  Leaves the run's
        answers alone."""
        b = np.ascontiguousarray(budgets, np.int32).reshape(-1)
        out = np.zeros(b.size, PAIR_OBJECTIVE)
        _check(lib.dg_dp_answer_objectives(self.h, b.ctypes.data if b.size else None, b.size, out.ctypes.data if out.size else None), "dg_dp_answer_objectives")
        return out

    def dp_solve(self, g):
        self.dp_load_graph(g)
        return self.dp_run()

    def dp_solve_haploid(self, R, out_off, out_dst, out_w, n_colours):
        """haploid (vertex, r) DP: returns dp, back_vtx, back_r as [n, R+1] int32 arrays"""
        out_off = np.ascontiguousarray(out_off, np.int64); out_dst = np.ascontiguousarray(out_dst, np.int32)
        out_w = np.ascontiguousarray(out_w, np.uint8); n_colours = np.ascontiguousarray(n_colours, np.int32)
        n = out_off.size - 1
        g = HapGraph(n, R, out_off.ctypes.data, out_dst.ctypes.data if out_dst.size else 0, out_w.ctypes.data if out_w.size else 0, n_colours.ctypes.data)
        arrs = [np.zeros((n, R + 1), np.int32) for _ in range(3)]
        _check(lib.dg_dp_solve_haploid(self.h, C.byref(g), *(a.ctypes.data for a in arrs)), "dg_dp_solve_haploid")
        return arrs

    def dp_timing(self):
        t = DpTiming()
        _check(lib.dg_dp_get_timing(self.h, C.byref(t)), "dg_dp_get_timing")
        return t

    def dp_launch_profile(self):
        """{kernel variant: launches} of the last dp_run"""
        buf = C.create_string_buffer(8192)
        _check(lib.dg_dp_get_launch_profile(self.h, buf, 8192), "dg_dp_get_launch_profile")
        return {k: int(v) for k, v in (item.rsplit(":", 1) for item in buf.value.decode().split())}

    def dp_pair_profile(self):
        """{pair kernel variant: launches} of the last dp_run: launches that swept two adjacent levels at once (not in dp_launch_profile)"""
        buf = C.create_string_buffer(1024)
        _check(lib.dg_dp_get_pair_profile(self.h, buf, 1024), "dg_dp_get_pair_profile")
        return {k: int(v) for k, v in (item.rsplit(":", 1) for item in buf.value.decode().split())}

    @staticmethod
    def dp_pair_variants():
        """the names of every pair kernel the library can launch, in dp_pair_profile's order (needs no device)"""
        buf = C.create_string_buffer(1024)
        _check(lib.dg_dp_list_pair_variants(buf, 1024), "dg_dp_list_pair_variants")
        return buf.value.decode().split()

    @staticmethod
    def dp_sweep_variants():
        """the names of every sweep kernel variant the library can launch, in dp_launch_profile's order (needs no device)"""
        buf = C.create_string_buffer(8192)
        _check(lib.dg_dp_list_sweep_variants(buf, 8192), "dg_dp_list_sweep_variants")
        return buf.value.decode().split()

    TABLES = ["descs", "in_off", "in_edge", "in_dst", "dtrans", "dblk_first", "grp_begin", "dead_cols", "heavy_rows", "rowrec", "rowx", "slots"]

    def dp_table_digest(self):
        """{table: FNV-1a digest} of the tables dg_dp_load_graph built for the resident graph"""
        out = np.zeros(12, np.uint64)
        _check(lib.dg_dp_get_table_digest(self.h, out.ctypes.data, 12), "dg_dp_get_table_digest")
        return dict(zip(self.TABLES, (int(x) for x in out)))

    def dp_level_digest(self, n_levels):
        out = np.zeros(n_levels, np.uint64)
        _check(lib.dg_dp_get_level_digest(self.h, out.ctypes.data, n_levels), "dg_dp_get_level_digest")
        return out

    # ---- sketch ----
    def sketch_reads(self, reads, k, w):
        """reads: list of bytes. Returns (sorted distinct hashes uint64[], n_reads_with_hash int32[])."""
        bases = b"".join(reads)
        off = np.zeros(len(reads) + 1, np.int64)
        np.cumsum([len(r) for r in reads], out=off[1:])
        return self.sketch_reads_flat(bases, off, k, w)

    def sketch_reads_flat(self, bases, off, k, w):
        hp, cp, n = C.c_void_p(), C.c_void_p(), C.c_int64()
        off = np.ascontiguousarray(off, np.int64)
        _check(lib.dg_sketch_reads(self.h, bases, off.ctypes.data, off.size - 1, k, w, C.byref(hp), C.byref(cp), C.byref(n)),
               "dg_sketch_reads")
        h = np.ctypeslib.as_array(C.cast(hp, C.POINTER(C.c_uint64)), (n.value,)).copy() if n.value else np.zeros(0, np.uint64)
        c = np.ctypeslib.as_array(C.cast(cp, C.POINTER(C.c_int32)), (n.value,)).copy() if n.value else np.zeros(0, np.int32)
        lib.dg_free(hp)
        lib.dg_free(cp)
        return h, c

    def sketch_haplotype(self, seq, k, w):
        hp, pp, n = C.c_void_p(), C.c_void_p(), C.c_int64()
        _check(lib.dg_sketch_haplotype(self.h, seq, len(seq), k, w, C.byref(hp), C.byref(pp), C.byref(n)), "dg_sketch_haplotype")
        h = np.ctypeslib.as_array(C.cast(hp, C.POINTER(C.c_uint64)), (n.value,)).copy() if n.value else np.zeros(0, np.uint64)
        p = np.ctypeslib.as_array(C.cast(pp, C.POINTER(C.c_int64)), (n.value,)).copy() if n.value else np.zeros(0, np.int64)
        lib.dg_free(hp)
        lib.dg_free(pp)
        return h, p

    def sketch_tag_reads(self, reads, k, w, hash_a, hash_b):
        """reads: list of bytes; hash_a, hash_b: uint64 lists (any order, duplicates allowed, may be empty).  Returns int32[n_reads, 4]:
        per read n_min, only_a, only_b, both (ReadTag)."""
        bases = b"".join(reads)
        off = np.zeros(len(reads) + 1, np.int64)
        np.cumsum([len(r) for r in reads], out=off[1:])
        return self.sketch_tag_reads_flat(bases, off, k, w, hash_a, hash_b)

    def sketch_tag_reads_flat(self, bases, off, k, w, hash_a, hash_b):
        off = np.ascontiguousarray(off, np.int64)
        ha = np.ascontiguousarray(hash_a, np.uint64).ravel()
        hb = np.ascontiguousarray(hash_b, np.uint64).ravel()
        out = np.zeros((off.size - 1, 4), np.int32)                    # one ReadTag per row
        _check(lib.dg_sketch_tag_reads(self.h, bases, off.ctypes.data, off.size - 1, k, w, ha.ctypes.data if ha.size else None, ha.size,
                                       hb.ctypes.data if hb.size else None, hb.size, out.ctypes.data), "dg_sketch_tag_reads")
        return out

    def hash_kmers(self, kmers, k):
        n = len(kmers) // k if k > 0 else 0          # (k outside 1..255 is the library's to reject)
        out = np.zeros(n, np.uint64)
        _check(lib.dg_hash_kmers(self.h, kmers, n, k, out.ctypes.data), "dg_hash_kmers")
        return out

    # ---- anchors ----
    def anchor_begin(self, n_haps, n_vertices, top_order_map, k, w):
        top = np.ascontiguousarray(top_order_map, np.int32)
        _check(lib.dg_anchor_begin(self.h, n_haps, n_vertices, top.ctypes.data if top.size else None, k, w), "dg_anchor_begin")

    @staticmethod
    def _steps(step_vtx, step_start):
        sv = np.ascontiguousarray(step_vtx, np.int32)
        ss = np.ascontiguousarray(step_start, np.int64)
        if ss.size != sv.size + 1:
            raise ValueError("step_start needs one entry more than step_vtx")
        return sv if sv.size else np.zeros(1, np.int32), ss, sv.size      # (a non-NULL pointer for a haplotype of zero steps)

    def anchor_add_haplotype(self, h, seq, step_vtx, step_start):
        """haplotype h (bytes) with its walk: step s is vertex step_vtx[s] over bases [step_start[s], step_start[s + 1]).
        Returns the minimizer count."""
        sv, ss, n_steps = self._steps(step_vtx, step_start)
        n = C.c_int64()
        _check(lib.dg_anchor_add_haplotype(self.h, h, seq, len(seq), sv.ctypes.data, ss.ctypes.data, n_steps, C.byref(n)), "dg_anchor_add_haplotype")
        return n.value

    def anchor_add_haplotype_sketched(self, h, length, hash, pos, step_vtx, step_start):
        """the same for a minimizer list computed elsewhere (sketch_haplotype's output)"""
        sv, ss, n_steps = self._steps(step_vtx, step_start)
        hs = np.ascontiguousarray(hash, np.uint64)
        ps = np.ascontiguousarray(pos, np.int64)
        if hs.size != ps.size:
            raise ValueError("hash and pos differ in length")
        _check(lib.dg_anchor_add_haplotype_sketched(self.h, h, length, hs.ctypes.data if hs.size else None, ps.ctypes.data if ps.size else None, hs.size,
                                                    sv.ctypes.data, ss.ctypes.data, n_steps), "dg_anchor_add_haplotype_sketched")

    def anchor_finish(self, sp_hash, min_shared):
        """join with the sorted read spectrum, filter, sort: dict of occ_id, occ_hap int32[n_occ], occ_off, occ_len uint32[n_occ],
        vpool int32[n_vtx] (Anchor_hits order) and the counters n_candidates, n_unstable_groups"""
        sp = np.ascontiguousarray(sp_hash, np.uint64)
        res = AnchorResult()
        try:
            _check(lib.dg_anchor_finish(self.h, sp.ctypes.data if sp.size else None, sp.size, float(min_shared), C.byref(res)), "dg_anchor_finish")
            def arr(p, ct, dt, n):
                return np.ctypeslib.as_array(C.cast(p, C.POINTER(ct)), (n,)).astype(dt, copy=True) if n and p else np.zeros(0, dt)
            return dict(occ_id=arr(res.occ_id, C.c_int32, np.int32, res.n_occ), occ_hap=arr(res.occ_hap, C.c_int32, np.int32, res.n_occ),
                        occ_off=arr(res.occ_off, C.c_uint32, np.uint32, res.n_occ), occ_len=arr(res.occ_len, C.c_uint32, np.uint32, res.n_occ),
                        vpool=arr(res.vpool, C.c_int32, np.int32, res.n_vtx), n_candidates=res.n_candidates, n_unstable_groups=res.n_unstable_groups)
        finally:
            for p in (res.occ_id, res.occ_hap, res.occ_off, res.occ_len, res.vpool):
                if p:
                    lib.dg_free(p)

    def sketch_set_option(self, name, value):
        _check(lib.dg_sketch_set_option(self.h, name.encode(), int(value)), "dg_sketch_set_option")

    def sketch_get_option(self, name):
        v = C.c_int64(0)
        _check(lib.dg_sketch_get_option(self.h, name.encode(), C.byref(v)), "dg_sketch_get_option")
        return v.value

    def sketch_options(self, **kv):
        """with ctx.sketch_options(spectrum_mode=1, ...): the given sketch options for the body, then the values they had before"""
        return _options(self.sketch_get_option, self.sketch_set_option, kv)

    def sketch_stat(self, name):
        v = C.c_int64(0)
        _check(lib.dg_sketch_get_stat(self.h, name.encode(), C.byref(v)), "dg_sketch_get_stat")
        return v.value

    def sketch_timing(self):
        t = SketchTiming()
        _check(lib.dg_sketch_get_timing(self.h, C.byref(t)), "dg_sketch_get_timing")
        return t

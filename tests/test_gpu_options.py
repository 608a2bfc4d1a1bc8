"""-m gpu: the option tables of the DP and of the sketch stage -- the getters, the setters' clamps, and Context.dp_options /
Context.sketch_options, which put back what they found.  DP_DEFAULTS is the ABI pin of the defaults, the only table of them in the tests."""
import os

import numpy as np
import pytest

import oracle_py as orc
from dipgenie_amd import capi

pytestmark = pytest.mark.gpu

DP_DEFAULTS = {
    "digest": 0, "fast": 1, "adaptive_rc": 1, "coop": 1, "rowx": 1, "lean_chain": 1, "graph_batch": -1, "l2_prefetch": 6, "pf_far": 128,
    "delta_overlap": 1, "warm_ahead": 128, "segment_cells": 0, "lattice_chunk_cells": 4 << 30, "delta_cap_entries": 4 << 30, "plane_limit": 1,
    "sync_every": 0, "side_stream": -1, "test_poison_level": 0, "test_poison_byte": 0xFF, "test_force_rc": 0, "score_slab_bytes": 256 << 20,
    "partner_slab_bytes": 4 << 30, "host_tables": 0, "rc_t0_ns": 3000, "rc_tg_ps": 20000, "rc_tw_ps": 50, "rc_cap": 65536,
    "bp_nt_min_cells": 262144, "max_blocks": 1024, "host_threads": 16, "pair_digest": 0, "test_force_pair_rc": 0,
}
NONPOSITIVE_IS_DEFAULT = ["delta_cap_entries", "rc_cap", "max_blocks", "score_slab_bytes", "partner_slab_bytes"]
LOWER_CLAMP = {"graph_batch": -1, "side_stream": -1, "host_threads": 1}          # every other clamped key: 0
SKETCH_DEFAULTS = dict.fromkeys(["spectrum_mode", "bucket_bits", "bucket_stride", "spill_cap", "residual_cap", "host_buckets"], 0)


@pytest.fixture
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _dp(c):
    return {k: c.dp_get_option(k) for k in DP_DEFAULTS}


def _sketch(c):
    return {k: c.sketch_get_option(k) for k in SKETCH_DEFAULTS}


def test_defaults_are_pinned_once(ctx):
    assert _dp(ctx) == DP_DEFAULTS and _sketch(ctx) == SKETCH_DEFAULTS
    for k in NONPOSITIVE_IS_DEFAULT:
        for v in (7, 0, 9, -5):
            ctx.dp_set_option(k, v)
            assert ctx.dp_get_option(k) == (v if v > 0 else DP_DEFAULTS[k]), (k, v)
    for k in set(DP_DEFAULTS) - set(NONPOSITIVE_IS_DEFAULT) - {"lattice_chunk_cells"}:
        ctx.dp_set_option(k, LOWER_CLAMP.get(k, 0) - 3)
        assert ctx.dp_get_option(k) == LOWER_CLAMP.get(k, 0), k
        ctx.dp_set_option(k, DP_DEFAULTS[k])
    ctx.dp_set_option("lattice_chunk_cells", 3001)
    assert ctx.dp_get_option("lattice_chunk_cells") == 3002
    with pytest.raises(capi.DgError, match="rc=-1.*lattice_chunk_cells must be positive"):
        ctx.dp_set_option("lattice_chunk_cells", 0)
    assert ctx.dp_get_option("lattice_chunk_cells") == 3002
    ctx.dp_set_option("lattice_chunk_cells", DP_DEFAULTS["lattice_chunk_cells"])
    assert _dp(ctx) == DP_DEFAULTS
    for call in (lambda: ctx.dp_set_option("sym", 1), lambda: ctx.dp_get_option("sym"), lambda: ctx.sketch_set_option("sym", 1), lambda: ctx.sketch_get_option("sym")):
        with pytest.raises(capi.DgError, match="rc=-1.*unknown option '?sym"):
            call()


def test_options_are_restored_on_error(ctx):
    g = capi.DpGraphArrays.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "toy1_k5w3_R2.dpg"))
    ref = orc.dp_solve(g)
    changed = dict(fast=0, graph_batch=0, lattice_chunk_cells=3000, score_slab_bytes=1, test_force_rc=4)
    with pytest.raises(RuntimeError, match="boom"):
        with ctx.dp_options(**changed):
            assert _dp(ctx) == {**DP_DEFAULTS, **changed}
            ctx.dp_solve(g)
            raise RuntimeError("boom")
    assert _dp(ctx) == DP_DEFAULTS
    out = ctx.dp_solve(g)
    assert (out.value, out.s_het, out.p1, out.p2) == (ref["value"], ref["s_het"], ref["p1"], ref["p2"])
    with pytest.raises(capi.DgError, match="must be positive"), ctx.dp_options(fast=0, lattice_chunk_cells=0):   # a refused value: what was set before it is put back
        pass
    assert _dp(ctx) == DP_DEFAULTS
    rng = np.random.default_rng(0)
    reads = [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 150).tobytes()) for _ in range(256)]
    ho, co = orc.sketch_reads(reads, 31, 25)
    with pytest.raises(RuntimeError, match="boom"):
        with ctx.sketch_options(spectrum_mode=1, spill_cap=100):
            assert _sketch(ctx) == {**SKETCH_DEFAULTS, "spectrum_mode": 1, "spill_cap": 100}
            ctx.sketch_reads(reads, 31, 25)
            raise RuntimeError("boom")
    assert _sketch(ctx) == SKETCH_DEFAULTS
    h, c = ctx.sketch_reads(reads, 31, 25)
    assert np.array_equal(h, ho) and np.array_equal(c, co)


def test_nested_managers_restore_the_outer_value(ctx):
    with ctx.dp_options(graph_batch=7, segment_cells=5000, test_force_rc=3):
        with ctx.dp_options(graph_batch=0, lattice_chunk_cells=3000, test_force_rc=16):
            assert _dp(ctx) == {**DP_DEFAULTS, "graph_batch": 0, "segment_cells": 5000, "lattice_chunk_cells": 3000, "test_force_rc": 16}
        assert _dp(ctx) == {**DP_DEFAULTS, "graph_batch": 7, "segment_cells": 5000, "test_force_rc": 3}
    assert _dp(ctx) == DP_DEFAULTS
    with ctx.sketch_options(bucket_bits=9, bucket_stride=256):
        with ctx.sketch_options(bucket_bits=3, spill_cap=-1):
            assert _sketch(ctx) == {**SKETCH_DEFAULTS, "bucket_bits": 3, "bucket_stride": 256, "spill_cap": -1}
        assert _sketch(ctx) == {**SKETCH_DEFAULTS, "bucket_bits": 9, "bucket_stride": 256}
    assert _sketch(ctx) == SKETCH_DEFAULTS


def test_force_rc_zero_changes_no_launch(ctx):
    """test_force_rc = 0, set explicitly and after a forced run: the recorded launch profiles (golden/launch_profiles.json) of the eight
    graphs under default options; a forced chunk size in between does change them, and one that is no candidate runs the all-planes chunk"""
    import json
    import test_gpu_sweep_variants as sw
    want = json.load(open(sw.GOLDEN))
    for q, make in enumerate(sw.GRAPHS):
        g = make()
        with ctx.dp_options(test_force_rc=0):
            ctx.dp_solve(g)
            assert sw._profile_text(ctx) == want[f"graph{q}"], q
        if q in (0, 2):                                                     # R + 1 = 19 and 8: all-planes chunks 19 and 8
            with ctx.dp_options(test_force_rc=2, coop=0):
                ctx.dp_solve(g)
                assert set(ctx.dp_launch_profile()) <= {"dp_sweep_fast_kernel<2,lean>", "dp_sweep_fast_kernel<2,general>"}, q
            for n in (7, 33, 1000):                                         # not in the table / above the run's all-planes chunk
                with ctx.dp_options(test_force_rc=n):
                    ctx.dp_solve(g)
                    assert sw._profile_text(ctx) == want[f"graph{q} adaptive_rc=0"], (q, n)
            ctx.dp_solve(g)
            assert sw._profile_text(ctx) == want[f"graph{q}"], q

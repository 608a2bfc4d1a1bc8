"""-m gpu: which sweep kernel variant the host launches for every level, and what a run leaves in the caller's options.
golden/launch_profiles.json holds dg_dp_get_launch_profile of the commit before the variants were described by one table
(dg_dp_sweep.hip: SWEEP_RCS, SweepVariant): the RC choice, the dispatch and the printed names must still give the same strings.
Recorded by this module itself: DG_RECORD_LAUNCH_PROFILES=<output file> (with DG_LIB naming the library to record from) writes
the file instead of comparing."""
import json
import os
import re

import numpy as np
import pytest

import graphgen
import oracle_py as orc
from dipgenie_amd import capi
from test_gpu_parity import _fan_in_graph

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_profiles.json")
RECORD_TO = os.environ.get("DG_RECORD_LAUNCH_PROFILES")

GRAPHS = [
    lambda: graphgen.random_levelized(7000 + 2, max_width=40, n_levels=60, R=18, p_w1=0.5),
    lambda: graphgen.random_levelized(7100 + 6, max_width=60, n_levels=40, R=32, p_w1=0.6),
    lambda: graphgen.random_levelized(9700 + 17, min_width=15, max_width=18, n_levels=40, R=7, p_colour=0.6),
    lambda: graphgen.random_levelized(9700 + 19, min_width=120, max_width=200, n_levels=6, R=5, p_colour=0.3, extra_edges=0.5),
    lambda: graphgen.random_levelized(9100 + 12, max_width=3, n_levels=6, R=1, extra_edges=300.0, dup_edges=False),   # in-degree > 255: generic kernel
    lambda: _fan_in_graph(90),
    # wide levels of very different sizes: the six graphs above are small enough for RC = 1 nearly everywhere, these two reach RC 2, 3, 4, 5, 10, 11
    lambda: graphgen.random_levelized(9900 + 3, min_width=30, max_width=300, n_levels=12, R=18, p_w1=0.5, extra_edges=0.5),
    lambda: graphgen.random_levelized(9900 + 4, min_width=30, max_width=300, n_levels=12, R=32, p_w1=0.5, extra_edges=0.5),
]
OPTION_SETS = [{}, {"adaptive_rc": 0}, {"coop": 0}, {"coop": 2}, {"fast": 0}]
# (graph, options): every graph under every option set, and the first graph in segments, where pass 2 sweeps fewer planes
CASES = [(q, o) for q in range(len(GRAPHS)) for o in OPTION_SETS] + [(0, {"segment_cells": 5000, "plane_limit": p}) for p in (1, 0)]


def _case_name(q, opts):
    return f"graph{q}" + "".join(f" {k}={v}" for k, v in opts.items())


def _profile_text(ctx):
    return " ".join(f"{k}:{n}" for k, n in ctx.dp_launch_profile().items())     # the C string again: same items, same order


def test_launch_profiles_equal_the_recorded_ones(gpu_ctx):
    graphs = [make() for make in GRAPHS]
    refs = [orc.dp_solve(g) for g in graphs]                                # whatever was launched, the answer is the oracle's
    got, all_planes = {}, {}
    for q, opts in CASES:
        with gpu_ctx.dp_options(**opts):
            out = gpu_ctx.dp_solve(graphs[q])
            got[_case_name(q, opts)] = _profile_text(gpu_ctx)
        assert (out.value, out.s_het, out.p1, out.p2) == (refs[q]["value"], refs[q]["s_het"], refs[q]["p1"], refs[q]["p2"]), _case_name(q, opts)
        all_planes[_case_name(q, opts)] = 8 if graphs[q].R + 1 <= 8 else 19 if graphs[q].R + 1 <= 19 else 33
    if RECORD_TO:
        with open(RECORD_TO, "w") as f:
            json.dump(got, f, indent=1)
            f.write("\n")
    want = json.load(open(RECORD_TO or GOLDEN))
    # the recorded set must itself reach every kind of variant, or a wrong table could hide behind it
    items = [(all_planes[name], item) for name, text in want.items() for item in text.split()]
    assert any("dp_sweep_coop_kernel<" in i for _, i in items) and any(",general>" in i for _, i in items)
    assert any(i.startswith("dp_sweep_kernel:") for _, i in items)
    for sel in (8, 19, 33):
        rcs = {int(m.group(1)) for s, i in items if s == sel for m in [re.match(r"dp_sweep_fast_kernel<(\d+),", i)] if m}
        assert len(rcs) >= 4, (sel, sorted(rcs))
    for name in got:
        print(f"{name}: {got[name]}")
        assert got[name] == want[name], name
    assert list(got) == list(want)


def test_a_run_leaves_the_callers_options_alone(gpu_ctx):
    """a segmented run (value-only pass with digests, then re-sweeps without them and below the path's plane), clean, with a
    poisoned lattice level (which may end in DG_ERR_STATE half way through pass 2) and clean again: the options read back as set"""
    g = graphgen.random_levelized(8000 + 12, max_width=45, n_levels=70, R=18, p_w1=0.5)
    ref = orc.dp_solve(g, want_digest=True)
    opts = dict(segment_cells=5000, digest=1, plane_limit=1)
    with gpu_ctx.dp_options(**opts):
        for poison in (0, 35, 0):
            with gpu_ctx.dp_options(test_poison_level=poison, test_poison_byte=0xFF):
                gpu_ctx.dp_load_graph(g)
                try:
                    out = gpu_ctx.dp_run()
                except capi.DgError as e:
                    assert poison and ("corrupt" in str(e) or "disagree" in str(e)), (poison, str(e))
                    out = None
                assert {k: gpu_ctx.dp_get_option(k) for k in opts} == opts, poison
                if not poison:
                    assert (out.value, out.s_het, out.p1, out.p2) == (ref["value"], ref["s_het"], ref["p1"], ref["p2"])
                    assert np.array_equal(gpu_ctx.dp_level_digest(g.n_levels)[1:], ref["digest"][1:])

"""-m gpu: every instantiated sweep kernel variant against the oracle, cell by cell.

The per-level choice of the chunk size (choose_rc, dg_dp_sweep.hip) is a cost model fitted to large levels: on graphs a test can
afford it picks RC = 1 nearly everywhere.  Option test_force_rc makes it consider one table entry only, so with coop = 0 | 2 a run
launches one (kernel, RC) on every level where that is a candidate, lean or general as the level demands.  For every graph of
sweep_variant_graphs.py and every (kernel, RC) of Context.dp_sweep_variants() that is a candidate at the graph's R + 1:
  digest = 1: value, s_het, both edge lists, cells, relaxations and EVERY level digest equal the oracle's;
  digest = 0 (the instantiations the product runs): value, s_het and the edge lists;
  both:       the sink's value on every plane 0..R against the oracle solved once per budget.
The launch profile of every run must be exactly what the graph's in-degrees and the targeted variant imply (so the targeted
variant ran, on every level that has its form, and nothing else did), and over the module the launched names must be all of
dp_sweep_variants(): a variant added to the table fails that line until a graph here reaches it.  All comparisons are integer
equality."""
import re

import numpy as np
import pytest

import sweep_variant_graphs as sv
from dipgenie_amd import capi

pytestmark = pytest.mark.gpu

VARIANTS = capi.Context.dp_sweep_variants()
GENERIC = "dp_sweep_kernel"
ALL_PLANES = (8, 19, 33)                                    # the all-planes chunks: the first that holds R + 1 planes is the run's
PARTIAL_ONLY_BELOW = {19, 33}                               # ... and these two are no partial chunk of a larger one
_LAUNCHED = set()                                           # names launched by the cases of this module, for the last test


def _target_of(name):
    """("generic", 0), ("fast", rc) or ("coop", rc): what a run can be made to launch; lean or general follows from the level"""
    m = re.fullmatch(r"dp_sweep_(fast|coop)_kernel<(\d+),(lean|general)>", name)
    assert m or name == GENERIC, name
    return (m.group(1), int(m.group(2))) if m else ("generic", 0)


TARGETS = list(dict.fromkeys(_target_of(name) for name in VARIANTS))          # in the list's order, each once


def _eligible(rc, R):
    rc_sel = next(a for a in ALL_PLANES if a >= R + 1)
    return rc == rc_sel or (rc < rc_sel and rc not in PARTIAL_ONLY_BELOW)


def _options(kernel, rc):
    return {"fast": 0} if kernel == "generic" else {"test_force_rc": rc, "coop": 2 if kernel == "coop" else 0}


def _expected_profile(g, kernel, rc):
    """one launch per destination level: general where a vertex has more than 64 in-edges, cooperative (if asked for) where one has more than 8"""
    want = {}
    for deg in sv.in_degrees(g):
        if kernel == "generic":
            name = GENERIC
        else:
            name = f"dp_sweep_{'coop' if kernel == 'coop' and deg.max() > 8 else 'fast'}_kernel<{rc},{'general' if deg.max() > 64 else 'lean'}>"
        want[name] = want.get(name, 0) + 1
    return want


def _check_profile(ctx, g, kernel, rc, passes=1):
    got = ctx.dp_launch_profile()
    want = {k: passes * n for k, n in _expected_profile(g, kernel, rc).items()}
    assert got == want, (kernel, rc, got, want)
    assert sum(got.values()) == passes * (g.n_levels - 1) and set(got) <= set(VARIANTS)
    assert any(_target_of(k) == (kernel, rc) for k in got), (kernel, rc, got)
    _LAUNCHED.update(got)


def _equals_the_oracle(ctx, g, out, ref, digests, what):
    assert (out.value, out.s_het) == (ref["value"], ref["s_het"]), what
    assert out.p1 == ref["p1"] and out.p2 == ref["p2"], what
    if digests:
        assert (out.cells, out.relaxations) == (ref["cells"], ref["relaxations"]), what
        got = ctx.dp_level_digest(g.n_levels)[1:]
        assert np.array_equal(got, ref["digest"][1:]), (what, "first level that differs", 1 + int(np.argmax(got != ref["digest"][1:])))


def test_the_variant_list_is_the_table(gpu_ctx):
    assert VARIANTS == gpu_ctx.dp_sweep_variants() and len(set(VARIANTS)) == len(VARIANTS) and VARIANTS[0] == GENERIC
    rcs = sorted({rc for k, rc in TARGETS if k == "fast"})
    assert set(ALL_PLANES) <= set(rcs) and rcs[-1] == ALL_PLANES[-1]
    for rc in rcs:                                          # index order: per chunk size lean, lean cooperative, general, general cooperative
        assert f"dp_sweep_fast_kernel<{rc},lean>" in VARIANTS and f"dp_sweep_fast_kernel<{rc},general>" in VARIANTS
    for k, rc in TARGETS:
        if k == "coop":
            q = VARIANTS.index(f"dp_sweep_fast_kernel<{rc},lean>")
            assert VARIANTS[q:q + 4] == [f"dp_sweep_fast_kernel<{rc},lean>", f"dp_sweep_coop_kernel<{rc},lean>", f"dp_sweep_fast_kernel<{rc},general>", f"dp_sweep_coop_kernel<{rc},general>"]
    buf = capi.C.create_string_buffer(16)
    assert capi.lib.dg_dp_list_sweep_variants(buf, 16) != 0 and b"too small" in capi.lib.dg_last_error()
    assert capi.lib.dg_dp_list_sweep_variants(None, 8192) != 0


def every_variant_equals_the_oracle(ctx, g, ref, planes, digest, case):
    """the variant loop: g under every (kernel, RC) that is a candidate at its R + 1, against the oracle's answer ref (with digests)
    and the oracle's sink value per budget 0..R (planes); tests/test_gpu_colour_lists.py runs its graphs through it as well"""
    n_run = 0
    for kernel, rc in TARGETS:
        if kernel != "generic" and not _eligible(rc, g.R):
            continue
        with ctx.dp_options(digest=digest, **_options(kernel, rc)):
            out = ctx.dp_solve(g)
            _equals_the_oracle(ctx, g, out, ref, digest, (case, kernel, rc))
            assert [int(v) for v in ctx.dp_budget_values()] == planes, (case, kernel, rc)
            _check_profile(ctx, g, kernel, rc)
        n_run += 1
    assert n_run >= 12, n_run                               # generic + at least RC 1..6, 8 fast + RC 1..4 cooperative


@pytest.mark.parametrize("digest", [1, 0])
@pytest.mark.parametrize("case", list(sv.GRAPHS))
def test_every_variant_equals_the_oracle(gpu_ctx, case, digest):
    every_variant_equals_the_oracle(gpu_ctx, sv.graph(case), sv.oracle(case), [r["value"] for r in sv.oracle_per_budget(case)], digest, case)


@pytest.mark.parametrize("case", ["lean-R18", "general-R18"])
def test_plane_limited_resweep(gpu_ctx, case):
    """segments whose path stays below a plane are swept again up to that plane only: the number of chunks then comes from the
    planes swept while the kernel bounds its planes by R + 1 -- at chunk sizes that divide neither"""
    g = sv.graph(case)
    ref = sv.oracle(case)
    for rc in (3, 6, 16):
        with gpu_ctx.dp_options(test_force_rc=rc, coop=0, segment_cells=max(1, int(ref["cells"]) // 7), plane_limit=1, digest=1):
            out = gpu_ctx.dp_solve(g)
            _equals_the_oracle(gpu_ctx, g, out, ref, True, (case, rc))
            assert gpu_ctx.dp_timing().n_segments > 1
            _check_profile(gpu_ctx, g, "fast", rc, passes=2)


def test_every_instantiated_variant_was_compared():
    """runs last in the module: the union of the launch profiles above is the whole list"""
    assert _LAUNCHED == set(VARIANTS), (sorted(set(VARIANTS) - _LAUNCHED), sorted(_LAUNCHED - set(VARIANTS)))
    assert len(VARIANTS) == 1 + sum(1 for k, _ in TARGETS if k != "generic") * 2

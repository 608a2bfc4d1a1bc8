"""GPU: dg_anchor_* at its entry points (span kernels, dictionary join, fingerprint filter and its exact fallback, the two
comparator sorts, the unstable-group detector) against the plain model of tests/anchor_model.py, on the seeded inputs of
tests/anchor_cases.py (whose properties tests/test_anchor_model.py checks on the CPU).  Every comparison is exact equality of the
five result arrays and the two counters.  Malformed input is only ever sent where the host-side validation stops it."""
import re

import numpy as np
import pytest

import anchor_cases as ac
import anchor_model as am
import oracle_py as orc
from dipgenie_amd import capi

pytestmark = pytest.mark.gpu

ARRAYS = ["occ_id", "occ_hap", "occ_len", "occ_off", "vpool"]


def run_device(ctx, case, sketched=True, seqs=None):
    ctx.anchor_begin(case["n_haps"], case["n_vertices"], case["top"], case["k"], case["w"])
    for h, (hs, ps, sv, ss) in enumerate(case["haps"]):
        if sketched:
            ctx.anchor_add_haplotype_sketched(h, int(ss[-1]), hs, ps, sv, ss)
        else:
            assert ctx.anchor_add_haplotype(h, seqs[h], sv, ss) == hs.size
    return ctx.anchor_finish(case["sp_hash"], case["min_shared"])


def run_model(case):
    return am.run(case["k"], case["top"], case["haps"], case["sp_hash"], case["min_shared"])


def assert_same(dev, mod):
    want = mod.arrays()
    for name in ARRAYS:
        got = dev[name]
        assert got.dtype == want[name].dtype and got.shape == want[name].shape, (name, got.shape, want[name].shape)
        bad = np.flatnonzero(got != want[name])
        assert bad.size == 0, f"{name}: first mismatch at {bad[0]}: device {got[bad[0]]}, model {want[name][bad[0]]} ({bad.size} in all)"
    assert dev["n_candidates"] == mod.n_candidates


def check(ctx, case):
    mod = run_model(case)
    assert mod.unstable == []
    dev = run_device(ctx, case)
    assert_same(dev, mod)
    assert dev["n_unstable_groups"] == 0
    return dev, mod


@pytest.fixture(scope="module")
def big():
    return ac.big_top()


# ---------------------------------------------------------------------------------------------------------------- spans
@pytest.mark.parametrize("variant", ac.SPAN_VARIANTS)
@pytest.mark.parametrize("k", [5, 31, 40])
def test_spans(gpu_ctx, k, variant):
    dev, mod = check(gpu_ctx, ac.span_case(k, variant))
    assert dev["occ_id"].size == mod.n_candidates                                 # min_shared = +inf: every span came back


# ------------------------------------------------------------------------------------------------------------ key order
def test_key_order(gpu_ctx, big):
    """n_vertices = 16,000,000 (a 64 MB top_order_map)"""
    check(gpu_ctx, ac.key_order_case(big))


# --------------------------------------------------------------------------------------------------- stability boundary
@pytest.mark.parametrize("where", ["start", "middle", "end"])
def test_group_of_16_is_stable_17_is_reported(gpu_ctx, big, where):
    check(gpu_ctx, ac.boundary_case(big, 16, where, "different"))
    case = ac.boundary_case(big, 17, where, "different")
    mod = run_model(case)
    dev = run_device(gpu_ctx, case)
    assert mod.unstable == [(1, 0)] and dev["n_unstable_groups"] >= 1
    keep = [q for q, o in enumerate(mod.occs) if (o[0], o[1]) != (1, 0)]          # the other groups are still the model's
    assert [(int(dev["occ_id"][q]), int(dev["occ_hap"][q]), dev["vpool"][dev["occ_off"][q]:dev["occ_off"][q] + dev["occ_len"][q]].tolist()) for q in keep] == \
        [mod.occs[q] for q in keep]
    assert dev["n_candidates"] == mod.n_candidates and dev["occ_id"].size == len(mod.occs)


@pytest.mark.parametrize("size,where,tie", [(17, "start", "identical"), (17, "middle", "identical"), (17, "end", "identical"), (17, "middle", "none"),
                                            (5000, "middle", "identical"), (5000, "end", "none")])
def test_large_groups_without_a_real_tie(gpu_ctx, big, size, where, tie):
    check(gpu_ctx, ac.boundary_case(big, size, where, tie))


# --------------------------------------------------------------------------------------------------------------- filter
@pytest.mark.parametrize("n_haps,min_shared", ac.FILTER_SETTINGS)
def test_filter(gpu_ctx, n_haps, min_shared):
    case, must_drop = ac.filter_case(n_haps, min_shared)
    dev, mod = check(gpu_ctx, case)
    assert mod.dropped == must_drop
    assert set(range(case["sp_hash"].size)) - set(dev["occ_id"].tolist()) >= must_drop
    assert set(dev["occ_id"].tolist()).isdisjoint(must_drop)


# ----------------------------------------------------------------------------------------------------------- join sizes
@pytest.mark.parametrize("n_sp", [1, 2, 3, 255, 256, 257, 65536, 65537])
def test_join_sizes(gpu_ctx, n_sp):
    case = ac.join_case(n_sp)
    case["min_shared"] = ac.INF
    dev, mod = check(gpu_ctx, case)
    assert {0, n_sp - 1} <= set(dev["occ_id"].tolist())
    case["min_shared"] = np.float32(2.0)
    check(gpu_ctx, case)


def test_empty_results(gpu_ctx):
    case = ac.join_case(0)                                                        # no spectrum
    dev, mod = check(gpu_ctx, case)
    assert dev["occ_id"].size == 0 and dev["vpool"].size == 0
    case = ac.join_case(257)                                                      # every id dropped
    case["min_shared"] = np.float32(1.0)
    dev, mod = check(gpu_ctx, case)
    assert dev["occ_id"].size == 0 and mod.n_candidates > 0
    sp = case["sp_hash"]                                                          # no hash of the spectrum among the haplotypes'
    case["sp_hash"] = ac.spectrum(np.random.default_rng(3), 50, forbid=set(int(x) for hs, _, _, _ in case["haps"] for x in hs) | set(int(x) for x in sp))
    dev, mod = check(gpu_ctx, case)
    assert dev["occ_id"].size == 0 and mod.n_candidates == 0


def test_large(gpu_ctx):
    check(gpu_ctx, ac.large_case())


# -------------------------------------------------------------------------------------------------- exact-filter fallback
def collisions_of(err):
    m = re.findall(r"anchors: (\d+) fingerprint collisions", err)
    assert len(m) == 1, err
    return int(m[0])


@pytest.mark.parametrize("name", ["key_order", "filter0", "filter2", "filter4", "large"])
def test_exact_filter_fallback(gpu_ctx, big, name, monkeypatch, capfd):
    """DG_ANCHOR_FP_BITS narrows the list fingerprints until different lists of one id collide: the filter must notice (the
    DG_DEBUG line counts the collisions), take its exact order, and give what the 64-bit run and the model give"""
    if name == "key_order":
        case = ac.key_order_case(big)
        case["min_shared"] = np.float32(2.0)                                      # (so that the filter decides something)
    elif name == "large":
        case = ac.large_case()
    else:
        case = ac.filter_case(*ac.FILTER_SETTINGS[int(name[6:])])[0]
    mod = run_model(case)
    assert mod.unstable == [] and mod.dropped and len(mod.occs)
    monkeypatch.setenv("DG_DEBUG", "1")
    for bits in (64, 4, 0):
        monkeypatch.setenv("DG_ANCHOR_FP_BITS", str(bits))
        capfd.readouterr()
        dev = run_device(gpu_ctx, case)
        n = collisions_of(capfd.readouterr().err)
        assert (n > 0) == (bits < 64), (bits, n)
        assert_same(dev, mod)
        assert dev["n_unstable_groups"] == 0
    monkeypatch.setenv("DG_ANCHOR_FP_BITS", "65")
    with pytest.raises(capi.DgError):
        run_device(gpu_ctx, case)


# ------------------------------------------------------------------------------------------------------- one real sketch
def test_real_sketch(gpu_ctx):
    """dg_anchor_add_haplotype (its own sketch) = _sketched fed Context.sketch_haplotype = the model fed the oracle's sketch"""
    rng = np.random.default_rng(41)
    k, w, n_vertices = 11, 5, 900
    top = ac.random_top(rng, n_vertices)
    base = rng.choice(np.frombuffer(b"ACGT", np.uint8), 2000)
    names = rng.permutation(n_vertices)
    lens = []
    while sum(lens) < 2000:
        lens.append(min(int(rng.integers(1, 31)), 2000 - sum(lens)))
    ss = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=ss[1:])
    seqs, steps = [], []
    for h in range(3):
        s = base.copy()
        flip = rng.choice(2000, 25, replace=False)
        s[flip] = rng.choice(np.frombuffer(b"ACGT", np.uint8), 25)
        seqs.append(s.tobytes())
        alt = rng.random(len(lens)) < 0.1                                         # a bubble allele here and there
        steps.append(np.where(alt, names[len(lens):2 * len(lens)], names[:len(lens)]).astype(np.int32))
    sk_orc = [orc.minimizers(s, k, w) for s in seqs]
    sk_dev = [gpu_ctx.sketch_haplotype(s, k, w) for s in seqs]
    every = np.unique(np.concatenate([h for h, _ in sk_orc]))
    sp = np.unique(np.concatenate([every[rng.random(every.size) < 0.8], ac.spectrum(rng, 50)]))
    def case(sk):
        return dict(n_haps=3, n_vertices=n_vertices, top=top, k=k, w=w, haps=[(hs, ps, sv, ss) for (hs, ps), sv in zip(sk, steps)], sp_hash=sp,
                    min_shared=np.float32(1.0) * np.float32(3))
    mod = run_model(case(sk_orc))
    assert mod.unstable == [] and mod.dropped and len(mod.occs) > 100
    for dev in (run_device(gpu_ctx, case(sk_orc), sketched=False, seqs=seqs), run_device(gpu_ctx, case(sk_dev))):
        assert_same(dev, mod)
        assert dev["n_unstable_groups"] == 0


# ------------------------------------------------------------------------------------- errors leave the context usable
def test_errors_leave_the_context_usable(gpu_ctx):
    """every malformed input below is refused by the host-side checks of dg_anchor_*, before anything is launched"""
    ctx = gpu_ctx
    good = ac.join_case(3)
    want = run_model(good)
    hs, ps, sv, ss = good["haps"][0]
    L, k = int(ss[-1]), good["k"]
    begin = lambda: ctx.anchor_begin(3, good["n_vertices"], good["top"], k, 3)
    def add0(**kw):
        a = dict(length=L, hash=hs, pos=ps, step_vtx=sv, step_start=ss)
        a.update(kw)
        ctx.anchor_add_haplotype_sketched(0, **a)
    bad_end = ss.copy(); bad_end[-1] += 1
    bad_vtx = sv.copy(); bad_vtx[len(bad_vtx) // 2] = good["n_vertices"]
    desc = ps.copy(); desc[[4, 5]] = desc[5] + 1, desc[4]
    assert desc[4] > desc[5]
    late = ps.copy(); late[-1] = L - k + 1
    failures = [
        lambda: ctx.anchor_add_haplotype_sketched(1, L, hs, ps, sv, ss),                          # haplotypes out of order
        lambda: (add0(), ctx.anchor_finish(good["sp_hash"], 3.0)),                                # finish before all haplotypes are in
        lambda: add0(step_start=bad_end),                                                         # step_start does not end at len
        lambda: add0(step_vtx=bad_vtx),                                                           # a vertex >= n_vertices
        lambda: add0(pos=desc),                                                                   # descending pos
        lambda: add0(pos=late),                                                                   # pos + k > len
        lambda: add0(hash=hs[:0], pos=ps[:0], step_vtx=sv[:0], step_start=ss[:1]),                # zero steps, len > 0
        lambda: ctx.anchor_add_haplotype(0, b"ACGT" * 10, sv[:0], ss[:1]),                        # the same through the sketching entry
    ]
    for fail in failures:
        begin()
        with pytest.raises(capi.DgError):
            fail()
        assert_same(run_device(ctx, good), want)
    begin()                                                                                       # zero steps and len = 0 is a haplotype
    ctx.anchor_add_haplotype_sketched(0, 0, hs[:0], ps[:0], sv[:0], ss[:1])
    for h in (1, 2):
        ctx.anchor_add_haplotype_sketched(h, int(good["haps"][h][3][-1]), *good["haps"][h])
    ctx.anchor_finish(good["sp_hash"], 3.0)

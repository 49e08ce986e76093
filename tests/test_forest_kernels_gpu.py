"""forest_kernel_dual, forest_kernel<false/true>, forest_kernel_ilpN and
finalize_kernel (csrc/creditcore_kernels.hip) on hand-built forests, through
three entry points:

  A  ScoringEngine.score_arrays(with_drift=False): forest_kernel_dual +
     finalize_kernel under graph replay
  B  ext.score_forest_pipeline: forest_kernel<false>, forest_kernel<true> and
     finalize_kernel (averaging forests only)
  C  ext.forest_ilp_bench, use_ilp 0..4: the raw f64 accumulator of
     forest_kernel<false> and of the four forest_kernel_ilpN variants

Bounds. Every leaf is a multiple of 2^-16 with |v| <= 64 and T <= 5000, so
the leaf sums are exact in f64 in any order: C is compared bit for bit. The
averaging probability is acc * (1.0 / T): one rounding in the reciprocal and
one in the product, so A and B lie within 2 ulp of the exact quotient (and
equal it where the sum is 0 or 1). Isolation scores and the sigmoid keep the
project's GPU-vs-CPU bound of 1e-9 (exp2 / exp of the device library against
numpy's). The reference is the naive walker of _forest_cases.py, cpu_ref
above 50k (row, tree) pairs, and for the visit-once forests the analytic
answer as well.

The tests without the gpu mark run anywhere: they cross-check the references
and show that the committed cases can see each kind of kernel error, by
running deliberately wrong copies of the walker on the CPU. Run the rest on a
real MI355X (`pytest -m gpu`)."""

from __future__ import annotations

import functools

import numpy as np
import pytest

import _forest_cases as fc
from creditcore.ops import cpu_ref

gpu = pytest.mark.gpu

ATOL = 1e-9
BLOCK = 256  # rows per block of every forest kernel
GRID_TARGET = 2048  # blocks the launchers aim for
CPU_REF_MAX_PAIRS = 16384 * 129  # largest cpu_ref call of this file

# visit-once (classifier trees, isolation trees): always different counts
VO_PAIR = {
    1: 2, 2: 1, 3: 5, 4: 5, 5: 3,
    32: 33, 33: 32, 64: 65, 65: 64, 127: 129, 129: 127,
    2048: 2049, 2049: 2048, 4096: 4097, 4097: 4096, 5000: 4097,
}  # fmt: skip
VO_SMALL = [(t, b) for t in (1, 2, 3, 4, 5) for b in (1, 64, 65, 256, 257)]
VO_ENGINE = VO_SMALL + [
    (64, 16384), (65, 16384), (127, 16384), (129, 16384),  # chunk cap 32
    (2048, 257), (2049, 257),  # cap 1024
    (4096, 1), (4097, 1), (5000, 1),  # cap 2048
]  # fmt: skip
VO_PIPELINE = [(t, b) for t in (1, 2, 3) for b in (1, 257)] + [(32, 16384), (33, 16384)]
VO_RAW = [(t, b) for t in (1, 2, 3, 4, 5, 7, 8, 9) for b in (1, 257)] + [
    (128, 16384), (129, 16384), (131, 16384),
]  # fmt: skip
RAGGED_B = [1, 63, 64, 65, 255, 256, 257, 513]
RAGGED = {"odd": fc.RAGGED_ODD, "even": fc.RAGGED_EVEN}


def _cap(b: int) -> int:
    return -(-GRID_TARGET // -(-b // BLOCK))


def dual_chunks(b: int, n_trees: int) -> int:
    """gridDim.y share of one forest in forest_kernel_dual (ScoreSession::record)."""
    return max(1, min(_cap(b), (n_trees + 1) // 2))


def plain_chunks(b: int, n_trees: int) -> int:
    """gridDim.y of forest_kernel<> (score_forest_pipeline, forest_ilp_bench 0)."""
    return max(1, min(_cap(b), n_trees))


def ilp_chunks(b: int, n_trees: int, ilp: int) -> int:
    """Tree chunks of forest_kernel_ilpN (forest_ilp_bench 1..4)."""
    return max(1, min(_cap(b), -(-n_trees // ilp)))


def _vo_model(t_cls: int):
    return fc.visit_once_model(t_cls, VO_PAIR.get(t_cls, 1))


def _vo_rows(p, b: int, start: int = 0):
    return fc.visit_once_rows(b, max(p.cls_n_trees, p.if_n_trees), start)


@functools.lru_cache(maxsize=None)
def _vo_reference(t_cls: int, b: int, start: int = 0):
    """Analytic (leaf sum, isolation score) of a visit-once batch, confirmed
    by the walker or cpu_ref wherever that costs at most the 16384 x 129 call
    (computed once per shape, shared by A, B, C and the CPU tests)."""
    p = _vo_model(t_cls)
    codes, nums = _vo_rows(p, b, start)
    s, iscore = fc.visit_once_expected(p, nums)
    if b * max(p.cls_n_trees, p.if_n_trees) <= CPU_REF_MAX_PAIRS:
        s_ref, iscore_ref, _ = fc.reference(p, codes, nums)
        np.testing.assert_array_equal(s_ref, s)
        np.testing.assert_array_equal(iscore_ref, iscore)
    s.setflags(write=False)
    iscore.setflags(write=False)
    return s, iscore


@functools.lru_cache(maxsize=None)
def _ragged_reference(name: str):
    p = fc.ragged_model(RAGGED[name])
    ref = fc.reference(p, *fc.ragged_rows())
    for a in ref:
        a.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def _edge_reference():
    ref = fc.reference(fc.edge_model(), *fc.edge_rows())
    for a in ref:
        a.setflags(write=False)
    return ref


def _ulps(got, want) -> float:
    """max |got - want| in units of the spacing of want (0 where equal)."""
    err = np.abs(np.asarray(got) - want)
    return float(np.max(np.where(err == 0.0, 0.0, err / np.spacing(np.abs(want))), initial=0.0))


# ------------------------------------------------------------------ CPU tests


def test_walker_agrees_with_cpu_ref():
    """The naive walker and cpu_ref (level-synchronous, vectorised) are two
    independent traversals; on every family they must agree exactly: the
    classifier output bit for bit, the isolation score bit for bit (same
    numpy expression of the same exact sum)."""
    for name, p, codes, nums in fc.small_cases():
        imp = cpu_ref.impute_nums(p, nums)
        s = fc.naive_sums(p, codes, nums, "cls")
        d = fc.naive_sums(p, codes, nums, "if")
        assert (s / fc.Q == np.round(s / fc.Q)).all(), name
        with np.errstate(over="ignore"):  # exp(800) in the sigmoid
            proba = cpu_ref.score_forest_cpu(p, codes, imp)
        np.testing.assert_array_equal(proba, fc.proba_of(p, s), err_msg=name)
        iscore, flags = cpu_ref.score_iforest_cpu(p, imp)
        np.testing.assert_array_equal(iscore, fc.iscore_of(p, d), err_msg=name)
        np.testing.assert_array_equal(flags, (iscore > p.if_threshold).astype(np.float64))
        if p.cls_kind == 0:  # the sum recovered from cpu_ref's quotient is exact
            np.testing.assert_array_equal(
                np.round(cpu_ref.score_forest_cpu(p, codes, imp) * p.cls_n_trees / fc.Q) * fc.Q, s
            )


@pytest.mark.parametrize("t_cls,b", [(1, 1), (3, 257), (5, 257), (129, 16384), (5000, 1)])
def test_visit_once_is_one_per_row(t_cls, b):
    """Every row of a visit-once batch whose x is below T sums to exactly 1.0
    (one tree answers, every other tree answers 0), confirmed by cpu_ref or
    the walker inside _vo_reference; the isolation forest likewise."""
    s, iscore = _vo_reference(t_cls, b)
    p = _vo_model(t_cls)
    x = _vo_rows(p, b)[1][:, 0]
    np.testing.assert_array_equal(s, x < t_cls)
    np.testing.assert_array_equal(iscore, np.where(x < p.if_n_trees, 0.0, 0.5))
    assert s.max() == 1.0


def test_shapes_reach_the_chunk_formulas():
    """The visit-once shapes hit what they were chosen for: the chunk cap from
    below, exactly and from above, an absent second ILP lane, T < ILP and the
    ragged 4-lane tails."""
    assert [_cap(b) for b in (1, 257, 16384)] == [2048, 1024, 32]
    for b, at, over in ((16384, 64, 65), (257, 2048, 2049), (1, 4096, 4097)):
        assert dual_chunks(b, at) == _cap(b) == dual_chunks(b, over)
        assert (-1 not in sum(fc.ilp_lanes(at, _cap(b), 2), ())) and (
            (over - 1, -1) in fc.ilp_lanes(over, _cap(b), 2)
        )
    assert dual_chunks(16384, 127) == 32 and dual_chunks(16384, 129) == 32
    assert plain_chunks(16384, 32) == 32 == plain_chunks(16384, 33)
    for t in (128, 129, 131):
        assert ilp_chunks(16384, t, 4) == 32 and ilp_chunks(16384, t, 2) == 32
    assert (128, -1, -1, -1) in fc.ilp_lanes(129, 32, 4)
    assert (130, -1, -1, -1) in fc.ilp_lanes(131, 32, 4)
    assert fc.ilp_lanes(3, 1, 4) == [(0, 1, 2, -1)]
    # every tree sits in exactly one lane, whatever the split
    for t, n, ilp in ((129, 32, 4), (5000, 2048, 2), (4097, 2048, 2), (5, 3, 2), (9, 3, 4)):
        lanes = [k for lane in fc.ilp_lanes(t, n, ilp) for k in lane if k >= 0]
        assert sorted(lanes) == list(range(t))
    # the ragged forests at the engine's split: stump with caterpillar in
    # either lane, both stumps, and (odd T only) a caterpillar on its own
    for name, kinds in RAGGED.items():
        n = dual_chunks(513, len(kinds))
        assert n == (len(kinds) + 1) // 2 == dual_chunks(1, len(kinds))
        pairs = {(kinds[a], kinds[c] if c >= 0 else "-") for a, c in fc.ilp_lanes(len(kinds), n, 2)}
        assert {("S", "C"), ("C", "S"), ("S", "S")} <= pairs
        assert (("C", "-") in pairs) == (name == "odd")


@pytest.mark.parametrize("mutation", fc.MUTATIONS)
def test_cases_see_mutation(mutation):
    """A walker with one deliberate error disagrees with the true walker on
    at least one committed case: the inputs can see that error. (The kernels
    themselves are never run wrong.)"""
    seen = []
    for name, p, codes, nums in fc.small_cases():
        for forest in ("cls", "if"):
            if mutation == "ignore_unknown" and forest == "if":
                continue
            good = fc.naive_sums(p, codes, nums, forest)
            with np.errstate(invalid="ignore"):
                bad = fc.mutant_sums(p, codes, nums, mutation, forest)
            if not np.array_equal(good, bad):
                seen.append(f"{name}/{forest}")
    print(f"{mutation}: seen by {seen}")
    assert seen


# ------------------------------------------------------------------ GPU tests


@pytest.fixture(scope="module")
def ext():
    from creditcore.ops import gpu as gpu_ops

    assert gpu_ops.available(), (
        "HIP extension must be present on a GPU box (no silent CPU fallback)"
    )
    return gpu_ops.ext()


@pytest.fixture(scope="module")
def engine_of(ext):
    """One GPU engine per hand model, built on first use."""
    from creditcore.engine import ScoringEngine

    cache = {}

    def get(p):
        if id(p) not in cache:
            cache[id(p)] = (p, ScoringEngine(p, device="cuda", device_index=0))
        return cache[id(p)][1]

    return get


def _dev(a, dtype=None):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def run_engine(engine_of, p, codes, nums):
    out = engine_of(p).score_arrays(codes, nums, with_drift=False)
    return out["predictions"], out["instance_score"], out["outliers"]


def run_pipeline(ext, p, codes, nums):
    assert p.cls_kind == 0  # the entry point averages leaf values
    outs = ext.score_forest_pipeline(
        _dev(codes), _dev(nums),
        _dev(p.cls_nodes, np.int32), _dev(p.cls_tree_offsets, np.int32),
        _dev(p.feat_col, np.int32), _dev(p.feat_code, np.int32),
        _dev(p.medians, np.float32), int(p.n_onehot),
        _dev(p.if_nodes, np.int32), _dev(p.if_tree_offsets, np.int32),
        float(p.if_denom), float(p.if_offset), float(p.if_threshold),
    )  # fmt: skip
    return tuple(t.cpu().numpy() for t in outs)


def run_raw(ext, p, codes, nums):
    """Raw accumulators of forest_kernel<false> and the four ilpN variants."""
    model = (
        _dev(p.cls_nodes, np.int32), _dev(p.cls_tree_offsets, np.int32),
        _dev(p.feat_col, np.int32), _dev(p.feat_code, np.int32),
        _dev(p.medians, np.float32),
    )  # fmt: skip
    c, n = _dev(codes), _dev(nums)
    return [ext.forest_ilp_bench(c, n, *model, v).cpu().numpy() for v in range(5)]


def check_scored(tag, p, got, s, iscore_ref, flag_ref):
    """Outputs of A or B against exact leaf sums s and the reference score.
    Returns (ulps of the probability, max |err| of the score)."""
    proba, iscore, flags = got
    b = len(s)
    assert proba.shape == iscore.shape == flags.shape == (b,) and proba.dtype == np.float64
    want = fc.proba_of(p, s)
    ulps, err = _ulps(proba, want), float(np.abs(iscore - iscore_ref).max())
    print(f"{tag}: proba max err = {ulps:.2f} ulp, iscore max |err| = {err:.3e}")
    exact = (s == 0.0) | (s == 1.0)  # acc * fl(1/T) is then 0 or fl(1/T) itself
    np.testing.assert_array_equal(proba[exact], want[exact], err_msg=tag)
    assert (np.abs(proba - want) <= 2.0 * np.spacing(np.abs(want))).all(), (tag, ulps)
    np.testing.assert_allclose(iscore, iscore_ref, rtol=0, atol=ATOL, err_msg=tag)
    # the kernel's own consistency, then the reference away from the threshold
    np.testing.assert_array_equal(flags, (iscore > p.if_threshold).astype(np.float64))
    far = np.abs(iscore_ref - p.if_threshold) > ATOL
    np.testing.assert_array_equal(flags[far], flag_ref[far], err_msg=tag)
    return ulps, err, int((~far).sum())


# family 1: visit-once forests


def _starts(b: int, t_cls: int, t_if: int) -> list[int]:
    """A one-row batch sees one tree, so it is repeated with x on the first
    tree, around the ends of the first and the second ILP lane of the chunk
    grid and on the last tree of either forest."""
    if b > 1:
        return [0]
    cap, period = _cap(b), max(t_cls, t_if)
    edges = {0, 1, cap - 1, cap, 2 * cap - 1, 2 * cap, 2 * cap + 1, t_cls - 1, t_if - 1}
    return sorted(x for x in edges if 0 <= x < period)


@gpu
@pytest.mark.parametrize("t_cls,b", VO_ENGINE)
def test_visit_once_engine(engine_of, t_cls, b):
    """A: forest_kernel_dual deals every tree of both forests to exactly one
    (chunk, lane). Raw sum 1.0 per row with x < T: probability exactly
    fl(1/T); a missed or doubled isolation tree moves the score by >= 0.25.
    Measured on MI355X: probability bit-exact, isolation score max |err| 0."""
    p = _vo_model(t_cls)
    for start in _starts(b, t_cls, p.if_n_trees):
        codes, nums = _vo_rows(p, b, start)
        s, iscore = _vo_reference(t_cls, b, start)
        got = run_engine(engine_of, p, codes, nums)
        np.testing.assert_array_equal(got[0], s / t_cls)
        check_scored(f"A visit-once T={t_cls}/{p.if_n_trees} b={b} x0={start}", p, got, s,
                     iscore, np.zeros(b))  # fmt: skip


@gpu
@pytest.mark.parametrize("t_cls,b", VO_PIPELINE)
def test_visit_once_pipeline(ext, t_cls, b):
    """B: forest_kernel<false/true> stride trees by gridDim.y; T = 32 and 33
    at 16384 rows sit on and one past the chunk cap.
    Measured on MI355X: probability bit-exact, isolation score max |err| 0."""
    p = _vo_model(t_cls)
    for start in _starts(b, t_cls, p.if_n_trees):
        codes, nums = _vo_rows(p, b, start)
        s, iscore = _vo_reference(t_cls, b, start)
        got = run_pipeline(ext, p, codes, nums)
        np.testing.assert_array_equal(got[0], s / t_cls)
        check_scored(f"B visit-once T={t_cls}/{p.if_n_trees} b={b} x0={start}", p, got, s,
                     iscore, np.zeros(b))  # fmt: skip


@gpu
@pytest.mark.parametrize("t_cls,b", VO_RAW)
def test_visit_once_raw(ext, t_cls, b):
    """C: the raw accumulator of all five kernels is the visit count of tree
    x, bit for bit: T below the ILP width, ragged 2- and 4-lane tails and the
    swapped grid with 64 row blocks."""
    p = _vo_model(t_cls)
    for start in _starts(b, t_cls, 1):
        codes, nums = _vo_rows(p, b, start)
        s, _ = _vo_reference(t_cls, b, start)
        for v, raw in enumerate(run_raw(ext, p, codes, nums)):
            np.testing.assert_array_equal(raw, s, err_msg=f"use_ilp={v} x0={start}")
    print(f"C visit-once T={t_cls} b={b}: bit-exact")


# family 2: ragged depth


@gpu
@pytest.mark.parametrize("b", RAGGED_B)
def test_ragged_engine(engine_of, b):
    """A: a root-is-leaf tree in one ILP lane and the 26-split caterpillar in
    the other (both orders), two stumps, and an absent second lane (odd T).
    acc_if follows acc_cls[b] in the session, so a write past n_rows would
    show in the isolation score of row 0: both outputs are held for every b.
    Measured on MI355X: probability max err 1 ulp, isolation score max |err| 5.6e-17."""
    codes, nums = fc.ragged_rows()
    for name, kinds in RAGGED.items():
        p = fc.ragged_model(kinds)
        s, iscore, flags = (a[:b] for a in _ragged_reference(name))
        got = run_engine(engine_of, p, codes[:b], nums[:b])
        check_scored(f"A ragged {name} b={b}", p, got, s, iscore, flags)


@gpu
@pytest.mark.parametrize("b", RAGGED_B)
def test_ragged_pipeline(ext, b):
    """B on the ragged forests.
    Measured on MI355X: probability max err 1 ulp, isolation score max |err| 5.6e-17."""
    codes, nums = fc.ragged_rows()
    for name, kinds in RAGGED.items():
        p = fc.ragged_model(kinds)
        s, iscore, flags = (a[:b] for a in _ragged_reference(name))
        got = run_pipeline(ext, p, codes[:b], nums[:b])
        check_scored(f"B ragged {name} b={b}", p, got, s, iscore, flags)


@gpu
@pytest.mark.parametrize("b", RAGGED_B)
def test_ragged_raw(ext, b):
    """C on the ragged forests: with four lanes a stump, a caterpillar and a
    depth-3 tree share one thread and end up to 26 steps apart."""
    codes, nums = fc.ragged_rows()
    for name, kinds in RAGGED.items():
        p = fc.ragged_model(kinds)
        s = _ragged_reference(name)[0][:b]
        for v, raw in enumerate(run_raw(ext, p, codes[:b], nums[:b])):
            np.testing.assert_array_equal(raw, s, err_msg=f"{name} use_ilp={v}")
    print(f"C ragged b={b}: bit-exact")


# family 3: compare edges


@gpu
def test_edges_engine(engine_of):
    """A: v <= thr at equality and one f32 step to either side, -0.0 against
    +0.0, denormals (no flush to zero), +-inf, +-FLT_MAX, NaN imputed onto a
    threshold, one-hot splits at 0.0 / 0.5 / 1.0 with codes -1, 0, 1, 2, 32767.
    Measured on MI355X: probability max err 1 ulp, isolation score max |err| 5.6e-17."""
    p = fc.edge_model()
    got = run_engine(engine_of, p, *fc.edge_rows())
    check_scored("A edges", p, got, *_edge_reference())


@gpu
def test_edges_pipeline(ext):
    """B on the compare edges.
    Measured on MI355X: probability max err 1 ulp, isolation score max |err| 5.6e-17."""
    p = fc.edge_model()
    got = run_pipeline(ext, p, *fc.edge_rows())
    check_scored("B edges", p, got, *_edge_reference())


@gpu
def test_edges_raw(ext):
    """C on the compare edges: one flipped branch changes the exact sum."""
    p = fc.edge_model()
    s = _edge_reference()[0]
    for v, raw in enumerate(run_raw(ext, p, *fc.edge_rows())):
        np.testing.assert_array_equal(raw, s, err_msg=f"use_ilp={v}")
    print("C edges: bit-exact")


# family 4: finalize_kernel


@gpu
def test_gbt_sigmoid(engine_of, ext):
    """A, cls_kind = 1: logit = leaf sum + cls_bias of 0, +-1, +-40, +-800.
    0.5 at 0, exactly 1.0 / 0.0 at +-800 (exp underflows / overflows to inf),
    no NaN, 1e-9 elsewhere; the raw sums (C) are exact.
    Measured on MI355X: probability max |err| 7.7e-34, isolation score 1.1e-16."""
    p = fc.gbt_model()
    codes, nums = fc.gbt_rows()
    s, iscore, flags = fc.reference(p, codes, nums)
    logit = s + p.cls_bias
    np.testing.assert_array_equal(logit, np.array(fc.GBT_LOGITS)[nums[:, 0].astype(int)])
    proba, got_iscore, _ = run_engine(engine_of, p, codes, nums)
    want = fc.proba_of(p, s)
    print(f"A gbt: proba max |err| = {np.abs(proba - want).max():.3e}, "
          f"iscore max |err| = {np.abs(got_iscore - iscore).max():.3e}")  # fmt: skip
    assert not np.isnan(proba).any()
    np.testing.assert_array_equal(proba[logit == 0.0], 0.5)
    np.testing.assert_array_equal(proba[logit == 800.0], 1.0)
    np.testing.assert_array_equal(proba[logit == -800.0], 0.0)
    np.testing.assert_allclose(proba, want, rtol=0, atol=ATOL)
    np.testing.assert_allclose(got_iscore, iscore, rtol=0, atol=ATOL)
    for v, raw in enumerate(run_raw(ext, p, codes, nums)):
        np.testing.assert_array_equal(raw, s, err_msg=f"use_ilp={v}")


@gpu
@pytest.mark.parametrize("step", [-1, 0, 1])
def test_outlier_flag_at_threshold(engine_of, ext, step):
    """if_threshold on the reference score of one depth class and one f64
    step to either side (A with cls_kind = 1, B with the same trees averaged).
    The flag is exactly (returned score > threshold) on every row and equals
    the reference flag on every row further than 1e-9 from the threshold; the
    rows left out are exactly those built to sit on it."""
    codes, nums = fc.gbt_rows()
    built_on = int((nums[:, 1] == fc.GBT_THRESHOLD_CLASS).sum())
    assert 0 < built_on < len(codes)
    for path, kind in (("A", 1), ("B", 0)):
        p = fc.gbt_model(step, kind)
        s, iscore, flags = fc.reference(p, codes, nums)
        assert 0 < flags.sum() < len(flags)  # classes on both sides
        if path == "A":
            got = run_engine(engine_of, p, codes, nums)
            np.testing.assert_allclose(got[0], fc.proba_of(p, s), rtol=0, atol=ATOL)
            _, got_iscore, got_flags = got
            np.testing.assert_allclose(got_iscore, iscore, rtol=0, atol=ATOL)
            np.testing.assert_array_equal(got_flags, (got_iscore > p.if_threshold).astype(float))
            far = np.abs(iscore - p.if_threshold) > ATOL
            np.testing.assert_array_equal(got_flags[far], flags[far])
            on = int((~far).sum())
            print(f"A threshold step={step}: iscore max |err| = "
                  f"{np.abs(got_iscore - iscore).max():.3e}, "
                  f"on-threshold rows flagged {int(got_flags[~far].sum())}/{on}")  # fmt: skip
        else:
            got = run_pipeline(ext, p, codes, nums)
            _, _, on = check_scored(f"B threshold step={step}", p, got, s, iscore, flags)
        assert on == built_on


@gpu
def test_zero_after_read(engine_of):
    """finalize_kernel re-zeros the accumulator rows it read. A 16384-row
    batch, then one-row batches of other families' rows on the same engine:
    what is left in acc_cls / acc_if would add to the next sum, so the small
    batches must still give exactly 0 or fl(1/T)."""
    p = _vo_model(129)
    s, iscore = _vo_reference(129, 16384)
    singles = [fc.visit_once_rows(1, 129, 128), fc.visit_once_rows(1, 129, 3)]
    for codes, nums in (fc.ragged_rows(), fc.edge_rows(), fc.gbt_rows()):
        singles += [(codes[i : i + 1], nums[i : i + 1]) for i in (0, len(codes) - 1)]
    for k, (codes1, nums1) in enumerate(singles):
        got = run_engine(engine_of, p, *_vo_rows(p, 16384))
        np.testing.assert_array_equal(got[0], s / 129)
        np.testing.assert_allclose(got[1], iscore, rtol=0, atol=ATOL)
        s1, iscore1, flags1 = fc.reference(p, codes1, nums1)
        assert s1[0] in (0.0, 1.0)
        for _ in range(2):  # the second replay reads what the first one left
            got1 = run_engine(engine_of, p, codes1, nums1)
            np.testing.assert_array_equal(got1[0], s1 / 129, err_msg=f"single {k}")
            check_scored(f"A after 16384 rows, single {k}", p, got1, s1, iscore1, flags1)

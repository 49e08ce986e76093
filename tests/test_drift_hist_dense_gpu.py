"""cat_hist_kernel, impute_transpose_kernel, dense_score_kernel and the plain
score_forest_pipeline launches of csrc/creditcore_kernels.hip, called through
the extension on numpy-built inputs at the tile, stride and block edges that
the engine-level tests never reach. Run on a real MI355X (`pytest -m gpu`)."""

from __future__ import annotations

import numpy as np
import pytest

from _kernel_cases import cat_hist_reference
from creditcore.ops import cpu_ref

pytestmark = pytest.mark.gpu

B_HIST = [1, 255, 256, 257, 2048, 2049, 5000]
# 9 columns, 2..40 bins, 121 bins in all (no multiple of 64)
N_BINS = np.array([2, 40, 3, 17, 5, 33, 7, 2, 12])


@pytest.fixture(scope="module")
def ext():
    from creditcore.ops import gpu

    assert gpu.available(), (
        "HIP extension must be present on a GPU box (no silent CPU fallback)"
    )
    return gpu.ext()


@pytest.fixture(scope="module")
def engine(packed):
    from creditcore.engine import ScoringEngine

    return ScoringEngine(packed, device="cuda", device_index=0)


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------ cat_hist_kernel


def _code_cases(rng, b, n_bins):
    """Codes in the encoder's range [-1, nbins - 2] per column."""
    top = (n_bins - 2).astype(np.int16)
    return {
        "all_unseen": np.full((b, len(n_bins)), -1, dtype=np.int16),
        "all_zero": np.zeros((b, len(n_bins)), dtype=np.int16),
        "all_max": np.broadcast_to(top, (b, len(n_bins))).copy(),
        "random": np.stack(
            [rng.integers(-1, nb - 1, size=b) for nb in n_bins], axis=1
        ).astype(np.int16),
    }


@pytest.mark.parametrize("b", B_HIST)
def test_cat_hist_drift_stats(ext, b):
    """drift_stats: one block up to 256 rows, several blocks with atomics
    into the pre-zeroed histogram above. Exact against np.bincount."""
    assert N_BINS.sum() % 64 != 0
    cat_off = np.concatenate([[0], np.cumsum(N_BINS)]).astype(np.int32)
    rng = np.random.default_rng(b)
    nums = _dev(rng.normal(size=(b, 14)).astype(np.float32))
    med = _dev(np.zeros(14, dtype=np.float32))
    ref = _dev(np.arange(14, dtype=np.float32))
    rs_off = _dev(np.arange(15, dtype=np.int64))
    for name, codes in _code_cases(rng, b, N_BINS).items():
        hist, _ = ext.drift_stats(
            _dev(codes), nums, med, ref, rs_off, _dev(cat_off), int(cat_off[-1])
        )
        want = cat_hist_reference(codes, cat_off)
        assert want.sum() == 9 * b
        np.testing.assert_array_equal(hist.cpu().numpy(), want, err_msg=name)


@pytest.mark.parametrize("b", B_HIST)
def test_cat_hist_engine(engine, packed, b):
    """The session: one block with plain stores up to 2048 rows, memset plus
    atomics above, with the model's own bin offsets."""
    n_bins = np.diff(packed.ref_cat_offsets)
    rng = np.random.default_rng(b + 1)
    nums = rng.normal(5000.0, 3000.0, size=(b, 14)).astype(np.float32)
    for name, codes in _code_cases(rng, b, n_bins).items():
        got = engine.score_arrays(codes, nums, with_drift=True)["cat_hist"]
        want, _ = cpu_ref.drift_stats_cpu(packed, codes, cpu_ref.impute_nums(packed, nums))
        np.testing.assert_array_equal(got, want, err_msg=name)
        np.testing.assert_array_equal(got, cat_hist_reference(codes, packed.ref_cat_offsets))


# --------------------------------------------------- impute_transpose_kernel


@pytest.mark.parametrize(
    "b,f", [(1, 1), (1, 33), (33, 1), (31, 33), (32, 32), (33, 31), (100, 65), (257, 70)]
)
def test_impute_transpose(ext, b, f):
    """32x32 tiles with ragged edges on either side; bit patterns compared,
    so -0.0 (in the data and as a median) and +-inf must survive."""
    rng = np.random.default_rng(100 * b + f)
    x = rng.normal(size=(b, f)).astype(np.float32)
    x[rng.uniform(size=x.shape) < 0.1] = np.nan
    if b > 1:
        x[b // 2, :] = np.nan
    if f > 1:
        x[:, f // 2] = np.nan
    spots = [(0, 0), (0, f - 1), (b - 1, 0)]
    for (r, c), v in zip(spots, (np.inf, -np.inf, -0.0)):
        if b * f >= 4:
            x[r, c] = v
    if b * f == 1:
        x[0, 0] = np.nan
    med = rng.normal(size=f).astype(np.float32)
    med[f // 2] = -0.0
    got = ext.impute_transpose(_dev(x), _dev(med)).cpu().numpy()
    want = np.ascontiguousarray(np.where(np.isnan(x), med[None, :], x).T)
    assert got.shape == (f, b) and got.dtype == np.float32
    assert not np.isnan(got).any()
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


# -------------------------------------------------------- dense_score_kernel

Z_THR = 6.1  # not a float32: the kernel compares against float32(6.1)
B_DENSE = [1, 2, 3, 4, 5, 1023]


def _dense_problem(b, f, seed):
    rng = np.random.default_rng(seed)
    med = rng.normal(size=f).astype(np.float32)
    inv = (1.0 / rng.uniform(0.5, 2.0, size=f)).astype(np.float32)
    # mixed sign and scale; 1/sqrt(F) keeps the logit of order one
    w = (rng.normal(size=f) * 10.0 ** rng.uniform(-3, 0, size=f) / np.sqrt(f)).astype(np.float32)
    x = (med + rng.normal(size=(b, f)) * 2.0).astype(np.float32)
    x[rng.uniform(size=x.shape) < 0.05] = np.nan
    # feature k has median 0 and unit scale: z = |v| exactly
    k = f // 3
    med[k], inv[k] = 0.0, 1.0
    thr = np.float32(Z_THR)
    rows = {}
    if b > 0:  # the largest z in the last feature (lane (F-1) mod 64)
        x[0] = med
        x[0, f - 1] = med[f - 1] + np.float32(40.0) / inv[f - 1]
        rows["max_last"] = 0
    if b > 1:  # the largest z in feature 0
        x[1] = med
        x[1, 0] = med[0] - np.float32(30.0) / inv[0]
        rows["max_first"] = 1
    if b > 2:
        x[2] = np.nan
        rows["all_nan"] = 2
    if b > 3:  # z equal to the threshold bit for bit: strict >, not flagged
        x[3] = med
        x[3, k] = thr
        rows["at_threshold"] = 3
    if b > 4:  # one float32 above it: flagged
        x[4] = med
        x[4, k] = -np.nextafter(thr, np.float32(np.inf))
        rows["above_threshold"] = 4
    return x, med, inv, w, np.float32(rng.normal()), rows


@pytest.mark.parametrize("f", [1, 2, 63, 64, 65, 127, 128, 1000])
def test_dense_score(ext, f):
    """One wavefront per row striding F: F below, at and off the 64-lane
    stride, and row counts that leave partial 4-row blocks.

    iscore / outlier: exact against the float32 emulation (subtract, abs,
    multiply, max: nothing to contract). proba: the kernel sums float32
    products in an order of its own, so per row
    |dlogit| <= (F + 1) 2^-24 sum|v w| (F 2^-24 for the summation, 2^-24
    for the rounding of each product), |dp| <= |dlogit| / 4, plus 1e-15 for
    the f64 logistic."""
    for b in B_DENSE:
        x, med, inv, w, bias, rows = _dense_problem(b, f, seed=1000 * f + b)
        proba, iscore, outlier = (
            t.cpu().numpy()
            for t in ext.dense_score(
                _dev(x), _dev(med), _dev(inv), _dev(w), float(bias), Z_THR
            )
        )
        assert proba.shape == iscore.shape == outlier.shape == (b,)

        v = np.where(np.isnan(x), med[None, :], x)
        assert v.dtype == np.float32
        z = np.abs(v - med[None, :]) * inv[None, :]
        assert z.dtype == np.float32
        zmax = np.maximum(z.max(axis=1), np.float32(0.0))
        np.testing.assert_array_equal(iscore, zmax.astype(np.float64))
        flags = (zmax > np.float32(Z_THR)).astype(np.float64)
        np.testing.assert_array_equal(outlier, flags)
        if "max_last" in rows:
            assert z[0].argmax() == f - 1 and flags[0] == 1.0
        if "max_first" in rows and f > 1:
            assert z[1].argmax() == 0 and flags[1] == 1.0
        if "all_nan" in rows:
            assert iscore[2] == 0.0 and outlier[2] == 0.0
        if "at_threshold" in rows:
            assert zmax[3] == np.float32(Z_THR) and outlier[3] == 0.0
        if "above_threshold" in rows:
            assert outlier[4] == 1.0

        prod = v.astype(np.float64) * w.astype(np.float64)[None, :]
        logit = prod.sum(axis=1) + np.float64(bias)
        want = 1.0 / (1.0 + np.exp(-logit))
        bound = 0.25 * (f + 1) * 2.0**-24 * np.abs(prod).sum(axis=1) + 1e-15
        if f == 64:  # no weaker than test_dense_gpu_parity's atol
            assert bound.max() < 1e-5
        err = np.abs(proba - want)
        assert (err <= bound).all(), (b, err.max(), bound[err.argmax()])


# ------------------------------------------------------ score_forest_pipeline


def test_score_forest_pipeline(ext, engine, packed, score_batch):
    """The stand-alone forest_kernel<false> / forest_kernel<true> + finalize
    launches (the engine runs forest_kernel_dual instead) vs the CPU
    reference and vs the engine, on the 512-row scoring batch and on row
    counts around one 256-row block."""
    from creditcore.pack import encode_batch

    assert packed.cls_kind == 0  # the pipeline entry averages leaf values
    codes, nums = encode_batch(score_batch, packed.vocabs)
    p = packed
    i32 = lambda a: _dev(np.asarray(a, dtype=np.int32))  # noqa: E731
    model = [i32(a) for a in (p.cls_nodes, p.cls_tree_offsets, p.feat_col, p.feat_code)]
    med = _dev(p.medians)
    iforest = [i32(p.if_nodes), i32(p.if_tree_offsets)]
    for b in (512, 1, 255, 257):
        c, n = np.ascontiguousarray(codes[:b]), np.ascontiguousarray(nums[:b])
        proba, iscore, outlier = (
            t.cpu().numpy()
            for t in ext.score_forest_pipeline(
                _dev(c), _dev(n), *model, med, int(p.n_onehot), *iforest,
                float(p.if_denom), float(p.if_offset), float(p.if_threshold),
            )
        )
        imp = cpu_ref.impute_nums(p, n)
        np.testing.assert_allclose(proba, cpu_ref.score_forest_cpu(p, c, imp), atol=1e-9)
        ref_iscore, ref_flags = cpu_ref.score_iforest_cpu(p, imp)
        np.testing.assert_allclose(iscore, ref_iscore, atol=1e-9)
        np.testing.assert_array_equal(outlier, ref_flags)
        out = engine.score_arrays(c, n, with_drift=False)
        np.testing.assert_allclose(proba, out["predictions"], atol=1e-9)
        np.testing.assert_allclose(iscore, out["instance_score"], atol=1e-9)
        np.testing.assert_array_equal(outlier, out["outliers"])

"""knn_topk_kernel against the f64 reference cpu_ref.knn_topk_cpu, and a GPU
engine against a CPU engine.

Exact cases use integer embeddings, where every product, norm and distance is
exact in f32: the kernel must return the reference's distances and indices
with no tolerance, ties included. For real entries the bound is derived, not
tuned: two f32 norms, one f32 dot product of Dp terms and two additions give
|d2_gpu - d2| <= (2 Dp + 4) 2^-24 (n_i + n_j) to first order."""

from __future__ import annotations

import numpy as np
import pytest

from creditcore import mmd
from creditcore.ops import cpu_ref

pytestmark = pytest.mark.gpu

EPS = 2.0**-24


def topk_gpu(zb, zr, k, exclude_self=False, cols=0, launch_rows=0):
    import torch

    from creditcore.ops import gpu

    def up(z):
        return (torch.from_numpy(mmd.pad_columns(z)).cuda(),
                torch.from_numpy(mmd.squared_norms(z).astype(np.float32)).cuda())

    r, nr = up(zr)
    b, nb = (r, nr) if exclude_self else up(zb)
    return gpu.knn_topk(b, r, nb, nr, k, exclude_self, cols, launch_rows)


@pytest.mark.parametrize(
    "b,m,dp,k,cols,launch_rows,loo",
    [
        (1, 2, 4, 1, 0, 0, False),  # M = k + 1, one row, one float4
        (1, 11, 4, 10, 0, 0, False),  # M = k + 1
        (64, 33, 4, 32, 0, 0, False),  # M = k + 1 at the largest k: ties everywhere
        (64, 63, 52, 10, 0, 0, False),  # one ragged tile
        (64, 64, 52, 32, 0, 0, False),  # exact tiles
        (65, 65, 68, 10, 64, 0, False),  # one past the tile both ways, two d-chunks
        (65, 63, 132, 1, 0, 0, False),  # three d-chunks, k = 1
        (1, 130, 68, 1, 64, 0, False),  # three splits for one row
        (65, 130, 132, 32, 64, 0, False),  # last split holds 2 < k rows
        (65, 130, 52, 10, 64, 64, False),  # two launches over the batch rows
        (65, 65, 52, 10, 64, 0, True),  # leave-one-out with duplicated rows
        (130, 130, 4, 32, 64, 64, True),  # ... across splits and launches
    ],
)
def test_exact_cases(b, m, dp, k, cols, launch_rows, loo):
    rng = np.random.default_rng(1000 * m + dp + k)
    zr = rng.integers(-3, 4, size=(m, dp)).astype(np.float32)
    zr[m // 2] = zr[0]  # duplicates: distance 0 off the diagonal
    zr[m - 1] = zr[0]
    zb = zr if loo else rng.integers(-3, 4, size=(b, dp)).astype(np.float32)
    want_d2, want_idx = cpu_ref.knn_topk_cpu(zb, zr, k, exclude_self=loo)
    d2, idx = topk_gpu(zb, zr, k, loo, cols, launch_rows)
    assert d2.dtype == np.float32 and idx.dtype == np.int32 and d2.shape == (b, k)
    assert np.array_equal(idx, want_idx)
    assert np.array_equal(d2.astype(np.float64), want_d2)
    for other in (0, 64, 16384):  # the default, the smallest split, one split
        again = topk_gpu(zb, zr, k, loo, other)
        assert again[0].tobytes() == d2.tobytes() and again[1].tobytes() == idx.tobytes()


def test_real_valued_within_bound():
    b, m, dp, k = 130, 257, 52, 10
    rng = np.random.default_rng(7)
    zb = rng.normal(size=(b, dp)).astype(np.float32)
    zr = rng.normal(size=(m, dp)).astype(np.float32)
    want_d2, _ = cpu_ref.knn_topk_cpu(zb, zr, k)
    d2, idx = topk_gpu(zb, zr, k)
    nb, nr = mmd.squared_norms(zb), mmd.squared_norms(zr)
    diff = zb.astype(np.float64)[:, None, :] - zr.astype(np.float64)[idx]
    true_d2 = (diff * diff).sum(-1)  # f64 d2 of the returned pairs
    bound = (2 * dp + 4) * EPS * (nb[:, None] + nr[idx])
    print(f"largest |d2 - d2_f64| / bound {(np.abs(d2 - true_d2) / bound).max():.3f}, "
          f"largest excess over the k-th / bound {((true_d2 - want_d2[:, -1:]) / bound).max():.3f}")
    assert (np.abs(d2 - true_d2) <= bound).all()
    assert (true_d2 <= want_d2[:, -1:] + bound).all()
    assert (np.diff(d2, axis=1) >= 0).all() and (idx >= 0).all() and (idx < m).all()
    again = topk_gpu(zb, zr, k, cols=64)
    assert again[0].tobytes() == d2.tobytes() and again[1].tobytes() == idx.tobytes()


@pytest.mark.parametrize("score", ["kth", "mean"])
def test_engine_gpu_vs_cpu(packed, score_batch, score):
    from creditcore.engine import ScoringEngine
    from creditcore.pack import encode_batch

    codes, nums = encode_batch(score_batch, packed.vocabs)
    nums = nums.copy()
    nums[:32] += (3.0 * np.nanstd(packed.bg_nums, axis=0)).astype(np.float32)  # far rows
    want = ScoringEngine(packed, device="cpu").knn_outliers(codes, nums, score=score)
    got = ScoringEngine(packed, device="cuda").knn_outliers(codes, nums, score=score)

    # the d2 bound of a row against any reference row, as a distance:
    # |sqrt(a) - sqrt(b)| <= min(|a - b| / sqrt(a), sqrt(|a - b|)), with a no
    # smaller than the nearest neighbour's d2; order statistics, their mean and
    # the quantile of the reference's scores move by no more than their inputs
    mu, sd = mmd.reference_scale(packed, packed.bg_nums)
    z_ref = mmd.embed(packed, packed.bg_codes, packed.bg_nums, mu, sd)
    z = mmd.embed(packed, codes, nums, mu, sd)
    dp = mmd.pad_columns(z).shape[1]
    n_ref = mmd.squared_norms(z_ref)

    def distance_tol(rows, near_d2):
        e = (2 * dp + 4) * EPS * (mmd.squared_norms(rows) + n_ref.max())
        with np.errstate(divide="ignore"):
            return np.minimum(e / np.sqrt(near_d2), np.sqrt(e))

    tol = distance_tol(z, cpu_ref.knn_topk_cpu(z, z_ref, 1)[0][:, 0])
    tol_thr = distance_tol(
        z_ref, cpu_ref.knn_topk_cpu(z_ref, z_ref, 1, exclude_self=True)[0][:, 0]
    ).max()
    err = np.abs(got["instance_score"] - want["instance_score"])
    clear = np.abs(want["instance_score"] - want["threshold"]) > tol + tol_thr
    print(f"score err / tol {np.max(err / tol):.3f}; threshold gpu {got['threshold']:.9f} "
          f"cpu {want['threshold']:.9f} (tol {tol_thr:.2e}); clear rows {clear.mean():.3f}; "
          f"outliers {int(want['is_outlier'].sum())}")
    assert (err <= tol).all()
    assert abs(got["threshold"] - want["threshold"]) <= tol_thr
    assert clear.mean() >= 0.95
    assert np.array_equal(got["is_outlier"][clear], want["is_outlier"][clear])
    assert 0 < want["is_outlier"].sum() < len(codes)

"""mmd_perm_kernel and mmd_sum_kernel on the hand-built problems of
_mmd_cases.py: cluster problems whose W is an integer count, compared bit for
bit; identity read-outs that compare every K[i, j] on its own against the
pairwise-difference definition in f64, within the per-entry bound derived in
_mmd_cases's docstring from f32 rounding; the extremes of gamma; the binding's
checks; and the engine's refusal of non-finite rows."""

from __future__ import annotations

import functools

import numpy as np
import pytest

import _mmd_cases as mc
from creditcore import mmd

pytestmark = pytest.mark.gpu


def device_args(z, ind):
    import torch

    return (
        torch.from_numpy(mmd.pad_columns(z)).cuda(),
        torch.from_numpy(mmd.squared_norms(z).astype(np.float32)).cuda(),
        torch.from_numpy(np.ascontiguousarray(ind)).cuda(),
    )


def w_gpu(z, gamma, ind, cols, launch_rows=0):
    from creditcore.ops import gpu

    zt, norms, it = device_args(z, ind)
    return gpu.mmd_perm_w(zt, norms, gamma, it, cols, launch_rows=launch_rows)


def w_slice(z, gamma, ind, cols, row_begin, row_count):
    from creditcore.ops import gpu

    zt, norms, it = device_args(z, ind)
    out = gpu.ext().mmd_perm_w(zt, norms, float(gamma), it, cols, row_begin, row_count)
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def read_out(case):
    """(z, gamma, ind, j_q, K[:, j_q] by definition, its bound), computed once."""
    z, gamma, ind, j_q = mc.read_out_problem(case)
    want = mc.k_definition(z, gamma)[:, j_q]
    bound = mc.k_bound(z, gamma, exact_gram=case.dyadic)[:, j_q]
    for a in (want, bound):
        a.setflags(write=False)
    return z, gamma, ind, j_q, want, bound


@pytest.mark.parametrize("case", mc.CLUSTER_CASES, ids=lambda c: c.id)
def test_cluster_counts_bit_exact(case):
    z, gamma, ind, want = mc.cluster_problem(case)
    want = want.astype(np.float64)
    got = w_gpu(z, gamma, ind, case.cols)
    assert got.shape == want.shape and got.dtype == np.float64
    wrong = np.argwhere(got != want)
    print(f"{case.id}: {len(wrong)} of {want.size} counts differ"
          + (f", first at {wrong[0]}: {got[tuple(wrong[0])]} for {want[tuple(wrong[0])]}"
             if len(wrong) else ""))
    assert np.array_equal(got, want)
    assert np.array_equal(w_gpu(z, gamma, ind, case.cols), got)  # run to run
    for launch_rows in (64, 128):
        assert np.array_equal(w_gpu(z, gamma, ind, case.cols, launch_rows=launch_rows), got)
    for a, r in mc.slices_of(case.n):
        assert np.array_equal(w_slice(z, gamma, ind, case.cols, a, r), got[a : a + r]), (a, r)


@pytest.mark.parametrize("case", (*mc.READ_OUT_CASES, mc.ONE_HOT_CASE), ids=lambda c: c.id)
def test_read_out_per_entry(case):
    z, gamma, ind, j_q, want, bound = read_out(case)
    got = w_gpu(z, gamma, ind, case.cols)
    err = np.abs(got - want)
    ratio = err / bound
    at = np.unravel_index(np.argmax(ratio), ratio.shape)
    print(f"{case.id}: gamma {gamma:.4e}; largest error / bound {ratio[at]:.3f} at "
          f"i {at[0]} j {j_q[at[1]]} (error {err[at]:.3e}, bound {bound[at]:.3e}, "
          f"K {want[at]:.3e}); largest error {err.max():.3e}")
    assert (err <= bound).all()
    cols = np.arange(len(j_q))
    assert (got[j_q, cols] == 0.0).all()  # the diagonal is exactly 0
    sub = got[j_q]  # K[j_q, j_q'] against its transpose
    assert (np.abs(sub - sub.T) <= 2.0 * bound[j_q]).all()
    assert np.array_equal(w_gpu(z, gamma, ind, case.cols, launch_rows=64), got)


@pytest.mark.parametrize("cols", [64, 128])
def test_gamma_extremes(cols):
    """On generic rows: with every off-diagonal exponent below -200 every k is
    0 in f32 and so is W; with gamma max d2 < 2^-26 every k is 1 and W counts
    the indicator's other rows."""
    case = mc.ReadOutCase(200, 41, cols, False)
    z = mc.read_out_rows(case)
    ind = mc.make_indicator(case.n, 17)
    d2 = mc.d2_definition(z)
    e_d2 = mc.d2_error(z)
    off = ~np.eye(case.n, dtype=bool)

    big = 400.0 / d2[off].min()
    assert np.float32(big) * (d2 - e_d2)[off].min() > 200.0 and np.isfinite(np.float32(big))
    got = w_gpu(z, big, ind, cols)
    print(f"gamma {big:.3e}: largest W {np.abs(got).max():.3e}")
    assert np.array_equal(got, np.zeros_like(got))

    small = 2.0**-27 / d2.max()
    assert np.float32(small) > 0 and np.float32(small) * (d2 + e_d2).max() < 2.0**-26
    got = w_gpu(z, small, ind, cols)
    want = (ind.sum(axis=0, dtype=np.int64)[None, :] - ind).astype(np.float64)
    print(f"gamma {small:.3e}: largest |W - count| {np.abs(got - want).max():.3e}")
    assert np.array_equal(got, want)


def test_binding_refuses_the_rest():
    """The TORCH_CHECKs of mmd_perm_w that test_mmd_gpu.py leaves uncovered."""
    import torch

    from creditcore.ops import gpu

    f = gpu.ext().mmd_perm_w
    z = torch.zeros(130, 8, device="cuda")
    norms = torch.zeros(130, device="cuda")
    ind = torch.ones(130, 3, dtype=torch.uint8, device="cuda")
    assert f(z, norms, 1.0, ind, 64, 64, 66).shape == (66, 3)  # the arguments are good
    with pytest.raises(RuntimeError):  # row_begin not on a tile
        f(z, norms, 1.0, ind, 64, 32, 10)
    with pytest.raises(RuntimeError):  # row_begin + row_count > N
        f(z, norms, 1.0, ind, 64, 64, 67)
    with pytest.raises(RuntimeError):  # row_begin past N
        f(z, norms, 1.0, ind, 64, 192, -1)
    with pytest.raises(RuntimeError):  # row_count == 0
        f(z, norms, 1.0, ind, 64, 64, 0)
    for gamma in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(RuntimeError):
            f(z, norms, gamma, ind, 64, 0, -1)
    with pytest.raises(RuntimeError):  # ind with another row count
        f(z, norms, 1.0, ind[:129], 64, 0, -1)
    with pytest.raises(RuntimeError):  # N = 1
        f(z[:1], norms[:1], 1.0, ind[:1], 64, 0, -1)
    with pytest.raises(RuntimeError):  # Dp = 0
        f(z[:, :0].contiguous(), norms, 1.0, ind, 64, 0, -1)
    with pytest.raises(RuntimeError):  # a non-contiguous z
        f(torch.zeros(130, 16, device="cuda")[:, ::2], norms, 1.0, ind, 64, 0, -1)
    with pytest.raises(RuntimeError):  # cols_per_block == 0
        f(z, norms, 1.0, ind, 0, 0, -1)
    torch.cuda.synchronize()


def test_engine_refuses_non_finite_rows(packed, score_batch):
    from creditcore.engine import ScoringEngine
    from creditcore.pack import encode_batch

    codes, nums = encode_batch(score_batch.iloc[:40], packed.vocabs)
    mc.check_engine_refuses_non_finite(ScoringEngine(packed, device="cuda"), packed, codes, nums)

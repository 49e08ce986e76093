"""mmd_perm_kernel against the f64 reference cpu_ref.mmd_perm_w_cpu, and a GPU
engine against a CPU engine.

The bound is derived, not tuned. With eps = 2^-24 and c = gamma * max over
i != j of (|z_i|^2 + |z_j|^2) from the test's own data, an entry of K errs by
at most eps (2 c (Dp + 4) + 3) (f32 products and sums of the Gram entry and
the norms, the exponent, exp itself), a row of W adds at most cols_per_block
f32 partial sums per split, so |W_gpu - W_ref| / N <= eps (2 c (Dp + 4) + 3)
+ cols_per_block eps, and every mmd2 errs by at most 4 times that."""

from __future__ import annotations

import numpy as np
import pytest

from creditcore import mmd
from creditcore.ops import cpu_ref

pytestmark = pytest.mark.gpu

EPS = 2.0**-24


def w_bound(z, gamma, cols_per_block):
    top = np.sort(mmd.squared_norms(z))[-2:].sum()
    dp = mmd.pad_columns(z).shape[1]
    return EPS * (2.0 * gamma * top * (dp + 4) + 3.0) + cols_per_block * EPS


def w_gpu(z, gamma, ind, cols_per_block, launch_rows=0):
    import torch

    from creditcore.ops import gpu

    return gpu.mmd_perm_w(
        torch.from_numpy(mmd.pad_columns(z)).cuda(),
        torch.from_numpy(mmd.squared_norms(z).astype(np.float32)).cuda(),
        gamma,
        torch.from_numpy(ind).cuda(),
        cols_per_block,
        launch_rows=launch_rows,
    )


@pytest.mark.parametrize(
    "n,m,d,n_perm,cols,dup",
    [
        (5, 11, 5, 1, 64, False),  # below one tile
        (64, 64, 41, 14, 64, False),  # exact tiles, Q = 16 exact, two splits
        (37, 64, 41, 15, 64, False),  # ragged everything, Q = 17
        (200, 131, 41, 100, 128, False),  # several splits, ragged last one
        (33, 40, 9, 254, 64, False),  # maximum P
        (40, 56, 1000, 14, 64, False),  # wide rows streamed through LDS
        (20, 30, 3, 7, 64, False),  # D = 3, padded by the host
        (37, 64, 41, 15, 64, True),  # exact duplicate rows: k = 1 off the diagonal
    ],
)
def test_kernel_matches_reference(n, m, d, n_perm, cols, dup):
    rng = np.random.default_rng(n * 1000 + d)
    z = rng.normal(size=(n + m, d)).astype(np.float32)
    z[:n] += np.float32(0.25)
    if dup:
        z[1] = z[0]  # inside the batch
        z[n + 1] = z[n]  # inside the reference
        z[n + 2] = z[0]  # across the two
    gamma = mmd.median_gamma(z[n:])
    ind = mmd.indicator(n, m, n_perm, seed=1)
    ref = cpu_ref.mmd_perm_w_cpu(z, gamma, ind)
    got = w_gpu(z, gamma, ind, cols)
    assert got.shape == ref.shape and got.dtype == np.float64
    tol = w_bound(z, gamma, cols)
    err = np.abs(got - ref).max() / (n + m)
    s_err = np.abs(mmd.statistics(got, ind, n, m) - mmd.statistics(ref, ind, n, m)).max()
    print(f"W err / N {err:.3e} (bound {tol:.3e}); mmd2 err {s_err:.3e} (bound {4 * tol:.3e})")
    assert err <= tol
    assert s_err <= 4 * tol
    assert np.array_equal(w_gpu(z, gamma, ind, cols), got)  # run to run
    assert np.array_equal(w_gpu(z, gamma, ind, cols, launch_rows=64), got)  # sliced over i


def test_binding_refuses_bad_shapes():
    import torch

    from creditcore.ops import gpu

    z = torch.zeros(8, 6, device="cuda")
    norms = torch.zeros(8, device="cuda")
    ind = torch.ones(8, 3, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError):  # Dp % 4
        gpu.ext().mmd_perm_w(z, norms, 1.0, ind, 64)
    z = torch.zeros(8, 8, device="cuda")
    with pytest.raises(RuntimeError):  # cols_per_block not a tile multiple
        gpu.ext().mmd_perm_w(z, norms, 1.0, ind, 48)
    with pytest.raises(RuntimeError):  # P > 254
        gpu.ext().mmd_perm_w(z, norms, 1.0, ind.repeat(1, 86), 64)
    with pytest.raises(RuntimeError):  # norms of another length
        gpu.ext().mmd_perm_w(z, norms[:7], 1.0, ind, 64)


def test_engine_gpu_vs_cpu(packed, score_batch):
    from creditcore.engine import ScoringEngine
    from creditcore.pack import encode_batch

    n, m, n_perm, cols = 37, 64, 100, 64
    cpu = ScoringEngine(packed, device="cpu")
    dev = ScoringEngine(packed, device="cuda")
    codes, nums = encode_batch(score_batch.iloc[:n], packed.vocabs)
    ref = (packed.bg_codes[:m], packed.bg_nums[:m])
    mu, sd = mmd.reference_scale(packed, ref[1])
    shift = (0.5 * sd).astype(np.float32)
    for x, drifted in ((nums, False), (nums + shift, True)):
        kw = dict(reference=ref, n_permutations=n_perm, seed=2)
        want = cpu.mmd_drift(codes, x, **kw)
        got = dev.mmd_drift(codes, x, cols_per_block=cols, **kw)
        z = np.concatenate([mmd.embed(packed, codes, x, mu, sd),
                            mmd.embed(packed, ref[0], ref[1], mu, sd)])
        tol = 4 * w_bound(z, want["gamma"], cols)
        ind = mmd.indicator(n, m, n_perm, 2)
        stats = mmd.statistics(cpu_ref.mmd_perm_w_cpu(z, want["gamma"], ind), ind, n, m)
        p_lo = (1 + int((stats[1:] >= stats[0] + tol).sum())) / (n_perm + 1)
        p_hi = (1 + int((stats[1:] >= stats[0] - tol).sum())) / (n_perm + 1)
        print(f"mmd2 gpu {got['mmd2']:.9e} cpu {want['mmd2']:.9e} tol {tol:.3e}; "
              f"p {got['p_val']:.4f} in [{p_lo:.4f}, {p_hi:.4f}]")
        assert got["gamma"] == want["gamma"]
        assert abs(got["mmd2"] - want["mmd2"]) <= tol
        assert p_lo <= got["p_val"] <= p_hi
        if drifted:
            assert got["p_val"] == 1 / (n_perm + 1) and got["is_drift"] == 1

"""Multivariate drift: the MMD two-sample test with a permutation p-value
(the statistic of alibi-detect's MMDDrift), on whole encoded rows.

Everything here is host code shared by the CPU and the GPU engine: the
embedding of rows, the median-heuristic bandwidth, the indicator matrix of the
permutations and the statistics. The one heavy product, ``W = K . ind`` with
the RBF Gram matrix K of the pooled rows, is cpu_ref.mmd_perm_w_cpu on a CPU
engine and mmd_perm_kernel (csrc/creditcore_kernels.hip) on a GPU engine; K
itself is never held.

Pooled order is batch first, then reference: N = n + m rows. Column 0 of
``ind`` is the observed split, columns 1..P are the permutations, column
P + 1 is all ones (row sums of K).
"""

from __future__ import annotations

import numpy as np

from .pack import N_CAT, N_NUM, PackedModel

MMD_MAX_ROWS = 16384  # batch rows per call
MMD_MAX_REFERENCE = 16384  # reference rows per call
MMD_MAX_PERMUTATIONS = 254  # Q = P + 2 <= 256: 64 accumulator registers a lane
MMD_TILE = 64  # rows of a kernel tile; cols_per_block is a multiple of it

_ONE_HOT = np.float32(np.sqrt(0.5))  # a category mismatch adds 1 to d^2


def check_rows(codes, nums, what: str, min_rows: int = 2, caller: str = "mmd_drift"):
    codes = np.ascontiguousarray(codes, dtype=np.int16)
    nums = np.ascontiguousarray(nums, dtype=np.float32)
    r = len(codes)
    if codes.shape != (r, N_CAT) or nums.shape != (r, N_NUM):
        raise ValueError(f"{what} must be (codes [R, {N_CAT}], nums [R, {N_NUM}])")
    if r < min_rows:
        least = "two" if min_rows == 2 else str(min_rows)
        raise ValueError(f"{caller} needs at least {least} {what} rows (got {r})")
    if np.isinf(nums).any():  # NaN is a missing value and is imputed
        raise ValueError(f"{what} rows hold an infinite numeric")
    return codes, nums


def check_embedding(z: np.ndarray, what: str) -> np.ndarray:
    """z unchanged, or ValueError naming the side: every entry of the f32
    embedding and every squared row norm, once cast to f32 (what the kernel is
    given), must be finite. A NaN distance would otherwise read as 0 in the
    kernel (fmaxf) and as NaN in the f64 reference."""
    if not np.isfinite(z).all():
        raise ValueError(f"{what} rows do not embed to finite f32 values")
    with np.errstate(over="ignore"):
        n32 = squared_norms(z).astype(np.float32)
    if not np.isfinite(n32).all():
        raise ValueError(
            f"{what} rows embed too far from the reference: a squared norm overflows f32"
        )
    return z


def check_permutations(n_permutations) -> int:
    p = int(n_permutations)
    if p != n_permutations or not 1 <= p <= MMD_MAX_PERMUTATIONS:
        raise ValueError(
            f"n_permutations must be an integer in [1, {MMD_MAX_PERMUTATIONS}]"
        )
    return p


def impute(packed: PackedModel, nums: np.ndarray) -> np.ndarray:
    nums = np.asarray(nums, dtype=np.float32)
    return np.where(np.isnan(nums), packed.medians[None, :], nums).astype(np.float32)


def reference_scale(packed: PackedModel, ref_nums: np.ndarray):
    """f64 mean and population standard deviation (0 -> 1) of the reference
    sample's imputed numeric columns."""
    x = impute(packed, ref_nums).astype(np.float64)
    mu = x.mean(axis=0)
    sd = x.std(axis=0)
    return mu, np.where(sd == 0.0, 1.0, sd)


def embed(packed: PackedModel, codes: np.ndarray, nums: np.ndarray, mu, sd) -> np.ndarray:
    """Z f32[R, n_onehot + 14]: one-hot block over the scorer's vocabulary
    (a hit is sqrt(0.5), an unknown or missing category all zeros), then the
    imputed numerics standardised by the reference's (mu, sd) in f64 and
    rounded to f32."""
    r = len(codes)
    n_oh = int(packed.n_onehot)
    z = np.zeros((r, n_oh + N_NUM), dtype=np.float32)
    col = np.asarray(packed.feat_col[:n_oh])
    code = np.asarray(packed.feat_code[:n_oh])
    z[:, :n_oh] = (np.asarray(codes)[:, col] == code[None, :]) * _ONE_HOT
    x = impute(packed, nums).astype(np.float64)
    with np.errstate(over="ignore"):  # an overflow is refused by check_embedding
        z[:, n_oh:] = ((x - mu[None, :]) / sd[None, :]).astype(np.float32)
    return z


def squared_norms(z: np.ndarray) -> np.ndarray:
    z = z.astype(np.float64)
    return np.einsum("ij,ij->i", z, z)


def median_gamma(z_ref: np.ndarray) -> float:
    """1 / (lower median of the m (m - 1) / 2 squared distances between
    reference rows i < j), in f64 from the f32 embedding. Holds the upper
    triangle (8 bytes a pair: 1.07 GB at MMD_MAX_REFERENCE); cached by the
    engine per reference sample."""
    z = z_ref.astype(np.float64)
    m = len(z)
    nrm = np.einsum("ij,ij->i", z, z)
    out = np.empty(m * (m - 1) // 2, dtype=np.float64)
    at = 0
    step = max(1, (32 << 20) // (8 * m))
    for a in range(0, m, step):
        b = min(a + step, m)
        d2 = np.maximum(nrm[a:b, None] + nrm[None, :] - 2.0 * (z[a:b] @ z.T), 0.0)
        for i in range(a, b):
            k = m - 1 - i
            out[at : at + k] = d2[i - a, i + 1 :]
            at += k
    mid = (len(out) - 1) // 2
    med = float(np.partition(out, mid)[mid])
    if not med > 0.0:
        raise ValueError("the reference sample's median squared distance is 0")
    return 1.0 / med


def indicator(n: int, m: int, n_permutations: int, seed: int) -> np.ndarray:
    """ind u8[N, P + 2]: column 0 the observed split, column p the rows
    ``rng.permutation(N)[:n]`` of draw p from one default_rng(seed), the last
    column all ones."""
    big = n + m
    ind = np.zeros((big, n_permutations + 2), dtype=np.uint8)
    ind[:n, 0] = 1
    rng = np.random.default_rng(seed)
    for p in range(1, n_permutations + 1):
        ind[rng.permutation(big)[:n], p] = 1
    ind[:, -1] = 1
    return ind


def statistics(w: np.ndarray, ind: np.ndarray, n: int, m: int) -> np.ndarray:
    """mmd2 f64[P + 1] (the unbiased estimator; entry 0 is the observed split)
    from W = K . ind, in f64."""
    w = np.asarray(w, dtype=np.float64)
    a_ind = ind[:, :-1].astype(np.float64)
    A = (a_ind * w[:, :-1]).sum(axis=0)
    C = (a_ind * w[:, -1:]).sum(axis=0)
    T = w[:, -1].sum()
    X = C - A
    B = T - 2.0 * C + A
    return A / (n * (n - 1)) + B / (m * (m - 1)) - 2.0 * X / (n * m)


def decide(mmd2: np.ndarray, drift_p_val: float) -> dict:
    """p-value, decision and threshold statistic from mmd2[0] (observed) and
    mmd2[1:] (permuted), as alibi-detect's MMDDrift reports them."""
    perm = mmd2[1:]
    n_perm = len(perm)
    p_val = (1 + int((perm >= mmd2[0]).sum())) / (n_perm + 1)
    rank = int(drift_p_val * n_perm)
    return {
        "mmd2": float(mmd2[0]),
        "p_val": float(p_val),
        "is_drift": int(p_val < drift_p_val),
        "threshold": float(drift_p_val),
        "distance_threshold": float(np.sort(perm)[::-1][rank]),
    }


def pad_columns(z: np.ndarray, multiple: int = 4) -> np.ndarray:
    """z with D zero-padded to a multiple of 4 (the kernel reads float4)."""
    d = z.shape[1]
    dp = -(-d // multiple) * multiple
    if dp == d:
        return np.ascontiguousarray(z, dtype=np.float32)
    out = np.zeros((len(z), dp), dtype=np.float32)
    out[:, :d] = z
    return out


def default_cols_per_block(n_pooled: int, target_blocks: int = 2048) -> int:
    """Columns j per block: as few splits as fill the GPU (about 2048 blocks
    with the 64-row tiles), each a multiple of the tile."""
    tiles = -(-n_pooled // MMD_TILE)
    splits = max(1, min(tiles, target_blocks // tiles))
    return -(-tiles // splits) * MMD_TILE

"""Hand-built problems, an independent reference, a per-entry error bound and
deliberately wrong emulations for mmd_perm_kernel / mmd_sum_kernel: what
test_mmd_cases.py (CPU) and test_mmd_kernels_gpu.py share (no test in here).

Cluster problems (exact)
    Row j is ``base + 16 e_p`` with p the coordinate of cluster(j): ``base``
    holds small integers, so every product, Gram entry and squared norm is an
    integer far below 2^24 and exact in f32 in any summation order. Squared
    distances are 0 inside a cluster and 16^2 + 16^2 = 512 across, gamma is 1:
    K is 1 inside a cluster, 0 on the diagonal and exp(-512) across, which is
    4e-223 in f64 and rounds to 0 in f32 (below 2^-150). So the kernel must
    return the integer ``W[i, q] = #{j != i: cluster(j) = cluster(i),
    ind[j, q] = 1}`` bit for bit. cluster(j) = (m j + j // 64) % C is not
    periodic in 4, 16 or 64, and the coordinates sit on the edges of the
    kernel's d-chunks (64), MFMA steps (16) and float4 loads (see
    cluster_coordinates).

Read-out problems (per entry)
    ``ind = eye(N)`` gives W = K; for N > 256 the columns are one-hot at
    chosen j (read_out_columns). Rows are either dyadic (multiples of 1/4 in
    [-2, 2]: Gram entries, norms and n_i + n_j - 2 S are exact in f32) or
    generic normal draws.

Reference
    k_definition: f64, from the pairwise differences sum_d (z_id - z_jd)^2.
    It shares no algebra with the kernel or with cpu_ref.mmd_perm_w_cpu, which
    both expand the norms.

Per-entry bound (k_bound), u = 2^-24 the f32 unit roundoff
    The kernel forms, in f32, S = sum_d z_id z_jd (Dp products and sums in
    some order), d2 = max(n_i + n_j - 2 S, 0) from norms that were rounded
    from f64 to f32, x = -gamma_f32 * d2 and k = expf(x). To first order

      |S^ - S|        <= Dp u A_ij            A_ij = sum_d |z_id z_jd|
      |n^ - n|        <= u n                  (the host's cast to f32)
      |fl(n_i + n_j)| adds u (n_i + n_j)
      |fl(. - 2 S)|   adds u |d2^| <= 2 u (n_i + n_j)     (2 |S| <= n_i + n_j)
      E_d2 = u (2 (Dp + 1) A_ij + 4 (n_i + n_j))

    ((Dp + 1) for Dp covers the second-order term of (1 + u)^Dp - 1 for
    Dp <= 4000.) The clamp at 0 moves d2^ towards the true value, never away.
    gamma_f32 and the product each add a relative u:

      E_x = gamma (E_d2 + 2 u (d2 + E_d2))

    and expf is within 1 ulp, a relative 2 u at most, or flushes a result
    below the smallest normal f32 to 0 (2^-126 absolute):

      |k^ - k| <= k expm1(E_x) + 2 u k exp(E_x) + 2^-126

    all but the last term times (1 + 2^-10) for every neglected higher-order
    term (each is below (Dp + 8) u < 2^-16 of a first-order one). On dyadic
    rows S, the norms and d2 are exact, so E_d2 = 0. GEMM 2 adds one k and
    zeros, and the slab sum is exact, so this is the bound on W[i, q] too.

Emulation and mutations
    emulate_w is the kernel's tiling in f64: 64-row i tiles, splits of
    cols_per_block walked in 64-row j tiles, 64-wide d-chunks staged in a
    buffer that keeps its state as LDS does, 16-wide steps, the lane layout
    j = 16 js + 4 g + r of the accumulators, slabs, row slices and the sum
    over splits. A k below 2^-150 is 0, as it is in f32. MUTATIONS names the
    wrong variants it can run instead; each must be seen by a committed case.
    One of them needs two faults at once: the kernel masks rows j >= N, and
    the binding zero-pads the indicator there as well, so dropping the mask
    alone changes nothing (test_mmd_cases.py asserts that); pad_j_unmasked
    drops the mask and fills the indicator's padding with ones.
"""

from __future__ import annotations

import dataclasses

import numpy as np

from creditcore import mmd

U = 2.0**-24
TILE = 64  # rows of an i tile and of a j tile
DC = 64  # d-chunk
STEP = 16  # d covered by the four MFMA steps of one float4 read
F32_FLUSH = 2.0**-150  # a positive value below this rounds to 0 in f32

MUTATIONS = (
    "diag_kept",  # diagonal not zeroed
    "diag_local",  # diagonal zeroed at j == i - row0
    "pad_j_unmasked",  # rows j >= N neither masked nor zero in the indicator
    "ind_bytes_reversed",  # byte r of the indicator dword pairs with j = 4 g + 3 - r
    "ind_g_r_swapped",  # the indicator side reads j = 4 r + g
    "last_chunk_skipped",  # the last of several d-chunks
    "last_step_of_chunk_skipped",  # kk == 3 of every chunk
    "ragged_step_skipped",  # a 16-wide step that is not wholly inside Dp
    "zi_not_reloaded",  # zi_once taken when Dp > 64
    "last_split_dropped",
    "first_split_twice",
    "last_q_tile_dropped",
    "nj_from_lane_g",  # n_j of row 16 js + g instead of 16 js + 4 g + r
    "slice_guard_dropped",  # my_i < row0 + rows: rows past the slice are stored
)


# ------------------------------------------------------------------ reference
def d2_definition(z: np.ndarray) -> np.ndarray:
    """f64[N, N] squared distances from the pairwise differences."""
    z = np.asarray(z, dtype=np.float64)
    out = np.empty((len(z), len(z)), dtype=np.float64)
    for i in range(len(z)):
        diff = z - z[i]
        out[i] = np.einsum("jd,jd->j", diff, diff)
    return out


def k_definition(z: np.ndarray, gamma: float) -> np.ndarray:
    """K f64[N, N]: exp(-gamma sum_d (z_id - z_jd)^2) off the diagonal, 0 on it."""
    k = np.exp(-float(gamma) * d2_definition(z))
    np.fill_diagonal(k, 0.0)
    return k


def d2_error(z: np.ndarray) -> np.ndarray:
    """E_d2 f64[N, N] of the module docstring: the bound on the error of the
    kernel's f32 n_i + n_j - 2 S."""
    z64 = np.asarray(z, dtype=np.float64)
    dp = mmd.pad_columns(np.asarray(z, dtype=np.float32)).shape[1]
    n = mmd.squared_norms(z64)
    a = np.abs(z64) @ np.abs(z64).T
    return U * (2.0 * (dp + 1) * a + 4.0 * (n[:, None] + n[None, :]))


def k_bound(z: np.ndarray, gamma: float, exact_gram: bool = False) -> np.ndarray:
    """f64[N, N] bound on |K_gpu - k_definition| per entry (module docstring)."""
    d2 = d2_definition(z)
    e_d2 = np.zeros_like(d2) if exact_gram else d2_error(z)
    e_x = float(gamma) * (e_d2 + 2.0 * U * (d2 + e_d2))
    k = np.exp(-float(gamma) * d2)
    return (k * np.expm1(e_x) + 2.0 * U * k * np.exp(e_x)) * (1.0 + 2.0**-10) + 2.0**-126


# ------------------------------------------------------------ cluster problems
_CLUSTER_STRIDE = {1: 0, 5: 3, 7: 5}  # m of cluster(j), coprime to C


def cluster_ids(n: int, c: int) -> np.ndarray:
    j = np.arange(n)
    return (_CLUSTER_STRIDE[c] * j + j // 64) % c


def cluster_coordinates(d: int, c: int) -> list[int]:
    """c distinct columns below d, edges first: the last two columns (the last
    float4 of a ragged final chunk; d - 1 is the one real column of the last
    float4 when the host pads D = 4 k + 1), column 0, two in the last 16-wide
    step of chunk 0 (50, 63), the first and last of chunk 1 (64, 127)."""
    want = [d - 1, d - 2, 0, 50, 63, 64, 127, 17, 33, 1, 2, 3]
    cols = []
    for p in want:
        if 0 <= p < d and p not in cols:
            cols.append(p)
    assert len(cols) >= c, (d, c)
    return cols[:c]


@dataclasses.dataclass(frozen=True)
class ClusterCase:
    n: int  # pooled rows N
    d: int  # columns before the host's padding
    cols: int  # cols_per_block
    q: int
    c: int = 7  # clusters

    @property
    def id(self) -> str:
        return f"N{self.n}-d{self.d}-cols{self.cols}-Q{self.q}"


CLUSTER_CASES = (
    ClusterCase(203, 132, 64, 32),  # three chunks, ragged last; four splits; ragged tile
    ClusterCase(203, 132, 128, 32),  # two j tiles a block on the multi-chunk path
    ClusterCase(203, 132, 256, 32),  # cols > N, four tiles in the one split
    ClusterCase(65, 64, 64, 3),  # one live row in the last tile; last zi_once value
    ClusterCase(129, 68, 64, 17),  # second chunk 4 wide; Q one past a q tile
    ClusterCase(128, 48, 64, 16),  # exact tiles; 16-step edge
    ClusterCase(128, 80, 64, 16),  # exact tiles; 16-step edge
    ClusterCase(130, 128, 128, 256),  # two exact chunks; maximum Q
    ClusterCase(2, 4, 64, 1, c=1),  # the smallest legal problem
    ClusterCase(70, 5, 64, 9, c=5),  # D = 5 padded to Dp = 8 by the host
)

SLICES = ((64, 1), (64, 63), (64, 65))  # (row_begin, row_count) of the direct calls


def slices_of(n: int):
    return [(a, r) for a, r in SLICES if a + r <= n]


def make_indicator(n_rows: int, q: int, seed: int = 3) -> np.ndarray:
    """u8[N, Q]: mmd.indicator's columns where Q = P + 2 allows, random bits
    for the narrower ones."""
    if q >= 3:
        n = max(1, (2 * n_rows) // 5)
        return mmd.indicator(n, n_rows - n, q - 2, seed=seed)
    return np.random.default_rng(seed).integers(0, 2, size=(n_rows, q), dtype=np.uint8)


def cluster_problem(case: ClusterCase):
    """(z f32[N, d], gamma = 1.0, ind u8[N, Q], W int64[N, Q] by counting)."""
    cl = cluster_ids(case.n, case.c)
    coords = np.asarray(cluster_coordinates(case.d, case.c))
    base = np.random.default_rng(case.d).integers(-2, 3, size=case.d)
    z = np.tile(base.astype(np.float32), (case.n, 1))
    z[np.arange(case.n), coords[cl]] += np.float32(16.0)
    ind = make_indicator(case.n, case.q)
    same = (cl[:, None] == cl[None, :]).astype(np.int64)
    np.fill_diagonal(same, 0)
    return z, 1.0, ind, same @ ind.astype(np.int64)


# ----------------------------------------------------------- read-out problems
@dataclasses.dataclass(frozen=True)
class ReadOutCase:
    n: int
    d: int
    cols: int
    dyadic: bool

    @property
    def id(self) -> str:
        return f"N{self.n}-d{self.d}-cols{self.cols}-{'dyadic' if self.dyadic else 'generic'}"


READ_OUT_CASES = tuple(
    ReadOutCase(n, d, cols, dyadic)
    for n in (16, 64, 65, 200, 256)
    for d in (5, 41, 64, 68)
    for cols in (64, 128)
    for dyadic in (True, False)
)
ONE_HOT_CASE = ReadOutCase(331, 41, 128, False)


def read_out_rows(case: ReadOutCase) -> np.ndarray:
    rng = np.random.default_rng(1000 * case.n + case.d)
    if case.dyadic:
        return (rng.integers(-8, 9, size=(case.n, case.d)) / 4.0).astype(np.float32)
    z = rng.normal(size=(case.n, case.d)).astype(np.float32)
    z[: case.n // 3] += np.float32(0.25)
    return z


def read_out_columns(n: int) -> np.ndarray:
    """The j read out by the one-hot columns: all of them up to N = 256, else
    the first and last row of every j tile, every (js, g, r) of tile 1, and
    the first and last live row of the ragged last tile."""
    if n <= 256:
        return np.arange(n)
    js = set(range(TILE, 2 * TILE))
    for t in range(0, n, TILE):
        js.update((t, min(t + TILE, n) - 1))
    return np.asarray(sorted(js))


def read_out_problem(case: ReadOutCase):
    """(z, gamma, ind u8[N, Q], j_q int[Q]): W[i, q] = K[i, j_q]."""
    z = read_out_rows(case)
    gamma = mmd.median_gamma(z)
    j_q = read_out_columns(case.n)
    ind = np.zeros((case.n, len(j_q)), dtype=np.uint8)
    ind[j_q, np.arange(len(j_q))] = 1
    return z, gamma, ind, j_q


def dyadic_is_exact(z: np.ndarray) -> bool:
    """Every partial sum of a Gram entry, a norm or n_i + n_j - 2 S of these
    rows is a multiple of 1/16 below 2^24 / 16 in magnitude: exact in f32 in
    any order."""
    z = np.asarray(z, dtype=np.float64)
    on_grid = np.array_equal(z * 4.0, np.rint(z * 4.0))
    return bool(on_grid and 4.0 * (z * z).sum(axis=1).max() * 16.0 < 2.0**24)


# ------------------------------------------------------------------- emulation
def emulate_w(z, gamma, ind, cols, row_begin=0, row_count=None, mutation=None,
              mask_pad_j=True):
    """W[row_begin .. row_begin + row_count) f64[row_count, Q] by the kernel's
    tiling in f64 (module docstring). ``mutation`` is None or one of MUTATIONS;
    ``mask_pad_j=False`` drops the j < N mask alone."""
    assert mutation is None or mutation in MUTATIONS, mutation
    z = mmd.pad_columns(np.asarray(z, dtype=np.float32)).astype(np.float64)
    n, dp = z.shape
    q = ind.shape[1]
    row0 = int(row_begin)
    rows = n - row0 if row_count is None else int(row_count)
    assert cols % TILE == 0 and row0 % TILE == 0 and rows >= 1 and row0 + rows <= n
    n_pad = -(-n // TILE) * TILE
    nqt = -(-q // 16)
    qp = nqt * 16
    splits = -(-n // cols)
    norms = np.zeros(n_pad)
    norms[:n] = mmd.squared_norms(z)
    ind_p = np.zeros((n_pad, qp))
    ind_p[:n, :q] = ind
    if mutation == "pad_j_unmasked":
        ind_p[n:, :q] = 1.0
        mask_pad_j = False

    jl = np.arange(TILE)  # accumulator (js, g, r) holds k[j = 16 js + 4 g + r]
    js, g, r = jl // 16, (jl % 16) // 4, jl % 4
    ind_row = jl
    if mutation == "ind_bytes_reversed":
        ind_row = 16 * js + 4 * g + (3 - r)
    elif mutation == "ind_g_r_swapped":
        ind_row = 16 * js + 4 * r + g
    nj_row = 16 * js + g if mutation == "nj_from_lane_g" else jl

    part = np.full(splits * rows * qp, np.nan)  # torch::empty: nothing is pre-zeroed
    stray = []
    chunks = list(range(0, dp, DC))
    zi_once = dp <= DC or mutation == "zi_not_reloaded"
    for y in range(splits):
        j_begin = y * cols
        j_end = min(j_begin + cols, n)
        for bx in range(-(-rows // TILE)):
            i_base = row0 + bx * TILE
            my_i = i_base + np.arange(TILE)
            i_ok = my_i < n
            n_i = norms[np.minimum(my_i, n_pad - 1)]
            acc = np.zeros((TILE, qp))
            zi_s = np.zeros((TILE, DC))
            zj_s = np.zeros((TILE, DC))
            for j0 in range(j_begin, j_end, TILE):
                s = np.zeros((TILE, TILE))  # [j, i]
                for d0 in chunks:
                    if mutation == "last_chunk_skipped" and len(chunks) > 1 and d0 == chunks[-1]:
                        continue
                    width = min(DC, dp - d0)
                    if not zi_once or j0 == j_begin:
                        zi_s[:] = 0.0
                        live = min(TILE, n - i_base)
                        zi_s[:live, :width] = z[i_base : i_base + live, d0 : d0 + width]
                    zj_s[:] = 0.0
                    live = min(TILE, n - j0)
                    zj_s[:live, :width] = z[j0 : j0 + live, d0 : d0 + width]
                    for kk in range(DC // STEP):
                        if d0 + kk * STEP >= dp:
                            continue
                        if mutation == "last_step_of_chunk_skipped" and kk == DC // STEP - 1:
                            continue
                        if mutation == "ragged_step_skipped" and d0 + (kk + 1) * STEP > dp:
                            continue
                        lo, hi = kk * STEP, (kk + 1) * STEP
                        s += zj_s[:, lo:hi] @ zi_s[:, lo:hi].T
                n_j = norms[j0 + nj_row]
                d2 = np.maximum(n_i[None, :] + n_j[:, None] - 2.0 * s, 0.0)
                k = np.exp(-float(gamma) * d2)
                k[k < F32_FLUSH] = 0.0
                j_glob = (j0 + jl)[:, None]
                keep = np.broadcast_to(i_ok[None, :], k.shape).copy()
                if mask_pad_j:
                    keep &= j_glob < n
                if mutation == "diag_local":
                    keep &= j_glob != (my_i - row0)[None, :]
                elif mutation != "diag_kept":
                    keep &= j_glob != my_i[None, :]
                acc += np.where(keep, k, 0.0).T @ ind_p[j0 + ind_row]
            if mutation == "last_q_tile_dropped":
                acc[:, (nqt - 1) * 16 :] = 0.0
            for il in np.flatnonzero(i_ok):
                local = int(my_i[il]) - row0
                at = (y * rows + local) * qp
                if local < rows:
                    part[at : at + qp] = acc[il]
                elif mutation == "slice_guard_dropped" and at + qp <= len(part):
                    stray.append((at, acc[il].copy()))
    for at, row in stray:  # the unguarded stores race with the owners'; let them win
        part[at : at + qp] = row
    part = part.reshape(splits, rows, qp)
    if mutation == "last_split_dropped" and splits > 1:
        w = part[:-1].sum(axis=0)
    elif mutation == "first_split_twice":
        w = part.sum(axis=0) + part[0]
    else:
        w = part.sum(axis=0)
    return w[:, :q]


# ------------------------------------------------------------ non-finite rows
def check_engine_refuses_non_finite(engine, packed, codes, nums):
    """mmd_drift of ``engine`` refuses infinite numerics and rows whose
    embedding overflows f32, naming the side, leaves no poisoned reference
    cache behind, and still imputes NaN. Shared by the CPU and the GPU test."""
    import pytest

    codes = np.asarray(codes)
    nums = np.asarray(nums, dtype=np.float32)
    ref = (packed.bg_codes[:64], np.asarray(packed.bg_nums[:64], dtype=np.float32))
    kw = dict(n_permutations=10, seed=1)
    good = engine.mmd_drift(codes, nums, reference=ref, **kw)
    assert np.isfinite([good["mmd2"], good["p_val"], good["distance_threshold"]]).all()
    cached = engine._mmd_ref
    assert cached is not None

    big = np.float32(3.0e38)  # finite in f32; its standardised square is not
    _, sd = mmd.reference_scale(packed, ref[1])
    z_big = float(np.float32(big / sd[2]))
    assert np.isfinite(z_big) and z_big**2 > float(np.finfo(np.float32).max)
    for bad in (np.inf, -np.inf, big):
        x = nums.copy()
        x[3, 2] = bad
        with pytest.raises(ValueError, match="batch"):
            engine.mmd_drift(codes, x, reference=ref, **kw)
        assert engine._mmd_ref is cached
    for bad in (np.inf, -np.inf):
        r = ref[1].copy()
        r[5, 2] = bad
        with pytest.raises(ValueError, match="reference"):
            engine.mmd_drift(codes, nums, reference=(ref[0], r), **kw)
        assert engine._mmd_ref is cached  # the good sample is still the cached one
        engine._mmd_ref = None
        with pytest.raises(ValueError, match="reference"):
            engine.mmd_drift(codes, nums, reference=(ref[0], r), **kw)
        assert engine._mmd_ref is None  # nothing was cached for the refused one
        engine._mmd_ref = cached
    # the embedding checks themselves, on values check_rows cannot see
    z = mmd.embed(packed, codes, nums, *mmd.reference_scale(packed, ref[1]))
    for value in (np.inf, np.nan, np.float32(2.0e19)):
        bad_z = z.copy()
        bad_z[1, -1] = value
        for what in ("batch", "reference"):
            with pytest.raises(ValueError, match=what):
                mmd.check_embedding(bad_z, what)
    assert mmd.check_embedding(z, "batch") is z
    assert engine.mmd_drift(codes, nums, reference=ref, **kw) == good

    x = nums.copy()
    x[3, 2] = np.nan  # a missing value: imputed, accepted
    out = engine.mmd_drift(codes, x, reference=ref, **kw)
    assert np.isfinite([out["mmd2"], out["p_val"], out["distance_threshold"]]).all()

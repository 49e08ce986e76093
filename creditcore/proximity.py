"""Forest proximity (Breiman): two rows are as close as the share of the
classifier's trees in which they end in the same leaf. For a batch row i and a
reference row j, ``c(i, j) = #{t : leaf_t(x_i) == leaf_t(r_j)}``, an integer in
[0, T]; the proximity is ``c / T``. It is the model's own metric: a column the
forest never splits on does not count, and a column counts by how often and
where the forest cuts it. Rows are walked exactly as /score walks them (NaN
numerics take the median, an unknown category fails every one-hot test, f32
``v <= thr`` compares), so it serves every family of the packed node table.

Everything here is host code shared by the CPU and the GPU engine. The two
heavy steps are the leaf of every (row, tree), cpu_ref.forest_leaves_cpu or
forest_leaf_kernel, and per batch row the k reference rows in the order
``(c descending, j ascending)``, cpu_ref.forest_prox_topk_cpu or
forest_prox_topk_kernel (csrc/creditcore_kernels.hip); rows that share no leaf
fill the list, lowest j first. The B x M count matrix is never held. All of it
is integer up to the final division, so the two engines agree exactly.

``instance_score`` is ``1 - c_k / T`` (``score="mean"``: 1 - the mean of the k
proximities). The threshold is the ``1 - fpr`` quantile of the reference's own
leave-one-out scores, the pair (j, j) left out by index as knn.threshold does.
"""

from __future__ import annotations

import numpy as np

from .pack import N_CAT, N_NUM

PROX_MAX_ROWS = 16384  # batch rows per call
PROX_MAX_REFERENCE = 16384  # reference rows per call: 14-bit j, u16 row lists
PROX_MAX_K = 32  # key slots of the kernel's selection
PROX_MAX_TREES = 4096  # (T - c) << 14 | j stays a u32 key
SCORES = ("kth", "mean")


def check_rows(codes, nums, what: str, min_rows: int):
    """(codes i16[R, N_CAT], nums f32[R, N_NUM]) contiguous, or ValueError.
    Infinite numerics are fine: a walk only compares them."""
    codes = np.ascontiguousarray(codes, dtype=np.int16)
    nums = np.ascontiguousarray(nums, dtype=np.float32)
    r = len(codes)
    if codes.shape != (r, N_CAT) or nums.shape != (r, N_NUM):
        raise ValueError(f"{what} must be (codes [R, {N_CAT}], nums [R, {N_NUM}])")
    if r < min_rows:
        raise ValueError(f"proximity needs at least {min_rows} {what} row(s) (got {r})")
    return codes, nums


def check_args(k, score, fpr, n_ref: int):
    """(k, score, fpr) validated against a reference of ``n_ref`` rows."""
    kk = int(k)
    if kk != k or not 1 <= kk <= PROX_MAX_K:
        raise ValueError(f"k must be an integer in [1, {PROX_MAX_K}]")
    if kk >= n_ref:
        raise ValueError(
            f"k must be smaller than the number of reference rows ({n_ref}): the "
            "leave-one-out threshold needs k other rows"
        )
    if score not in SCORES:
        raise ValueError(f"score must be one of {SCORES}")
    fpr = float(fpr)
    if not 0.0 < fpr < 1.0:
        raise ValueError("fpr must lie in (0, 1)")
    return kk, score, fpr


def scores(count: np.ndarray, n_trees: int, score: str) -> np.ndarray:
    """f64[B] from the descending shared-leaf counts count[B, k]: one division
    of an integer by an integer per row."""
    count = np.asarray(count, dtype=np.int64)
    if score == "kth":
        return 1.0 - count[:, -1] / float(n_trees)
    return 1.0 - count.sum(axis=1) / float(n_trees * count.shape[1])


def threshold(reference_count: np.ndarray, n_trees: int, score: str, fpr: float) -> float:
    """The 1 - fpr quantile of the reference's leave-one-out scores."""
    return float(np.quantile(scores(reference_count, n_trees, score), 1.0 - fpr))


def lanes_per_tree(leaf_sizes_sq_sum: float, n_entries: int) -> int:
    """Lanes of forest_prox_topk_kernel that share one tree: the power of two
    next above the length of the list a row meets on average (a list of length
    L is met by L of the reference's own rows, hence sum L^2 / sum L), between
    1 and a whole wave. It changes the time, never the result."""
    mean = leaf_sizes_sq_sum / max(n_entries, 1)
    return int(min(64, max(1, 1 << int(np.ceil(np.log2(max(mean, 1.0)))))))


def result(count, idx, reference_count, n_trees: int, k: int, score: str, fpr: float,
           neighbors: bool) -> dict:
    """The response of ScoringEngine.proximity from the batch's neighbours
    (count[B, k] descending, idx[B, k]) and the reference's leave-one-out
    count[M, k]."""
    s = scores(count, n_trees, score)
    thr = threshold(reference_count, n_trees, score, fpr)
    out = {
        "instance_score": s,
        "is_outlier": (s > thr).astype(np.int8),
        "threshold": thr,
        "k": k,
        "score": score,
        "fpr": fpr,
        "n": len(s),
        "n_ref": len(reference_count),
        "n_trees": int(n_trees),
    }
    if neighbors:
        out["neighbor_index"] = np.asarray(idx, dtype=np.int32)
        out["neighbor_proximity"] = np.asarray(count, dtype=np.int64) / float(n_trees)
    return out

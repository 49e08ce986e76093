"""Nearest-neighbour outlier scores (alibi-detect's ``KNN`` detector): a row is
scored by its distance to its k-th nearest row of a reference sample, in the
embedding the MMD drift test uses (creditcore/mmd.py: one-hot block at
sqrt(0.5) per hit, numerics standardised on the reference), so a categorical
mismatch adds 1 to the squared distance.

Everything here is host code shared by the CPU and the GPU engine. The one
heavy step, the k smallest ``d2[i, j] = max(n_i + n_j - 2 z_i . z_j, 0)`` per
batch row in the order ``(d2, j)``, is cpu_ref.knn_topk_cpu on a CPU engine and
knn_topk_kernel (csrc/creditcore_kernels.hip) on a GPU engine; the B x M
distance matrix is never held.

The threshold is alibi-detect's ``infer_threshold``: the reference sample is
scored against itself leave-one-out (the pair (j, j) is left out by index, so
duplicate rows still count as each other's neighbours) and the threshold is
the ``1 - fpr`` quantile of those scores.
"""

from __future__ import annotations

import numpy as np

KNN_MAX_ROWS = 16384  # batch rows per call
KNN_MAX_REFERENCE = 16384  # reference rows per call
KNN_MAX_K = 32  # slots of the kernel's per-row best list
KNN_TILE = 64  # rows of a kernel tile; cols_per_block is a multiple of it
SCORES = ("kth", "mean")


def check_args(k, score, fpr, n_ref: int):
    """(k, score, fpr) validated against a reference of ``n_ref`` rows."""
    kk = int(k)
    if kk != k or not 1 <= kk <= KNN_MAX_K:
        raise ValueError(f"k must be an integer in [1, {KNN_MAX_K}]")
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


def scores(d2: np.ndarray, score: str) -> np.ndarray:
    """f64[B] from the ascending squared neighbour distances d2[B, k]: the
    distance of the k-th neighbour, or the mean of the k distances."""
    dist = np.sqrt(np.asarray(d2, dtype=np.float64))
    return dist[:, -1].copy() if score == "kth" else dist.mean(axis=1)


def threshold(reference_d2: np.ndarray, score: str, fpr: float) -> float:
    """The 1 - fpr quantile of the reference's leave-one-out scores."""
    return float(np.quantile(scores(reference_d2, score), 1.0 - fpr))


def default_cols_per_block(n_batch: int, n_ref: int, target_blocks: int = 1024) -> int:
    """Reference columns per block, a multiple of the tile: as few splits as
    give about 1024 blocks with the 64-row tiles (two rounds of the 512 blocks
    an MI355X holds at two per CU), and no split under four tiles: a row
    meets about k ln(columns / k) candidates below its bound in every split,
    so short splits spend their time sorting."""
    row_tiles = -(-n_batch // KNN_TILE)
    col_tiles = -(-n_ref // KNN_TILE)
    splits = max(1, min(col_tiles // 4, target_blocks // row_tiles))
    return -(-col_tiles // splits) * KNN_TILE


def result(d2, idx, reference_d2, k: int, score: str, fpr: float, neighbors: bool) -> dict:
    """The response of knn_outliers from the batch's neighbours (d2[B, k]
    ascending, idx[B, k]) and the reference's leave-one-out d2[M, k]."""
    s = scores(d2, score)
    thr = threshold(reference_d2, score, fpr)
    out = {
        "instance_score": s,
        "is_outlier": (s > thr).astype(np.int8),
        "threshold": thr,
        "k": k,
        "score": score,
        "fpr": fpr,
        "n": len(s),
        "n_ref": len(reference_d2),
    }
    if neighbors:
        out["neighbor_index"] = np.asarray(idx, dtype=np.int32)
        out["neighbor_distance"] = np.sqrt(np.asarray(d2, dtype=np.float64))
    return out

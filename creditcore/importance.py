"""Permutation feature importance of the classifier (Breiman 2001; the
estimator of ``sklearn.inspection.permutation_importance``): request parsing,
the caps, the permutations, the table of a launch and the metrics.

The forest work (per repeat: every sample row scored with ONE column taken
from another row) is forest_permute_kernel on the GPU and
cpu_ref.forest_permute_cpu on the host; ScoringEngine.permutation_importance
ties them together. Everything in here is host-side numpy and knows nothing
about devices, so both engines return the same numbers.

The importance of a feature in repeat k is ``score(sample) - score(sample
with the feature's column permuted by permutation k)``; a score is one of
SCORINGS on the model's probabilities and the 0/1 labels, each signed so that
higher is better.
"""

from __future__ import annotations

import numpy as np

from .counterfactual import check_threshold  # noqa: F401  (the same rule)
from .schema import FEATURES

# caps of one permutation_importance call (conditions, not measurements)
IMPORTANCE_MAX_ROWS = 65536  # sample rows
IMPORTANCE_MAX_REPEATS = 32  # permutations per feature

# table rows of one kernel job (csrc PERM_ILP): launches are cut at its multiples
PERM_ILP = 4

SCORINGS = ("accuracy", "neg_log_loss", "neg_brier_score", "roc_auc")


class ImportanceTooLarge(ValueError):
    """A permutation-importance request exceeded one of the caps above (the
    engine re-raises it as ExplainTooLarge)."""


def parse_features(features) -> list[str]:
    """``features`` as a list of known, distinct feature names (categorical
    and numeric alike); None means all of them."""
    if features is None:
        return list(FEATURES)
    if isinstance(features, str) or not isinstance(features, (list, tuple)):
        raise ValueError("features must be a list of feature names")
    if not features:
        raise ValueError("features must name at least one feature")
    for n in features:
        if not isinstance(n, str) or n not in FEATURES:
            raise ValueError(f"unknown feature {n!r}")
    if len(set(features)) != len(features):
        raise ValueError("features names a feature twice")
    return list(features)


def check_args(n_repeats, scoring) -> int:
    if isinstance(n_repeats, bool) or not isinstance(n_repeats, (int, np.integer)):
        raise ValueError("n_repeats must be an integer")
    if n_repeats < 1:
        raise ValueError("n_repeats must be at least 1")
    if n_repeats > IMPORTANCE_MAX_REPEATS:
        raise ImportanceTooLarge(f"n_repeats is capped at {IMPORTANCE_MAX_REPEATS}")
    if scoring not in SCORINGS:
        raise ValueError(f"scoring must be one of {SCORINGS} (got {scoring!r})")
    return int(n_repeats)


def check_labels(labels, n_rows: int, scoring: str) -> np.ndarray:
    """The labels as i64[R]: one 0/1 per sample row, at least two rows, and
    both classes where the metric needs them."""
    try:
        y = np.asarray(labels, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError("labels must be a list of 0/1 values") from None
    if len(y) != n_rows:
        raise ValueError(f"labels has {len(y)} entries for {n_rows} sample rows")
    if n_rows < 2:
        raise ValueError("permutation importance needs at least two labelled rows")
    if not np.isin(y, (0.0, 1.0)).all():
        raise ValueError("labels must be 0 or 1")
    if scoring == "roc_auc" and y.min() == y.max():
        raise ValueError("roc_auc needs rows of both classes")
    return y.astype(np.int64)


def permutation_source(permutations, seed, n_features: int, n_repeats: int, n_rows: int):
    """``take(n) -> i32[n, R]``: the next n permutations in (feature in
    request order, repeat) order. One ``rng.permutation(R)`` of
    ``np.random.default_rng(seed)`` each, unless ``permutations``
    ([n_features, n_repeats, R], every row a permutation of 0..R-1) gives
    them."""
    if permutations is not None:
        given = np.asarray(permutations)
        if given.shape != (n_features, n_repeats, n_rows) or given.dtype.kind not in "iu":
            raise ValueError(
                f"permutations must be integers [{n_features}, {n_repeats}, {n_rows}]"
            )
        flat = given.reshape(-1, n_rows)
        if not (np.sort(flat, axis=1) == np.arange(n_rows)).all():
            raise ValueError("every row of permutations must be a permutation of the sample rows")
        flat, at = flat.astype(np.int32), [0]

        def take(n: int) -> np.ndarray:
            at[0] += n
            return flat[at[0] - n : at[0]]

        return take
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or seed < 0:
        raise ValueError("seed must be a non-negative integer")
    rng = np.random.default_rng(int(seed))

    def take(n: int) -> np.ndarray:
        return np.stack([rng.permutation(n_rows) for _ in range(n)]).astype(np.int32)

    return take


def launch_slices(perm_player: np.ndarray, n_rows: int, launch_pairs: int, ilp: int):
    """Table-row slices [a, b) of launches of at most ``launch_pairs`` (table
    row, sample row) pairs (one table row at the least). A slice ends where a
    job ends (a job: up to ``ilp`` consecutive table rows of one player,
    counted from the start of the player's run) unless not even one job
    fits."""
    q = len(perm_player)
    step = max(1, int(launch_pairs) // max(1, n_rows))
    run_start = np.zeros(q, dtype=np.int64)  # first table row of the row's run
    for i in range(1, q):
        run_start[i] = run_start[i - 1] if perm_player[i] == perm_player[i - 1] else i
    out, a = [], 0
    while a < q:
        b = min(a + step, q)
        if b < q and perm_player[b] == perm_player[b - 1]:
            cut = b - (b - run_start[b]) % ilp  # the job boundary at or before b
            if cut > a:
                b = int(cut)
        out.append((a, b))
        a = b
    return out


def _roc_auc(y: np.ndarray, prob: np.ndarray) -> float:
    """Area under the ROC curve as the Mann-Whitney statistic (mid-ranks for
    ties), which is the trapezoid area exactly."""
    from scipy.stats import rankdata

    pos = y == 1
    n1 = int(pos.sum())
    n0 = len(y) - n1
    return float((rankdata(prob)[pos].sum() - n1 * (n1 + 1) / 2.0) / (n1 * n0))


def score(scoring: str, y: np.ndarray, prob: np.ndarray, threshold: float) -> float:
    """One of SCORINGS on labels i64[R] and probabilities f64[R]; higher is
    better. Log loss clips the probabilities to [eps, 1 - eps] (f64 eps), as
    scikit-learn does."""
    if scoring == "accuracy":
        return float(((prob > threshold).astype(np.int64) == y).mean())
    if scoring == "neg_log_loss":
        eps = np.finfo(np.float64).eps
        p = np.clip(prob, eps, 1.0 - eps)
        return float(np.where(y == 1, np.log(p), np.log(1.0 - p)).mean())
    if scoring == "neg_brier_score":
        return float(-((prob - y) ** 2).mean())
    if scoring == "roc_auc":
        return _roc_auc(y, prob)
    raise ValueError(f"scoring must be one of {SCORINGS} (got {scoring!r})")

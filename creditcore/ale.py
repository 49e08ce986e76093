"""Accumulated local effects (ALE, Apley & Zhu 2020) of the classifier on a
numeric feature: request parsing, the edge rule, the caps and the finish of
the raw forest sums into a centred curve.

The forest work (per row: its grid interval and the raw sums at the
interval's two edges) is forest_ale_kernel on the GPU and
cpu_ref.forest_ale_cpu on the host; ScoringEngine.accumulated_local_effects
ties them together. Everything in here is host-side numpy and knows nothing
about devices.

Edge rule, on the imputed sample column: ``z = unique(f32(quantile(col as
f64, linspace(0, 1, K + 1))))`` with linear interpolation, K =
``grid_resolution``; after ``unique`` there are Ke + 1 <= K + 1 edges. A row
with value x lies in interval ``k = clip(searchsorted(z, x, "left"), 1, Ke)``,
i.e. (z[k-1], z[k]] with both ends clamped, all compares in f32. Its local
effect is ``g(S | x = z[k]) - g(S | x = z[k-1])`` (S the raw forest sum, g
pdp.finalize); ``m_k`` is the mean local effect of interval k (0 where no row
lies), ``A_k = A_{k-1} + m_k`` from ``A_0 = 0``, and the curve is A minus its
count-weighted trapezoid mean ``sum n_k (A_{k-1} + A_k) / 2 / sum n_k``.
"""

from __future__ import annotations

import numpy as np

from .pack import N_CAT, N_NUM
from .pdp import (
    PDP_KINDS,
    PDP_RESPONSES,
    PdpTooLarge,
    check_grid_args,
    check_grid_override,
    finalize,
)
from .schema import FEATURES

ALE_KINDS = PDP_KINDS  # "average", or "both" with the per-row local effects
ALE_RESPONSES = PDP_RESPONSES

# caps of one accumulated_local_effects call (conditions, not measurements)
ALE_MAX_ROWS = 65536  # sample rows
ALE_MAX_GRID = 100  # grid_resolution; a grid= override holds at most one more edge
ALE_MAX_ENTRIES = N_NUM  # entries per call


class AleTooLarge(ValueError):
    """An ALE request exceeded one of the caps above (the engine re-raises it
    as ExplainTooLarge)."""


def parse_features(features) -> list[str]:
    """``features`` as a list of known numeric feature names; ValueError on
    anything else (categorical features have no intervals, pairs are out of
    scope), AleTooLarge on the entry cap."""
    if isinstance(features, str) or not isinstance(features, (list, tuple)):
        raise ValueError("features must be a list of feature names")
    if not features:
        raise ValueError("features must name at least one feature")
    for name in features:
        if not isinstance(name, str):
            raise ValueError(f"bad features entry {name!r}: ALE takes single feature names")
        if name not in FEATURES:
            raise ValueError(f"unknown feature {name!r}")
        if FEATURES.index(name) < N_CAT:
            raise ValueError(
                f"{name!r} is categorical: unordered categories have no intervals "
                "to accumulate over"
            )
    if len(features) > ALE_MAX_ENTRIES:
        raise AleTooLarge(f"at most {ALE_MAX_ENTRIES} entries per call")
    return list(features)


def check_args(grid_resolution, grid) -> tuple[int, dict]:
    """(K, overrides) of a call, through pdp's own checks (same cap)."""
    try:
        res, _ = check_grid_args(grid_resolution, (0.0, 1.0))
    except PdpTooLarge as e:
        raise AleTooLarge(str(e)) from None
    return res, check_grid_override(grid)


def quantile_edges(column: np.ndarray, grid_resolution: int) -> np.ndarray:
    """f32 edges of one imputed numeric sample column (module docstring);
    a single edge for a constant column."""
    col = np.asarray(column, dtype=np.float32).astype(np.float64)
    q = np.quantile(col, np.linspace(0.0, 1.0, grid_resolution + 1))
    return np.unique(q.astype(np.float32))


def override_edges(name: str, override) -> np.ndarray:
    """The caller's grid= entry as f32 edges: at least 2 finite, strictly
    ascending float32 numbers."""
    if isinstance(override, np.ndarray):
        override = override.tolist()
    if isinstance(override, (str, bytes)) or not isinstance(override, (list, tuple)):
        raise ValueError(f"grid[{name!r}] must be a list of numbers")
    for v in override:
        if isinstance(v, (bool, str)) or not isinstance(v, (int, float, np.number)):
            raise ValueError(f"grid[{name!r}]: {v!r} is not a number")
    if len(override) > ALE_MAX_GRID + 1:
        raise AleTooLarge(f"grid[{name!r}] is capped at {ALE_MAX_GRID + 1} edges")
    with np.errstate(over="ignore"):
        z = np.asarray(override, dtype=np.float64).astype(np.float32)
    if len(z) < 2 or not np.isfinite(z).all() or not (np.diff(z) > 0).all():
        raise ValueError(
            f"grid[{name!r}] must hold at least 2 finite, strictly ascending float32 edges"
        )
    return z


def edge_table(edge_lists: list[np.ndarray]) -> tuple[np.ndarray, np.ndarray]:
    """The ragged table of a launch: (edge_off i32[E + 1], edges f32)."""
    off = np.zeros(len(edge_lists) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(z) for z in edge_lists])
    return off, np.ascontiguousarray(np.concatenate(edge_lists), dtype=np.float32)


def finish(interval, sums, n_intervals, cls_kind, cls_bias, n_trees, response):
    """(ale f64[Ke + 1], counts i64[Ke], local_effect f64[R]) of one entry
    from its rows' intervals i32[R] and raw sums f64[R, 2]."""
    vals = finalize(np.asarray(sums, dtype=np.float64), cls_kind, cls_bias, n_trees, response)
    local = vals[:, 1] - vals[:, 0]
    slot = np.asarray(interval, dtype=np.int64) - 1
    counts = np.bincount(slot, minlength=n_intervals)
    # bincount adds in row order, in f64
    total = np.bincount(slot, weights=local, minlength=n_intervals)
    mean = np.divide(total, counts, out=np.zeros(n_intervals), where=counts > 0)
    acc = np.concatenate([[0.0], np.cumsum(mean)])
    centre = float((counts * (acc[:-1] + acc[1:]) / 2.0).sum() / counts.sum())
    return acc - centre, counts, local

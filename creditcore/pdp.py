"""Partial dependence and ICE curves of the classifier: request parsing,
grids, the what-if job table and the finalisation of the raw forest sums.

The what-if itself (every sample row scored under every grid point's column
override) is forest_whatif_kernel on the GPU and cpu_ref.forest_whatif_cpu on
the host; ScoringEngine.partial_dependence ties them together. Everything in
here is host-side numpy and knows nothing about devices.

Grid rule (scikit-learn's ``partial_dependence`` rule, on the imputed sample
column, every value rounded to f32 so that the kernel, the reference and
scikit-learn see the same numbers): a numeric column with at most
``grid_resolution`` distinct values takes those values, a wider one takes
``grid_resolution`` equally spaced points between the two empirical
percentiles (``scipy.stats.mstats.mquantiles``, as scikit-learn), and a
degenerate range (both percentiles equal) a single point. A categorical
column takes its whole vocabulary, in vocabulary order.
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .pack import N_CAT
from .schema import FEATURES

# caps of one partial_dependence call (conditions, not measurements)
PDP_MAX_ROWS = 1024  # sample rows
PDP_MAX_GRID = 100  # grid_resolution, and the length of a grid= override
PDP_MAX_PAIR_AXIS = 32  # points per axis of a two-way entry
PDP_MAX_ONE_WAY = len(FEATURES)  # one-way entries per call
PDP_MAX_PAIRS = 8  # two-way entries per call

PDP_KINDS = ("average", "both")
PDP_RESPONSES = ("probability", "raw")


class PdpTooLarge(ValueError):
    """A partial-dependence request exceeded one of the caps above (the
    engine re-raises it as ExplainTooLarge)."""


@dataclass
class Axis:
    """One grid axis: the schema feature index, the values as the caller sees
    them (f32-rounded floats or category strings) and the job-table bits
    (f32 bit patterns or category codes)."""

    name: str
    player: int
    values: list
    bits: np.ndarray  # i32[G]


def parse_features(features) -> list[tuple[str, ...]]:
    """Normalise ``features`` to a list of 1- or 2-tuples of known, distinct
    feature names; ValueError on anything else, PdpTooLarge on the entry
    caps."""
    if isinstance(features, str) or not isinstance(features, (list, tuple)):
        raise ValueError("features must be a list of names or pairs of names")
    if not features:
        raise ValueError("features must name at least one feature")
    out = []
    for entry in features:
        names = (entry,) if isinstance(entry, str) else tuple(entry) if isinstance(
            entry, (list, tuple)
        ) else None
        if names is None or len(names) not in (1, 2) or not all(
            isinstance(n, str) for n in names
        ):
            raise ValueError(f"bad features entry {entry!r}: a name or a pair of names")
        for n in names:
            if n not in FEATURES:
                raise ValueError(f"unknown feature {n!r}")
        if len(names) == 2 and names[0] == names[1]:
            raise ValueError(f"the two features of a pair must differ ({names[0]!r})")
        out.append(names)
    if sum(len(n) == 1 for n in out) > PDP_MAX_ONE_WAY:
        raise PdpTooLarge(f"at most {PDP_MAX_ONE_WAY} one-way entries per call")
    if sum(len(n) == 2 for n in out) > PDP_MAX_PAIRS:
        raise PdpTooLarge(f"at most {PDP_MAX_PAIRS} two-way entries per call")
    return out


def check_grid_args(grid_resolution, percentiles) -> tuple[int, tuple[float, float]]:
    if isinstance(grid_resolution, bool) or not isinstance(grid_resolution, (int, np.integer)):
        raise ValueError("grid_resolution must be an integer")
    if grid_resolution < 2:
        raise ValueError("grid_resolution must be at least 2")
    if grid_resolution > PDP_MAX_GRID:
        raise PdpTooLarge(f"grid_resolution is capped at {PDP_MAX_GRID}")
    try:
        lo, hi = (float(x) for x in percentiles)
    except (TypeError, ValueError):
        raise ValueError("percentiles must be a pair of numbers") from None
    if not (0.0 <= lo < hi <= 1.0):
        raise ValueError("percentiles must satisfy 0 <= low < high <= 1")
    return int(grid_resolution), (lo, hi)


def numeric_grid(column: np.ndarray, grid_resolution: int, percentiles) -> np.ndarray:
    """f32 grid of one imputed numeric sample column (module docstring)."""
    from scipy.stats.mstats import mquantiles

    col = np.asarray(column, dtype=np.float32)
    uniques = np.unique(col)
    if len(uniques) <= grid_resolution:
        return uniques
    lo, hi = mquantiles(col.astype(np.float64), prob=list(percentiles), axis=0)
    if np.float32(lo) == np.float32(hi):
        return np.array([lo], dtype=np.float32)
    return np.linspace(lo, hi, num=grid_resolution, endpoint=True).astype(np.float32)


def _f32_bits(values: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(values, dtype=np.float32).view(np.int32).copy()


def build_axis(name, vocabs, nums_imp, grid_resolution, percentiles, override) -> Axis:
    """The grid axis of one feature: ``override`` (the caller's grid= entry)
    or the rule of the module docstring."""
    player = FEATURES.index(name)
    if player < N_CAT:
        vocab = list(vocabs[player])
        if override is None:
            cats = vocab
        else:
            cats = _as_list(name, override)
            for v in cats:
                if not isinstance(v, str) or v not in vocab:
                    raise ValueError(f"grid[{name!r}]: {v!r} is not a known category")
        bits = np.array([vocab.index(v) for v in cats], dtype=np.int32)
        return Axis(name, player, list(cats), bits)
    if override is None:
        vals = numeric_grid(nums_imp[:, player - N_CAT], grid_resolution, percentiles)
    else:
        raw = _as_list(name, override)
        for v in raw:
            if isinstance(v, (bool, str)) or not isinstance(v, (int, float, np.number)):
                raise ValueError(f"grid[{name!r}]: {v!r} is not a number")
        with np.errstate(over="ignore"):
            vals = np.asarray(raw, dtype=np.float64).astype(np.float32)
        if not np.isfinite(vals).all():
            raise ValueError(f"grid[{name!r}] must hold finite float32 numbers")
    return Axis(name, player, [float(v) for v in vals], _f32_bits(vals))


def _as_list(name: str, override) -> list:
    if isinstance(override, np.ndarray):
        override = override.tolist()
    if isinstance(override, (str, bytes)) or not isinstance(override, (list, tuple)):
        raise ValueError(f"grid[{name!r}] must be a list of values")
    if not override:
        raise ValueError(f"grid[{name!r}] is empty")
    if any(isinstance(v, (list, tuple, dict)) for v in override):
        raise ValueError(f"grid[{name!r}] must be one-dimensional")
    if len(override) > PDP_MAX_GRID:
        raise PdpTooLarge(f"grid[{name!r}] is capped at {PDP_MAX_GRID} values")
    return list(override)


def check_grid_override(grid) -> dict:
    if grid is None:
        return {}
    if not isinstance(grid, dict):
        raise ValueError("grid must map feature names to lists of values")
    for name in grid:
        if name not in FEATURES:
            raise ValueError(f"grid names an unknown feature {name!r}")
    return grid


def entry_jobs(axes: list[Axis]) -> np.ndarray:
    """i32[G, 4] job table of one entry, axis 0 major: {player0, bits0,
    player1, bits1}, player1 = -1 for a one-way entry."""
    if len(axes) == 1:
        a = axes[0]
        jobs = np.zeros((len(a.bits), 4), dtype=np.int32)
        jobs[:, 0], jobs[:, 1], jobs[:, 2] = a.player, a.bits, -1
        return jobs
    a, b = axes
    for ax in axes:
        if len(ax.bits) > PDP_MAX_PAIR_AXIS:
            raise PdpTooLarge(
                f"{ax.name!r} has {len(ax.bits)} grid points; an axis of a pair "
                f"is capped at {PDP_MAX_PAIR_AXIS}"
            )
    jobs = np.zeros((len(a.bits), len(b.bits), 4), dtype=np.int32)
    jobs[:, :, 0], jobs[:, :, 2] = a.player, b.player
    jobs[:, :, 1] = a.bits[:, None]
    jobs[:, :, 3] = b.bits[None, :]
    return jobs.reshape(-1, 4)


def finalize(raw: np.ndarray, cls_kind: int, cls_bias: float, n_trees: int, response: str):
    """Model output per (job, row) from the raw forest sums, with the very
    expressions of cpu_ref.score_forest_cpu."""
    if cls_kind == 1:
        z = raw + cls_bias
        return z if response == "raw" else 1.0 / (1.0 + np.exp(-z))
    return (raw / n_trees).astype(np.float64)


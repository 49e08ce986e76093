"""Single-feature counterfactuals of the classifier: breakpoint tables,
request parsing, the raw-space decision cut and the assembly of the answer.

With every other feature held fixed the model output is piecewise constant in
one numeric feature, and its only breakpoints are the thresholds the forest
tests on that column. For numeric column ``c`` with sorted distinct f32
thresholds ``T[0..K)``, interval ``k`` is ``(T[k-1], T[k]]`` (``T[-1] = -inf``,
``T[K] = +inf``): K + 1 intervals, matching the kernels' ``v <= thr -> left``
rule. A row's own interval ``k0`` is the number of thresholds below its
(imputed) value.

The exact curve of a (row, column) job over all K + 1 intervals is
forest_sweep_kernel on the GPU and cpu_ref.forest_sweep_cpu on the host;
ScoringEngine.counterfactuals ties them together. Categorical features go by
brute force through the what-if kernel of partial dependence (a one-hot test
is no rank interval). Everything in here is host-side numpy and knows nothing
about devices.
"""

from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from .pack import N_NUM, PackedModel
from .schema import FEATURES

# caps of one counterfactuals call (conditions, not measurements)
CF_MAX_ROWS = 1024  # rows per call, as ScoringEngine.SHAP_MAX_ROWS
# curves=True: curve points (probabilities, K + 1 per row and numeric feature)
# returned by one call. A point and its threshold are about 30 bytes of JSON,
# so a response stays near 30 MB.
CF_MAX_CURVE_POINTS = 1 << 20
# deepest tree forest_sweep_kernel walks (its compile-time stack bound,
# SWEEP_MAX_DEPTH in csrc/creditcore_kernels.hip)
SWEEP_MAX_DEPTH = 64


class CfTooLarge(ValueError):
    """A counterfactuals request exceeded one of the caps above (the engine
    re-raises it as ExplainTooLarge)."""


@dataclass
class BreakpointTables:
    """Per numeric column the sorted distinct thresholds, and per classifier
    node the rank of its threshold in its column's list."""

    thresholds: list  # N_NUM arrays f32[K_c], ascending, distinct
    thr: np.ndarray  # f32[sum K_c]: the lists, column after column
    thr_off: np.ndarray  # i32[N_NUM + 1] offsets into thr
    node_rank: np.ndarray  # i32[n_nodes]; -1 for leaves and one-hot nodes
    max_depth: int  # edges on the longest root-to-leaf path of any tree


def forest_depth(nodes: np.ndarray, offsets: np.ndarray) -> int:
    """Edges on the longest root-to-leaf path over all trees (level by level;
    the loop is bounded by the node count, so malformed links cannot spin)."""
    base = np.repeat(offsets[:-1], np.diff(offsets)).astype(np.int64)
    cur = np.asarray(offsets[:-1], dtype=np.int64)
    depth = 0
    for _ in range(len(nodes)):
        split = cur[nodes[cur, 0] >= 0]
        if not len(split):
            break
        cur = np.concatenate([base[split] + nodes[split, 2], base[split] + nodes[split, 3]])
        cur = cur[(cur >= 0) & (cur < len(nodes))]
        depth += 1
    return depth


def build_tables(p: PackedModel) -> BreakpointTables:
    nodes = np.ascontiguousarray(p.cls_nodes, dtype=np.int32)
    feat = nodes[:, 0]
    split = feat >= 0
    safe = np.where(split, feat, 0)
    numeric = split & (p.feat_code[safe] < 0)
    col = np.where(numeric, p.feat_col[safe], -1)
    value = nodes[:, 1].copy().view(np.float32)
    node_rank = np.full(len(nodes), -1, dtype=np.int32)
    thresholds = []
    for c in range(N_NUM):
        own = col == c
        t = np.unique(value[own])  # sorted, distinct (-0.0 and 0.0 are one)
        node_rank[own] = np.searchsorted(t, value[own], side="left")
        thresholds.append(np.ascontiguousarray(t, dtype=np.float32))
    thr_off = np.zeros(N_NUM + 1, dtype=np.int32)
    thr_off[1:] = np.cumsum([len(t) for t in thresholds])
    return BreakpointTables(
        thresholds=thresholds,
        thr=np.ascontiguousarray(np.concatenate(thresholds), dtype=np.float32),
        thr_off=thr_off,
        node_rank=node_rank,
        max_depth=forest_depth(nodes, np.asarray(p.cls_tree_offsets)),
    )


def check_depth(tables: BreakpointTables) -> None:
    if tables.max_depth > SWEEP_MAX_DEPTH:
        raise ValueError(
            f"the forest's deepest tree has depth {tables.max_depth}; the sweep "
            f"kernel walks at most {SWEEP_MAX_DEPTH}"
        )


def own_interval(thresholds: np.ndarray, v) -> np.ndarray:
    """k0: the number of thresholds < v (v already imputed)."""
    return np.searchsorted(thresholds, np.asarray(v, dtype=np.float32), side="left")


def representatives(thresholds: np.ndarray) -> np.ndarray:
    """One f32 value inside each of the K + 1 intervals: T[k] for k < K and
    the next f32 above T[K-1] for the last (any value when K = 0)."""
    t = np.asarray(thresholds, dtype=np.float32)
    last = np.nextafter(t[-1], np.float32(np.inf)) if len(t) else np.float32(0.0)
    return np.append(t, np.float32(last)).astype(np.float32)


def check_threshold(threshold) -> float:
    if isinstance(threshold, (bool, str)) or not isinstance(threshold, (int, float, np.number)):
        raise ValueError("threshold must be a number")
    t = float(threshold)
    if not (0.0 < t < 1.0):
        raise ValueError("threshold must lie strictly between 0 and 1")
    return t


def raw_cut(p: PackedModel, threshold: float) -> float:
    """The decision threshold in the raw space of the forest sums: class 1 is
    ``raw > cut``. Averaging families: threshold * n_trees; boosted families:
    logit(threshold) - bias."""
    if int(getattr(p, "cls_kind", 0)) == 1:
        return math.log(threshold / (1.0 - threshold)) - float(p.cls_bias)
    return float(threshold) * int(p.cls_n_trees)


def parse_features(features) -> list[str]:
    if features is None:
        return list(FEATURES)
    if isinstance(features, str) or not isinstance(features, (list, tuple)):
        raise ValueError("features must be a list of feature names")
    if not features:
        raise ValueError("features must name at least one feature")
    out = []
    for n in features:
        if not isinstance(n, str) or n not in FEATURES:
            raise ValueError(f"unknown feature {n!r}")
        if n not in out:
            out.append(n)
    return out


def sweep_jobs(n_rows: int, cols: list[int]) -> np.ndarray:
    """i32[R * C, 2] job table {row, numeric column}, row major."""
    jobs = np.empty((n_rows, len(cols), 2), dtype=np.int32)
    jobs[:, :, 0] = np.arange(n_rows, dtype=np.int32)[:, None]
    jobs[:, :, 1] = np.asarray(cols, dtype=np.int32)[None, :]
    return jobs.reshape(-1, 2)


def category_jobs(vocabs, players: list[int]) -> np.ndarray:
    """i32[G, 4] what-if job table: every known code of every requested
    categorical column, column after column in vocabulary order."""
    rows = [[pl, code, -1, 0] for pl in players for code in range(len(vocabs[pl]))]
    return np.asarray(rows, dtype=np.int32).reshape(-1, 4)


def side_entry(thresholds, k: int, above: bool, own: float, prob: float) -> dict:
    """The counterfactual on one side: the value of interval ``k`` closest to
    the row's own. Above, that is the next f32 after the interval's lower
    threshold; below, the interval's upper threshold itself."""
    t = np.asarray(thresholds, dtype=np.float32)
    v = np.nextafter(t[k - 1], np.float32(np.inf)) if above else t[k]
    return {"value": float(v), "delta": float(v) - float(own), "probability": float(prob)}

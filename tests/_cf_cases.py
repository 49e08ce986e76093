"""Helpers shared by test_counterfactual.py and test_counterfactual_gpu.py (no
test in here): tiny trained pipelines, hand-built forests for the interval
walk, and forests sized to the sweep kernel's chunk, list and stack bounds."""

from __future__ import annotations

import numpy as np

from _shap_models import N_ONEHOT, f32bits, hand_model
from creditcore.pack import (
    N_CAT,
    N_NUM,
    PackedModel,
    pack_classifier_pipeline,
    pack_drift,
    pack_isolation_forest,
)

# tiny models: tens of trees, depth <= 8. The averaging families take an odd
# tree count: an even count of pure leaves ties at exactly 0.5.
FAMILY_PARAMS = {
    "rf": {"n_estimators": 21, "max_depth": 6, "random_state": 0},
    "et": {"n_estimators": 13, "max_depth": 8, "random_state": 0},
    "gbt": {"n_estimators": 20, "max_depth": 3, "random_state": 0},
    "hgbt": {"n_estimators": 20, "max_depth": 4, "random_state": 0, "device": "cpu"},
}
FAMILIES = tuple(FAMILY_PARAMS)

# the sweep kernel's compile-time shape (csrc/creditcore_kernels.hip); the GPU
# test asserts that the extension agrees
SWEEP_BLOCK = 256
SWEEP_CHUNK = 1024
SWEEP_SEG_CAP = 8
SWEEP_MAX_DEPTH = 64


def fit_pipe(train_df, algorithm: str, params: dict | None = None):
    from creditcore.models.forest import make_classifier_pipeline
    from creditcore.schema import FEATURES, TARGET

    pipe = make_classifier_pipeline(dict(params or FAMILY_PARAMS[algorithm]), algorithm=algorithm)
    pipe.fit(train_df[FEATURES], train_df[TARGET].values.ravel())
    return pipe


def pack_pipe(pipe, detectors) -> PackedModel:
    drift, outlier = detectors
    c = pack_classifier_pipeline(pipe)
    return PackedModel(**c, **pack_isolation_forest(outlier), **pack_drift(drift, c["vocabs"]))


def sample_frame(train_df, n: int = 64):
    """n rows of train_df with NaN numerics and an unknown category."""
    from creditcore.schema import FEATURES

    df = train_df[FEATURES].sample(n, random_state=11).reset_index(drop=True).copy()
    df.loc[0, "bill_amount_3"] = np.nan
    df.loc[5, "credit_limit"] = np.nan
    df.loc[1, "education"] = "phd_never_seen"
    return df


def up(x) -> np.float32:
    return np.nextafter(np.float32(x), np.float32(np.inf))


def down(x) -> np.float32:
    return np.nextafter(np.float32(x), np.float32(-np.inf))


# ------------------------------------------------------------ hand-built trees


def num(j: int) -> int:
    """Virtual feature index of numeric column j in hand_model."""
    return N_ONEHOT + j


def onehot(col: int, code: int) -> int:
    return 2 * col + code


def bfs(tree) -> np.ndarray:
    """[n, 4] BFS node table of a nested tree: a leaf is a number, a split
    ``(feature, threshold, left, right)`` (left: value <= threshold)."""
    rows, queue = [None], [(tree, 0)]
    while queue:
        t, i = queue.pop(0)
        if isinstance(t, tuple):
            left = len(rows)
            rows += [None, None]
            rows[i] = [t[0], f32bits(t[1]), left, left + 1]
            queue += [(t[2], left), (t[3], left + 1)]
        else:
            rows[i] = [-1, f32bits(t), 0, 0]
    return np.asarray(rows, dtype=np.int32)


def forest_of(trees, cls_kind: int = 0, cls_bias: float = 0.0) -> PackedModel:
    tables = [bfs(t) for t in trees]
    return hand_model(tables, [np.ones(len(t)) for t in tables], cls_kind=cls_kind, cls_bias=cls_bias)


SWEPT = 3  # the numeric column the hand-built forest is swept on
OTHER = 5  # a numeric column tested next to it
NAN_COL = 2  # another tested column; a row holds NaN there


def hand_forest(cls_kind: int = 0, cls_bias: float = 0.0) -> PackedModel:
    """Dyadic leaves (sums exact in any order). Column SWEPT carries the
    thresholds -1, 0.5, 1, up(1), 2; see the tests for what each tree is
    there for."""
    s = num(SWEPT)
    one_up = float(up(1.0))
    trees = [
        # nested thresholds: under "<= 1" the test "<= 2" has an empty right,
        # under "> 1" the test "<= 0.5" an empty left
        (s, 1.0, (s, 2.0, 8 / 64, 16 / 64), (s, 0.5, 32 / 64, 4 / 64)),
        # the same threshold twice on a path
        (s, 1.0, (s, 1.0, 2 / 64, 1.0), 1 / 64),
        # never tests the column: a constant over all intervals
        (num(OTHER), 0.0, 3 / 64, 5 / 64),
        # a single leaf
        0.3125,
        # 1.0 shared with the trees above, and a threshold one ulp over it
        (s, one_up, (s, 1.0, 7 / 64, 9 / 64), 11 / 64),
        # one-hot nodes above and below the swept node
        (
            onehot(0, 0), 0.5,
            (s, -1.0, 13 / 64, (onehot(0, 1), 0.5, 17 / 64, 19 / 64)),
            23 / 64,
        ),
        # another tested column, NaN in one row (imputed by the median)
        (num(NAN_COL), -0.5, (s, 2.0, 1 / 32, 3 / 32), (s, -1.0, 5 / 32, 7 / 32)),
    ]
    return forest_of(trees, cls_kind, cls_bias)


def hand_rows() -> tuple[np.ndarray, np.ndarray]:
    """Rows on a threshold, one ulp over it, far out on both sides, NaN in
    the swept column, NaN in another tested column, unknown category."""
    values = [1.0, float(up(1.0)), float(down(1.0)), 1e30, -1e30, np.nan, 0.75, 2.0, -1.0, 1.5]
    n = len(values)
    codes = np.zeros((n, N_CAT), dtype=np.int16)
    nums = np.zeros((n, N_NUM), dtype=np.float32)
    nums[:, SWEPT] = values
    nums[:, OTHER] = [(-1.0) ** i for i in range(n)]
    nums[:, NAN_COL] = np.linspace(-2.0, 1.0, n)
    nums[6, NAN_COL] = np.nan
    codes[:, 0] = [0, 1, -1, 0, 1, -1, -1, 1, 0, -1]
    return codes, nums


# ------------------------------------------------------------- sized forests


def chain(col: int, thresholds, leaves) -> tuple:
    """A left-going chain on numeric column ``col``: thresholds descending
    from the root, every right child a leaf, so all len(thresholds) + 1
    segments are alive and the walk's stack holds len(thresholds) entries."""
    thresholds = sorted((float(t) for t in thresholds), reverse=True)
    assert len(leaves) == len(thresholds) + 1
    node = float(leaves[-1])
    for t, leaf in zip(reversed(thresholds), reversed(leaves[:-1])):
        node = (num(col), t, node, float(leaf))
    return node


def ladder_forest(k: int, sizes=(1, 2, 3, 9, 1, 2, 1), col: int = 0, seed: int = 0) -> PackedModel:
    """A forest with exactly k distinct thresholds 0..k-1 on column ``col``,
    dealt to chains of the cycled ``sizes``: trees of up to 10 segments (more
    than the kernel's segment list holds), a second tree every so often that
    tests another column first, and one single-leaf tree."""
    rng = np.random.default_rng(seed)
    order = rng.permutation(k).astype(np.float64)
    trees, at, i = [], 0, 0
    while at < k:
        n = min(sizes[i % len(sizes)], k - at)
        leaves = rng.integers(-32, 33, size=n + 1) / 64.0
        tree = chain(col, order[at : at + n], leaves)
        if i % 5 == 2:  # decided by the row before the swept nodes
            tree = (num(col + 1), 0.0, tree, float(rng.integers(-32, 33) / 64.0))
        trees.append(tree)
        at += n
        i += 1
    trees += [0.25, (num(col + 2), 0.0, 0.5, -0.5)]
    return forest_of(trees)


def ladder_rows(k: int) -> tuple[np.ndarray, np.ndarray]:
    codes = np.zeros((3, N_CAT), dtype=np.int16)
    nums = np.zeros((3, N_NUM), dtype=np.float32)
    nums[:, 0] = [-5.0, k / 2.0, k + 5.0]
    nums[:, 1] = [-1.0, 1.0, -1.0]
    return codes, nums


def deep_forest(depth: int) -> PackedModel:
    """One chain of ``depth`` splits on column 0 (every push of the walk's
    stack alive at once) next to a stump."""
    rng = np.random.default_rng(depth)
    leaves = rng.integers(-32, 33, size=depth + 1) / 64.0
    return forest_of([chain(0, np.arange(depth), leaves), (num(0), 0.5, 0.25, 0.5)])

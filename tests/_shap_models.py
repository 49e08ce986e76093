"""Models shared by test_shap.py and test_shap_gpu.py: small forests trained on
the suite's train_df and hand-built trees (no test in here)."""

from __future__ import annotations

import numpy as np

from creditcore.pack import (
    N_CAT,
    N_NUM,
    PackedModel,
    _node_values,
    pack_classifier_pipeline,
    pack_drift,
    pack_isolation_forest,
)

N_SRC = N_CAT + N_NUM
N_ONEHOT = 2 * N_CAT  # hand-built models: two categories per column


def fit_packed(train_df, detectors, params: dict, algorithm: str) -> PackedModel:
    """Train one classifier family on train_df and pack it with the given
    (drift, outlier) detectors."""
    from creditcore.models.forest import make_classifier_pipeline
    from creditcore.schema import FEATURES, TARGET

    pipe = make_classifier_pipeline(params, algorithm=algorithm)
    pipe.fit(train_df[FEATURES], train_df[TARGET].values.ravel())
    drift, outlier = detectors
    c = pack_classifier_pipeline(pipe)
    return PackedModel(**c, **pack_isolation_forest(outlier), **pack_drift(drift, c["vocabs"]))


def f32bits(x) -> int:
    return int(np.float32(x).view(np.int32))


def hand_model(trees, covers, cls_kind: int = 0, cls_bias: float = 0.0) -> PackedModel:
    """A PackedModel around hand-written BFS trees ([n, 4] int32 each) with
    per-node covers. Virtual features: 0..17 one-hot (col = f // 2,
    code = f % 2) over 9 two-category columns, 18..31 the 14 numerics."""
    trees = [np.asarray(t, dtype=np.int32) for t in trees]
    covers = [np.asarray(c, dtype=np.float64) for c in covers]
    values = [_node_values(t, w) for t, w in zip(trees, covers)]
    offsets = np.zeros(len(trees) + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([len(t) for t in trees])
    roots = np.array([float(v[0]) for v in values], dtype=np.float64)
    leaf = np.array([[-1, f32bits(0.0), 0, 0]], dtype=np.int32)
    return PackedModel(
        vocabs=[["a", "b"] for _ in range(N_CAT)],
        medians=np.linspace(-1.0, 1.0, N_NUM).astype(np.float32),
        feat_col=np.array(
            [f // 2 for f in range(N_ONEHOT)] + list(range(N_NUM)), dtype=np.int32
        ),
        feat_code=np.array([f % 2 for f in range(N_ONEHOT)] + [-1] * N_NUM, dtype=np.int32),
        n_onehot=N_ONEHOT,
        cls_nodes=np.concatenate(trees),
        cls_tree_offsets=offsets,
        if_nodes=leaf,
        if_tree_offsets=np.array([0, 1], dtype=np.int32),
        if_denom=1.0,
        if_offset=-0.5,
        if_threshold=0.95,
        n_ref=1,
        drift_p_val=0.05,
        ref_sorted=np.zeros(N_NUM, dtype=np.float32),
        ref_sorted_offsets=np.arange(N_NUM + 1, dtype=np.int32),
        ref_cat_counts=np.ones(3 * N_CAT, dtype=np.int32),
        ref_cat_offsets=(3 * np.arange(N_CAT + 1)).astype(np.int32),
        cls_kind=cls_kind,
        cls_bias=cls_bias,
        cls_node_value=np.concatenate(values),
        cls_base_value=float(cls_bias + roots.sum() if cls_kind == 1 else roots.mean()),
        cls_node_cover=np.concatenate(covers).astype(np.float32),
    )


# The caterpillar: one long chain of splits, every off-chain child a leaf.
# Chain split i sits at node 2i, its off-chain leaf at 2i+1 and the next
# chain node at 2i+2. The chain touches all 23 players; categorical column 0
# is split on both of its one-hot features and numeric columns 3 and 9 carry
# two thresholds each, so three players have two splits on the long path.
CATERPILLAR_SPLITS = (
    [(2 * c, 0.5) for c in range(N_CAT)]  # one-hot (col c, code 0)
    + [(N_ONEHOT + j, 0.25 * (j - 6)) for j in range(N_NUM)]
    + [(1, 0.5), (N_ONEHOT + 3, 1.5), (N_ONEHOT + 9, -2.0)]
)


def caterpillar_model() -> PackedModel:
    rng = np.random.default_rng(23)
    n_split = len(CATERPILLAR_SPLITS)
    n = 2 * n_split + 1
    nodes = np.zeros((n, 4), dtype=np.int32)
    cover = np.zeros(n, dtype=np.float64)
    cover[0] = 4096.0
    for i, (feat, thr) in enumerate(CATERPILLAR_SPLITS):
        k = 2 * i
        on_left = i % 3 != 1  # the chain continues left or right, mixed
        nodes[k] = [feat, f32bits(thr), k + 2 if on_left else k + 1, k + 1 if on_left else k + 2]
        nodes[k + 1] = [-1, f32bits(rng.uniform(0.0, 1.0)), 0, 0]
        keep = rng.uniform(0.55, 0.95)
        cover[k + 2] = np.float32(cover[k] * keep)
        cover[k + 1] = cover[k] - cover[k + 2]
    nodes[n - 1] = [-1, f32bits(0.875), 0, 0]
    return hand_model([nodes], [cover])


def caterpillar_rows() -> tuple[np.ndarray, np.ndarray]:
    """Row 0 follows the whole chain; each of the next seven rows breaks one
    chain split (shallow to deepest), so they leave the chain at different
    depths; the last four rows are random (one with a NaN)."""
    rng = np.random.default_rng(5)
    p = caterpillar_model()
    n_split = len(CATERPILLAR_SPLITS)
    codes0 = np.zeros(N_CAT, dtype=np.int16)
    nums0 = np.zeros(N_NUM, dtype=np.float32)
    # column 0: feature 0 (code 0) and feature 1 (code 1) are both on the
    # chain; the code that satisfies both directions is fixed below
    want = {}
    for i, (feat, thr) in enumerate(CATERPILLAR_SPLITS):
        want.setdefault(feat, []).append((thr, i % 3 != 1))  # (thr, go left?)
    for c in range(N_CAT):
        (thr, left) = want[2 * c][0]
        codes0[c] = 1 if left else 0  # one-hot(code 0) <= 0.5 means "not a"
    # feature 1 = (col 0 == "b"): split 23 (i=23, 23 % 3 == 2 -> left) wants
    # the one-hot to be 0, i.e. col 0 != "b"; split 0 (left) wants != "a"
    codes0[0] = -1
    for j in range(N_NUM):
        lo, hi = -np.inf, np.inf
        for thr, left in want[N_ONEHOT + j]:
            if left:
                hi = min(hi, thr)
            else:
                lo = max(lo, thr)
        assert lo < hi
        nums0[j] = hi - 0.125 if np.isfinite(hi) else lo + 0.125
        assert lo < nums0[j] <= hi
    rows_c, rows_n = [codes0.copy()], [nums0.copy()]
    for leave_at in (0, 4, 9, 15, 22, 23, 24):
        c, x = codes0.copy(), nums0.copy()
        feat, thr = CATERPILLAR_SPLITS[leave_at]
        left = leave_at % 3 != 1
        if feat < N_ONEHOT:
            c[feat // 2] = feat % 2 if left else -1
        else:
            x[feat - N_ONEHOT] = thr + 1.0 if left else thr - 1.0
        rows_c.append(c)
        rows_n.append(x)
    for _ in range(4):
        rows_c.append(rng.integers(-1, 2, size=N_CAT).astype(np.int16))
        rows_n.append(rng.normal(0.0, 2.0, size=N_NUM).astype(np.float32))
    rows_n[-1][2] = np.nan
    assert n_split == 26 and len(p.cls_nodes) == 53
    return np.stack(rows_c).astype(np.int16), np.stack(rows_n).astype(np.float32)

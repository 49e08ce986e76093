"""Shared data of test_hrf_deep.py and test_hrf_deep_gpu.py."""

from __future__ import annotations

import numpy as np

from creditcore.models.hrf import HistForestClassifier

DEEP_SEED = 11  # deep_data / fit_deep below grow a tree past level 12 on the CPU


def deep_data(n=2000, seed=DEEP_SEED):
    """n x 9: six continuous columns (up to 256 bins), a coarse one, a one-hot
    one and a constant; labels are one column's sign under heavy noise, so
    min_samples_leaf=1 trees keep splitting far past level 12."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, 9)).astype(np.float32)
    x[:, 6] = rng.integers(0, 5, size=n)
    x[:, 7] = rng.random(n) < 0.3
    x[:, 8] = 1.0
    y = (x[:, 0] + 2.0 * rng.normal(size=n) > 0).astype(np.int64)
    return x, y


def fit_deep(device, dense_levels=8, bootstrap=True, max_depth=16, deep_trees=True):
    clf = HistForestClassifier(
        n_estimators=5, max_depth=max_depth, max_features=3, min_samples_leaf=1,
        bootstrap=bootstrap, random_state=DEEP_SEED, device=device, deep_trees=deep_trees,
    )
    clf._dense_levels = dense_levels
    return clf.fit(*deep_data())


def max_tree_depth(clf) -> int:
    """Deepest node of the forest; a child's id is above its parent's."""
    best = 0
    for i in range(clf.n_trees_):
        t = clf.tree_arrays(i)
        depth = np.zeros(len(t["feature"]), dtype=np.int64)
        for p in np.flatnonzero(t["children_left"] >= 0):
            depth[[t["children_left"][p], t["children_right"][p]]] = depth[p] + 1
        best = max(best, int(depth.max()))
    return best

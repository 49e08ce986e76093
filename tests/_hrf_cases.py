"""Shared cases of test_hrf.py and test_hrf_gpu.py: the feature key of the
specification in Python integers, the hand-built candidate-rule histograms
and forest comparison helpers."""

from __future__ import annotations

import numpy as np

from creditcore.models.forest import make_classifier_pipeline
from creditcore.schema import FEATURES, TARGET

M64 = (1 << 64) - 1


def spec_key(seed, tree, node_id, f):
    """The specified feature key, in Python integers."""
    z = (seed ^ (tree * 0x9E3779B97F4A7C15) ^ (node_id * 0xC2B2AE3D27D4EB4F)
         ^ (f * 0x165667B19E3779F9)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def spec_order(seed, tree, node_id, n_feat):
    """Features by ascending (key, f): order[rank] = feature."""
    return sorted(range(n_feat), key=lambda f: (spec_key(seed, tree, node_id, f), f))


BIN_OFF6 = np.arange(0, 25, 4, dtype=np.int32)  # 6 features x 4 bins


def hand_hist(strength):
    """One slot, W = 120, P = 48. strength[f] = None: feature f is constant
    (all weight in bin 0); s >= 1: bins 0/1 hold 60 weight each and bin 0
    holds 24 - s of the positives (a larger s separates the classes more)."""
    hist = np.zeros((1, 2, 24), dtype=np.int64)
    for f, s in enumerate(strength):
        if s is None:
            hist[0, :, 4 * f] = [48, 120]
        else:
            hist[0, :, 4 * f] = [24 - s, 60]
            hist[0, :, 4 * f + 1] = [24 + s, 60]
    return hist


def candidate_cases(seed=5, tree=3, node_id=17):
    """(name, hist, expected feature) for slot (tree, node_id), F = 6, m = 2."""
    order = spec_order(seed, tree, node_id, 6)
    meta = np.asarray([[tree, node_id]], dtype=np.int32)
    cases = []
    # every feature splits; the strongest ones sit outside the first m ranks
    s = [0] * 6
    for rank, f in enumerate(order):
        s[f] = 2 + rank
    cases.append(("inside_m", hand_hist(s), order[1]))
    # the first three ranks are constant: the set extends to rank 3, no further
    s = [None] * 6
    s[order[3]], s[order[4]], s[order[5]] = 1, 9, 9
    cases.append(("extends", hand_hist(s), order[3]))
    cases.append(("no_split", hand_hist([None] * 6), -1))
    return seed, meta, order, cases


def fit_hrf(df, params, tree_batch=None, algorithm="hrf"):
    pipe = make_classifier_pipeline(params, algorithm=algorithm)
    if tree_batch is not None:
        pipe.named_steps["classifier"]._tree_batch = tree_batch
    pipe.fit(df[FEATURES], df[TARGET].values.ravel())
    return pipe


FOREST_KEYS = ("tree_offsets_", "children_left_", "children_right_", "feature_",
               "threshold_", "value_", "cover_")


def assert_same_forest(a, b):
    for key in FOREST_KEYS:
        u, v = getattr(a, key), getattr(b, key)
        assert u.dtype == v.dtype and u.tobytes() == v.tobytes(), key

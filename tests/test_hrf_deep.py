"""HistForestClassifier(deep_trees=True) on the CPU backend: the segmented
levels change how a level is computed, never the forest (models/hrf.py)."""

from __future__ import annotations

import numpy as np
import pytest
from _hrf_cases import assert_same_forest, fit_hrf
from _hrf_deep_cases import fit_deep, max_tree_depth

from creditcore import train
from creditcore.models import hrf
from creditcore.models.hrf import HistForestClassifier


@pytest.mark.parametrize("bootstrap", [True, False])
def test_shallow_fit_ignores_the_switch(bootstrap):
    a = fit_deep("cpu", bootstrap=bootstrap, max_depth=10, deep_trees=False)
    b = fit_deep("cpu", bootstrap=bootstrap, max_depth=10, deep_trees=True)
    assert max_tree_depth(a) == 10
    assert_same_forest(a, b)


@pytest.mark.parametrize("dense_levels", [0, 3])
def test_segmented_levels_do_not_change_the_forest(dense_levels, monkeypatch):
    ref = fit_deep("cpu", 16)  # every level dense: the plain algorithm, continued
    assert max_tree_depth(ref) > 12
    # 64 KiB of histogram: a level runs in chunks of two slots
    monkeypatch.setattr(hrf, "_CPU_SEG_HIST_BYTES", 1 << 16)
    assert_same_forest(fit_deep("cpu", dense_levels), ref)


def test_deep_forest_packs_and_scores(train_df, score_batch):
    from creditcore.engine import ScoringEngine
    from creditcore.pack import (
        PackedModel,
        encode_batch,
        pack_classifier_pipeline,
        pack_drift,
        pack_isolation_forest,
    )
    from creditcore.schema import FEATURES

    pipe = fit_hrf(train_df, {"n_estimators": 6, "max_depth": 16, "random_state": 1,
                              "device": "cpu", "deep_trees": True})
    assert max_tree_depth(pipe.named_steps["classifier"]) > 12
    drift, outlier = train.fit_detectors(train_df)
    c = pack_classifier_pipeline(pipe)
    packed = PackedModel(**c, **pack_isolation_forest(outlier), **pack_drift(drift, c["vocabs"]))
    codes, nums = encode_batch(score_batch, packed.vocabs)
    eng = ScoringEngine(packed, device="cpu")
    got = eng.score_arrays(codes, nums, with_drift=False)["predictions"]
    want = pipe.predict_proba(score_batch[FEATURES])[:, 1]
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-7)


def test_limits():
    x = np.zeros((2**31 // 255 + 1, 1), dtype=np.float32)
    with pytest.raises(ValueError, match="rows"):
        HistForestClassifier(deep_trees=True, device="cpu").fit(x, np.zeros(len(x)))
    x = np.arange(40, dtype=np.float32).reshape(20, 2)
    with pytest.raises(ValueError, match=r"max_depth must be in \[1, 24\]"):
        HistForestClassifier(deep_trees=True, max_depth=25, device="cpu").fit(x, x[:, 0] > 9)
    assert hrf.MAX_DEPTH_DEEP == 24 and hrf.MAX_DEPTH == 12


def test_search_depth_clamp_and_cli_switch():
    from creditcore import __main__ as cli

    draw = {"max_depth": 30, "criterion": "gini"}
    deep = train._family_params(draw, "hrf", "cpu", deep_trees=True)
    assert deep["max_depth"] == 24 and deep["deep_trees"] is True
    plain = train._family_params(draw, "hrf", "cpu")
    assert plain["max_depth"] == 12 and "deep_trees" not in plain
    for algorithm in ("rf", "hgbt"):
        with pytest.raises(ValueError, match="deep_trees"):
            train._family_params(draw, algorithm, "cpu", deep_trees=True)
        with pytest.raises(SystemExit):
            cli._cmd_train(["--algorithm", algorithm, "--deep-trees"])

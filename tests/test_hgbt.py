"""HistGBTClassifier (creditcore/models/hgbt.py) on the CPU: the numpy
reference of the trainer (device="cpu"), its packing into the node-SoA, and
the public surface (pipeline, lifecycle, CLI). The HIP kernels are tested
against the same references in test_hgbt_gpu.py."""

from __future__ import annotations

import pickle

import numpy as np
import pytest

from creditcore.engine import ScoringEngine
from creditcore.models.forest import make_classifier_pipeline
from creditcore.models.hgbt import HistGBTClassifier, bin_features
from creditcore.ops import cpu_ref
from creditcore.pack import (
    PackedModel,
    build_shap_paths,
    encode_batch,
    pack_classifier_pipeline,
    pack_drift,
    pack_isolation_forest,
)
from creditcore.schema import FEATURES, TARGET
from creditcore.train import fit_detectors


def _stump_data(n=200, t=0.25, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, 2)).astype(np.float32)
    return x, (x[:, 0] > np.float32(t)).astype(np.int64)


def test_stump_picks_the_separating_edge():
    x, y = _stump_data()
    m = HistGBTClassifier(
        n_estimators=1, max_depth=1, learning_rate=1.0, min_samples_leaf=1, device="cpu"
    ).fit(x, y)
    assert m.n_trees_ == 1 and list(m.feature_) == [0, -2, -2]
    lo, hi = x[y == 0, 0].max(), x[y == 1, 0].min()
    assert lo <= m.threshold_[0] < hi  # the one edge between the classes
    assert list(m.cover_) == [len(y), int((y == 0).sum()), int((y == 1).sum())]
    assert (m.predict(x) == y).all()
    assert m.predict_proba(x).shape == (len(x), 2)


def test_tie_break_lowest_feature():
    x, y = _stump_data()
    x[:, 1] = x[:, 0]
    m = HistGBTClassifier(n_estimators=1, max_depth=1, min_samples_leaf=1, device="cpu").fit(x, y)
    assert m.feature_[0] == 0


@pytest.mark.parametrize("case", ["constant_column", "min_samples_leaf"])
def test_no_valid_split_keeps_the_prior(case):
    x, y = _stump_data(n=100)
    kw = {}
    if case == "constant_column":
        x = np.ones((100, 1), dtype=np.float32)
    else:
        kw["min_samples_leaf"] = 51
    m = HistGBTClassifier(n_estimators=3, max_depth=3, device="cpu", **kw).fit(x, y)
    assert list(m.tree_offsets_) == [0, 1, 2, 3] and (m.children_left_ == -1).all()
    # the root's Newton step from the prior is 0 up to the gradient rounding
    assert np.abs(m.value_).max() < 1e-5
    np.testing.assert_allclose(m.predict_proba(x)[:, 1], y.mean(), rtol=0, atol=1e-5)


def test_threshold_exact_for_f32_inputs():
    """bin <= b must be x <= edges[b] for every training value, including
    adjacent floats, quantile bins (> max_bins distinct) and one-hot columns."""
    rng = np.random.default_rng(1)
    n = 3000
    one = np.float32(1.0)
    x = np.stack(
        [
            rng.normal(size=n),  # quantile path
            rng.integers(0, 2, size=n),  # one-hot
            rng.integers(0, 40, size=n) * 0.1,  # few distinct values
            np.where(rng.random(n) < 0.5, one, np.nextafter(one, np.float32(2))),
        ],
        axis=1,
    ).astype(np.float32)
    bins, off, thr = bin_features(x, 256)
    nb = np.diff(off)
    assert nb[0] == 256 and nb[1] == 2 and nb[2] == 40 and nb[3] == 2
    assert thr[off[1]] == np.float32(0.5)
    for f in range(x.shape[1]):
        for b in range(nb[f] - 1):
            np.testing.assert_array_equal(bins[f] <= b, x[:, f] <= thr[off[f] + b])
    # and on a fitted model: every packed split agrees with its bin split
    y = (x[:, 0] + x[:, 2] + rng.normal(size=n) > 2).astype(int)
    m = HistGBTClassifier(n_estimators=5, max_depth=4, device="cpu").fit(x, y)
    inner = np.flatnonzero(m.children_left_ >= 0)
    assert len(inner) > 10
    for i in inner:
        f, t = m.feature_[i], m.threshold_[i]
        b = int(np.flatnonzero(thr[off[f] : off[f + 1]] == t)[0])
        np.testing.assert_array_equal(x[:, f] <= t, bins[f] <= b)


@pytest.fixture(scope="module")
def hgbt_packed(train_df):
    pipe = make_classifier_pipeline(
        {"n_estimators": 30, "max_depth": 4, "random_state": 0, "device": "cpu"},
        algorithm="hgbt",
    )
    pipe.fit(train_df[FEATURES], train_df[TARGET].values.ravel())
    drift, outlier = fit_detectors(train_df)
    c = pack_classifier_pipeline(pipe)
    o = pack_isolation_forest(outlier)
    d = pack_drift(drift, c["vocabs"])
    return PackedModel(**c, **o, **d), pipe


def test_pack_parity(hgbt_packed, score_batch):
    """Same bound as test_gbt.py for sklearn GBT; score_batch carries NaN
    numerics and unknown categories."""
    packed, pipe = hgbt_packed
    clf = pipe.named_steps["classifier"]
    assert packed.cls_kind == 1 and packed.cls_bias == clf.init_raw_
    assert packed.cls_n_trees == 30
    assert (packed.cls_nodes[:, 0] >= 0).sum() > 100
    assert packed.cls_node_cover[0] == 3000
    codes, nums = encode_batch(score_batch, packed.vocabs)
    nums_imp = cpu_ref.impute_nums(packed, nums)
    ours = cpu_ref.score_forest_cpu(packed, codes, nums_imp)
    sk = pipe.predict_proba(score_batch[FEATURES])[:, 1]
    np.testing.assert_allclose(ours, sk, atol=1e-7)


def test_existing_families_pack_through_plain_arrays(train_df):
    """The factored BFS repack: sklearn tree_ and its plain arrays agree."""
    from creditcore.pack import _pack_sklearn_tree, _pack_tree_arrays

    pipe = make_classifier_pipeline(
        {"n_estimators": 3, "max_depth": 5, "random_state": 0}, algorithm="rf"
    )
    pipe.fit(train_df[FEATURES], train_df[TARGET].values.ravel())
    t = pipe.named_steps["classifier"].estimators_[0].tree_
    leaf = np.asarray(t.value)[:, 0, 1]
    a = _pack_sklearn_tree(t, leaf, with_values=True)
    b = _pack_tree_arrays(
        t.children_left, t.children_right, t.feature, t.threshold, leaf,
        cover=t.weighted_n_node_samples,
    )
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()
    assert _pack_sklearn_tree(t, leaf).tobytes() == a[0].tobytes()


def test_explain_additivity(hgbt_packed, score_batch):
    """Saabas and TreeSHAP on the packed hgbt model: base + sum of the
    contributions is the model's log-odds (tolerances of test_explain.py
    and test_shap.py for GBT)."""
    packed, pipe = hgbt_packed
    codes, nums = encode_batch(score_batch.iloc[:64], packed.vocabs)
    nums_imp = cpu_ref.impute_nums(packed, nums)
    score = cpu_ref.score_forest_cpu(packed, codes, nums_imp)
    raw = np.log(score / (1.0 - score))
    eng = ScoringEngine(packed, device="cpu")

    out = eng.explain_arrays(codes, nums)
    assert out["output_space"] == "log_odds"
    assert np.abs(out["contributions"]).max() > 1e-3
    total = packed.cls_base_value + out["contributions"].sum(1)
    np.testing.assert_allclose(total, raw, rtol=0, atol=1e-9)
    sk = pipe.predict_proba(score_batch[FEATURES].iloc[:64])[:, 1]
    np.testing.assert_allclose(1.0 / (1.0 + np.exp(-total)), sk, rtol=0, atol=1e-7)

    out = eng.explain_arrays(codes, nums, method="shap")
    assert out["base_value"] == build_shap_paths(packed)[1]
    total = out["base_value"] + out["contributions"].sum(1)
    np.testing.assert_allclose(total, raw, rtol=0, atol=1e-9)
    np.testing.assert_allclose(out["predictions"], score, rtol=0, atol=1e-9)


def test_pickle_roundtrip(hgbt_packed, score_batch):
    _, pipe = hgbt_packed
    clf = pipe.named_steps["classifier"]
    for k, v in vars(clf).items():  # plain numpy / python state only
        assert isinstance(v, (np.ndarray, int, float, str, type(None))), k
    re = pickle.loads(pickle.dumps(pipe))
    x = score_batch[FEATURES]
    np.testing.assert_array_equal(re.predict_proba(x), pipe.predict_proba(x))
    np.testing.assert_array_equal(re.predict(x), pipe.predict(x))


def test_lifecycle_train_and_register(train_df, tmp_path, monkeypatch):
    from creditcore import registry, train
    from creditcore.models import tpe
    from creditcore.pack import pack_pyfunc_dir

    # one draw from the reference space can ask for ~1000 trees; keep the
    # search small and above the depth cap to see the clamp
    monkeypatch.setattr(
        tpe,
        "reference_space",
        lambda: {
            "n_estimators": tpe.IntDim(8, 12),
            "max_depth": tpe.IntDim(20, 24),
            "criterion": tpe.CatDim(("gini", "entropy")),
        },
    )
    d = str(tmp_path / "model")
    out = train.train_and_register(
        model_dir=d, max_evals=1, df=train_df, register=False,
        algorithm="hgbt", train_device="cpu",
    )
    assert out == d
    m = registry.load_pyfunc_model(d).python_model
    clf = m.classifier.named_steps["classifier"]
    assert isinstance(clf, HistGBTClassifier)
    assert clf.max_depth == 12 and clf.device == "cpu" and 8 <= clf.n_trees_ <= 12
    packed = pack_pyfunc_dir(d)
    assert packed.cls_kind == 1 and packed.cls_n_trees == clf.n_trees_


def test_cli_passes_algorithm_and_device(monkeypatch):
    from creditcore import __main__ as cli
    from creditcore import train

    seen = {}
    monkeypatch.setattr(
        train, "train_and_register", lambda **kw: seen.update(kw) or "uri"
    )
    cli._cmd_train(["--algorithm", "hgbt", "--train-device", "cpu", "--max-evals", "1"])
    assert seen["algorithm"] == "hgbt" and seen["train_device"] == "cpu"
    seen.clear()
    cli._cmd_train(["--algorithm", "hgbt"])
    assert seen["train_device"] == "auto"
    with pytest.raises(SystemExit):
        cli._cmd_train(["--train-device", "tpu"])


def test_rejects_unsupported_settings():
    x, y = _stump_data(n=50)
    with pytest.raises(ValueError, match="max_depth"):
        HistGBTClassifier(max_depth=13, device="cpu").fit(x, y)
    with pytest.raises(ValueError, match="max_bins"):
        HistGBTClassifier(max_bins=257, device="cpu").fit(x, y)
    with pytest.raises(ValueError, match="binary"):
        HistGBTClassifier(device="cpu").fit(x, np.arange(50) % 3)
    with pytest.raises(ValueError, match="finite"):
        HistGBTClassifier(device="cpu").fit(np.full_like(x, np.nan), y)


@pytest.mark.parametrize("seed", range(5))
def test_quality_vs_sklearn_gbt(seed):
    """Held-out ROC-AUC on probabilities vs sklearn GradientBoostingClassifier
    at equal n_estimators=60 / max_depth=3 / learning_rate=0.1, 3000 synthetic
    rows (data seed 100 + seed), 75/25 split (random_state=seed).

    Measured on the CPU, auc_sklearn - auc_hgbt per seed 0..4:
        +0.003724  -0.014685  +0.006779  +0.003244  -0.016387
    (sklearn 0.6978 0.6784 0.6920 0.7065 0.6483; hgbt 0.6941 0.6930 0.6852
    0.7033 0.6647). Worst gap +0.006779, sample standard deviation of the
    gap across the seeds 0.011118: margin = 0.006779 + 0.011118 = 0.0179."""
    from sklearn.metrics import roc_auc_score
    from sklearn.model_selection import train_test_split

    from creditcore.data import make_uci_shaped_frame

    margin = 0.0179
    df = make_uci_shaped_frame(n_rows=3000, seed=100 + seed)
    tr, te = train_test_split(df, test_size=0.25, random_state=seed)
    auc = {}
    for algo, extra in (("gbt", {}), ("hgbt", {"device": "cpu"})):
        pipe = make_classifier_pipeline(
            {"n_estimators": 60, "max_depth": 3, "learning_rate": 0.1,
             "random_state": 0, **extra},
            algo,
        )
        pipe.fit(tr[FEATURES], tr[TARGET].values.ravel())
        auc[algo] = roc_auc_score(te[TARGET], pipe.predict_proba(te[FEATURES])[:, 1])
    print(f"seed {seed}: sklearn {auc['gbt']:.6f} hgbt {auc['hgbt']:.6f} "
          f"gap {auc['gbt'] - auc['hgbt']:+.6f}")
    assert auc["hgbt"] >= auc["gbt"] - margin

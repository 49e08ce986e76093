"""HistForestClassifier (creditcore/models/hrf.py) on the CPU: the numpy
reference of the tree-batched trainer (device="cpu"), its packing as a
leaf-mean forest, and the public surface (pipeline, lifecycle, CLI). The HIP
kernels are tested against the same references in test_hrf_gpu.py."""

from __future__ import annotations

from fractions import Fraction

import numpy as np
import pytest

from _hrf_cases import (
    BIN_OFF6,
    assert_same_forest,
    candidate_cases,
    fit_hrf,
    hand_hist,
    spec_key,
    spec_order,
)

from creditcore.engine import ScoringEngine
from creditcore.models import hrf
from creditcore.models.forest import make_classifier_pipeline
from creditcore.models.hrf import HistForestClassifier, bootstrap_weights
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

def test_keys_match_the_specification():
    got = cpu_ref.hrf_feature_keys(2**63 + 12345, [0, 7, 499], [0, 3, 4094], 9)
    assert got.dtype == np.uint64 and got.shape == (3, 9)
    for i, (t, nd) in enumerate(((0, 0), (7, 3), (499, 4094))):
        assert [int(k) for k in got[i]] == [spec_key(2**63 + 12345, t, nd, f) for f in range(9)]
    assert cpu_ref.HRF_C1 % 2 == cpu_ref.HRF_C2 % 2 == cpu_ref.HRF_C3 % 2 == 1


# -- 1. bootstrap ------------------------------------------------------------
def test_bootstrap_weights():
    n = 500
    w = [bootstrap_weights(11, t, n) for t in range(4)]
    for t, wt in enumerate(w):
        assert wt.dtype == np.uint8 and wt.sum() == n
        ref = np.bincount(np.random.default_rng([11, t]).integers(0, n, n), minlength=n)
        np.testing.assert_array_equal(wt, ref)
        np.testing.assert_array_equal(wt, bootstrap_weights(11, t, n))
    assert not (w[0] == w[1]).all() and not (w[1] == w[2]).all()
    assert not (w[0] == bootstrap_weights(12, 0, n)).all()
    np.testing.assert_array_equal(bootstrap_weights(11, 3, n, bootstrap=False), np.ones(n))


# -- 2. candidate rule ---------------------------------------------------------
def test_candidate_rule():
    seed, meta, order, cases = candidate_cases()
    got = {}
    for name, hist, want in cases:
        rec = cpu_ref.hrf_split_cpu(hist, BIN_OFF6, meta, 2, 1, seed)
        assert rec.shape == (1, cpu_ref.HRF_REC)
        assert rec[0, 1] == want, name
        assert list(rec[0, 5:7]) == [48, 120]
        got[name] = rec[0]
    # chosen within the candidate set {rank 0, rank 1}; higher proxy wins
    assert got["inside_m"][1] in order[:2] and got["inside_m"][2] == 0
    pl, wl = got["inside_m"][3:5]
    assert (pl, wl) == (24 - 3, 60)
    proxy = got["inside_m"][:1].view(np.float64)[0]
    assert proxy == (21.0 * 21.0) / 60.0 + (27.0 * 27.0) / 60.0 - (48.0 * 48.0) / 120.0
    # with m = 6 the strongest feature (rank 5) wins instead
    rec = cpu_ref.hrf_split_cpu(cases[0][1], BIN_OFF6, meta, 6, 1, seed)
    assert rec[0, 1] == order[5]
    # extension: rank 3 is taken although ranks 4 and 5 split much better
    assert got["extends"][1] == order[3] and got["extends"][3] == 23
    # leaf record: feat -1 and zeros, totals still reported
    assert list(got["no_split"][:5]) == [0, -1, 0, 0, 0]


def test_split_ties_and_min_leaf():
    seed, meta, order, _ = candidate_cases()
    # identical features tie on the proxy: the lower rank wins
    rec = cpu_ref.hrf_split_cpu(hand_hist([4] * 6), BIN_OFF6, meta, 6, 1, seed)
    assert rec[0, 1] == order[0]
    # bins 1 and 2 empty: "<= 0", "<= 1", "<= 2" are one split; lowest bin
    hist = np.zeros((1, 2, 4), dtype=np.int64)
    hist[0, :, 0], hist[0, :, 3] = [5, 40], [30, 40]
    rec = cpu_ref.hrf_split_cpu(hist, np.asarray([0, 4], dtype=np.int32), meta, 1, 1, seed)
    assert list(rec[0, 1:5]) == [0, 0, 5, 40]
    # min_samples_leaf counts weight on both sides
    assert cpu_ref.hrf_split_cpu(hist, np.asarray([0, 4]), meta, 1, 40, seed)[0, 1] == 0
    assert cpu_ref.hrf_split_cpu(hist, np.asarray([0, 4]), meta, 1, 41, seed)[0, 1] == -1


# -- 3. split optimality ---------------------------------------------------------
def test_root_split_is_the_exhaustive_optimum():
    rng = np.random.default_rng(4)
    n, n_feat = 400, 5
    x = rng.integers(0, 16, size=(n, n_feat)).astype(np.float32)
    y = ((x[:, 1] > 8) ^ (x[:, 3] < 3) ^ (rng.random(n) < 0.15)).astype(np.int64)
    m = HistForestClassifier(
        n_estimators=4, max_depth=3, max_features=None, bootstrap=False,
        random_state=9, device="cpu",
    ).fit(x, y)

    p_all, w_all = int(y.sum()), n
    best, best_at = None, []
    for f in range(n_feat):
        for v in np.unique(x[:, f])[:-1]:
            left = x[:, f] <= v
            wl, pl = int(left.sum()), int(y[left].sum())
            wr, pr = w_all - wl, p_all - pl
            # Gini decrease * W / 2, exactly
            dec = Fraction(pl * pl, wl) + Fraction(pr * pr, wr) - Fraction(p_all * p_all, w_all)
            if best is None or dec > best:
                best, best_at = dec, []
            if dec == best:
                best_at.append((f, float(v)))
    assert best > 0
    # ties: the lower-ranked feature of the root of tree 0, then the lowest threshold
    rank = {f: r for r, f in enumerate(spec_order(9, 0, 0, n_feat))}
    f_want, v_want = min(best_at, key=lambda fv: (rank[fv[0]], fv[1]))
    assert m.feature_[0] == f_want
    np.testing.assert_array_equal(x[:, f_want] <= m.threshold_[0], x[:, f_want] <= v_want)

    first = m.tree_arrays(0)
    assert len(first["feature"]) > 3
    for i in range(1, m.n_trees_):
        for key, ref in first.items():
            assert m.tree_arrays(i)[key].tobytes() == ref.tobytes(), (i, key)


# -- 4. min_samples_leaf, pure nodes, values -----------------------------------------
def node_sums(tree, x, y, w):
    """(P, W) per node from the training rows, routed with x <= threshold."""
    n_nodes = len(tree["feature"])
    p_sum = np.zeros(n_nodes, dtype=np.int64)
    w_sum = np.zeros(n_nodes, dtype=np.int64)
    at = np.zeros(len(x), dtype=np.int64)
    live = np.arange(len(x))
    while len(live):
        np.add.at(w_sum, at[live], w[live])
        np.add.at(p_sum, at[live], w[live] * y[live])
        nd = at[live]
        inner = tree["children_left"][nd] >= 0
        live, nd = live[inner], nd[inner]
        go_left = x[live, tree["feature"][nd]] <= tree["threshold"][nd]
        at[live] = np.where(go_left, tree["children_left"][nd], tree["children_right"][nd])
    return p_sum, w_sum


def test_min_samples_leaf_pure_nodes_and_values():
    rng = np.random.default_rng(6)
    n = 600
    x = rng.normal(size=(n, 6)).astype(np.float32)
    x[:, 4] = rng.integers(0, 3, size=n)
    y = ((x[:, 0] > 0.3) | ((x[:, 1] < -1) & (x[:, 4] == 2))).astype(np.int64)  # no noise: pure nodes
    min_leaf = 7
    m = HistForestClassifier(
        n_estimators=6, max_depth=6, min_samples_leaf=min_leaf, random_state=2, device="cpu"
    ).fit(x, y)
    n_pure_leaves = 0
    for i in range(m.n_trees_):
        t = m.tree_arrays(i)
        w = bootstrap_weights(2, i, n).astype(np.int64)
        p_sum, w_sum = node_sums(t, x, y, w)
        np.testing.assert_array_equal(t["cover"], w_sum)
        assert t["cover"][0] == n and t["cover"].dtype == np.int64
        np.testing.assert_array_equal(t["value"], (p_sum / w_sum).astype(np.float32))
        leaf = t["children_left"] < 0
        assert (t["cover"][leaf] >= min_leaf).all() and (t["cover"] >= min_leaf).all()
        pure = (p_sum == 0) | (p_sum == w_sum)
        assert leaf[pure].all()  # a pure node never splits
        n_pure_leaves += int(pure.sum())
        assert (~leaf).sum() >= 2
    assert n_pure_leaves >= m.n_trees_


# -- 5. batching invariance -----------------------------------------------------------
def test_tree_batch_does_not_change_the_forest(train_df):
    params = {"n_estimators": 8, "max_depth": 5, "random_state": 3, "device": "cpu"}
    ref = fit_hrf(train_df, params, 1).named_steps["classifier"]
    assert ref.n_trees_ == 8 and ref.fit_device_ == "cpu"
    assert (np.diff(ref.tree_offsets_) > 7).all()
    assert ref.tree_arrays(0)["feature"].tobytes() != ref.tree_arrays(1)["feature"].tobytes()
    for tb in (3, 8):
        assert_same_forest(fit_hrf(train_df, params, tb).named_steps["classifier"], ref)
    assert_same_forest(fit_hrf(train_df, params).named_steps["classifier"], ref)
    assert hrf.tree_batch_size(1000, 10**6, 3456, 8, 1) == (1 << 30) // (128 * 2 * 3456 * 8)
    assert hrf.tree_batch_size(100, 10**6, 262144, 12, 1) == 1
    assert hrf.tree_batch_size(10, 50, 100, 12, 40) == 10  # slot floor of 1


# -- 6. quality --------------------------------------------------------------------------
def test_quality_vs_sklearn_random_forest():
    """Held-out ROC-AUC against sklearn RandomForestClassifier at equal
    n_estimators=100 / max_depth=8 / max_features="sqrt": 3000 rows of
    make_uci_shaped_frame (seed 7), 75/25 split (random_state 0). hrf must
    reach sklearn's mean over five seeds minus sklearn's own max - min range.

    Measured (profiles/bench_results/hrf_quality.txt):
        sklearn random_state 0..4: 0.654643 0.642860 0.654473 0.661436 0.656030
        mean 0.653888, range 0.018576, bound 0.635312; hrf (random_state 0) 0.656045"""
    from sklearn.metrics import roc_auc_score
    from sklearn.model_selection import train_test_split

    from creditcore.data import make_uci_shaped_frame

    df = make_uci_shaped_frame(n_rows=3000, seed=7)
    tr, te = train_test_split(df, test_size=0.25, random_state=0)
    common = {"n_estimators": 100, "max_depth": 8, "max_features": "sqrt"}

    def auc(pipe):
        return roc_auc_score(te[TARGET], pipe.predict_proba(te[FEATURES])[:, 1])

    sk = np.asarray([
        auc(fit_hrf(tr, {**common, "random_state": s}, algorithm="rf")) for s in range(5)
    ])
    ours = auc(fit_hrf(tr, {**common, "random_state": 0, "device": "cpu"}))
    bound = sk.mean() - (sk.max() - sk.min())
    print("sklearn", " ".join(f"{v:.6f}" for v in sk), f"mean {sk.mean():.6f}",
          f"range {sk.max() - sk.min():.6f} bound {bound:.6f} hrf {ours:.6f}")
    assert ours >= bound


# -- 7. pack and serve on the CPU engine ---------------------------------------------------
@pytest.fixture(scope="module")
def hrf_packed(train_df):
    pipe = fit_hrf(train_df, {"n_estimators": 30, "max_depth": 6, "random_state": 0, "device": "cpu"})
    drift, outlier = fit_detectors(train_df)
    c = pack_classifier_pipeline(pipe)
    return PackedModel(**c, **pack_isolation_forest(outlier), **pack_drift(drift, c["vocabs"])), pipe


def test_pack_parity(hrf_packed, score_batch):
    packed, pipe = hrf_packed
    assert packed.cls_kind == 0 and packed.cls_bias == 0.0 and packed.cls_n_trees == 30
    assert (packed.cls_nodes[:, 0] >= 0).sum() > 300
    assert packed.cls_node_cover[0] == 3000
    codes, nums = encode_batch(score_batch, packed.vocabs)
    ours = cpu_ref.score_forest_cpu(packed, codes, cpu_ref.impute_nums(packed, nums))
    sk = pipe.predict_proba(score_batch[FEATURES])
    np.testing.assert_allclose(ours, sk[:, 1], rtol=0, atol=1e-9)
    np.testing.assert_allclose(sk.sum(1), 1.0, rtol=0, atol=1e-15)
    np.testing.assert_array_equal(pipe.predict(score_batch[FEATURES]), (sk[:, 1] > 0.5).astype(int))


def test_explain_additivity(hrf_packed, score_batch):
    """Saabas (1e-12, test_explain.py's RF bound) and TreeSHAP (1e-9,
    test_shap.py's) on the packed model: base + sum == the probability."""
    packed, _ = hrf_packed
    codes, nums = encode_batch(score_batch.iloc[:64], packed.vocabs)
    score = cpu_ref.score_forest_cpu(packed, codes, cpu_ref.impute_nums(packed, nums))
    eng = ScoringEngine(packed, device="cpu")

    out = eng.explain_arrays(codes, nums)
    assert out["output_space"] == "probability"
    assert np.abs(out["contributions"]).max() > 1e-3
    total = packed.cls_base_value + out["contributions"].sum(1)
    np.testing.assert_allclose(total, score, rtol=0, atol=1e-12)

    out = eng.explain_arrays(codes, nums, method="shap")
    assert out["base_value"] == build_shap_paths(packed)[1]
    assert np.abs(out["contributions"]).max() > 1e-3
    total = out["base_value"] + out["contributions"].sum(1)
    np.testing.assert_allclose(total, score, rtol=0, atol=1e-9)
    np.testing.assert_allclose(out["predictions"], score, rtol=0, atol=1e-9)


def test_fitted_state_is_plain(hrf_packed, score_batch):
    import pickle

    _, pipe = hrf_packed
    clf = pipe.named_steps["classifier"]
    for k, v in vars(clf).items():
        assert isinstance(v, (np.ndarray, int, float, str, bool, type(None))), k
    re = pickle.loads(pickle.dumps(pipe))
    x = score_batch[FEATURES]
    np.testing.assert_array_equal(re.predict_proba(x), pipe.predict_proba(x))


# -- 8. lifecycle ------------------------------------------------------------------------------
def test_cli_trains_a_loadable_model(train_df, tmp_path, monkeypatch):
    from creditcore import __main__ as cli
    from creditcore import registry
    from creditcore.models import tpe
    from creditcore.pack import pack_pyfunc_dir

    # a draw from the reference space can ask for ~1000 trees: keep the search
    # small, above the depth cap to see the clamp, and with both criteria
    monkeypatch.setattr(
        tpe,
        "reference_space",
        lambda: {
            "n_estimators": tpe.IntDim(6, 10),
            "max_depth": tpe.IntDim(20, 24),
            "criterion": tpe.CatDim(("gini", "entropy")),
        },
    )
    csv = tmp_path / "train.csv"
    train_df.to_csv(csv, index=False)
    d = str(tmp_path / "model")
    cli._cmd_train(["--algorithm", "hrf", "--train-device", "cpu", "--max-evals", "2",
                    "--model-dir", d, "--no-register", "--data", str(csv)])
    clf = registry.load_pyfunc_model(d).python_model.classifier.named_steps["classifier"]
    assert isinstance(clf, HistForestClassifier)
    assert clf.max_depth == 12 and clf.device == "cpu" and 6 <= clf.n_trees_ <= 10
    packed = pack_pyfunc_dir(d)
    assert packed.cls_kind == 0 and packed.cls_n_trees == clf.n_trees_
    with pytest.raises(SystemExit):
        cli._cmd_train(["--algorithm", "hrf", "--train-device", "tpu"])


# -- 9. parameter validation ------------------------------------------------------------------------
def test_rejects_unsupported_settings():
    rng = np.random.default_rng(0)
    x = rng.normal(size=(50, 3)).astype(np.float32)
    y = (x[:, 0] > 0).astype(np.int64)

    def fit(xx=x, yy=y, **kw):
        return HistForestClassifier(n_estimators=2, device="cpu", **kw).fit(xx, yy)

    with pytest.raises(ValueError, match="max_depth"):
        fit(max_depth=13)
    with pytest.raises(ValueError, match="max_depth"):
        fit(max_depth=0)
    with pytest.raises(ValueError, match="max_bins"):
        fit(max_bins=257)
    for bad in ("log2", 0, 4, 0.5, True):
        with pytest.raises(ValueError, match="max_features"):
            fit(max_features=bad)
    with pytest.raises(ValueError, match="1024 features"):
        fit(xx=np.zeros((50, 1025), dtype=np.float32))
    with pytest.raises(ValueError, match="binary"):
        fit(yy=np.arange(50) % 3)
    with pytest.raises(ValueError, match="finite"):
        fit(xx=np.where(np.arange(150).reshape(50, 3) == 7, np.inf, x))
    with pytest.raises(TypeError):  # Gini only: there is no criterion knob
        HistForestClassifier(criterion="entropy")
    # ... and the pipeline factory drops the search space's draw
    pipe = make_classifier_pipeline({"criterion": "entropy", "max_depth": 20}, "hrf")
    assert pipe.named_steps["classifier"].max_depth == hrf.MAX_DEPTH
    assert fit(max_features=3).n_trees_ == 2 and fit(max_features=None).n_trees_ == 2
    assert hrf.resolve_max_features("sqrt", 51) == 7 and hrf.resolve_max_features("sqrt", 1) == 1

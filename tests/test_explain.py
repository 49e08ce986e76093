"""Per-row feature attributions ("reason codes"): the prediction-path
(Saabas) decomposition of the classifier forest — pack (per-node expected
values), CPU reference, engine API and POST /explain. The decomposition is
exact by construction: base_value + contributions.sum(1) == model output."""

from __future__ import annotations

import numpy as np
import pytest

from creditcore.engine import ExplainTooLarge, ExplainUnavailable, ScoringEngine
from creditcore.models.forest import make_classifier_pipeline
from creditcore.ops import cpu_ref
from creditcore.pack import (
    N_CAT,
    N_NUM,
    PackedModel,
    _node_values,
    encode_batch,
    pack_classifier_pipeline,
    pack_drift,
    pack_isolation_forest,
)
from creditcore.schema import FEATURES, SAMPLE_REQUEST, TARGET
from creditcore.train import fit_detectors

N_SRC = N_CAT + N_NUM


def _contrib(packed, codes, nums):
    return cpu_ref.forest_contrib_cpu(packed, codes, cpu_ref.impute_nums(packed, nums))


@pytest.fixture(scope="module")
def rf_contrib(packed, score_batch):
    """The session RF model's attributions on score_batch, computed once."""
    codes, nums = encode_batch(score_batch, packed.vocabs)
    out = _contrib(packed, codes, nums)
    out.setflags(write=False)
    return codes, nums, out


def _max_depth(nodes: np.ndarray, offsets: np.ndarray) -> int:
    """Deepest leaf (in edges) over all trees of a packed forest."""
    deepest = 0
    for t in range(len(offsets) - 1):
        tn = nodes[offsets[t] : offsets[t + 1]]
        depth = np.zeros(len(tn), dtype=np.int64)
        for k in range(len(tn)):  # BFS order: parents come first
            if tn[k, 0] >= 0:
                depth[tn[k, 2]] = depth[tn[k, 3]] = depth[k] + 1
        deepest = max(deepest, int(depth.max()))
    return deepest


# ------------------------------------------------------------------ pack


def test_pack_node_values_layout(packed):
    v = packed.cls_node_value
    assert v is not None and v.dtype == np.float32
    assert v.shape == (len(packed.cls_nodes),)
    leaf = packed.cls_nodes[:, 0] < 0
    # leaves: bit-identical to the payload the scorer sums
    np.testing.assert_array_equal(
        v[leaf].view(np.int32), packed.cls_nodes[leaf, 1]
    )
    roots = v[packed.cls_tree_offsets[:-1]].astype(np.float64)
    assert packed.cls_base_value == pytest.approx(roots.mean(), abs=1e-15)
    assert 0.0 < packed.cls_base_value < 1.0


# ----------------------------------------------------------- additivity


def test_additivity_rf(packed, rf_contrib):
    codes, nums, contrib = rf_contrib
    assert contrib.shape == (len(codes), N_SRC) and contrib.dtype == np.float64
    ref = cpu_ref.score_forest_cpu(packed, codes, cpu_ref.impute_nums(packed, nums))
    err = np.abs(packed.cls_base_value + contrib.sum(1) - ref).max()
    print(f"RF additivity max |err| = {err:.3e}")
    np.testing.assert_allclose(
        packed.cls_base_value + contrib.sum(1), ref, rtol=0, atol=1e-12
    )


def test_independent_oracle_rf(packed, loaded_pyfunc, score_batch, rf_contrib):
    """Contributions recomputed straight from the sklearn objects (never
    through pack): preprocessor transform, each estimator's decision_path,
    node values = tree_.value class-1 fractions, transformed columns mapped
    back to source columns through the OHE categories.

    Tolerance is derived: every stored node value is an f32 rounding of a
    number in [0, 1] (off by at most 2^-25), each path step uses two of them,
    so |delta| <= 2 * d_max * 2^-25 with d_max the deepest tree."""
    _, _, contrib = rf_contrib
    pipe = loaded_pyfunc.python_model.classifier
    pre = pipe.named_steps["preprocessor"]
    clf = pipe.named_steps["classifier"]
    x = pre.transform(score_batch[FEATURES])
    x = np.asarray(x.todense()) if hasattr(x, "todense") else np.asarray(x)

    ohe = pre.named_transformers_["categorical"].named_steps["ohe"]
    src = []
    for col, cats in enumerate(ohe.categories_):
        src += [col] * len(cats)
    src += [N_CAT + j for j in range(N_NUM)]
    src = np.asarray(src)
    assert len(src) == x.shape[1]

    oracle = np.zeros((len(x), N_SRC), dtype=np.float64)
    for est in clf.estimators_:
        t = est.tree_
        val = np.asarray(t.value, dtype=np.float64)[:, 0, :]
        p1 = val[:, 1] / val.sum(axis=1)
        path = est.decision_path(x).tocsr()
        for r in range(len(x)):
            # node ids along a root-to-leaf path are increasing (preorder)
            ids = path.indices[path.indptr[r] : path.indptr[r + 1]]
            for n, child in zip(ids[:-1], ids[1:]):
                oracle[r, src[t.feature[n]]] += p1[child] - p1[n]
    oracle /= len(clf.estimators_)

    d_max = _max_depth(packed.cls_nodes, packed.cls_tree_offsets)
    tol = 2.0 * d_max * 2.0**-25
    err = np.abs(contrib - oracle).max()
    print(f"oracle: d_max={d_max} tol={tol:.3e} max |delta|={err:.3e}")
    np.testing.assert_allclose(contrib, oracle, rtol=0, atol=tol)


def _fit_family(train_df, params, algorithm):
    pipe = make_classifier_pipeline(params, algorithm=algorithm)
    pipe.fit(train_df[FEATURES], train_df[TARGET].values.ravel())
    drift, outlier = fit_detectors(train_df)
    c = pack_classifier_pipeline(pipe)
    o = pack_isolation_forest(outlier)
    d = pack_drift(drift, c["vocabs"])
    return PackedModel(**c, **o, **d), pipe


@pytest.fixture(scope="module")
def gbt_packed(train_df):
    return _fit_family(
        train_df, {"n_estimators": 60, "max_depth": 3, "random_state": 0}, "gbt"
    )


@pytest.fixture(scope="module")
def et_packed(train_df):
    return _fit_family(
        train_df, {"n_estimators": 80, "max_depth": 8, "random_state": 0}, "et"
    )


def test_gbt_log_odds_vs_sklearn(gbt_packed, score_batch):
    packed, pipe = gbt_packed
    assert packed.cls_kind == 1
    codes, nums = encode_batch(score_batch, packed.vocabs)
    out = ScoringEngine(packed, device="cpu").explain_arrays(codes, nums)
    assert out["output_space"] == "log_odds"
    raw = packed.cls_base_value + out["contributions"].sum(1)
    sk = pipe.predict_proba(score_batch[FEATURES])[:, 1]
    np.testing.assert_allclose(1.0 / (1.0 + np.exp(-raw)), sk, rtol=0, atol=1e-7)
    np.testing.assert_allclose(out["predictions"], sk, rtol=0, atol=1e-7)


def test_extratrees_additivity(et_packed, score_batch):
    packed, _ = et_packed
    assert packed.cls_kind == 0
    codes, nums = encode_batch(score_batch, packed.vocabs)
    contrib = _contrib(packed, codes, nums)
    ref = cpu_ref.score_forest_cpu(packed, codes, cpu_ref.impute_nums(packed, nums))
    np.testing.assert_allclose(
        packed.cls_base_value + contrib.sum(1), ref, rtol=0, atol=1e-12
    )


# ------------------------------------------------------------- structure


def _tiny_packed() -> PackedModel:
    """Hand-made 3-tree averaging forest over 9 two-category columns and the
    14 numerics. Virtual features: 0..17 one-hot (col = f // 2, code = f % 2),
    18..31 numeric.
      tree 0: root splits numeric col 2 (<= 0.5)         -> leaves 0.2 / 0.8
      tree 1: root splits one-hot (col 1 == code 0) <= 0.5
                left (not that category): leaf 0.1
                right: splits numeric col 5 (<= 10)      -> leaves 0.3 / 0.9
      tree 2: a lone leaf 0.6
    """

    def f32bits(x):
        return int(np.float32(x).view(np.int32))

    t0 = np.array(
        [[18 + 2, f32bits(0.5), 1, 2], [-1, f32bits(0.2), 0, 0], [-1, f32bits(0.8), 0, 0]],
        dtype=np.int32,
    )
    t1 = np.array(
        [
            [2, f32bits(0.5), 1, 2],
            [-1, f32bits(0.1), 0, 0],
            [18 + 5, f32bits(10.0), 3, 4],
            [-1, f32bits(0.3), 0, 0],
            [-1, f32bits(0.9), 0, 0],
        ],
        dtype=np.int32,
    )
    t2 = np.array([[-1, f32bits(0.6), 0, 0]], dtype=np.int32)
    weights = [
        np.array([10.0, 6.0, 4.0]),
        np.array([10.0, 5.0, 5.0, 1.0, 4.0]),
        np.array([10.0]),
    ]
    trees = [t0, t1, t2]
    values = [_node_values(t, w) for t, w in zip(trees, weights)]
    offsets = np.array([0, 3, 8, 9], dtype=np.int32)
    feat_col = np.array([f // 2 for f in range(18)] + list(range(N_NUM)), dtype=np.int32)
    feat_code = np.array([f % 2 for f in range(18)] + [-1] * N_NUM, dtype=np.int32)
    roots = np.array([float(v[0]) for v in values], dtype=np.float64)
    return PackedModel(
        vocabs=[["a", "b"] for _ in range(N_CAT)],
        medians=np.zeros(N_NUM, dtype=np.float32),
        feat_col=feat_col,
        feat_code=feat_code,
        n_onehot=18,
        cls_nodes=np.concatenate(trees),
        cls_tree_offsets=offsets,
        if_nodes=t2.copy(),
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
        cls_node_value=np.concatenate(values),
        cls_base_value=float(roots.mean()),
    )


def test_tiny_forest_by_hand():
    p = _tiny_packed()
    # internal values: cover-weighted means of the f32 children
    f = lambda x: np.float64(np.float32(x))  # noqa: E731
    v_t0 = (6 * f(0.2) + 4 * f(0.8)) / 10
    v_t1_r = np.float64(np.float32((1 * f(0.3) + 4 * f(0.9)) / 5))
    v_t1 = (5 * f(0.1) + 5 * v_t1_r) / 10
    assert p.cls_node_value[0] == np.float32(v_t0)
    assert p.cls_node_value[5] == np.float32(v_t1_r)
    assert p.cls_node_value[3] == np.float32(v_t1)
    # a root-only tree puts its leaf into the base and nothing anywhere else
    assert p.cls_node_value[8] == np.float32(0.6)
    assert p.cls_base_value == pytest.approx(
        (f(np.float32(v_t0)) + f(np.float32(v_t1)) + f(0.6)) / 3, abs=1e-15
    )

    codes = np.full((3, N_CAT), -1, dtype=np.int16)
    nums = np.zeros((3, N_NUM), dtype=np.float32)
    codes[0, 1] = 0  # row 0: category hit -> right subtree; num5=0 -> 0.3
    nums[1, 2] = 1.0  # row 1: tree 0 goes right (0.8); tree 1 left leaf 0.1
    nums[2, 5] = np.nan  # row 2: NaN imputes to median 0 -> same as 0.0
    codes[2, 1] = 0
    contrib = _contrib(p, codes, nums)

    # only categorical col 1 and numeric cols 2 and 5 are ever split on
    used = {1, N_CAT + 2, N_CAT + 5}
    for c in range(N_SRC):
        if c not in used:
            assert (contrib[:, c] == 0.0).all(), c
    v = p.cls_node_value.astype(np.float64)
    np.testing.assert_allclose(
        contrib[0, 1], (v[5] - v[3]) / 3, rtol=0, atol=1e-15
    )
    np.testing.assert_allclose(
        contrib[0, N_CAT + 5], (v[6] - v[5]) / 3, rtol=0, atol=1e-15
    )
    np.testing.assert_allclose(
        contrib[0, N_CAT + 2], (v[1] - v[0]) / 3, rtol=0, atol=1e-15
    )
    np.testing.assert_allclose(
        contrib[1, N_CAT + 2], (v[2] - v[0]) / 3, rtol=0, atol=1e-15
    )
    assert contrib[1, N_CAT + 5] == 0.0  # never reached that split
    np.testing.assert_array_equal(contrib[2], contrib[0])  # NaN == median
    ref = cpu_ref.score_forest_cpu(p, codes, cpu_ref.impute_nums(p, nums))
    np.testing.assert_allclose(
        p.cls_base_value + contrib.sum(1), ref, rtol=0, atol=1e-12
    )


def test_root_leaf_forest_contributes_nothing():
    p = _tiny_packed()
    p.cls_nodes = p.cls_nodes[8:9].copy()
    p.cls_node_value = p.cls_node_value[8:9].copy()
    p.cls_tree_offsets = np.array([0, 1], dtype=np.int32)
    p.cls_base_value = float(p.cls_node_value[0])
    codes = np.zeros((4, N_CAT), dtype=np.int16)
    nums = np.ones((4, N_NUM), dtype=np.float32)
    out = ScoringEngine(p, device="cpu").explain_arrays(codes, nums)
    assert (out["contributions"] == 0.0).all()
    np.testing.assert_array_equal(out["predictions"], np.float64(np.float32(0.6)))


def test_unsplit_column_does_not_matter():
    p = _tiny_packed()
    codes = np.zeros((2, N_CAT), dtype=np.int16)
    nums = np.full((2, N_NUM), 3.0, dtype=np.float32)
    nums[1, 7] = -1e6  # numeric col 7: no tree splits on it
    codes[1, 4] = 1  # categorical col 4: likewise
    contrib = _contrib(p, codes, nums)
    np.testing.assert_array_equal(contrib[0], contrib[1])


# ------------------------------------------------- persistence / errors


def test_save_load_roundtrip(packed, tmp_path, rf_contrib):
    path = str(tmp_path / "m.npz")
    packed.save(path)
    re = PackedModel.load(path)
    np.testing.assert_array_equal(
        re.cls_node_value.view(np.int32), packed.cls_node_value.view(np.int32)
    )
    assert re.cls_node_value.dtype == np.float32
    assert re.cls_base_value == packed.cls_base_value
    codes, nums, contrib = rf_contrib
    np.testing.assert_array_equal(_contrib(re, codes[:32], nums[:32]), contrib[:32])


def test_old_npz_loads_without_values(packed, tmp_path):
    path = str(tmp_path / "m.npz")
    packed.save(path)
    z = np.load(path, allow_pickle=True)
    old = {k: z[k] for k in z.files if k not in ("cls_node_value", "cls_base_value")}
    assert len(old) == len(z.files) - 2
    old_path = str(tmp_path / "old.npz")
    np.savez_compressed(old_path, **old)

    re = PackedModel.load(old_path)
    assert re.cls_node_value is None and re.cls_base_value == 0.0
    eng = ScoringEngine(re, device="cpu")
    codes, nums = encode_batch(SAMPLE_REQUEST, re.vocabs)
    # scoring is untouched; only explain refuses
    assert 0.0 <= eng.score_arrays(codes, nums, with_drift=False)["predictions"][0] <= 1.0
    with pytest.raises(ExplainUnavailable):
        eng.explain_arrays(codes, nums)
    with pytest.raises(ValueError, match="cls_node_value"):
        _contrib(re, codes, nums)
    # and saving a model without values writes no such keys
    re.save(str(tmp_path / "again.npz"))
    assert "cls_node_value" not in np.load(str(tmp_path / "again.npz"), allow_pickle=True)


def test_engine_explain_records_and_cap(packed):
    eng = ScoringEngine(packed, device="cpu")
    out = eng.explain_records(SAMPLE_REQUEST * 3)
    assert out["output_space"] == "probability"
    assert out["contributions"].shape == (3, N_SRC)
    assert out["base_value"] == packed.cls_base_value
    score = eng.score_records(SAMPLE_REQUEST * 3)["response"]["predictions"]
    np.testing.assert_allclose(out["predictions"], score, rtol=0, atol=1e-12)
    n = ScoringEngine.EXPLAIN_MAX_ROWS + 1
    assert ScoringEngine.EXPLAIN_MAX_ROWS == 16384
    with pytest.raises(ExplainTooLarge):
        eng.explain_arrays(
            np.zeros((n, N_CAT), dtype=np.int16), np.zeros((n, N_NUM), dtype=np.float32)
        )


# ----------------------------------------------------------------- HTTP


@pytest.fixture(scope="module")
def client(model_dir):
    from fastapi.testclient import TestClient

    from creditcore.config import ServeConfig
    from creditcore.serve import create_app

    cfg = ServeConfig()
    cfg.model_directory = model_dir
    cfg.device = "cpu"
    with TestClient(create_app(cfg)) as c:
        yield c


def test_explain_sample_request(client):
    r = client.post("/explain", json=SAMPLE_REQUEST)
    assert r.status_code == 200
    body = r.json()
    assert set(body) == {
        "output_space", "base_value", "features", "predictions",
        "contributions", "top_reasons",
    }
    assert body["features"] == list(FEATURES) and len(body["features"]) == 23
    assert body["output_space"] == "probability"
    assert len(body["contributions"]) == 1 and len(body["contributions"][0]) == 23
    assert len(body["top_reasons"]) == 1 and len(body["top_reasons"][0]) <= 3
    total = body["base_value"] + sum(body["contributions"][0])
    assert total == pytest.approx(body["predictions"][0], abs=1e-12)
    # /predict on the same app still answers, and agrees
    p = client.post("/predict", json=SAMPLE_REQUEST)
    assert p.status_code == 200
    assert set(p.json()) == {"predictions", "outliers", "feature_drift_batch"}
    assert p.json()["predictions"][0] == pytest.approx(total, abs=1e-12)


def test_explain_top_reasons(client):
    from creditcore.data import make_request_batch

    batch = make_request_batch(48, seed=5)
    r = client.post("/explain?top_k=5", json=batch)
    assert r.status_code == 200
    body = r.json()
    assert len(body["top_reasons"]) == 48
    saw_reason = False
    for row, reasons in zip(body["contributions"], body["top_reasons"]):
        assert len(reasons) <= 5
        vals = [x["contribution"] for x in reasons]
        assert all(v > 0.0 for v in vals)
        assert vals == sorted(vals, reverse=True)
        # exactly the largest positive entries, ties by feature index
        want = sorted(
            (j for j in range(23) if row[j] > 0.0), key=lambda j: (-row[j], j)
        )[:5]
        assert [x["feature"] for x in reasons] == [FEATURES[j] for j in want]
        assert vals == [row[j] for j in want]
        saw_reason = saw_reason or bool(reasons)
    assert saw_reason
    all_k = client.post("/explain?top_k=23", json=batch[:4]).json()
    for row, reasons in zip(all_k["contributions"], all_k["top_reasons"]):
        assert len(reasons) == sum(1 for v in row if v > 0.0)


def test_explain_top_k_bounds(client):
    r = client.post("/explain?top_k=0", json=SAMPLE_REQUEST * 2)
    assert r.status_code == 200
    assert r.json()["top_reasons"] == [[], []]
    assert client.post("/explain?top_k=24", json=SAMPLE_REQUEST).status_code == 422
    assert client.post("/explain?top_k=-1", json=SAMPLE_REQUEST).status_code == 422


def test_explain_bad_bodies(client):
    assert client.post("/explain", json=[]).status_code == 400
    r = client.post("/explain", json=[{"credit_limit": "not-a-number"}])
    assert r.status_code == 422


def test_explain_counted_in_metrics(client):
    before = client.get("/metrics").json()
    assert client.post("/explain", json=SAMPLE_REQUEST * 4).status_code == 200
    after = client.get("/metrics").json()
    assert after["requests_total"] == before["requests_total"] + 1
    assert after["rows_total"] == before["rows_total"] + 4


def test_explain_in_openapi(client):
    spec = client.get("/openapi.json").json()
    post = spec["paths"]["/explain"]["post"]
    assert "requestBody" in post
    ok = post["responses"]["200"]["content"]["application/json"]["schema"]
    assert ok["$ref"].endswith("/ExplainOutput")
    assert "ExplainOutput" in spec["components"]["schemas"]


def test_explain_http_errors(model_dir, packed, tmp_path, monkeypatch):
    """501 for a model packed without node values, 413 above the row cap,
    503 with no live replica."""
    from fastapi.testclient import TestClient

    from creditcore import serve
    from creditcore.config import ServeConfig

    old = PackedModel.load(_save_without_values(packed, tmp_path))
    cfg = ServeConfig()
    cfg.model_directory = model_dir
    cfg.device = "cpu"
    with TestClient(serve.create_app(cfg)) as c:
        engines = serve.state["engines"]
        monkeypatch.setattr(ScoringEngine, "EXPLAIN_MAX_ROWS", 2)
        assert c.post("/explain", json=SAMPLE_REQUEST * 3).status_code == 413
        assert c.post("/explain", json=SAMPLE_REQUEST * 2).status_code == 200
        monkeypatch.undo()

        serve.state["pool"].alive = [False] * len(engines)
        assert c.post("/explain", json=SAMPLE_REQUEST).status_code == 503
        serve.state["pool"].alive = [True] * len(engines)

        serve.state["engines"] = [ScoringEngine(old, device="cpu")]
        r = c.post("/explain", json=SAMPLE_REQUEST)
        assert r.status_code == 501 and "node" in r.json()["detail"]
        serve.state["engines"] = engines


def _save_without_values(packed, tmp_path) -> str:
    import dataclasses

    path = str(tmp_path / "novalues.npz")
    dataclasses.replace(packed, cls_node_value=None, cls_base_value=0.0).save(path)
    return path

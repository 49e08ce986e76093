"""Partial dependence and ICE curves on the CPU: the engine against
scikit-learn's brute-force ``partial_dependence`` on the project's own
pipelines, the grid rule, identities of the what-if reference, the monotone
guarantee of hgbt made visible, the HTTP and CLI surface, caps and slicing.

The 1e-7 bound of the oracle test is the one test_pack_parity.py holds the
packed scorer to against ``predict_proba``: the what-if reference runs that
scorer's traversal on a copy of the sample with one or two columns replaced,
which is exactly what the brute method does with the pipeline."""

from __future__ import annotations

import dataclasses
import json
import subprocess
import sys

import numpy as np
import pytest

from _pdp_cases import (
    CATEGORICAL,
    ENTRIES,
    FAMILY_PARAMS,
    NUMERIC,
    fit_pipe,
    num_job,
    pack_pipe,
    sample_frame,
)
from _shap_models import N_ONEHOT, f32bits, hand_model
from creditcore import pdp
from creditcore.engine import ExplainTooLarge, ExplainUnavailable, ScoringEngine
from creditcore.ops import cpu_ref
from creditcore.pack import N_CAT, N_NUM, encode_batch
from creditcore.schema import CATEGORICAL_FEATURES, FEATURES

ORACLE_ATOL = 1e-7


@pytest.fixture(scope="module")
def detectors(train_df):
    from creditcore.train import fit_detectors

    return fit_detectors(train_df)


@pytest.fixture(scope="module")
def sample_df(train_df):
    return sample_frame(train_df)


# ------------------------------------------------------------ 1. sklearn oracle


def _sklearn_pd(pipe, x_df, names, grids, response_method):
    from sklearn.inspection import partial_dependence

    return partial_dependence(
        pipe,
        x_df,
        features=list(names),
        custom_values={n: np.asarray(g, dtype=object if isinstance(g[0], str) else None)
                       for n, g in zip(names, grids)},
        categorical_features=CATEGORICAL_FEATURES,
        method="brute",
        kind="both",
        response_method=response_method,
    )


@pytest.mark.parametrize("family", ["rf", "et", "gbt", "hgbt"])
def test_sklearn_oracle(train_df, detectors, sample_df, family):
    pipe = fit_pipe(train_df, family)
    p = pack_pipe(pipe, detectors)
    assert p.cls_n_trees <= 20
    eng = ScoringEngine(p, device="cpu")
    sample = encode_batch(sample_df, p.vocabs)
    assert np.isnan(sample[1]).sum() == 2 and (sample[0] == -1).sum() >= 1
    responses = [("probability", "predict_proba")]
    if family == "hgbt":
        responses.append(("raw", "decision_function"))
    for response, method in responses:
        out = eng.partial_dependence(ENTRIES, sample=sample, kind="both", response=response)
        assert out["sample_rows"] == 64
        assert out["output_space"] == ("log_odds" if response == "raw" else "probability")
        for entry, res in zip(ENTRIES, out["results"]):
            names = (entry,) if isinstance(entry, str) else entry
            assert res["features"] == list(names)
            ref = _sklearn_pd(pipe, sample_df, names, res["grid_values"], method)
            shape = tuple(len(g) for g in res["grid_values"])
            assert res["average"].shape == shape and res["individual"].shape == (64, *shape)
            err_a = np.abs(res["average"] - ref["average"][0]).max()
            err_i = np.abs(res["individual"] - ref["individual"][0]).max()
            print(f"{family} {response} {names}: average {err_a:.3e} individual {err_i:.3e}")
            assert np.ptp(ref["individual"][0]) > 1e-3  # the curves are not flat
            np.testing.assert_allclose(res["average"], ref["average"][0], rtol=0, atol=ORACLE_ATOL)
            np.testing.assert_allclose(
                res["individual"], ref["individual"][0], rtol=0, atol=ORACLE_ATOL
            )
    if family in ("rf", "et"):  # the averaging forests have no log-odds
        with pytest.raises(ValueError, match="raw"):
            eng.partial_dependence([NUMERIC], sample=sample, response="raw")


# ---------------------------------------------------------------- 2. grid rule


@pytest.fixture(scope="module")
def grid_engine():
    """A stump on numeric column 0; the model is beside the point here."""
    tree = np.array(
        [[N_ONEHOT, f32bits(0.0), 1, 2], [-1, f32bits(0.25), 0, 0], [-1, f32bits(0.75), 0, 0]],
        dtype=np.int32,
    )
    return ScoringEngine(hand_model([tree], [np.ones(3)]), device="cpu")


def _grid_sample(n=200):
    rng = np.random.default_rng(0)
    codes = rng.integers(-1, 2, size=(n, N_CAT)).astype(np.int16)
    nums = rng.normal(0.0, 1.0, size=(n, N_NUM)).astype(np.float32)
    nums[:, 1] = rng.integers(0, 7, size=n)  # 7 distinct values
    nums[:, 2] = 4.5  # constant
    nums[:, 3] = np.arange(n) % 20  # exactly grid_resolution distinct values
    nums[:5, 4] = np.nan  # imputed to the median before the grid is built
    return codes, nums


def test_grid_rule(grid_engine):
    from scipy.stats.mstats import mquantiles

    eng, p = grid_engine, grid_engine.packed
    codes, nums = _grid_sample()
    names = ["credit_limit", "age", "bill_amount_1", "bill_amount_2", "bill_amount_3", "sex"]
    out = eng.partial_dependence(names, sample=(codes, nums))
    g = {r["features"][0]: r["grid_values"][0] for r in out["results"]}
    # wide column: the f32 linspace between the empirical percentiles
    lo, hi = mquantiles(nums[:, 0].astype(np.float64), prob=[0.05, 0.95])
    want = np.linspace(lo, hi, 20).astype(np.float32)
    assert g["credit_limit"] == [float(v) for v in want] and len(want) == 20
    assert all(np.float32(v) == v for v in g["credit_limit"])
    assert g["age"] == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0]  # few values: themselves
    assert g["bill_amount_1"] == [4.5]  # constant: one point
    assert g["bill_amount_2"] == [float(v) for v in range(20)]  # exactly grid_resolution
    imp = cpu_ref.impute_nums(p, nums)[:, 4].astype(np.float64)
    lo, hi = mquantiles(imp, prob=[0.05, 0.95])
    assert g["bill_amount_3"] == [float(v) for v in np.linspace(lo, hi, 20).astype(np.float32)]
    assert g["sex"] == list(p.vocabs[0]) == ["a", "b"]  # the vocabulary, in order
    assert out["results"][0]["average"].shape == (20,) and "individual" not in out["results"][0]
    # other percentiles and resolution
    out = eng.partial_dependence(
        ["credit_limit"], sample=(codes, nums), grid_resolution=5, percentiles=(0.1, 0.5)
    )
    lo, hi = mquantiles(nums[:, 0].astype(np.float64), prob=[0.1, 0.5])
    want = [float(v) for v in np.linspace(lo, hi, 5).astype(np.float32)]
    assert out["results"][0]["grid_values"][0] == want
    # a wide column whose two percentiles coincide: one point
    codes, spike = _grid_sample(600)
    spike[:, 0] = 2.0
    spike[:12, 0] = np.arange(12) - 20.0  # 25 distinct values, but fewer than
    spike[12:24, 0] = np.arange(12) + 20.0  # 5 % of the rows on either side of 2.0
    assert len(np.unique(spike[:, 0])) == 25
    out = eng.partial_dependence(["credit_limit"], sample=(codes, spike))
    assert out["results"][0]["grid_values"][0] == [2.0]
    assert pdp.numeric_grid(spike[:, 0], 20, (0.05, 0.95)).tolist() == [2.0]


def test_grid_override_and_junk(grid_engine):
    eng = grid_engine
    sample = _grid_sample()
    out = eng.partial_dependence(
        ["credit_limit", ("sex", "age")],
        sample=sample,
        grid={"credit_limit": [-1.0, 0.0, 0.1, 1], "sex": ["b"]},
        kind="both",
    )
    one, two = out["results"]
    assert one["grid_values"] == [[-1.0, 0.0, float(np.float32(0.1)), 1.0]]
    # the stump: x <= 0 -> 0.25, else 0.75, for every row
    np.testing.assert_array_equal(one["average"], [0.25, 0.25, 0.75, 0.75])
    np.testing.assert_array_equal(one["individual"], np.tile(one["average"], (200, 1)))
    assert two["grid_values"][0] == ["b"] and len(two["grid_values"][1]) == 7
    assert two["average"].shape == (1, 7) and two["individual"].shape == (200, 1, 7)
    for junk in (
        {"credit_limit": [0.0, float("nan")]},
        {"credit_limit": [0.0, float("inf")]},
        {"credit_limit": [1e39]},  # not a finite float32
        {"credit_limit": ["high"]},
        {"credit_limit": []},
        {"credit_limit": 3.0},
        {"credit_limit": [[0.0, 1.0]]},
        {"credit_limit": [True]},
        {"sex": ["c"]},
        {"sex": [0]},
        {"shoe_size": [1.0]},
        [1.0, 2.0],
    ):
        with pytest.raises(ValueError):
            eng.partial_dependence(["credit_limit", "sex"], sample=sample, grid=junk)
    for bad in (["shoe_size"], [("sex", "sex")], [("sex", "age", "education")], [], "sex", [3]):
        with pytest.raises(ValueError):
            eng.partial_dependence(bad, sample=sample)
    for kw in ({"kind": "individual"}, {"response": "logit"}, {"response": "raw"},
               {"grid_resolution": 1}, {"percentiles": (0.9, 0.1)}, {"percentiles": (0.1,)},
               {"percentiles": (-0.1, 0.5)}):
        with pytest.raises(ValueError):
            eng.partial_dependence(["sex"], sample=sample, **kw)
    with pytest.raises(ExplainUnavailable, match="background sample"):
        eng.partial_dependence(["sex"])  # a hand-built model carries no sample


# ---------------------------------------------------------------- 3. identities


def test_reference_identities(train_df, detectors, sample_df, grid_engine):
    p = pack_pipe(fit_pipe(train_df, "hgbt"), detectors)
    codes, nums = encode_batch(sample_df, p.vocabs)
    imp = cpu_ref.impute_nums(p, nums)
    score = cpu_ref.score_forest_cpu(p, codes, imp)
    raw = cpu_ref.forest_raw_cpu(p, codes, imp, tree_order=True)
    # a feature that no tree splits on: the unmodified sum for every row
    stump = grid_engine.packed  # splits on numeric column 0 alone
    sc, sx = _grid_sample(70)
    sx = cpu_ref.impute_nums(stump, sx)
    jobs = [num_job(5, v) for v in (-1e9, 0.0, 1e9)] + [[2, 0, -1, 0], [2, -1, N_CAT + 7, 0]]
    got = cpu_ref.forest_whatif_cpu(stump, sc, sx, np.asarray(jobs, dtype=np.int32))
    assert got.shape == (5, 70) and len(np.unique(got)) == 2
    np.testing.assert_array_equal(
        got, np.tile(cpu_ref.forest_raw_cpu(stump, sc, sx, tree_order=True), (5, 1))
    )
    # a row's own (imputed) value: the row's score. Job r carries row r's value.
    for player in (FEATURES.index(NUMERIC), FEATURES.index("bill_amount_3"),
                   FEATURES.index(CATEGORICAL), FEATURES.index("education")):
        if player < N_CAT:
            bits = codes[:, player].astype(np.int32)
        else:
            bits = imp[:, player - N_CAT].view(np.int32)
        jobs = np.stack([np.full(64, player), bits, np.full(64, -1), np.zeros(64, int)], axis=1)
        own = np.diagonal(cpu_ref.forest_whatif_cpu(p, codes, imp, jobs.astype(np.int32)))
        np.testing.assert_array_equal(own, raw)
        # tree order against the scorer's own order of the same <= 20 addends,
        # each below 8 in magnitude: 2 n eps sum|v| < 1e-12
        fin = pdp.finalize(own, p.cls_kind, p.cls_bias, p.cls_n_trees, "probability")
        np.testing.assert_allclose(fin, score, rtol=0, atol=1e-12)
    # a two-way job equals the two one-way overrides written one after the other
    a, b = FEATURES.index("age"), FEATURES.index("sex")
    two = cpu_ref.forest_whatif_cpu(
        p, codes, imp, np.asarray([[a, f32bits(40.0), b, 1]], dtype=np.int32)
    )
    c2, x2 = codes.copy(), imp.copy()
    c2[:, b] = 1
    x2[:, a - N_CAT] = 40.0
    np.testing.assert_array_equal(two[0], cpu_ref.forest_raw_cpu(p, c2, x2, tree_order=True))
    # the same job with its slots swapped
    swapped = cpu_ref.forest_whatif_cpu(
        p, codes, imp, np.asarray([[b, 1, a, f32bits(40.0)]], dtype=np.int32)
    )
    np.testing.assert_array_equal(swapped, two)
    for bad in ([[23, 0, -1, 0]], [[-1, 0, -1, 0]], [[3, 0, 3, 1]], [[3, 0, -2, 0]]):
        with pytest.raises(ValueError):
            cpu_ref.forest_whatif_cpu(p, codes, imp, np.asarray(bad, dtype=np.int32))
    with pytest.raises(ValueError):
        cpu_ref.forest_whatif_cpu(p, codes, imp, np.zeros((0, 4), dtype=np.int32))


# ------------------------------------------------------------------ 4. monotone


def test_monotone_ice_curves(train_df, detectors, sample_df):
    """Every ICE curve of a feature constrained to -1 is non-increasing,
    exactly: each tree is monotone in the feature (models/hgbt.py) and the
    what-if sums a row's leaves in one fixed order, tree by tree, so the f64
    sum is monotone too (fl(a + b) is monotone in a and in b), and so are
    bias + sum and the sigmoid of it."""
    params = {k: v for k, v in FAMILY_PARAMS["hgbt"].items()}
    mono = pack_pipe(
        fit_pipe(train_df, "hgbt", {**params, "monotone": {"credit_limit": -1}}), detectors
    )
    free = pack_pipe(fit_pipe(train_df, "hgbt", params), detectors)
    col = mono.feat_col[mono.cls_nodes[mono.cls_nodes[:, 0] >= 0, 0]]
    code = mono.feat_code[mono.cls_nodes[mono.cls_nodes[:, 0] >= 0, 0]]
    assert ((col == 0) & (code < 0)).any()  # credit_limit is split on
    sample = encode_batch(sample_df, mono.vocabs)
    for response in ("raw", "probability"):
        res = ScoringEngine(mono, device="cpu").partial_dependence(
            ["credit_limit"], sample=sample, kind="both", response=response, grid_resolution=50
        )["results"][0]
        ice = res["individual"]
        assert ice.shape == (64, 50)
        assert (np.diff(ice, axis=1) <= 0).all()
        assert (np.diff(res["average"]) <= 0).all()
        assert np.ptp(ice, axis=1).max() > 0  # and they do move
    out = ScoringEngine(free, device="cpu").partial_dependence(
        ["credit_limit"], sample=sample, kind="both"
    )["results"][0]
    assert out["individual"].shape == (64, 20) and np.isfinite(out["individual"]).all()


def test_train_and_register_stores_the_constrained_curves(train_df, tmp_path, monkeypatch):
    from creditcore import train as T
    from creditcore.models import tpe
    from creditcore.pack import pack_pyfunc_dir

    monkeypatch.setattr(
        tpe,
        "reference_space",
        lambda: {
            "n_estimators": tpe.IntDim(8, 12),
            "max_depth": tpe.IntDim(3, 5),
            "criterion": tpe.CatDim(("gini", "entropy")),
        },
    )
    d = str(tmp_path / "m")
    T.train_and_register(
        model_dir=d, max_evals=1, df=train_df, register=False, algorithm="hgbt",
        train_device="cpu", monotone={"credit_limit": -1},
    )
    import yaml

    with open(f"{d}/MLmodel") as f:
        meta = yaml.safe_load(f)["metadata"]
    assert meta["monotone"] == {"credit_limit": -1}
    curve = meta["monotone_pdp"]["credit_limit"]
    assert (np.diff(curve["average"]) <= 0).all() and len(curve["average"]) > 1
    want = ScoringEngine(pack_pyfunc_dir(d), device="cpu").partial_dependence(["credit_limit"])
    assert curve["grid_values"] == want["results"][0]["grid_values"][0]
    np.testing.assert_array_equal(curve["average"], want["results"][0]["average"])


# -------------------------------------------------------------- 5. HTTP and CLI

HTTP_BODY = {
    "features": ["credit_limit", ["sex", "age"]],
    "grid_resolution": 3,
    "kind": "both",
}


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


def test_http_pdp(client, packed):
    r = client.post("/explain/pdp", json=HTTP_BODY)
    assert r.status_code == 200, r.text
    body = r.json()
    assert set(body) == {"output_space", "sample_rows", "kind", "results"}
    assert body["output_space"] == "probability" and body["sample_rows"] == 256
    assert body["kind"] == "both" and len(body["results"]) == 2
    want = ScoringEngine(packed, device="cpu").partial_dependence(
        ["credit_limit", ("sex", "age")], grid_resolution=3, kind="both"
    )
    for got, ref in zip(body["results"], want["results"]):
        assert set(got) == {"features", "grid_values", "average", "individual"}
        assert got["features"] == ref["features"] and got["grid_values"] == ref["grid_values"]
        np.testing.assert_array_equal(np.asarray(got["average"]), ref["average"])
        np.testing.assert_array_equal(np.asarray(got["individual"]), ref["individual"])
    assert body["results"][1]["grid_values"][0] == list(packed.vocabs[0])
    # kind defaults to "average": no ICE curves in the answer
    r = client.post("/explain/pdp", json={"features": ["sex"], "grid": {"sex": ["male"]}})
    assert r.status_code == 200 and r.json()["kind"] == "average"
    assert set(r.json()["results"][0]) == {"features", "grid_values", "average"}
    assert r.json()["results"][0]["grid_values"] == [["male"]]
    # /explain keeps its answer
    assert "results" not in client.post("/explain", json=[{}]).json()


def test_http_pdp_in_openapi(client):
    spec = client.get("/openapi.json").json()
    post = spec["paths"]["/explain/pdp"]["post"]
    ok = post["responses"]["200"]["content"]["application/json"]["schema"]
    assert ok["$ref"].endswith("/PdpOutput")
    assert {"PdpOutput", "PdpCurve", "PdpRequest"} <= set(spec["components"]["schemas"])
    assert "/explain" in spec["paths"]


def test_http_pdp_errors(client, packed):
    from creditcore import serve

    for body in (
        {"features": ["shoe_size"]},
        {"features": ["sex"], "kind": "individual"},
        {"features": ["sex"], "response": "logit"},
        {"features": ["sex"], "response": "raw"},  # a random forest has no log-odds
        {"features": ["credit_limit"], "grid": {"credit_limit": ["high"]}},
        {"features": ["sex"], "grid": {"sex": ["martian"]}},
        {"features": [["sex", "sex"]]},
        {"features": ["sex"], "grid_resolution": 1},
        {"features": "sex"},
        {},
    ):
        r = client.post("/explain/pdp", json=body)
        assert r.status_code == 422, (body, r.status_code, r.text)
    for body in (
        {"features": ["credit_limit"], "grid_resolution": 101},
        {"features": [["credit_limit", "age"]], "grid_resolution": 33},
        {"features": [["sex", "age"]] * 9},
        {"features": ["sex"] * 24},
    ):
        r = client.post("/explain/pdp", json=body)
        assert r.status_code == 413, (body, r.status_code, r.text)
    engines = serve.state["engines"]
    serve.state["pool"].alive = [False] * len(engines)
    try:
        assert client.post("/explain/pdp", json={"features": ["sex"]}).status_code == 503
    finally:
        serve.state["pool"].alive = [True] * len(engines)
    bare = dataclasses.replace(packed, bg_codes=None, bg_nums=None)
    serve.state["engines"] = [ScoringEngine(bare, device="cpu")]
    try:
        r = client.post("/explain/pdp", json={"features": ["sex"]})
        assert r.status_code == 501 and "background sample" in r.json()["detail"]
    finally:
        serve.state["engines"] = engines
    assert client.post("/explain/pdp", json={"features": ["sex"]}).status_code == 200


def test_cli_pdp(model_dir, packed, train_df, tmp_path):
    out = str(tmp_path / "pdp.json")
    r = subprocess.run(
        [sys.executable, "-m", "creditcore", "pdp", "--model-directory", model_dir,
         "--features", "credit_limit,sex:age", "--grid-resolution", "3", "--kind", "both",
         "--device", "cpu", "--out", out],
        capture_output=True, text=True, timeout=240,
    )
    assert r.returncode == 0, r.stderr[-800:]
    with open(out) as f:
        doc = json.load(f)
    eng = ScoringEngine(packed, device="cpu")
    want = eng.partial_dependence(["credit_limit", ("sex", "age")], grid_resolution=3, kind="both")
    assert doc["sample_rows"] == 256 and doc["kind"] == "both"
    assert doc["output_space"] == "probability"
    for got, ref in zip(doc["results"], want["results"]):
        assert got["features"] == ref["features"] and got["grid_values"] == ref["grid_values"]
        np.testing.assert_array_equal(np.asarray(got["average"]), ref["average"])
        np.testing.assert_array_equal(np.asarray(got["individual"]), ref["individual"])
    # --data replaces the packed sample
    csv = str(tmp_path / "rows.csv")
    train_df.iloc[:40].to_csv(csv, index=False)
    r = subprocess.run(
        [sys.executable, "-m", "creditcore", "pdp", "--model-directory", model_dir,
         "--features", "sex", "--data", csv, "--device", "cpu", "--out", out],
        capture_output=True, text=True, timeout=240,
    )
    assert r.returncode == 0, r.stderr[-800:]
    with open(out) as f:
        doc = json.load(f)
    ref = eng.partial_dependence(["sex"], sample=encode_batch(train_df.iloc[:40], packed.vocabs))
    assert doc["sample_rows"] == 40 and "individual" not in doc["results"][0]
    np.testing.assert_array_equal(np.asarray(doc["results"][0]["average"]), ref["results"][0]["average"])


# ---------------------------------------------------------- 6. caps and slicing


def test_caps(grid_engine):
    eng = grid_engine
    codes, nums = _grid_sample(1025)
    with pytest.raises(ExplainTooLarge, match="1024"):
        eng.partial_dependence(["sex"], sample=(codes, nums))
    sample = (codes[:1024], nums[:1024])
    assert eng.partial_dependence(["sex"], sample=sample)["sample_rows"] == 1024
    sample = (codes[:50], nums[:50])
    with pytest.raises(ExplainTooLarge, match="100"):
        eng.partial_dependence(["credit_limit"], sample=sample, grid_resolution=101)
    out = eng.partial_dependence(["credit_limit"], sample=(codes[:300], nums[:300]),
                                 grid_resolution=100)
    assert out["results"][0]["average"].shape == (100,)
    with pytest.raises(ExplainTooLarge, match="100"):
        eng.partial_dependence(["credit_limit"], sample=sample,
                               grid={"credit_limit": list(range(101))})
    wide = (codes[:300], nums[:300])
    with pytest.raises(ExplainTooLarge, match="32"):
        eng.partial_dependence([("credit_limit", "sex")], sample=wide, grid_resolution=33)
    out = eng.partial_dependence([("credit_limit", "sex")], sample=wide, grid_resolution=32)
    assert out["results"][0]["average"].shape == (32, 2)
    # the one-way resolution of the same call is not held to the pair's cap
    assert eng.partial_dependence(["credit_limit"], sample=wide, grid_resolution=33)
    with pytest.raises(ExplainTooLarge, match="23"):
        eng.partial_dependence(["sex"] * 24, sample=sample)
    assert len(eng.partial_dependence(list(FEATURES), sample=sample)["results"]) == 23
    with pytest.raises(ExplainTooLarge, match="8"):
        eng.partial_dependence([("sex", "age")] * 9, sample=sample)
    assert len(eng.partial_dependence([("sex", "age")] * 8, sample=sample)["results"]) == 8
    assert issubclass(ExplainTooLarge, ValueError)


def test_launch_slicing(train_df, detectors, sample_df, monkeypatch):
    p = pack_pipe(fit_pipe(train_df, "rf"), detectors)
    eng = ScoringEngine(p, device="cpu")
    sample = encode_batch(sample_df, p.vocabs)
    whole = eng.partial_dependence(ENTRIES, sample=sample, kind="both")
    calls = []
    real = cpu_ref.forest_whatif_cpu

    def spy(packed, codes, nums_imp, jobs):
        calls.append(len(jobs))
        return real(packed, codes, nums_imp, jobs)

    monkeypatch.setattr(cpu_ref, "forest_whatif_cpu", spy)
    monkeypatch.setattr(ScoringEngine, "PDP_LAUNCH_PAIRS", 2 * 64 - 1)  # one job per launch
    sliced = eng.partial_dependence(ENTRIES, sample=sample, kind="both")
    n_jobs = sum(r["average"].size for r in whole["results"])
    assert calls == [1] * n_jobs and n_jobs > 30
    calls.clear()
    monkeypatch.setattr(ScoringEngine, "PDP_LAUNCH_PAIRS", 7 * 64 + 3)  # seven jobs
    sevens = eng.partial_dependence(ENTRIES, sample=sample, kind="both")
    assert calls == [7] * (n_jobs // 7) + ([n_jobs % 7] if n_jobs % 7 else [])
    for a, b, c in zip(whole["results"], sliced["results"], sevens["results"]):
        assert a["grid_values"] == b["grid_values"] == c["grid_values"]
        for key in ("average", "individual"):
            np.testing.assert_array_equal(a[key], b[key])
            np.testing.assert_array_equal(a[key], c[key])

"""Accumulated local effects on the CPU. The 1e-12 bounds: both sides finalise
bit-identical raw sums and differ only in the order of a few hundred f64
additions of values below 1 in magnitude (2 n eps sum|v| < 1e-13)."""

from __future__ import annotations

import dataclasses
import json
import subprocess
import sys

import numpy as np
import pytest

from _pdp_cases import FAMILY_PARAMS, fit_pipe, pack_pipe
from _shap_models import N_ONEHOT, f32bits, hand_model
from creditcore.engine import ExplainTooLarge, ExplainUnavailable, ScoringEngine
from creditcore.pack import N_CAT, N_NUM
from creditcore.schema import FEATURES

NAMES = ["bill_amount_3", "age", "credit_limit"]


@pytest.fixture(scope="module")
def detectors(train_df):
    from creditcore.train import fit_detectors

    return fit_detectors(train_df)


def _brute(eng, name, edges, response):
    """ALE from the definition: each row's two ICE columns on the edge grid."""
    ice = eng.partial_dependence([name], kind="both", grid={name: edges}, response=response)
    ice = ice["results"][0]["individual"]  # [R, Ke + 1]
    z = np.asarray(edges, dtype=np.float32)
    c = FEATURES.index(name) - N_CAT
    x = eng.packed.bg_nums[:, c]
    x = np.where(np.isnan(x), eng.packed.medians[c], x).astype(np.float32)
    k = np.clip(np.searchsorted(z, x, side="left"), 1, len(z) - 1)
    d = ice[np.arange(len(x)), k] - ice[np.arange(len(x)), k - 1]
    n = np.array([(k == j).sum() for j in range(1, len(z))])
    m = np.array([d[k == j].mean() if (k == j).any() else 0.0 for j in range(1, len(z))])
    acc = np.concatenate([[0.0], np.cumsum(m)])
    return acc - (n * (acc[:-1] + acc[1:]) / 2).sum() / n.sum(), n, k, d


@pytest.mark.parametrize(
    "family, response", [("rf", "probability"), ("hgbt", "probability"), ("hgbt", "raw")]
)
def test_engine_equals_the_definition(train_df, detectors, family, response):
    eng = ScoringEngine(pack_pipe(fit_pipe(train_df, family), detectors), device="cpu")
    out = eng.accumulated_local_effects(NAMES, kind="both", response=response)
    assert out["sample_rows"] == 256
    assert out["output_space"] == ("log_odds" if response == "raw" else "probability")
    for name, res in zip(NAMES, out["results"]):
        z = res["edges"]
        assert res["feature"] == name and 2 <= len(z) <= 21 and z == sorted(set(z))
        ale, n, k, d = _brute(eng, name, z, response)
        np.testing.assert_array_equal(res["counts"], n)
        np.testing.assert_array_equal(res["interval"], k)
        np.testing.assert_allclose(res["local_effect"], d, rtol=0, atol=1e-12)
        np.testing.assert_allclose(res["ale"], ale, rtol=0, atol=1e-12)
        mid = (res["ale"][:-1] + res["ale"][1:]) / 2
        assert abs((res["counts"] * mid).sum()) <= 1e-12  # the centring identity
        assert np.ptp(res["ale"]) > 0


def _split(col, thr, left, right):
    return [[N_ONEHOT + col, f32bits(thr), 1, 2], [-1, f32bits(left), 0, 0], [-1, f32bits(right), 0, 0]]


def _sample(n=300, seed=0):
    rng = np.random.default_rng(seed)
    codes = rng.integers(-1, 2, size=(n, N_CAT)).astype(np.int16)
    nums = rng.normal(0.0, 1.0, size=(n, N_NUM)).astype(np.float32)
    nums[:, 2] = 4.5  # constant
    nums[:7, 0] = np.nan
    return codes, nums


def test_additive_forest_ale_is_pdp():
    """Every tree tests one column only, so the model is additive and the ALE
    of a column is its PDP up to the centring constant."""
    trees = [_split(0, -0.5, 0.125, 0.5), _split(1, 0.25, 0.75, 0.25), _split(0, 0.5, 0.25, 0.875),
             _split(1, -1.0, 0.0, 0.375)]
    eng = ScoringEngine(hand_model(trees, [np.ones(3)] * 4), device="cpu")
    sample = _sample()
    for name in ("credit_limit", "age"):
        res = eng.accumulated_local_effects([name], sample=sample)["results"][0]
        pd = eng.partial_dependence([name], sample=sample, grid={name: res["edges"]})
        pd = pd["results"][0]["average"]
        assert np.ptp(pd) > 0.1
        np.testing.assert_allclose(res["ale"] - res["ale"][0], pd - pd[0], rtol=0, atol=1e-12)


def test_monotone_model_gives_a_monotone_curve(train_df, detectors):
    """Each tree is non-decreasing in the feature and both sums of a row add
    the same trees in the same order, so every local effect is >= 0 exactly,
    and so are the interval means and their running sum."""
    params = {**FAMILY_PARAMS["hgbt"], "monotone": {"bill_amount_1": 1}}
    eng = ScoringEngine(pack_pipe(fit_pipe(train_df, "hgbt", params), detectors), device="cpu")
    for response in ("raw", "probability"):
        res = eng.accumulated_local_effects(
            ["bill_amount_1"], kind="both", response=response, grid_resolution=50
        )["results"][0]
        assert (res["local_effect"] >= 0).all() and (np.diff(res["ale"]) >= 0).all()
        assert np.ptp(res["ale"]) > 0


def test_edge_rule_corners():
    """A stump on numeric column 0 (x <= 0: 0.25, else 0.75)."""
    eng = ScoringEngine(hand_model([_split(0, 0.0, 0.25, 0.75)], [np.ones(3)]), device="cpu")
    codes, nums = _sample()
    # grid override; rows outside it clamp into the first and last interval
    out = eng.accumulated_local_effects(
        ["credit_limit", "bill_amount_1"], sample=(codes, nums), kind="both",
        grid={"credit_limit": [-0.5, 0, 0.5]},
    )
    res, const = out["results"]
    x = np.where(np.isnan(nums[:, 0]), eng.packed.medians[0], nums[:, 0])
    assert (x < -0.5).any() and (x > 0.5).any()
    np.testing.assert_array_equal(res["interval"], np.where(x <= 0, 1, 2))
    np.testing.assert_array_equal(res["local_effect"], np.where(x <= 0, 0.0, 0.5))
    n2 = int((x > 0).sum())
    assert res["edges"] == [-0.5, 0.0, 0.5] and res["counts"].tolist() == [300 - n2, n2]
    np.testing.assert_allclose(res["ale"], np.array([0, 0, 0.5]) - 0.25 * n2 / 300, atol=1e-15)
    # a constant column: one edge, a zero curve, every row counted
    assert const["edges"] == [4.5] and const["ale"].tolist() == [0.0]
    assert const["counts"].tolist() == [300] and not const["local_effect"].any()
    # ties: three quantile positions interpolate between the same two values,
    # which leaves two intervals without a row
    ties = np.zeros((6, N_NUM), dtype=np.float32)
    ties[:, 0] = [0, 0, 0, 10, 10, 10]
    res = eng.accumulated_local_effects(["credit_limit"], sample=(codes[:6], ties))["results"][0]
    assert res["edges"] == [0.0, 2.5, 5.0, 7.5, 10.0] and res["counts"].tolist() == [3, 0, 0, 3]
    np.testing.assert_allclose(res["ale"], [-0.375, 0.125, 0.125, 0.125, 0.125], atol=1e-15)
    for junk in ([0.0], [0.0, 0.0], [1.0, 0.0], [0.0, float("nan")], [0.0, 1e39], ["a", "b"], 3.0):
        with pytest.raises(ValueError):
            eng.accumulated_local_effects(["age"], sample=(codes, nums), grid={"age": junk})
    for bad in (["sex"], ["shoe_size"], [("age", "credit_limit")], [], "age"):
        with pytest.raises(ValueError):
            eng.accumulated_local_effects(bad, sample=(codes, nums))
    with pytest.raises(ExplainUnavailable, match="background sample"):
        eng.accumulated_local_effects(["age"])
    # caps
    big = (np.zeros((65537, N_CAT), np.int16), np.zeros((65537, N_NUM), np.float32))
    for kw in ({"sample": big}, {"grid_resolution": 101}, {"grid": {"age": list(range(102))}}):
        with pytest.raises(ExplainTooLarge):
            eng.accumulated_local_effects(["age"], **{"sample": (codes, nums), **kw})
    with pytest.raises(ExplainTooLarge, match="14"):
        eng.accumulated_local_effects(["age"] * 15, sample=(codes, nums))


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


def test_http_and_cli(client, packed, model_dir, tmp_path):
    from creditcore import serve

    want = ScoringEngine(packed, device="cpu").accumulated_local_effects(
        ["age", "bill_amount_3"], grid_resolution=5, kind="both"
    )
    r = client.post("/explain/ale", json={"features": ["age", "bill_amount_3"],
                                          "grid_resolution": 5, "kind": "both"})
    assert r.status_code == 200, r.text
    out = str(tmp_path / "ale.json")
    run = subprocess.run(
        [sys.executable, "-m", "creditcore", "ale", "--model-directory", model_dir, "--features",
         "age,bill_amount_3", "--grid-resolution", "5", "--kind", "both", "--device", "cpu",
         "--out", out], capture_output=True, text=True, timeout=240,
    )
    assert run.returncode == 0, run.stderr[-800:]
    with open(out) as f:
        docs = [r.json(), json.load(f)]
    for doc in docs:
        assert doc["sample_rows"] == 256 and doc["kind"] == "both"
        assert doc["output_space"] == "probability"
        for got, ref in zip(doc["results"], want["results"]):
            assert got["feature"] == ref["feature"] and got["edges"] == ref["edges"]
            for key in ("ale", "counts", "interval", "local_effect"):
                np.testing.assert_array_equal(np.asarray(got[key]), ref[key])
    r = client.post("/explain/ale", json={"features": ["age"]})
    assert set(r.json()["results"][0]) == {"feature", "edges", "ale", "counts"}
    for body, status in (
        ({"features": ["sex"]}, 422),
        ({"features": ["shoe_size"]}, 422),
        ({"features": ["age"], "response": "raw"}, 422),
        ({"features": ["age"], "grid": {"age": [2.0, 1.0]}}, 422),
        ({"features": ["age"], "grid_resolution": 101}, 413),
        ({"features": ["age"] * 15}, 413),
    ):
        assert client.post("/explain/ale", json=body).status_code == status, body
    engines = serve.state["engines"]
    bare = dataclasses.replace(packed, bg_codes=None, bg_nums=None)
    serve.state["engines"] = [ScoringEngine(bare, device="cpu")]
    try:
        r = client.post("/explain/ale", json={"features": ["age"]})
        assert r.status_code == 501 and "background sample" in r.json()["detail"]
    finally:
        serve.state["engines"] = engines

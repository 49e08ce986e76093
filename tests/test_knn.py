"""Nearest-neighbour outlier scores on the CPU: the f64 reference against
scikit-learn and a hand-built case, the threshold rule, the engine, the POST
/outlier/knn route and the CLI."""

from __future__ import annotations

import dataclasses
import json
import sys

import numpy as np
import pytest

from creditcore import knn
from creditcore.engine import ExplainTooLarge, ExplainUnavailable, ScoringEngine
from creditcore.ops import cpu_ref
from creditcore.pack import encode_batch
from creditcore.schema import SAMPLE_REQUEST

KEYS = {"instance_score", "is_outlier", "threshold", "k", "score", "fpr", "n", "n_ref"}


@pytest.mark.parametrize("exclude_self", [False, True])
def test_reference_matches_sklearn(exclude_self):
    from sklearn.neighbors import NearestNeighbors

    rng = np.random.default_rng(3)
    zr = rng.normal(size=(83, 9)).astype(np.float32)
    zb = zr if exclude_self else rng.normal(size=(37, 9)).astype(np.float32)
    d2, idx = cpu_ref.knn_topk_cpu(zb, zr, 7, exclude_self=exclude_self, max_bytes=4096)
    nn = NearestNeighbors(algorithm="brute").fit(zr.astype(np.float64))
    # without X scikit-learn queries the fitted rows and leaves each one out
    dist, ind = nn.kneighbors(None if exclude_self else zb.astype(np.float64), n_neighbors=7)
    assert np.array_equal(idx, ind) and idx.dtype == np.int32
    assert np.abs(np.sqrt(d2) - dist).max() <= 1e-12


def test_tie_rule_and_exclude_self_by_hand():
    """Rows on a line at 0, 1, 1, 2, 5 (rows 1 and 2 are duplicates)."""
    z = np.array([[0.0], [1.0], [1.0], [2.0], [5.0]], dtype=np.float32)
    d2, idx = cpu_ref.knn_topk_cpu(z, z, 3)
    assert idx.tolist() == [[0, 1, 2], [1, 2, 0], [1, 2, 0], [3, 1, 2], [4, 3, 1]]
    assert d2.tolist() == [[0, 1, 1], [0, 0, 1], [0, 0, 1], [0, 1, 1], [0, 9, 16]]
    d2, idx = cpu_ref.knn_topk_cpu(z, z, 3, exclude_self=True)
    # the duplicate stays a neighbour at distance 0; only j == i is left out
    assert idx.tolist() == [[1, 2, 3], [2, 0, 3], [1, 0, 3], [1, 2, 0], [3, 1, 2]]
    assert d2.tolist() == [[1, 1, 4], [0, 1, 1], [0, 1, 1], [1, 1, 4], [9, 16, 16]]
    with pytest.raises(ValueError):
        cpu_ref.knn_topk_cpu(z, z, 5, exclude_self=True)  # only four other rows
    with pytest.raises(ValueError):
        cpu_ref.knn_topk_cpu(z[:4], z, 2, exclude_self=True)  # not the same rows


@pytest.mark.parametrize("score", ["kth", "mean"])
def test_engine_threshold_and_flags(packed, score_batch, score):
    from creditcore import mmd

    eng = ScoringEngine(packed, device="cpu")
    mu, sd = mmd.reference_scale(packed, packed.bg_nums)
    z_ref = mmd.embed(packed, packed.bg_codes, packed.bg_nums, mu, sd)
    loo = np.sqrt(cpu_ref.knn_topk_cpu(z_ref, z_ref, 5, exclude_self=True)[0])
    loo = loo[:, -1] if score == "kth" else loo.mean(axis=1)
    typical = int(np.argsort(loo)[len(loo) // 2])  # a copy of it scores below its own score

    codes, nums = encode_batch(score_batch.iloc[:40], packed.vocabs)
    codes[1], nums[1] = packed.bg_codes[typical], packed.bg_nums[typical]
    nums[0] = np.nan_to_num(nums[0]) + 50.0 * np.nanstd(packed.bg_nums, axis=0)  # far away
    out = eng.knn_outliers(codes, nums, k=5, score=score, fpr=0.1, neighbors=True)
    assert set(out) == KEYS | {"neighbor_index", "neighbor_distance"}
    assert (out["n"], out["n_ref"], out["k"], out["score"], out["fpr"]) == (40, 256, 5, score, 0.1)
    assert out["threshold"] == np.quantile(loo, 0.9)
    assert out["is_outlier"][0] == 1 and out["is_outlier"][1] == 0
    assert np.array_equal(out["is_outlier"], out["instance_score"] > out["threshold"])
    assert out["neighbor_index"][1, 0] == typical and out["neighbor_distance"][1, 0] == 0.0
    dist = out["neighbor_distance"]
    assert np.array_equal(out["instance_score"], dist[:, -1] if score == "kth" else dist.mean(1))
    # the reference override with the packed sample is the same call
    same = eng.knn_outliers(codes, nums, reference=(packed.bg_codes, packed.bg_nums),
                            k=5, score=score, fpr=0.1)
    assert np.array_equal(same["instance_score"], out["instance_score"])


def test_argument_errors_and_caps(packed, score_batch):
    eng = ScoringEngine(packed, device="cpu")
    codes, nums = encode_batch(score_batch.iloc[:8], packed.vocabs)
    for bad in (dict(k=0), dict(k=knn.KNN_MAX_K + 1), dict(k=2.5), dict(score="median"),
                dict(fpr=0.0), dict(fpr=1.0),
                dict(k=8, reference=(packed.bg_codes[:8], packed.bg_nums[:8]))):
        with pytest.raises(ValueError):
            eng.knn_outliers(codes, nums, **bad)
    with pytest.raises(ValueError):
        eng.knn_outliers(codes, np.where(np.arange(14) == 3, np.inf, nums).astype(np.float32))
    big = knn.KNN_MAX_ROWS + 1
    with pytest.raises(ExplainTooLarge):
        eng.knn_outliers(np.repeat(codes[:1], big, 0), np.repeat(nums[:1], big, 0))
    with pytest.raises(ExplainTooLarge):
        eng.knn_outliers(codes, nums,
                         reference=(np.repeat(codes[:1], big, 0), np.repeat(nums[:1], big, 0)))
    bare = ScoringEngine(dataclasses.replace(packed, bg_codes=None, bg_nums=None), device="cpu")
    with pytest.raises(ExplainUnavailable):
        bare.knn_outliers(codes, nums)
    assert bare.knn_outliers(codes, nums, reference=(packed.bg_codes, packed.bg_nums))["n"] == 8


def test_route(model_dir, packed):
    from fastapi.testclient import TestClient

    from creditcore import serve
    from creditcore.config import ServeConfig

    cfg = ServeConfig()
    cfg.model_directory = model_dir
    cfg.device = "cpu"
    with TestClient(serve.create_app(cfg)) as client:
        r = client.post("/outlier/knn", json={"records": SAMPLE_REQUEST, "neighbors": True})
        assert r.status_code == 200, r.text
        body = r.json()
        want = ScoringEngine(packed, device="cpu").knn_outliers_records(
            SAMPLE_REQUEST, neighbors=True)
        assert body["instance_score"] == want["instance_score"].tolist()
        assert body["is_outlier"] == want["is_outlier"].tolist() and body["k"] == 10
        assert body["neighbor_index"] == want["neighbor_index"].tolist()
        assert body["threshold"] == want["threshold"] and body["n_ref"] == 256
        r = client.post("/outlier/knn", json={"records": SAMPLE_REQUEST})
        assert set(r.json()) == KEYS  # no neighbours unless asked for
        for bad in ({"k": 0}, {"k": 33}, {"score": "max"}, {"fpr": 1.5}, {"records": []}):
            body = {"records": SAMPLE_REQUEST, **bad}
            assert client.post("/outlier/knn", json=body).status_code == 422, bad
        big = {"records": SAMPLE_REQUEST * (knn.KNN_MAX_ROWS + 1)}
        assert client.post("/outlier/knn", json=big).status_code == 413
        engines = serve.state["engines"]
        bare = dataclasses.replace(packed, bg_codes=None, bg_nums=None)
        serve.state["engines"] = [ScoringEngine(bare, device="cpu")]
        try:
            r = client.post("/outlier/knn", json={"records": SAMPLE_REQUEST})
            assert r.status_code == 501 and "background sample" in r.json()["detail"]
        finally:
            serve.state["engines"] = engines


def test_cli_round_trip(model_dir, packed, score_batch, tmp_path, monkeypatch, capsys):
    from creditcore import __main__ as cli

    data, out = tmp_path / "batch.csv", tmp_path / "out.json"
    score_batch.iloc[4:24].to_csv(data, index=False)
    monkeypatch.setattr(sys, "argv", [
        "creditcore", "outlier-knn", "--model-directory", model_dir, "--data", str(data),
        "--k", "3", "--score", "mean", "--neighbors", "--device", "cpu", "--out", str(out)])
    cli.main()
    doc = json.loads(out.read_text())
    want = ScoringEngine(packed, device="cpu").knn_outliers_records(
        score_batch.iloc[4:24], k=3, score="mean", neighbors=True)
    assert doc["instance_score"] == want["instance_score"].tolist()
    assert doc["neighbor_index"] == want["neighbor_index"].tolist()
    assert (doc["k"], doc["score"], doc["n"], doc["device"]) == (3, "mean", 20, "cpu")
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["n"] == 20

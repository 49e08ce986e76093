"""Forest proximity on the CPU: the leaf walk against scikit-learn's apply,
the properties of the definition, the engine's arguments and caps, the POST
/explain/proximity route and the CLI. Every comparison is exact."""

from __future__ import annotations

import dataclasses
import json
import sys

import numpy as np
import pytest

from creditcore import proximity as px
from creditcore.engine import ExplainTooLarge, ExplainUnavailable, ScoringEngine
from creditcore.ops import cpu_ref
from creditcore.pack import encode_batch
from creditcore.schema import FEATURES, SAMPLE_REQUEST

KEYS = {"instance_score", "is_outlier", "threshold", "k", "score", "fpr", "n", "n_ref", "n_trees"}


def test_leaves_co_membership_matches_sklearn(packed, loaded_pyfunc, score_batch):
    """The node numbering differs, so the pair counts are compared, not the
    ids: all 512 x 512 pairs, none left out."""
    pipe = loaded_pyfunc.python_model.classifier
    a = pipe[-1].apply(pipe[:-1].transform(score_batch[FEATURES]))
    a = np.asarray(a).reshape(len(score_batch), -1)
    codes, nums = encode_batch(score_batch, packed.vocabs)
    leaf = cpu_ref.forest_leaves_cpu(packed, codes, cpu_ref.impute_nums(packed, nums))
    assert leaf.shape == a.shape == (512, packed.cls_n_trees) and leaf.dtype == np.int32
    assert (packed.cls_nodes[leaf, 0] < 0).all()  # every id is a leaf of the table
    want = np.stack([(a[i][None] == a).sum(-1) for i in range(len(a))])
    got = np.stack([(leaf[i][None] == leaf).sum(-1) for i in range(len(leaf))])
    assert np.array_equal(got, want)


def test_definition_properties(packed):
    leaf = cpu_ref.forest_leaves_cpu(
        packed, packed.bg_codes, cpu_ref.impute_nums(packed, packed.bg_nums))[:90].copy()
    leaf[40] = leaf[7]  # a duplicate: row 40 finds row 7 first, not itself
    m, t = leaf.shape
    count, idx = cpu_ref.forest_prox_topk_cpu(leaf, leaf, 5, max_bytes=4096)
    first = np.arange(m)
    first[40] = 7
    assert np.array_equal(idx[:, 0], first) and (count[:, 0] == t).all()
    assert (np.diff(count, axis=1) <= 0).all()
    loo_count, loo_idx = cpu_ref.forest_prox_topk_cpu(leaf, leaf, 5, exclude_self=True)
    assert (loo_idx != np.arange(m)[:, None]).all()
    assert loo_idx[7, 0] == 40 and loo_idx[40, 0] == 7 and loo_count[40, 0] == t
    full, order = cpu_ref.forest_prox_topk_cpu(leaf, leaf, m)  # the whole matrix, sorted
    dense = np.empty((m, m), dtype=np.int32)
    np.put_along_axis(dense, order, full, axis=1)
    assert np.array_equal(dense, dense.T)
    # rows that share no leaf fill the list, lowest j first
    c, j = cpu_ref.forest_prox_topk_cpu(np.array([[5, 9]]), np.array([[0, 0], [5, 1], [2, 2]]), 3)
    assert c.tolist() == [[1, 0, 0]] and j.tolist() == [[1, 0, 2]]


@pytest.mark.parametrize("score", ["kth", "mean"])
def test_engine_scores_and_threshold(packed, score_batch, score):
    eng = ScoringEngine(packed, device="cpu")
    codes, nums = encode_batch(score_batch.iloc[:40], packed.vocabs)
    codes[1], nums[1] = packed.bg_codes[17], packed.bg_nums[17]
    out = eng.proximity(codes, nums, k=5, score=score, fpr=0.1)
    t = packed.cls_n_trees
    assert set(out) == KEYS | {"neighbor_index", "neighbor_proximity"}
    assert (out["n"], out["n_ref"], out["n_trees"], out["k"]) == (40, 256, t, 5)
    leaf = cpu_ref.forest_leaves_cpu(
        packed, packed.bg_codes, cpu_ref.impute_nums(packed, packed.bg_nums))
    loo = cpu_ref.forest_prox_topk_cpu(leaf, leaf, 5, exclude_self=True)[0]
    assert out["threshold"] == px.threshold(loo, t, score, 0.1)
    assert out["neighbor_index"][1, 0] == 17 and out["neighbor_proximity"][1, 0] == 1.0
    shared = np.rint(out["neighbor_proximity"] * t)  # the integer counts
    assert np.array_equal(out["instance_score"], px.scores(shared, t, score))
    assert np.array_equal(out["neighbor_proximity"], shared / t)
    assert np.array_equal(out["is_outlier"], out["instance_score"] > out["threshold"])
    same = eng.proximity(codes, nums, reference=(packed.bg_codes, packed.bg_nums),
                         k=5, score=score, fpr=0.1, neighbors=False)
    assert set(same) == KEYS and np.array_equal(same["instance_score"], out["instance_score"])


def test_argument_errors_and_caps(packed, score_batch):
    eng = ScoringEngine(packed, device="cpu")
    codes, nums = encode_batch(score_batch.iloc[:8], packed.vocabs)
    for bad in (dict(k=0), dict(k=px.PROX_MAX_K + 1), dict(k=2.5), dict(score="median"),
                dict(fpr=0.0), dict(fpr=1.0),
                dict(k=8, reference=(packed.bg_codes[:8], packed.bg_nums[:8]))):
        with pytest.raises(ValueError):
            eng.proximity(codes, nums, **bad)
    with pytest.raises(ValueError):
        eng.proximity(codes[:0], nums[:0])
    big = px.PROX_MAX_ROWS + 1
    with pytest.raises(ExplainTooLarge):
        eng.proximity(np.repeat(codes[:1], big, 0), np.repeat(nums[:1], big, 0))
    with pytest.raises(ExplainTooLarge):
        eng.proximity(codes, nums,
                      reference=(np.repeat(codes[:1], big, 0), np.repeat(nums[:1], big, 0)))
    off = np.zeros(px.PROX_MAX_TREES + 2, dtype=packed.cls_tree_offsets.dtype)
    with pytest.raises(ExplainTooLarge):
        ScoringEngine(dataclasses.replace(packed, cls_tree_offsets=off),
                      device="cpu").proximity(codes, nums)
    bare = ScoringEngine(dataclasses.replace(packed, bg_codes=None, bg_nums=None), device="cpu")
    with pytest.raises(ExplainUnavailable):
        bare.proximity(codes, nums)
    assert bare.proximity(codes, nums, reference=(packed.bg_codes, packed.bg_nums))["n"] == 8


def test_route(model_dir, packed):
    from fastapi.testclient import TestClient

    from creditcore import serve
    from creditcore.config import ServeConfig

    cfg = ServeConfig()
    cfg.model_directory = model_dir
    cfg.device = "cpu"
    with TestClient(serve.create_app(cfg)) as client:
        r = client.post("/explain/proximity", json={"records": SAMPLE_REQUEST * 3, "k": 4})
        assert r.status_code == 200, r.text
        body = r.json()
        want = ScoringEngine(packed, device="cpu").proximity_records(SAMPLE_REQUEST * 3, k=4)
        for key in KEYS | {"neighbor_index", "neighbor_proximity"}:
            w = want[key]
            assert body[key] == (w.tolist() if isinstance(w, np.ndarray) else w), key
        r = client.post("/explain/proximity", json={"records": SAMPLE_REQUEST, "neighbors": False})
        assert set(r.json()) == KEYS  # no neighbours when declined
        for bad in ({"k": 0}, {"k": 33}, {"score": "max"}, {"fpr": 1.5}, {"records": []}):
            body = {"records": SAMPLE_REQUEST, **bad}
            assert client.post("/explain/proximity", json=body).status_code == 422, bad
        big = {"records": SAMPLE_REQUEST * (px.PROX_MAX_ROWS + 1)}
        assert client.post("/explain/proximity", json=big).status_code == 413
        engines = serve.state["engines"]
        bare = dataclasses.replace(packed, bg_codes=None, bg_nums=None)
        serve.state["engines"] = [ScoringEngine(bare, device="cpu")]
        try:
            r = client.post("/explain/proximity", json={"records": SAMPLE_REQUEST})
            assert r.status_code == 501 and "background sample" in r.json()["detail"]
        finally:
            serve.state["engines"] = engines


def test_cli_round_trip(model_dir, packed, score_batch, tmp_path, monkeypatch, capsys):
    from creditcore import __main__ as cli

    data, out = tmp_path / "batch.csv", tmp_path / "out.json"
    score_batch.iloc[4:24].to_csv(data, index=False)
    monkeypatch.setattr(sys, "argv", [
        "creditcore", "proximity", "--model-directory", model_dir, "--data", str(data),
        "--k", "3", "--score", "mean", "--device", "cpu", "--out", str(out)])
    cli.main()
    doc = json.loads(out.read_text())
    want = ScoringEngine(packed, device="cpu").proximity_records(
        score_batch.iloc[4:24], k=3, score="mean")
    assert doc["instance_score"] == want["instance_score"].tolist()
    assert doc["neighbor_index"] == want["neighbor_index"].tolist()
    assert (doc["k"], doc["score"], doc["n"], doc["device"]) == (3, "mean", 20, "cpu")
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["n"] == 20

"""Anchor rules on the CPU engine: cpu_ref.forest_anchor_cpu against a brute
loop over written-out composite rows, the search against the definition, a
hand-built stump, and the HTTP route and CLI."""

from __future__ import annotations

import dataclasses
import json
import subprocess
import sys

import numpy as np
import pytest

from _pdp_cases import fit_pipe, pack_pipe
from _shap_models import N_ONEHOT, f32bits, hand_model
from creditcore import anchors as an
from creditcore.counterfactual import raw_cut
from creditcore.engine import ExplainTooLarge, ExplainUnavailable, ScoringEngine
from creditcore.ops import cpu_ref
from creditcore.pack import N_CAT, N_NUM
from creditcore.schema import FEATURES

FULL = (1 << (N_CAT + N_NUM)) - 1


@pytest.fixture(scope="module")
def hgbt(train_df):
    from creditcore.train import fit_detectors

    return pack_pipe(fit_pipe(train_df, "hgbt"), fit_detectors(train_df))


def _rows(p, n: int, seed: int):
    """n sample rows of the pack with a NaN numeric and an unknown category."""
    pick = np.random.default_rng(seed).integers(0, len(p.bg_codes), size=n)
    codes, nums = p.bg_codes[pick].copy(), p.bg_nums[pick].copy()
    nums[0, 4], codes[min(1, n - 1), 2] = np.nan, -1
    return codes, nums


def _tables(p, codes, nums):
    bg_imp = cpu_ref.impute_nums(p, p.bg_nums)
    edges = an.disc_edges(bg_imp, np.array([25.0, 50.0, 75.0]))
    nums_imp = cpu_ref.impute_nums(p, nums)
    return nums_imp, bg_imp, edges, an.sat_table(codes, nums_imp, p.bg_codes, bg_imp, edges)


def _composite(codes_i, nums_i, bg_codes, bg_imp, sat_i, mask):
    """The definition, row by row: sample row b with the players of
    ``mask & ~sat[b]`` taken from row i."""
    c, x = bg_codes.copy(), bg_imp.copy()
    for b in range(len(c)):
        for pl in range(N_CAT + N_NUM):
            if (mask >> pl) & 1 and not (int(sat_i[b]) >> pl) & 1:
                if pl < N_CAT:
                    c[b, pl] = codes_i[pl]
                else:
                    x[b, pl - N_CAT] = nums_i[pl - N_CAT]
    return c, x


def test_reference_against_scored_composites(packed):
    eng = ScoringEngine(packed, device="cpu")
    codes, nums = _rows(packed, 3, 1)
    nums_imp, bg_imp, _, sat = _tables(packed, codes, nums)
    rng = np.random.default_rng(2)
    lists = [np.array([0, FULL, 1 << 3, (1 << 9) | (1 << 20)], dtype=np.uint32),
             np.empty(0, dtype=np.uint32), rng.integers(0, FULL + 1, size=5).astype(np.uint32)]
    off = np.concatenate([[0], np.cumsum([len(m) for m in lists])]).astype(np.int32)
    counts, sums = cpu_ref.forest_anchor_cpu(
        packed, codes, nums_imp, packed.bg_codes, bg_imp, sat, np.concatenate(lists), off,
        raw_cut(packed, 0.5), want_sums=True,
    )
    assert counts.dtype == np.int32 and sums.shape == (9, len(bg_imp))
    at = 0
    for i, masks in enumerate(lists):
        for mask in masks:
            c, x = _composite(codes[i], nums_imp[i], packed.bg_codes, bg_imp, sat[i], int(mask))
            prob = eng.score_arrays(c, x, with_drift=False)["predictions"]
            assert counts[at] == int((prob > 0.5).sum())
            at += 1
    # the empty anchor leaves the sample as it is, for every row
    np.testing.assert_array_equal(
        sums[0], cpu_ref.forest_raw_cpu(packed, packed.bg_codes, bg_imp, tree_order=True)
    )


def test_stump_returns_its_feature():
    """One stump on numeric column 5 (credit-schema name below): the anchor of
    a row is exactly that column's interval, precise at once."""
    stump = np.array(
        [[N_ONEHOT + 5, f32bits(0.0), 1, 2], [-1, f32bits(0.0), 0, 0], [-1, f32bits(1.0), 0, 0]],
        dtype=np.int32,
    )
    rng = np.random.default_rng(4)
    bg_codes = rng.integers(0, 2, size=(64, N_CAT)).astype(np.int16)
    bg_nums = rng.normal(size=(64, N_NUM)).astype(np.float32)
    # linear-interpolation quartiles of 16 each of -3, -1, 1, 3: -1.5, 0, 1.5
    bg_nums[:, 5] = np.repeat([-3.0, -1.0, 1.0, 3.0], 16)
    p = dataclasses.replace(hand_model([stump], [np.ones(3)]), bg_codes=bg_codes, bg_nums=bg_nums)
    eng = ScoringEngine(p, device="cpu")
    out = eng.anchors(bg_codes[[0, 40]], bg_nums[[0, 40]])
    name = FEATURES[N_CAT + 5]
    lo_row, hi_row = out["rows"]
    assert out["sample_rows"] == 64 and out["beam_size"] == 2
    assert lo_row["anchor"] == [{"feature": name, "low": None, "high": -1.5}]
    assert lo_row["names"] == [f"{name} <= -1.5"] and lo_row["decision"] == 0
    assert hi_row["anchor"] == [{"feature": name, "low": 0.0, "high": 1.5}]
    assert hi_row["names"] == [f"0.0 < {name} <= 1.5"] and hi_row["decision"] == 1
    for row in out["rows"]:
        assert row["met"] and row["precision"] == 1.0 and row["coverage"] == 0.25
    # coverage(empty) == 1 always; precision(full) == 1 here because the
    # stump's threshold is an interval edge (a composite keeps the sample's
    # value inside the row's interval, so on a fitted forest it can be lower)
    codes, nums = bg_codes[::9], bg_nums[::9]
    nums_imp, bg_imp, _, sat = _tables(p, codes, nums)
    masks = np.tile(np.array([0, FULL], dtype=np.uint32), len(codes))
    off = (2 * np.arange(len(codes) + 1)).astype(np.int32)
    counts, _ = cpu_ref.forest_anchor_cpu(p, codes, nums_imp, bg_codes, bg_imp, sat, masks, off, 0.5)
    own = nums_imp[:, 5] > 0.0
    np.testing.assert_array_equal(counts[1::2], np.where(own, 64, 0))
    assert all(an.coverage_counts(sat[i], np.array([0]))[0] == 64 for i in range(len(codes)))


def test_hgbt_anchor_against_the_definition(hgbt):
    p = hgbt
    eng = ScoringEngine(p, device="cpu")
    codes, nums = _rows(p, 6, 5)
    out = eng.anchors(codes, nums, precision_threshold=0.9, beam_size=3, max_anchor_size=4)
    nums_imp, bg_imp, edges, sat = _tables(p, codes, nums)
    cut = raw_cut(p, 0.5)
    s = len(bg_imp)
    assert out["precision_threshold"] == 0.9 and out["beam_size"] == 3 and out["sample_rows"] == s
    for i, row in enumerate(out["rows"]):
        mask = sum(1 << FEATURES.index(e["feature"]) for e in row["anchor"])
        assert len(row["anchor"]) == len(row["names"]) <= 4
        c, x = _composite(codes[i], nums_imp[i], p.bg_codes, bg_imp, sat[i], mask)
        raw = cpu_ref.forest_raw_cpu(p, c, x, tree_order=True)
        own = cpu_ref.forest_raw_cpu(p, codes[i : i + 1], nums_imp[i : i + 1], tree_order=True)[0]
        assert row["decision"] == int(own > cut)
        assert row["precision"] == ((raw > cut) == (own > cut)).sum() / s
        assert row["coverage"] == ((sat[i] & mask) == mask).sum() / s
        assert row["met"] == (row["precision"] >= 0.9)
        for e in row["anchor"]:  # the row satisfies its own predicates
            pl = FEATURES.index(e["feature"])
            if pl >= N_CAT:
                v = nums_imp[i, pl - N_CAT]
                assert (e["low"] is None or e["low"] < v) and (e["high"] is None or v <= e["high"])
    with pytest.raises(ExplainTooLarge):
        eng.anchors(codes, nums, beam_size=5)
    with pytest.raises(ExplainTooLarge):
        eng.anchors(np.tile(codes, (171, 1)), np.tile(nums, (171, 1)))
    with pytest.raises(ExplainUnavailable):
        bare = dataclasses.replace(p, bg_codes=None, bg_nums=None)
        ScoringEngine(bare, device="cpu").anchors(codes, nums)


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


def test_http_and_cli(client, packed, model_dir, train_df, tmp_path):
    from creditcore import serve

    df = train_df[FEATURES].head(4)
    kw = {"precision_threshold": 0.9, "max_anchor_size": 3}
    want = ScoringEngine(packed, device="cpu").anchors_records(df, **kw)
    body = {"records": df.to_dict("records"), **kw}
    r = client.post("/explain/anchors", json=body)
    assert r.status_code == 200, r.text
    csv, out = str(tmp_path / "rows.csv"), str(tmp_path / "anchors.json")
    df.to_csv(csv, index=False)
    run = subprocess.run(
        [sys.executable, "-m", "creditcore", "anchors", "--model-directory", model_dir,
         "--data", csv, "--precision-threshold", "0.9", "--max-anchor-size", "3",
         "--device", "cpu", "--out", out], capture_output=True, text=True, timeout=240,
    )
    assert run.returncode == 0, run.stderr[-800:]
    with open(out) as f:
        docs = [r.json(), json.load(f)]
    for doc in docs:
        assert doc["rows"] == want["rows"] and doc["sample_rows"] == want["sample_rows"]
        assert set(doc["rows"][0]) == {
            "anchor", "names", "precision", "coverage", "met", "decision", "probability"
        }
    assert "/explain/anchors" in client.get("/openapi.json").json()["paths"]
    for change, status in (
        ({"records": body["records"] * 257}, 413),
        ({"beam_size": 5}, 413),
        ({"records": []}, 422),
        ({"precision_threshold": 1.5}, 422),
        ({"max_anchor_size": 0}, 422),
        ({"disc_perc": [50, 25]}, 422),
        ({"threshold": 1.0}, 422),
    ):
        assert client.post("/explain/anchors", json={**body, **change}).status_code == status
    engines = serve.state["engines"]
    bare = dataclasses.replace(packed, bg_codes=None, bg_nums=None)
    serve.state["engines"] = [ScoringEngine(bare, device="cpu")]
    try:
        r = client.post("/explain/anchors", json=body)
        assert r.status_code == 501 and "background sample" in r.json()["detail"]
    finally:
        serve.state["engines"] = engines

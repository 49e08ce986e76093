"""Single-feature counterfactuals on the CPU: breakpoint tables, the dumb
reference (cpu_ref.forest_sweep_cpu) against scikit-learn, exactness at the
breakpoints, the monotone guarantee, and the engine, route and CLI."""

from __future__ import annotations

import json
import subprocess
import sys

import numpy as np
import pytest

from _cf_cases import (
    FAMILIES,
    SWEPT,
    down,
    fit_pipe,
    forest_of,
    hand_forest,
    hand_rows,
    num,
    pack_pipe,
    sample_frame,
    up,
)
from creditcore import counterfactual as cf
from creditcore.engine import ExplainTooLarge, ScoringEngine
from creditcore.ops import cpu_ref
from creditcore.pack import N_CAT, N_NUM, encode_batch
from creditcore.schema import CATEGORICAL_FEATURES, FEATURES, NUMERIC_FEATURES


@pytest.fixture(scope="module")
def detectors(train_df):
    from creditcore.train import fit_detectors

    return fit_detectors(train_df)


@pytest.fixture(scope="module")
def sample_df(train_df):
    return sample_frame(train_df)


# ---------------------------------------------------------- breakpoint tables


def test_breakpoint_tables():
    p = hand_forest()
    t = cf.build_tables(p)
    one_up = up(1.0)
    np.testing.assert_array_equal(
        t.thresholds[SWEPT], np.array([-1.0, 0.5, 1.0, one_up, 2.0], dtype=np.float32)
    )
    assert [len(x) for x in t.thresholds] == [0, 0, 1, 5, 0, 1] + [0] * 8
    assert t.thr_off.tolist() == [0, 0, 0, 1, 6, 6] + [7] * 9 and t.thr.dtype == np.float32
    assert t.node_rank.dtype == np.int32 and len(t.node_rank) == len(p.cls_nodes)
    assert t.max_depth == 3
    # ranks: index-aligned with cls_nodes, -1 for leaves and one-hot nodes
    feat = p.cls_nodes[:, 0]
    value = p.cls_nodes[:, 1].copy().view(np.float32)
    on_swept = feat == num(SWEPT)
    assert (t.node_rank[feat < 0] == -1).all()
    assert (t.node_rank[(feat >= 0) & (feat < num(0))] == -1).all()  # one-hot nodes
    rank_of = {-1.0: 0, 0.5: 1, 1.0: 2, float(one_up): 3, 2.0: 4}
    assert [int(r) for r in t.node_rank[on_swept]] == [rank_of[float(v)] for v in value[on_swept]]
    # 1.0 is tested by three trees (and twice on one path): one shared rank;
    # the threshold one ulp above it has the next
    assert (value[on_swept] == 1.0).sum() == 4
    assert set(t.node_rank[on_swept & (value == 1.0)]) == {2}
    assert set(t.node_rank[on_swept & (value == one_up)]) == {3}


def test_own_interval():
    p = hand_forest()
    thr = cf.build_tables(p).thresholds[SWEPT]
    for v, k0 in (
        (1.0, 2),  # on a threshold: inside the interval that ends there
        (up(1.0), 3),  # one ulp above: the next interval (which ends at up(1))
        (up(up(1.0)), 4),
        (-1e30, 0),
        (-1.0, 0),
        (1e30, 5),
        (np.inf, 5),
    ):
        assert int(cf.own_interval(thr, v)) == k0
    # NaN: the kernel and the reference impute the median first
    codes, nums = hand_rows()
    assert np.isnan(nums[5, SWEPT])
    imp = cpu_ref.impute_nums(p, nums)
    assert imp[5, SWEPT] == p.medians[SWEPT]
    rec, _, curves = cpu_ref.forest_sweep_cpu(p, codes, imp, [[5, SWEPT], [0, SWEPT], [0, 0]])
    assert rec[0, 0] == int(cf.own_interval(thr, p.medians[SWEPT])) and rec[1, 0] == 2
    assert rec[2].tolist() == [0, -1, -1] and len(curves[2]) == 1  # K = 0
    reps = cf.representatives(thr)
    assert len(reps) == 6 and reps[-1] == up(2.0) and (reps[:-1] == thr).all()
    assert [int(cf.own_interval(thr, v)) for v in reps] == list(range(6))


def test_reference_walks_every_interval():
    """forest_sweep_cpu on the hand-built forest against a per-interval
    evaluation written out by hand for one row."""
    p = hand_forest()
    codes, nums = hand_rows()
    imp = cpu_ref.impute_nums(p, nums)
    rec, raw, curves = cpu_ref.forest_sweep_cpu(p, codes, imp, [[6, SWEPT]], cut=1.04)
    # row 6: code -1, OTHER = 1 (> 0), NAN_COL imputed by its median (<= -0.5)
    assert imp[6, 2] == p.medians[2] <= -0.5
    want = []
    for v in (-1.0, 0.5, 1.0, float(up(1.0)), 2.0, 3.0):
        t0 = (8 if v <= 1.0 else 4) / 64
        t1 = (2 if v <= 1.0 else 1) / 64
        t4 = (7 if v <= 1.0 else 9 if v <= float(up(1.0)) else 11) / 64
        t5 = (13 if v <= -1.0 else 17) / 64
        t6 = (1 if v <= 2.0 else 3) / 32
        want.append(t0 + t1 + 5 / 64 + 0.3125 + t4 + t5 + t6)
    np.testing.assert_array_equal(curves[0], np.asarray(want))
    k0 = 2  # 0.75 lies in (0.5, 1]
    assert rec[0, 0] == k0
    flips = [k for k in range(6) if (want[k] > 1.04) != (want[k0] > 1.04)]
    assert rec[0, 1] == max([k for k in flips if k < k0], default=-1)
    assert rec[0, 2] == min([k for k in flips if k > k0], default=-1)
    # a raw sum equal to the cut is not class 1
    rec_eq, _, _ = cpu_ref.forest_sweep_cpu(p, codes, imp, [[6, SWEPT]], cut=float(want[k0]))
    above = [k for k in range(6) if want[k] > want[k0]]
    assert rec_eq[0, 2] == min([k for k in above if k > k0], default=-1)


# ------------------------------------------------- the reference vs scikit-learn


def _with(df_row, name, value):
    row = df_row.copy()
    row[name] = value
    return row


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("threshold", [0.5, 0.3])
def test_sklearn_oracle(train_df, detectors, sample_df, family, threshold):
    """Every reported counterfactual, written into the row, gives the reported
    probability under the scikit-learn pipeline (1e-7, test_pdp's bound) and
    the opposite decision; the nearest representable value on the near side
    of the breakpoint still gives the original decision."""
    import pandas as pd

    pipe = fit_pipe(train_df, family)
    p = pack_pipe(pipe, detectors)
    codes, nums = encode_batch(sample_df, p.vocabs)
    out = ScoringEngine(p, device="cpu").counterfactuals(codes, nums, threshold=threshold)
    imp = cpu_ref.impute_nums(p, nums)
    frames, expect = [], []  # rows to score, (probability or None, decision)
    for i, row in enumerate(out["rows"]):
        own = sample_df.iloc[i].copy()
        for j, name in enumerate(NUMERIC_FEATURES):
            own[name] = float(imp[i, j])  # the imputed row, as the model sees it
        frames.append(own)
        expect.append((row["probability"], row["decision"]))
        for name, entry in row["counterfactuals"].items():
            if name in CATEGORICAL_FEATURES:
                for flip in entry["flips"]:
                    assert flip["category"] != entry["value"]
                    frames.append(_with(own, name, flip["category"]))
                    expect.append((flip["probability"], 1 - row["decision"]))
                continue
            assert entry["value"] == float(imp[i, FEATURES.index(name) - N_CAT])
            for side, near in (("below", up), ("above", down)):
                s = entry[side]
                if s is None:
                    continue
                assert (s["value"] < entry["value"]) == (side == "below")
                assert s["delta"] == s["value"] - entry["value"]
                frames.append(_with(own, name, s["value"]))
                expect.append((s["probability"], 1 - row["decision"]))
                # exactness: one f32 nearer to the row it has not flipped yet
                frames.append(_with(own, name, float(near(s["value"]))))
                expect.append((None, row["decision"]))
    x = pd.DataFrame(frames)[FEATURES]
    for c in NUMERIC_FEATURES:
        x[c] = x[c].astype(np.float64)
    proba = pipe.predict_proba(x)[:, 1]
    flips = 0
    for got, (prob, decision) in zip(proba, expect):
        if prob is not None:
            assert abs(got - prob) <= 1e-7
            flips += 1
        assert int(got > threshold) == decision
    assert flips > len(out["rows"]) + 20  # numeric and categorical flips exist
    sides = [e for r in out["rows"] for e in r["counterfactuals"].values()]
    assert any(e.get("below") for e in sides) and any(e.get("above") for e in sides)
    # categorical entries were checked above wherever they exist; the
    # depth-3 gbt flips no decision of these 64 rows through a category
    assert family == "gbt" or any(e.get("flips") for e in sides)


def test_monotone_curves(train_df, detectors):
    """On a feature constrained to -1 the exact curve of every background row
    is non-increasing over all K + 1 intervals, so a counterfactual exists on
    at most one side."""
    params = {"n_estimators": 20, "max_depth": 4, "random_state": 0, "device": "cpu",
              "monotone": {"credit_limit": -1}}
    p = pack_pipe(fit_pipe(train_df, "hgbt", params), detectors)
    assert len(p.bg_codes) == 256
    for threshold in (0.5, 0.25):
        out = ScoringEngine(p, device="cpu").counterfactuals(
            p.bg_codes, p.bg_nums, features=["credit_limit"], threshold=threshold, curves=True
        )
        moved = sided = 0
        for row in out["rows"]:
            e = row["counterfactuals"]["credit_limit"]
            assert len(e["probabilities"]) == len(e["thresholds"]) + 1 > 2
            assert (np.diff(e["probabilities"]) <= 0).all()
            assert e["below"] is None or e["above"] is None
            # class 1 can only be left by raising the limit, class 0 by lowering it
            assert (e["above"] is None) if row["decision"] == 0 else (e["below"] is None)
            moved += int(np.ptp(e["probabilities"]) > 0)
            sided += int(e["below"] is not None or e["above"] is not None)
        assert moved == 256
    assert sided > 0


# ------------------------------------------------------------ engine, route, CLI


@pytest.fixture(scope="module")
def engine(train_df, detectors):
    """A 21-tree forest: the reference costs one forest walk per interval, and
    the suite's packaged model carries thousands of thresholds per column."""
    return ScoringEngine(pack_pipe(fit_pipe(train_df, "rf"), detectors), device="cpu")


@pytest.fixture(scope="module")
def rows(engine, score_batch):
    return encode_batch(score_batch.iloc[:24], engine.packed.vocabs)


def _check_schema(out, names, n_rows, threshold, curves):
    assert out["threshold"] == threshold and out["features"] == list(names)
    assert len(out["rows"]) == n_rows
    for row in out["rows"]:
        assert set(row) == {"probability", "decision", "counterfactuals"}
        assert 0.0 <= row["probability"] <= 1.0 and row["decision"] in (0, 1)
        assert list(row["counterfactuals"]) == list(names)
        for name, e in row["counterfactuals"].items():
            if name in CATEGORICAL_FEATURES:
                assert set(e) == {"value", "flips"}
                assert all(set(f) == {"category", "probability"} for f in e["flips"])
                continue
            assert set(e) == {"value", "below", "above"} | (
                {"thresholds", "probabilities"} if curves else set()
            )
            for side in ("below", "above"):
                assert e[side] is None or set(e[side]) == {"value", "delta", "probability"}
            if curves:
                assert len(e["probabilities"]) == len(e["thresholds"]) + 1
                assert (np.diff(e["thresholds"]) > 0).all()


def test_engine_schema_and_arguments(engine, rows):
    codes, nums = rows
    packed = engine.packed
    out = engine.counterfactuals(codes, nums)
    _check_schema(out, FEATURES, 24, 0.5, False)
    scores = cpu_ref.score_forest_cpu(packed, codes, cpu_ref.impute_nums(packed, nums))
    np.testing.assert_allclose([r["probability"] for r in out["rows"]], scores, rtol=0, atol=1e-12)
    names = ["age", "sex", "credit_limit"]
    sub = engine.counterfactuals(codes, nums, features=names, threshold=0.3, curves=True)
    _check_schema(sub, names, 24, 0.3, True)
    assert [r["decision"] for r in sub["rows"]] == [int(s > 0.3) for s in scores]
    # the entry of a feature does not depend on what else was asked for
    alone = engine.counterfactuals(codes, nums, features=["sex"], threshold=0.3)
    for a, b in zip(sub["rows"], alone["rows"]):
        assert a["counterfactuals"]["sex"] == b["counterfactuals"]["sex"]
        assert a["probability"] == b["probability"] and a["decision"] == b["decision"]
    # the own interval of the curve carries the row's own probability
    t = cf.build_tables(packed)
    imp = cpu_ref.impute_nums(packed, nums)
    for i, r in enumerate(sub["rows"]):
        e = r["counterfactuals"]["age"]
        col = FEATURES.index("age") - N_CAT
        k0 = int(cf.own_interval(t.thresholds[col], imp[i, col]))
        assert e["probabilities"][k0] == r["probability"]
    for bad in (["no_such_feature"], "age", [], [3]):
        with pytest.raises(ValueError):
            engine.counterfactuals(codes, nums, features=bad)
    for bad in (0.0, 1.0, -1, 2, "0.5", None, float("nan")):
        with pytest.raises(ValueError):
            engine.counterfactuals(codes, nums, threshold=bad)
    with pytest.raises(ValueError):
        engine.counterfactuals(codes[:0], nums[:0])


def test_launch_slicing(engine, rows, monkeypatch):
    codes, nums = rows
    whole = engine.counterfactuals(codes, nums, curves=True)
    calls = []
    real = cpu_ref.forest_sweep_cpu

    def spy(p, c, x, jobs, *a):
        calls.append(len(jobs))
        return real(p, c, x, jobs, *a)

    monkeypatch.setattr(cpu_ref, "forest_sweep_cpu", spy)
    monkeypatch.setattr(ScoringEngine, "CF_LAUNCH_JOBS", 24 * N_NUM - 1)
    part = engine.counterfactuals(codes, nums, curves=True)
    assert calls == [24 * N_NUM - 1, 1]
    for a, b in zip(whole["rows"], part["rows"]):
        assert a["probability"] == b["probability"]
        for name in FEATURES:
            ea, eb = a["counterfactuals"][name], b["counterfactuals"][name]
            for key in ea:
                assert np.array_equal(ea[key], eb[key]) if key in (
                    "thresholds", "probabilities") else ea[key] == eb[key]


def test_caps(engine, rows, monkeypatch):
    codes, nums = rows
    big = (np.resize(codes, (cf.CF_MAX_ROWS + 1, N_CAT)), np.resize(nums, (cf.CF_MAX_ROWS + 1, N_NUM)))
    assert cf.CF_MAX_ROWS == ScoringEngine.SHAP_MAX_ROWS == 1024
    with pytest.raises(ExplainTooLarge, match="1024 rows"):
        engine.counterfactuals(*big, features=["sex"])
    t = cf.build_tables(engine.packed)
    points = 24 * sum(len(x) + 1 for x in t.thresholds)
    monkeypatch.setattr(cf, "CF_MAX_CURVE_POINTS", points - 1)
    with pytest.raises(ExplainTooLarge, match="curve points"):
        engine.counterfactuals(codes, nums, curves=True)
    engine.counterfactuals(codes, nums)  # the cap is on returned curves only
    monkeypatch.setattr(cf, "CF_MAX_CURVE_POINTS", points)
    engine.counterfactuals(codes, nums, curves=True)


def test_untested_column_and_leaf_forest():
    """K = 0: a forest that never tests a column has one interval there, no
    counterfactual on either side and no error; so for a forest of leaves."""
    codes, nums = hand_rows()
    for p in (hand_forest(), forest_of([0.75, 0.5, 0.25])):
        out = ScoringEngine(p, device="cpu").counterfactuals(codes, nums, curves=True)
        for row in out["rows"]:
            e = row["counterfactuals"]["age"]  # numeric column 0: never tested
            assert e["below"] is None and e["above"] is None
            assert len(e["thresholds"]) == 0 and list(e["probabilities"]) == [row["probability"]]
    assert all(r["counterfactuals"]["sex"]["flips"] == [] for r in out["rows"])


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


def _records(score_batch, n=6, start=4):
    return json.loads(score_batch.iloc[start : start + n].to_json(orient="records"))


def test_http_counterfactual(client, packed, score_batch):
    records = _records(score_batch)
    engine = ScoringEngine(packed, device="cpu")
    body = {"records": records, "features": ["age", "education"], "threshold": 0.35,
            "curves": True}
    r = client.post("/explain/counterfactual", json=body)
    assert r.status_code == 200, r.text
    got = r.json()
    want = engine.counterfactuals(
        *encode_batch(records, packed.vocabs), features=body["features"], threshold=0.35, curves=True
    )
    _check_schema(got, body["features"], 6, 0.35, True)
    for a, b in zip(got["rows"], want["rows"]):
        assert a["probability"] == b["probability"] and a["decision"] == b["decision"]
        ea, eb = a["counterfactuals"]["age"], b["counterfactuals"]["age"]
        assert (ea["below"], ea["above"], ea["value"]) == (eb["below"], eb["above"], eb["value"])
        np.testing.assert_array_equal(ea["probabilities"], eb["probabilities"])
        np.testing.assert_array_equal(ea["thresholds"], eb["thresholds"])
        assert a["counterfactuals"]["education"] == b["counterfactuals"]["education"]
    # defaults: threshold 0.5, no curves (features default to all 23: the
    # engine test; on this model that is thousands of intervals per column)
    d = client.post(
        "/explain/counterfactual", json={"records": records[:2], "features": ["sex", "age"]}
    ).json()
    _check_schema(d, ["sex", "age"], 2, 0.5, False)
    spec = client.get("/openapi.json").json()
    assert "/explain/counterfactual" in spec["paths"]


def test_http_counterfactual_errors(client, score_batch, monkeypatch):
    records = _records(score_batch, 2)

    def post(**kw):
        return client.post(
            "/explain/counterfactual", json={"records": records, "features": ["age"], **kw}
        )

    assert post(features=["no_such_feature"]).status_code == 422
    assert post(features=[]).status_code == 422
    for bad in (0.0, 1.0, 1.5, -0.1):
        assert post(threshold=bad).status_code == 422
    assert client.post("/explain/counterfactual", json={"features": ["age"]}).status_code == 422
    assert client.post("/explain/counterfactual", json={"records": []}).status_code == 400
    over = client.post(
        "/explain/counterfactual",
        json={"records": records * (cf.CF_MAX_ROWS // 2 + 1), "features": ["sex"]},
    )
    assert over.status_code == 413 and "1024" in over.json()["detail"]
    monkeypatch.setattr(cf, "CF_MAX_CURVE_POINTS", 10)
    assert post(curves=True).status_code == 413
    assert post(curves=False).status_code == 200
    monkeypatch.undo()

    def boom(*a, **k):
        raise RuntimeError("device fell over")

    monkeypatch.setattr(ScoringEngine, "counterfactuals", boom)
    r = post()
    assert r.status_code == 500 and "device fell over" in r.json()["detail"]


def test_cli_counterfactual(model_dir, packed, train_df, tmp_path):
    engine = ScoringEngine(packed, device="cpu")
    csv, out = str(tmp_path / "rows.csv"), str(tmp_path / "cf.json")
    train_df.iloc[:12].to_csv(csv, index=False)
    r = subprocess.run(
        [sys.executable, "-m", "creditcore", "counterfactual", "--model-directory", model_dir,
         "--data", csv, "--features", "age,sex", "--threshold", "0.4", "--curves",
         "--device", "cpu", "--out", out],
        capture_output=True, text=True, timeout=240,
    )
    assert r.returncode == 0, r.stderr[-800:]
    assert json.loads(r.stdout.strip().splitlines()[-1])["rows"] == 12
    with open(out) as f:
        doc = json.load(f)
    want = engine.counterfactuals(
        *encode_batch(train_df.iloc[:12], packed.vocabs), features=["age", "sex"],
        threshold=0.4, curves=True,
    )
    _check_schema(doc, ["age", "sex"], 12, 0.4, True)
    for a, b in zip(doc["rows"], want["rows"]):
        assert a["probability"] == b["probability"] and a["decision"] == b["decision"]
        ea, eb = a["counterfactuals"]["age"], b["counterfactuals"]["age"]
        assert (ea["below"], ea["above"]) == (eb["below"], eb["above"])
        np.testing.assert_array_equal(ea["probabilities"], eb["probabilities"])
        assert a["counterfactuals"]["sex"] == b["counterfactuals"]["sex"]

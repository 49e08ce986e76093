"""Permutation importance on the CPU. 1e-7 against scikit-learn's
predict_proba is the project's parity bound (test_pack_parity); 1e-12 against
sklearn.metrics: both sides reduce the same <= 64 f64 probabilities, and differ
by the order of that many additions of terms below 40 in magnitude (log loss
clipped at f64 eps: |log eps| < 37), 64 * 40 * 2^-53 < 1e-12."""

from __future__ import annotations

import json
import subprocess
import sys

import numpy as np
import pytest
from sklearn import metrics

from _pdp_cases import fit_pipe, pack_pipe
from creditcore import importance
from creditcore.engine import ExplainTooLarge, ScoringEngine
from creditcore.ops import cpu_ref
from creditcore.pack import N_CAT, N_NUM, encode_batch
from creditcore.pdp import finalize
from creditcore.schema import FEATURES, TARGET

NAMES = ["credit_limit", "repayment_status_1", "bill_amount_3"]
SKLEARN = {
    "accuracy": lambda y, p: metrics.accuracy_score(y, p > 0.5),
    "neg_log_loss": lambda y, p: -metrics.log_loss(y, p),
    "neg_brier_score": lambda y, p: -metrics.brier_score_loss(y, p),
    "roc_auc": metrics.roc_auc_score,
}


@pytest.fixture(scope="module")
def detectors(train_df):
    from creditcore.train import fit_detectors

    return fit_detectors(train_df)


@pytest.fixture(scope="module")
def labelled(train_df):
    """64 labelled rows with a NaN numeric and an unknown category."""
    df = train_df.sample(64, random_state=11).reset_index(drop=True)
    df.loc[0, "bill_amount_3"] = np.nan
    df.loc[1, "education"] = "phd_never_seen"
    assert 0 < df[TARGET].sum() < 64
    return df[FEATURES], df[TARGET].to_numpy()


@pytest.mark.parametrize("family", ["rf", "gbt"])
def test_against_scikit_learn(train_df, detectors, labelled, family):
    pipe = fit_pipe(train_df, family)
    p = pack_pipe(pipe, detectors)
    eng = ScoringEngine(p, device="cpu")
    x, y = labelled
    codes, nums = encode_batch(x, p.vocabs)
    rng = np.random.default_rng(1)
    perms = np.stack([[rng.permutation(64) for _ in range(2)] for _ in NAMES])
    players = np.repeat([FEATURES.index(n) for n in NAMES], 2)
    raw = cpu_ref.forest_permute_cpu(
        p, codes, cpu_ref.impute_nums(p, nums), players, perms.reshape(-1, 64)
    )
    prob = finalize(raw, int(p.cls_kind), float(p.cls_bias), int(p.cls_n_trees), "probability")
    for q, (name, perm) in enumerate((n, pm) for n, f in zip(NAMES, perms) for pm in f):
        shuffled = x.copy()
        shuffled[name] = x[name].to_numpy()[perm]
        want = pipe.predict_proba(shuffled)[:, 1]
        np.testing.assert_allclose(prob[q], want, rtol=0, atol=1e-7)
    assert (prob != prob[0]).any()
    base = cpu_ref.forest_raw_cpu(p, codes, cpu_ref.impute_nums(p, nums), tree_order=True)
    base = finalize(base, int(p.cls_kind), float(p.cls_bias), int(p.cls_n_trees), "probability")
    for scoring, fn in SKLEARN.items():
        out = eng.permutation_importance_records(
            x, y, features=NAMES, n_repeats=2, scoring=scoring, permutations=perms
        )
        assert (out["scoring"], out["n_repeats"], out["sample_rows"]) == (scoring, 2, 64)
        assert abs(out["baseline_score"] - fn(y, base)) <= 1e-12
        for f, res in enumerate(out["results"]):
            assert res["feature"] == NAMES[f]
            permuted = out["baseline_score"] - res["importances"]
            want = [fn(y, prob[2 * f + k]) for k in range(2)]
            np.testing.assert_allclose(permuted, want, rtol=0, atol=1e-12)
            assert res["importances_mean"] == res["importances"].mean()
            assert res["importances_std"] == res["importances"].std()


def test_identity_seed_and_errors(packed, labelled):
    eng = ScoringEngine(packed, device="cpu")
    x, y = labelled
    smp = encode_batch(x, packed.vocabs)
    # a feature permuted by the identity has importance exactly 0
    ident = np.tile(np.arange(64), (1, 3, 1))
    res = eng.permutation_importance(smp, y, features=["age"], n_repeats=3, permutations=ident)
    assert not res["results"][0]["importances"].any()
    # the same seed gives the same numbers, another seed other numbers
    a, b, c = (eng.permutation_importance(smp, y, seed=s)["results"] for s in (4, 4, 5))
    assert [r["feature"] for r in a] == FEATURES
    assert all(np.array_equal(ra["importances"], rb["importances"]) for ra, rb in zip(a, b))
    assert any(not np.array_equal(ra["importances"], rc["importances"]) for ra, rc in zip(a, c))
    base = {eng.permutation_importance(smp, y, seed=s)["baseline_score"] for s in (4, 5)}
    assert len(base) == 1
    for kw in (
        {"features": ["shoe_size"]}, {"features": ["age", "age"]}, {"features": []},
        {"scoring": "f1"}, {"n_repeats": 0}, {"threshold": 1.0}, {"seed": -1},
        {"permutations": ident}, {"permutations": np.zeros((23, 5, 64), dtype=np.int64)},
    ):
        with pytest.raises(ValueError):
            eng.permutation_importance(smp, y, **kw)
    for labels in (y[:-1], np.where(y == 1, 2, y), np.zeros(64), y.astype(float) / 2):
        with pytest.raises(ValueError):
            eng.permutation_importance(smp, labels)
    eng.permutation_importance(smp, np.zeros(64), features=["age"], scoring="accuracy")
    big = (np.zeros((65537, N_CAT), np.int16), np.zeros((65537, N_NUM), np.float32))
    with pytest.raises(ExplainTooLarge, match="65536"):
        eng.permutation_importance(big, np.zeros(65537))
    with pytest.raises(ExplainTooLarge, match="32"):
        eng.permutation_importance(smp, y, n_repeats=33)
    assert importance.IMPORTANCE_MAX_ROWS == 65536 and importance.IMPORTANCE_MAX_REPEATS == 32


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
    df = train_df.head(40)
    assert 0 < df[TARGET].sum() < 40
    kw = {"features": ["age", "sex"], "n_repeats": 3, "scoring": "neg_log_loss", "seed": 2}
    want = ScoringEngine(packed, device="cpu").permutation_importance_records(
        df[FEATURES], df[TARGET].to_numpy(), **kw
    )
    body = {"records": df[FEATURES].to_dict("records"), "labels": df[TARGET].tolist(), **kw}
    r = client.post("/explain/importance", json=body)
    assert r.status_code == 200, r.text
    csv, out = str(tmp_path / "labelled.csv"), str(tmp_path / "importance.json")
    df.to_csv(csv, index=False)
    run = subprocess.run(
        [sys.executable, "-m", "creditcore", "importance", "--model-directory", model_dir,
         "--data", csv, "--features", "age,sex", "--n-repeats", "3", "--scoring", "neg_log_loss",
         "--seed", "2", "--device", "cpu", "--out", out], capture_output=True, text=True,
        timeout=240,
    )
    assert run.returncode == 0, run.stderr[-800:]
    with open(out) as f:
        docs = [r.json(), json.load(f)]
    for doc in docs:
        assert doc["baseline_score"] == want["baseline_score"] and doc["sample_rows"] == 40
        assert [res["feature"] for res in doc["results"]] == ["age", "sex"]
        for got, ref in zip(doc["results"], want["results"]):
            np.testing.assert_array_equal(got["importances"], ref["importances"])
            assert got["importances_mean"] == ref["importances_mean"]
    for change, status in (
        ({"n_repeats": 33}, 413),
        ({"labels": body["labels"][:-1]}, 422),
        ({"labels": [2] * 40}, 422),
        ({"labels": [0] * 40, "scoring": "roc_auc"}, 422),
        ({"features": ["shoe_size"]}, 422),
        ({"scoring": "f1"}, 422),
    ):
        assert client.post("/explain/importance", json={**body, **change}).status_code == status

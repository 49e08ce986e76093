"""Monotone constraints of HistGBTClassifier on the CPU: the vectorised
reference of the constrained split search against a scalar brute force, the
trainer (bounds propagation, exact monotonicity of the fitted score), and the
public surface (pipeline, training job, CLI). The HIP kernel is tested
against the same reference in test_hgbt_mono_gpu.py."""

from __future__ import annotations

import json
import os

import numpy as np
import pytest
from _hgbt_mono_cases import INF, S, brute_force, hand_cases, run_case

from creditcore.models.forest import make_classifier_pipeline
from creditcore.models.hgbt import (
    _TREE_KEYS,
    HistGBTClassifier,
    _to_dense_f32,
    verify_monotone,
)
from creditcore.ops import cpu_ref
from creditcore.schema import FEATURES, NUMERIC_FEATURES, TARGET

CASES = hand_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_vs_brute_force_hand_built(name):
    got = run_case(cpu_ref.hgbt_split_mono_cpu, CASES[name])
    if name == "bounds_clamp_one_side":  # the clamp did change the gain
        free = dict(CASES[name], bounds=np.asarray([[-INF, INF]]))
        assert run_case(cpu_ref.hgbt_split_mono_cpu, free)[0, 0] != got[0, 0]


def test_reference_vs_brute_force_random():
    """Random small levels: signs, bounds of every kind, both (l2, min_leaf)."""
    rng = np.random.default_rng(0)
    n_bins = [2, 9, 5, 2]
    off = np.concatenate([[0], np.cumsum(n_bins)]).astype(np.int32)
    n, k = 400, 6
    bins = np.stack([rng.integers(0, nb, size=n) for nb in n_bins]).astype(np.uint8)
    node = rng.integers(0, k, size=n).astype(np.int32)
    p, y = rng.random(n), rng.integers(0, 2, size=n)
    gq = np.rint((p - y) * (1 << S)).astype(np.int32)
    hq = np.rint(p * (1 - p) * (1 << S)).astype(np.int32)
    hist = cpu_ref.hgbt_hist_cpu(bins, off, node, gq, hq, k)
    bounds = np.asarray(
        [[-INF, INF], [-INF, 0.1], [-0.2, INF], [-0.05, 0.05], [0.3, 0.3], [-1.0, -0.5]]
    )
    n_split = 0
    for mono in ([1, 1, 1, 1], [-1, -1, -1, -1], [0, 1, -1, 0], [1, 0, 0, -1]):
        mono = np.asarray(mono, dtype=np.int32)
        for lam, min_leaf in ((1.0, 5), (0.0, 1)):
            got = cpu_ref.hgbt_split_mono_cpu(hist, off, lam, min_leaf, mono, bounds)
            np.testing.assert_array_equal(
                got, brute_force(hist, off, lam, min_leaf, mono, bounds)
            )
            n_split += int((got[:, 1] >= 0).sum())
    assert n_split > 10


def _arrays(m):
    return {key: getattr(m, key + "_") for key in _TREE_KEYS}


def test_plain_fits_unchanged():
    rng = np.random.default_rng(2)
    x = rng.normal(size=(500, 3)).astype(np.float32)
    y = (x[:, 0] - x[:, 1] + rng.normal(size=500) > 0).astype(int)
    kw = {"n_estimators": 4, "max_depth": 3, "device": "cpu"}
    ref = HistGBTClassifier(**kw).fit(x, y)
    assert not ref.monotone_cst_.any() and ref.monotone_cst_.dtype == np.int32
    for cst in ([0, 0, 0], {}, {1: 0}):
        m = HistGBTClassifier(monotone_cst=cst, **kw).fit(x, y)
        for key, a in _arrays(ref).items():
            assert _arrays(m)[key].tobytes() == a.tobytes(), (cst, key)


@pytest.fixture(scope="module")
def sine():
    """y follows sin(3 x0): no monotone model fits it, so the constraint binds."""
    rng = np.random.default_rng(5)
    x = rng.uniform(-2.0, 2.0, size=(2000, 3)).astype(np.float32)
    y = (np.sin(3.0 * x[:, 0]) + 0.3 * x[:, 1] + 0.5 * rng.normal(size=2000) > 0).astype(int)
    kw = {"n_estimators": 20, "max_depth": 4, "device": "cpu"}
    plain = HistGBTClassifier(**kw).fit(x, y)
    grid = np.linspace(-2.0, 2.0, 200, dtype=np.float32)
    sweep = np.repeat(x[:50], 200, axis=0)
    sweep[:, 0] = np.tile(grid, 50)
    return x, y, kw, plain, sweep


@pytest.mark.parametrize("sign", [1, -1])
def test_fit_is_exactly_monotone(sine, sign):
    x, y, kw, plain, sweep = sine
    cst = [sign, 0, 0]
    m = HistGBTClassifier(monotone_cst=cst, **kw).fit(x, y)
    assert list(m.monotone_cst_) == cst
    assert (m.children_left_ >= 0).sum() > 20  # it still found splits
    step = np.diff(m.decision_function(sweep).reshape(50, 200), axis=1) * sign
    assert (step >= 0.0).all() and (step > 0.0).any()  # exact: no tolerance
    assert verify_monotone(m)
    # the constraint was binding: the plain fit goes the other way somewhere
    step = np.diff(plain.decision_function(sweep).reshape(50, 200), axis=1) * sign
    assert (step < 0.0).any()
    assert not verify_monotone(plain, cst)
    assert verify_monotone(plain)  # its own (empty) constraints hold trivially
    # the dict form with a negative index resolves to the same model
    d = HistGBTClassifier(monotone_cst={-3: sign}, **kw).fit(x, y)
    for key, a in _arrays(m).items():
        assert _arrays(d)[key].tobytes() == a.tobytes(), key


def test_validation_errors():
    x = np.random.default_rng(0).normal(size=(60, 3)).astype(np.float32)
    y = (x[:, 0] > 0).astype(int)
    for bad, match in (
        ([1, 0], "entries"),
        ([2, 0, 0], "-1, 0 or 1"),
        ({3: 1}, "out of range"),
        ({-4: 1}, "out of range"),
    ):
        with pytest.raises(ValueError, match=match):
            HistGBTClassifier(n_estimators=1, device="cpu", monotone_cst=bad).fit(x, y)
    with pytest.raises(ValueError, match="categorical"):
        make_classifier_pipeline({"monotone": {"education": 1}}, "hgbt")
    with pytest.raises(ValueError, match="unknown feature"):
        make_classifier_pipeline({"monotone": {"shoe_size": 1}}, "hgbt")
    with pytest.raises(ValueError, match="hgbt"):
        make_classifier_pipeline({"monotone": {"credit_limit": -1}}, "rf")
    pipe = make_classifier_pipeline({"monotone": {"credit_limit": -1, "age": 1}}, "hgbt")
    n = len(NUMERIC_FEATURES)
    assert pipe.named_steps["classifier"].monotone_cst == {-n: -1, 1 - n: 1}


def test_cli_monotone(monkeypatch):
    from creditcore import __main__ as cli
    from creditcore import train

    seen = {}
    monkeypatch.setattr(train, "train_and_register", lambda **kw: seen.update(kw) or "uri")
    cli._cmd_train(
        ["--algorithm", "hgbt", "--monotone", "credit_limit=-1,payment_amount_1=-1,age=+1"]
    )
    assert seen["monotone"] == {"credit_limit": -1, "payment_amount_1": -1, "age": 1}
    seen.clear()
    cli._cmd_train(["--algorithm", "hgbt"])
    assert seen["monotone"] is None
    for argv in (
        ["--algorithm", "rf", "--monotone", "credit_limit=-1"],
        ["--monotone", "credit_limit=-1"],  # the default algorithm is rf
        ["--algorithm", "hgbt", "--monotone", "credit_limit"],
        ["--algorithm", "hgbt", "--monotone", "credit_limit=2"],
        ["--algorithm", "hgbt", "--monotone", "education=1"],
    ):
        with pytest.raises(SystemExit) as exc:
            cli._cmd_train(argv)
        assert exc.value.code != 0


def test_cli_monotone_with_rf_exits_nonzero():
    import subprocess
    import sys

    r = subprocess.run(
        [sys.executable, "-m", "creditcore", "train", "--algorithm", "rf",
         "--monotone", "credit_limit=-1"],
        capture_output=True, text=True, timeout=240,
    )
    assert r.returncode != 0 and "--monotone" in r.stderr


def test_training_job_records_and_verifies(tmp_path, monkeypatch):
    from creditcore import registry, train
    from creditcore.data import make_uci_shaped_frame
    from creditcore.models import tpe

    monkeypatch.setattr(
        tpe,
        "reference_space",
        lambda: {
            "n_estimators": tpe.IntDim(8, 12),
            "max_depth": tpe.IntDim(3, 5),
            "criterion": tpe.CatDim(("gini", "entropy")),
        },
    )
    mono = {"credit_limit": -1, "payment_amount_1": -1}
    d, runs = str(tmp_path / "model"), str(tmp_path / "runs")
    train.train_and_register(
        model_dir=d, max_evals=2, df=make_uci_shaped_frame(n_rows=2000, seed=3),
        register=False, algorithm="hgbt", train_device="cpu", monotone=mono,
        runs_dir=runs,
    )
    import yaml

    with open(os.path.join(d, "MLmodel")) as f:
        meta = yaml.safe_load(f)["metadata"]
    assert meta["monotone"] == mono and meta["best_params"]["monotone"] == mono
    run_dirs = os.listdir(runs)
    assert len(run_dirs) == 2
    for rd in run_dirs:
        with open(os.path.join(runs, rd, "run.json")) as f:
            assert json.load(f)["params"]["monotone"] == mono
    pipe = registry.load_pyfunc_model(d).python_model.classifier
    clf = pipe.named_steps["classifier"]
    n = len(NUMERIC_FEATURES)
    assert clf.monotone_cst_[-n] == -1 and clf.monotone_cst_[-n + 8] == -1
    assert np.abs(clf.monotone_cst_).sum() == 2
    assert verify_monotone(pipe)
    with pytest.raises(ValueError, match="hgbt"):
        train.train_and_register(model_dir=d, max_evals=1, algorithm="rf", monotone=mono)


QUALITY_CST = {"credit_limit": -1, "age": 1, "payment_amount_1": -1}


def quality_gap(seed: int) -> tuple[float, float]:
    """Held-out log-loss (ours on the CPU path, sklearn) of constrained fits:
    16k UCI-shaped rows (data seed = split seed = ``seed``), 80/20 split,
    100 trees, depth 6, learning rate 0.1, the same three constraints."""
    from sklearn.ensemble import HistGradientBoostingClassifier
    from sklearn.metrics import log_loss
    from sklearn.model_selection import train_test_split

    from creditcore.data import make_uci_shaped_frame

    df = make_uci_shaped_frame(n_rows=16_000, seed=seed)
    tr, te = train_test_split(df, test_size=0.2, random_state=seed)
    pipe = make_classifier_pipeline(
        {"n_estimators": 100, "max_depth": 6, "learning_rate": 0.1, "device": "cpu",
         "monotone": QUALITY_CST},
        "hgbt",
    )
    pipe.fit(tr[FEATURES], tr[TARGET].values.ravel())
    pre = pipe.named_steps["preprocessor"]
    xtr, xte = (_to_dense_f32(pre.transform(d[FEATURES])) for d in (tr, te))
    cst = pipe.named_steps["classifier"].monotone_cst_
    sk = HistGradientBoostingClassifier(
        max_iter=100, max_depth=6, learning_rate=0.1, max_leaf_nodes=None,
        early_stopping=False, random_state=seed, monotonic_cst=cst,
    ).fit(xtr, tr[TARGET].values.ravel())
    ours = log_loss(te[TARGET], pipe.predict_proba(te[FEATURES])[:, 1])
    return float(ours), float(log_loss(te[TARGET], sk.predict_proba(xte)[:, 1]))


def test_quality_vs_sklearn_constrained():
    """Relative gap of the held-out log-loss to sklearn's constrained
    HistGradientBoostingClassifier, ``quality_gap``'s setup.

    Measured on the CPU path for seeds 0..4, (hgbt - sklearn) / sklearn
    (profiles/bench_results/hgbt_mono_quality.txt):
        -0.003743  +0.004763  +0.007838  -0.004293  -0.006092
    Largest absolute gap 0.007838; the bound is twice that, 0.015676, below
    the 2 % cap. Seed 2, the widest of the five, is the one asserted."""
    bound = 2 * 0.007838
    assert bound <= 0.02
    ours, sk = quality_gap(2)
    gap = (ours - sk) / sk
    print(f"seed 2: hgbt[cpu] {ours:.6f} sklearn_hist_gbt {sk:.6f} rel_gap {gap:+.6f}")
    assert abs(gap) <= bound

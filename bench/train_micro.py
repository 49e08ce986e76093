"""Training micro-benchmark: the GPU trainers vs sklearn.

    python bench/train_micro.py --rows 20000
    python bench/train_micro.py --rows 1000000 --skip-exact-gbt
    python bench/train_micro.py --mode forest --rows 20000 --depth 8
    python bench/train_micro.py --rows 20000 --monotone 3 --skip-exact-gbt

Every estimator gets the same preprocessed matrix (the pipeline's
[one-hot | 14 numerics] feature space, dense f32), the same 80/20 split and
the same n_estimators / max_depth / learning_rate. Prints one JSON line per
estimator with the fit wall time (host binning and transfers included for
hgbt) and the held-out log-loss, then one summary line. sklearn's exact
GradientBoostingClassifier is single-threaded; --skip-exact-gbt leaves it out
at row counts where it would run for many minutes. ``--monotone N`` adds a
second hgbt fit with monotone constraints on the first N numeric columns
(alternating +1 / -1) and reports its fit time and log-loss next to the
unconstrained ones.

``--mode forest`` times HistForestClassifier (hrf; host binning, bootstrap
draws and transfers included) against sklearn RandomForestClassifier on
``--sklearn-jobs`` threads at equal n_estimators / max_depth / max_features,
and reports the held-out log-loss and ROC-AUC of both.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _matrix(n_rows: int, seed: int):
    from creditcore.data import make_uci_shaped_frame
    from creditcore.models.forest import make_classifier_pipeline
    from creditcore.schema import FEATURES, TARGET

    df = make_uci_shaped_frame(n_rows=n_rows, seed=seed)
    pre = make_classifier_pipeline({}, "rf").named_steps["preprocessor"]
    x = pre.fit_transform(df[FEATURES])
    if hasattr(x, "toarray"):
        x = x.toarray()
    return np.ascontiguousarray(x, dtype=np.float32), df[TARGET].to_numpy().ravel()


def _log_loss(y, p) -> float:
    p = np.clip(p, 1e-15, 1 - 1e-15)
    return float(-np.mean(y * np.log(p) + (1 - y) * np.log(1 - p)))


def _forest(a, xtr, xte, ytr, yte, shape) -> None:
    from sklearn.ensemble import RandomForestClassifier
    from sklearn.metrics import roc_auc_score

    from creditcore.models.hrf import HistForestClassifier

    common = {"n_estimators": a.trees, "max_depth": a.depth,
              "max_features": a.max_features, "random_state": a.seed}
    ours = f"hrf[{a.device}]"
    makers = {
        ours: (lambda: HistForestClassifier(**common, device=a.device), a.repeats),
        "sklearn_rf": (lambda: RandomForestClassifier(**common, n_jobs=a.sklearn_jobs), 1),
    }
    results = {}
    for name, (make, repeats) in makers.items():
        fits = []
        for _ in range(repeats):
            est = make()
            t = time.perf_counter()
            est.fit(xtr, ytr)
            fits.append(time.perf_counter() - t)
        p = est.predict_proba(xte)[:, 1]
        results[name] = {"estimator": name, "fit_s": round(min(fits), 4),
                         "fit_s_all": [round(f, 4) for f in fits],
                         "log_loss": round(_log_loss(yte, p), 6),
                         "roc_auc": round(float(roc_auc_score(yte, p)), 6)}
        print(json.dumps(results[name]), flush=True)
    print(json.dumps({
        "event": "summary", **shape, "max_features": a.max_features,
        "sklearn_jobs": a.sklearn_jobs,
        **{f"{k}_{m}": v[m] for k, v in results.items()
           for m in ("fit_s", "log_loss", "roc_auc")},
        "speedup_vs_sklearn_rf": round(
            results["sklearn_rf"]["fit_s"] / results[ours]["fit_s"], 2),
    }), flush=True)


def main(argv=None) -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="gbt", choices=["gbt", "forest"],
                    help="gbt = hgbt vs sklearn boosting; forest = hrf vs sklearn RF")
    ap.add_argument("--max-features", default="sqrt",
                    help="forest mode: 'sqrt', an integer or 'none'")
    ap.add_argument("--sklearn-jobs", type=int, default=16,
                    help="forest mode: threads of sklearn's RandomForestClassifier")
    ap.add_argument("--rows", type=int, default=20_000)
    ap.add_argument("--trees", type=int, default=100)
    ap.add_argument("--depth", type=int, default=6)
    ap.add_argument("--learning-rate", type=float, default=0.1)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--device", default="cuda", choices=["cuda", "cpu"])
    ap.add_argument("--repeats", type=int, default=2,
                    help="hgbt fits; the first also pays one-time GPU start-up")
    ap.add_argument("--skip-exact-gbt", action="store_true")
    ap.add_argument("--monotone", type=int, default=0, metavar="N",
                    help="gbt mode: also fit hgbt with the first N numeric "
                         "columns constrained, signs alternating from +1")
    a = ap.parse_args(argv)

    from sklearn.model_selection import train_test_split

    from creditcore.models.hgbt import HistGBTClassifier

    t0 = time.perf_counter()
    x, y = _matrix(a.rows, a.seed)
    xtr, xte, ytr, yte = train_test_split(x, y, test_size=0.2, random_state=a.seed)
    shape = {"rows": a.rows, "train_rows": len(xtr), "features": x.shape[1],
             "trees": a.trees, "depth": a.depth, "learning_rate": a.learning_rate}
    print(json.dumps({"event": "data", **shape,
                      "prep_s": round(time.perf_counter() - t0, 3)}), flush=True)

    if a.mode == "forest":
        mf = a.max_features.lower()
        a.max_features = None if mf == "none" else mf if mf == "sqrt" else int(mf)
        shape.pop("learning_rate")
        return _forest(a, xtr, xte, ytr, yte, shape)

    common = {"n_estimators": a.trees, "max_depth": a.depth,
              "learning_rate": a.learning_rate}
    results = {}

    def run(name, make, repeats=1):
        fits = []
        for _ in range(repeats):
            est = make()
            t = time.perf_counter()
            est.fit(xtr, ytr)
            fits.append(time.perf_counter() - t)
        rec = {"estimator": name, "fit_s": round(min(fits), 4),
               "fit_s_all": [round(f, 4) for f in fits],
               "log_loss": round(_log_loss(yte, est.predict_proba(xte)[:, 1]), 6)}
        results[name] = rec
        print(json.dumps(rec), flush=True)

    run(f"hgbt[{a.device}]",
        lambda: HistGBTClassifier(**common, device=a.device), repeats=a.repeats)
    if a.monotone:
        from creditcore.schema import NUMERIC_FEATURES

        n_num = len(NUMERIC_FEATURES)  # the numeric block is last
        if not 1 <= a.monotone <= n_num:
            ap.error(f"--monotone takes 1..{n_num}")
        cst = {j - n_num: 1 - 2 * (j % 2) for j in range(a.monotone)}
        run(f"hgbt_mono{a.monotone}[{a.device}]",
            lambda: HistGBTClassifier(**common, device=a.device, monotone_cst=cst),
            repeats=a.repeats)
    try:
        from sklearn.ensemble import HistGradientBoostingClassifier
    except ImportError:
        print(json.dumps({"estimator": "sklearn_hist_gbt", "skipped": "not importable"}))
    else:
        run("sklearn_hist_gbt", lambda: HistGradientBoostingClassifier(
            max_iter=a.trees, max_depth=a.depth, learning_rate=a.learning_rate,
            max_leaf_nodes=None, early_stopping=False, random_state=a.seed))
    if a.skip_exact_gbt:
        print(json.dumps({"estimator": "sklearn_gbt", "skipped": "--skip-exact-gbt"}))
    else:
        from sklearn.ensemble import GradientBoostingClassifier

        run("sklearn_gbt", lambda: GradientBoostingClassifier(**common, random_state=a.seed))

    ours = results[f"hgbt[{a.device}]"]["fit_s"]
    print(json.dumps({
        "event": "summary", **shape,
        **{f"{k}_fit_s": v["fit_s"] for k, v in results.items()},
        **{f"{k}_log_loss": v["log_loss"] for k, v in results.items()
           if k.startswith("hgbt")},
        **({"mono_over_plain_fit": round(
            results[f"hgbt_mono{a.monotone}[{a.device}]"]["fit_s"] / ours, 3)}
           if a.monotone else {}),
        **{f"speedup_vs_{k}": round(v["fit_s"] / ours, 2)
           for k, v in results.items() if not k.startswith("hgbt")},
    }), flush=True)


if __name__ == "__main__":
    main()

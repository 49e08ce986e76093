"""Classifier pipeline — training-side model definition.

Reproduces the reference's sklearn pipeline exactly
(reference databricks/src/01-train-model.ipynb cell-6):

- categorical: SimpleImputer(constant, "missing") -> OneHotEncoder(ignore)
- numeric:     SimpleImputer(median)
- estimator:   RandomForestClassifier(n_estimators, max_depth, criterion,
               n_jobs=-1)

Training happens on CPU with sklearn (like the reference), except for the
"hgbt" and "hrf" families, which train on the GPU (models/hgbt.py,
models/hrf.py); *scoring* happens
on MI355X via the packed flat-buffer representation (creditcore.pack) and the
HIP forest-traversal kernel (csrc/creditcore_kernels.hip (forest_kernel_ilpN)). This module is the
golden CPU path the GPU path is tested against.
"""

from __future__ import annotations

from sklearn.compose import ColumnTransformer
from sklearn.ensemble import RandomForestClassifier
from sklearn.impute import SimpleImputer
from sklearn.pipeline import Pipeline
from sklearn.preprocessing import OneHotEncoder

from ..schema import CATEGORICAL_FEATURES, MISSING_CATEGORY, NUMERIC_FEATURES


def monotone_columns(monotone: dict) -> dict:
    """{numeric feature name: sign} -> {encoded column index: sign} for
    ``HistGBTClassifier(monotone_cst=...)``. The numeric block is last in the
    ColumnTransformer, so name j of NUMERIC_FEATURES is column
    j - len(NUMERIC_FEATURES) whatever the one-hot width turns out to be.
    One-hot columns carry no order: a categorical name is an error."""
    out = {}
    for name, sign in dict(monotone).items():
        if name in CATEGORICAL_FEATURES:
            raise ValueError(
                f"monotone constraint on categorical feature {name!r}: "
                "one-hot columns are not ordered"
            )
        if name not in NUMERIC_FEATURES:
            raise ValueError(f"monotone constraint on unknown feature {name!r}")
        if sign not in (-1, 0, 1):
            raise ValueError(f"monotone constraint for {name!r} must be -1, 0 or 1")
        out[NUMERIC_FEATURES.index(name) - len(NUMERIC_FEATURES)] = int(sign)
    return out


def make_classifier_pipeline(params: dict, algorithm: str = "rf") -> Pipeline:
    """Build the classifier pipeline (reference 01-train cell-6).

    ``params["monotone"]`` ({numeric feature name: -1 | 0 | +1}, "hgbt" only)
    sets monotone constraints; see ``monotone_columns``.

    ``params`` are estimator kwargs (n_estimators / max_depth / random_state
    ...). ``algorithm``: "rf" (the reference's RandomForest), "gbt"
    (GradientBoostingClassifier — the north star's "gradient-boosted-tree
    traversal" family; same packed node-SoA format, scored by the same HIP
    kernel with a sigmoid(sum + prior) finalize), "hgbt"
    (models.hgbt.HistGBTClassifier — histogram gradient boosting trained by
    HIP kernels on the GPU, packed and scored like "gbt"; ``params`` may
    carry ``device`` for the training device), "hrf"
    (models.hrf.HistForestClassifier — the random forest trained by HIP
    kernels, many trees per launch, packed and scored like "rf"; takes
    ``device`` too), or "et"
    (ExtraTreesClassifier — identical tree structure and leaf-fraction-mean
    semantics to RF, so it rides the RF pack/score path unchanged).
    """
    if params.get("monotone") and algorithm != "hgbt":
        raise ValueError("monotone constraints need algorithm 'hgbt'")
    if algorithm != "hgbt" and "monotone" in params:
        params = {k: v for k, v in params.items() if k != "monotone"}
    if algorithm == "gbt":
        from sklearn.ensemble import GradientBoostingClassifier

        params = dict(params)
        params.pop("criterion", None)  # rf-only knob from the search space
        params.setdefault("n_estimators", 200)
        estimator = GradientBoostingClassifier(**params)
    elif algorithm == "hgbt":
        from .hgbt import MAX_DEPTH, HistGBTClassifier

        params = dict(params)
        params.pop("criterion", None)  # rf-only knob from the search space
        params.setdefault("n_estimators", 200)
        if "max_depth" in params:  # the search space draws up to 24
            params["max_depth"] = min(int(params["max_depth"]), MAX_DEPTH)
        monotone = params.pop("monotone", None)
        if monotone:
            params["monotone_cst"] = monotone_columns(monotone)
        estimator = HistGBTClassifier(**params)
    elif algorithm == "hrf":
        from .hrf import MAX_DEPTH, HistForestClassifier

        params = dict(params)
        params.pop("criterion", None)  # Gini only (models/hrf.py)
        if "max_depth" in params:  # the search space draws up to 24
            params["max_depth"] = min(int(params["max_depth"]), MAX_DEPTH)
        estimator = HistForestClassifier(**params)
    elif algorithm == "et":
        from sklearn.ensemble import ExtraTreesClassifier

        estimator = ExtraTreesClassifier(**params, n_jobs=-1)
    elif algorithm == "rf":
        estimator = RandomForestClassifier(**params, n_jobs=-1)
    else:
        raise ValueError(f"unknown algorithm: {algorithm}")

    categorical_transformer = Pipeline(
        steps=[
            (
                "imputer",
                SimpleImputer(strategy="constant", fill_value=MISSING_CATEGORY),
            ),
            ("ohe", OneHotEncoder(handle_unknown="ignore")),
        ]
    )
    numeric_transformer = Pipeline(steps=[("imputer", SimpleImputer(strategy="median"))])
    preprocessor = ColumnTransformer(
        transformers=[
            ("categorical", categorical_transformer, CATEGORICAL_FEATURES),
            ("numeric", numeric_transformer, NUMERIC_FEATURES),
        ]
    )
    return Pipeline(
        [
            ("preprocessor", preprocessor),
            ("classifier", estimator),
        ]
    )

"""Request/response schema — the wire contract of the credit-default API.

Mirrors the reference contract exactly (reference: app/model.py:8-71 and the
response assembled at databricks/src/02-register-model.ipynb cell-9):

- 23 input features: 9 categorical strings + 14 numeric floats;
- response = per-row default probability, per-row outlier flag, and a
  per-feature batch-level drift score (1 - p_val).

The reference's ``age`` default of 18000.0 (a copy-paste of ``credit_limit``,
reference app/model.py:22) is reproduced because it is part of the observable
wire contract (sample-request.json uses it).
"""

from __future__ import annotations

from pydantic import BaseModel, ConfigDict

# Feature sets (reference: 01-train-model.ipynb cell-4, 02-register cell-4).
CATEGORICAL_FEATURES: list[str] = [
    "sex",
    "education",
    "marriage",
    "repayment_status_1",
    "repayment_status_2",
    "repayment_status_3",
    "repayment_status_4",
    "repayment_status_5",
    "repayment_status_6",
]

NUMERIC_FEATURES: list[str] = [
    "credit_limit",
    "age",
    "bill_amount_1",
    "bill_amount_2",
    "bill_amount_3",
    "bill_amount_4",
    "bill_amount_5",
    "bill_amount_6",
    "payment_amount_1",
    "payment_amount_2",
    "payment_amount_3",
    "payment_amount_4",
    "payment_amount_5",
    "payment_amount_6",
]

FEATURES: list[str] = CATEGORICAL_FEATURES + NUMERIC_FEATURES

TARGET = "default_payment_next_month"

# The imputation category used for missing categorical values
# (reference: SimpleImputer(strategy="constant", fill_value="missing"),
# 01-train-model.ipynb cell-6).
MISSING_CATEGORY = "missing"


class LoanApplicant(BaseModel):
    """One scoring record (reference app/model.py:8-34, defaults included)."""

    sex: str = "male"
    education: str = "university"
    marriage: str = "married"
    repayment_status_1: str = "duly_paid"
    repayment_status_2: str = "duly_paid"
    repayment_status_3: str = "duly_paid"
    repayment_status_4: str = "duly_paid"
    repayment_status_5: str = "no_delay"
    repayment_status_6: str = "no_delay"
    credit_limit: float = 18000.0
    age: float = 18000.0  # reference quirk kept: app/model.py:22
    bill_amount_1: float = 764.95
    bill_amount_2: float = 2221.95
    bill_amount_3: float = 1131.85
    bill_amount_4: float = 5074.85
    bill_amount_5: float = 18000.0
    bill_amount_6: float = 1419.95
    payment_amount_1: float = 2236.5
    payment_amount_2: float = 1137.55
    payment_amount_3: float = 5084.55
    payment_amount_4: float = 111.65
    payment_amount_5: float = 306.9
    payment_amount_6: float = 805.65

    model_config = ConfigDict(extra="ignore")


class FeatureBatchDrift(BaseModel):
    """Per-feature batch drift scores = 1 - p_val (reference app/model.py:37-61)."""

    sex: float
    education: float
    marriage: float
    repayment_status_1: float
    repayment_status_2: float
    repayment_status_3: float
    repayment_status_4: float
    repayment_status_5: float
    repayment_status_6: float
    credit_limit: float
    age: float
    bill_amount_1: float
    bill_amount_2: float
    bill_amount_3: float
    bill_amount_4: float
    bill_amount_5: float
    bill_amount_6: float
    payment_amount_1: float
    payment_amount_2: float
    payment_amount_3: float
    payment_amount_4: float
    payment_amount_5: float
    payment_amount_6: float


class ModelOutput(BaseModel):
    """Response envelope (reference app/model.py:64-70)."""

    predictions: list[float]
    outliers: list[float]
    feature_drift_batch: FeatureBatchDrift


class Reason(BaseModel):
    """One reason code: a feature and its attribution for one row."""

    feature: str
    contribution: float


class ExplainOutput(BaseModel):
    """POST /explain response: per-row attributions, prediction-path (Saabas)
    by default or exact TreeSHAP values with ``?method=shap``.
    base_value + sum(contributions[r]) is the model output for row r in
    ``output_space`` ("probability", or "log_odds" for gradient boosting).
    ``method`` echoes the query parameter and is absent when none was given.
    ``?method=interventional`` gives Shapley values of the interventional
    game against the model's background sample; ``base_value`` is then the
    mean model output over those rows and ``background_rows`` their number
    (absent for the other methods).
    ``?method=shap&interactions=true`` adds ``interactions``: per row the
    symmetric 23 x 23 matrix of exact SHAP interaction values in ``features``
    order on both axes, whose row r sums to ``contributions[r]`` (absent
    otherwise)."""

    output_space: str
    base_value: float
    features: list[str]
    predictions: list[float]
    contributions: list[list[float]]
    top_reasons: list[list[Reason]]
    method: str | None = None
    background_rows: int | None = None
    interactions: list[list[list[float]]] | None = None


class PdpRequest(BaseModel):
    """POST /explain/pdp request. ``features`` entries are a feature name
    (one-way) or a pair of distinct names (two-way); ``grid`` optionally
    replaces the grid of a feature (numbers for a numeric feature, known
    categories for a categorical one)."""

    features: list[str | list[str]]
    grid_resolution: int = 20
    percentiles: list[float] = [0.05, 0.95]
    kind: str = "average"
    response: str = "probability"
    grid: dict[str, list[float | str]] | None = None

    model_config = ConfigDict(extra="ignore")


class PdpCurve(BaseModel):
    """Partial dependence of the classifier on one feature or a pair.
    ``grid_values`` holds one list per axis (numbers, or category strings);
    ``average`` is indexed [g] or [g0][g1]; ``individual`` (the ICE curves,
    ``kind="both"`` only) is indexed [row][g] or [row][g0][g1]."""

    features: list[str]
    grid_values: list[list[float | str]]
    average: list[float] | list[list[float]]
    individual: list[list[float]] | list[list[list[float]]] | None = None


class PdpOutput(BaseModel):
    """POST /explain/pdp response: one curve per requested entry, computed on
    the model's ``sample_rows`` background rows, in ``output_space``
    ("probability", or "log_odds" with ``response="raw"``)."""

    output_space: str
    sample_rows: int
    kind: str
    results: list[PdpCurve]


class AleRequest(BaseModel):
    """POST /explain/ale request. ``features`` are numeric feature names;
    ``grid`` optionally replaces the quantile edges of a feature with at
    least 2 strictly ascending numbers."""

    features: list[str]
    grid_resolution: int = 20
    kind: str = "average"
    response: str = "probability"
    grid: dict[str, list[float]] | None = None

    model_config = ConfigDict(extra="ignore")


class AleCurve(BaseModel):
    """Accumulated local effects of the classifier on one numeric feature:
    ``ale[k]`` is the centred effect at ``edges[k]`` and ``counts[k]`` the
    sample rows in interval (edges[k], edges[k+1]] (a constant column has one
    edge, ``ale = [0.0]`` and all rows in ``counts[0]``). With
    ``kind="both"``, ``interval`` (1-based) and ``local_effect`` per row."""

    feature: str
    edges: list[float]
    ale: list[float]
    counts: list[int]
    interval: list[int] | None = None
    local_effect: list[float] | None = None


class AleOutput(BaseModel):
    """POST /explain/ale response: one curve per requested feature, computed
    on the model's ``sample_rows`` background rows, in ``output_space``
    ("probability", or "log_odds" with ``response="raw"``)."""

    output_space: str
    sample_rows: int
    kind: str
    results: list[AleCurve]


class ImportanceRequest(BaseModel):
    """POST /explain/importance request: the records as /score takes them,
    one 0/1 label per record, the features to permute (default: all), the
    shuffles per feature, the score (accuracy, neg_log_loss, neg_brier_score
    or roc_auc), the seed of the shuffles and the decision threshold of
    "accuracy"."""

    records: list[dict]
    labels: list[float]
    features: list[str] | None = None
    n_repeats: int = 5
    scoring: str = "roc_auc"
    seed: int = 0
    threshold: float = 0.5

    model_config = ConfigDict(extra="ignore")


class FeatureImportance(BaseModel):
    """``importances[k]`` is the baseline score minus the score with the
    feature's column shuffled by permutation k; ``importances_std`` has
    ddof 0."""

    feature: str
    importances: list[float]
    importances_mean: float
    importances_std: float


class ImportanceOutput(BaseModel):
    """POST /explain/importance response: one entry per requested feature,
    in request order."""

    baseline_score: float
    scoring: str
    n_repeats: int
    sample_rows: int
    results: list[FeatureImportance]


class CounterfactualRequest(BaseModel):
    """POST /explain/counterfactual request: the records as /explain takes
    them, the features to move (default: all), the decision threshold on the
    predicted probability and whether to return the whole exact curves."""

    records: list[dict]
    features: list[str] | None = None
    threshold: float = 0.5
    curves: bool = False

    model_config = ConfigDict(extra="ignore")


class CounterfactualSide(BaseModel):
    """The closest value on one side of a numeric feature whose decision
    differs from the row's own."""

    value: float
    delta: float
    probability: float


class NumericCounterfactual(BaseModel):
    """``value`` is the row's own (imputed) value; ``thresholds`` (K) and
    ``probabilities`` (K + 1, one per interval) only with ``curves``."""

    value: float
    below: CounterfactualSide | None = None
    above: CounterfactualSide | None = None
    thresholds: list[float] | None = None
    probabilities: list[float] | None = None


class CategoryFlip(BaseModel):
    category: str
    probability: float


class CategoricalCounterfactual(BaseModel):
    """``value`` is the row's own category (null if unknown); ``flips`` the
    other known categories whose decision differs, in vocabulary order."""

    value: str | None = None
    flips: list[CategoryFlip]


class CounterfactualRow(BaseModel):
    probability: float
    decision: int
    counterfactuals: dict[str, NumericCounterfactual | CategoricalCounterfactual]


class CounterfactualOutput(BaseModel):
    """POST /explain/counterfactual response: one entry per record."""

    threshold: float
    features: list[str]
    rows: list[CounterfactualRow]


class AnchorsRequest(BaseModel):
    """POST /explain/anchors request: the records as /explain takes them, the
    share of sample rows that must keep the record's decision under the
    anchor, the beam width and size limit of the search, the percentiles
    that cut numeric features into intervals and the decision threshold on
    the predicted probability."""

    records: list[dict]
    precision_threshold: float = 0.95
    beam_size: int = 2
    max_anchor_size: int = 6
    disc_perc: list[float] = [25.0, 50.0, 75.0]
    threshold: float = 0.5

    model_config = ConfigDict(extra="ignore")


class AnchorPredicate(BaseModel):
    """One predicate of an anchor: ``feature == category``, or ``low <
    feature <= high`` with null for an open end."""

    feature: str
    category: str | None = None
    low: float | None = None
    high: float | None = None


class AnchorRow(BaseModel):
    """``precision``: the share of sample rows that keep the record's
    ``decision`` once the anchor's features are set to the record's;
    ``coverage``: the share of sample rows the anchor applies to; ``met``:
    whether ``precision`` reached the requested threshold."""

    anchor: list[AnchorPredicate]
    names: list[str]
    precision: float
    coverage: float
    met: bool
    decision: int
    probability: float


class AnchorsOutput(BaseModel):
    """POST /explain/anchors response: one entry per record, exact on the
    model's ``sample_rows`` background rows."""

    rows: list[AnchorRow]
    precision_threshold: float
    beam_size: int
    sample_rows: int


class MmdDriftRequest(BaseModel):
    """POST /drift/mmd request: the records as /score takes them, the number
    of permutations behind the p-value and the seed they are drawn from."""

    records: list[dict]
    n_permutations: int = 100
    seed: int = 0

    model_config = ConfigDict(extra="ignore")


class MmdDriftOutput(BaseModel):
    """POST /drift/mmd response: the unbiased MMD^2 of the batch against the
    packed reference sample and its permutation p-value (``threshold`` is the
    model's drift p-value, ``distance_threshold`` the permuted statistic at
    that rank)."""

    mmd2: float
    p_val: float
    is_drift: int
    threshold: float
    distance_threshold: float
    gamma: float
    n: int
    n_ref: int
    n_permutations: int


class KnnOutlierRequest(BaseModel):
    """POST /outlier/knn request: the records as /score takes them, the
    number of neighbours, the score (``kth`` or ``mean``), the false-positive
    rate behind the threshold, and whether to return the neighbours."""

    records: list[dict]
    k: int = 10
    score: str = "kth"
    fpr: float = 0.05
    neighbors: bool = False

    model_config = ConfigDict(extra="ignore")


class KnnOutlierOutput(BaseModel):
    """POST /outlier/knn response: per record the distance to its k-th
    nearest row of the packed reference sample (or the mean of the k
    distances) and its comparison with ``threshold``, the ``1 - fpr``
    quantile of the sample's own leave-one-out scores. ``neighbor_index``
    holds row numbers of the reference sample, nearest first."""

    instance_score: list[float]
    is_outlier: list[int]
    threshold: float
    k: int
    score: str
    fpr: float
    n: int
    n_ref: int
    neighbor_index: list[list[int]] | None = None
    neighbor_distance: list[list[float]] | None = None


class ProximityInput(BaseModel):
    """POST /explain/proximity request: the records as /score takes them, the
    number of neighbours, the score (``kth`` or ``mean``), the false-positive
    rate behind the threshold, and whether to return the neighbours."""

    records: list[dict]
    k: int = 10
    score: str = "kth"
    fpr: float = 0.05
    neighbors: bool = True

    model_config = ConfigDict(extra="ignore")


class ProximityOutput(BaseModel):
    """POST /explain/proximity response: per record 1 - the forest proximity
    of its k-th closest row of the packed reference sample (or 1 - the mean of
    the k proximities) and its comparison with ``threshold``, the ``1 - fpr``
    quantile of the sample's own leave-one-out scores. ``neighbor_index``
    holds row numbers of the reference sample, closest first;
    ``neighbor_proximity`` the share of the ``n_trees`` trees in which record
    and neighbour end in the same leaf."""

    instance_score: list[float]
    is_outlier: list[int]
    threshold: float
    k: int
    score: str
    fpr: float
    n: int
    n_ref: int
    n_trees: int
    neighbor_index: list[list[int]] | None = None
    neighbor_proximity: list[list[float]] | None = None


# The one-record CI smoke-test fixture (reference app/sample-request.json).
SAMPLE_REQUEST: list[dict] = [
    {
        "sex": "male",
        "education": "university",
        "marriage": "married",
        "repayment_status_1": "duly_paid",
        "repayment_status_2": "duly_paid",
        "repayment_status_3": "duly_paid",
        "repayment_status_4": "duly_paid",
        "repayment_status_5": "no_delay",
        "repayment_status_6": "no_delay",
        "credit_limit": 18000,
        "age": 18000,
        "bill_amount_1": 764.95,
        "bill_amount_2": 2221.95,
        "bill_amount_3": 1131.85,
        "bill_amount_4": 5074.85,
        "bill_amount_5": 18000,
        "bill_amount_6": 1419.95,
        "payment_amount_1": 2236.5,
        "payment_amount_2": 1137.55,
        "payment_amount_3": 5084.55,
        "payment_amount_4": 111.65,
        "payment_amount_5": 306.9,
        "payment_amount_6": 805.65,
    }
]

# The sane single-record example used at registration time
# (reference 02-register-model.ipynb cell-4, INPUT_SAMPLE — age=33.0 there).
INPUT_SAMPLE: list[dict] = [dict(SAMPLE_REQUEST[0], age=33.0, bill_amount_5=3448.0)]

"""Helpers shared by test_pdp.py and test_pdp_gpu.py (no test in here): tiny
trained pipelines, the 64-row sample with its adversarial cells, job tables
and the hand-built what-if cases of the kernel test."""

from __future__ import annotations

import numpy as np

from _shap_models import (
    CATERPILLAR_SPLITS,
    N_ONEHOT,
    caterpillar_model,
    caterpillar_rows,  # noqa: F401  (re-exported to the tests)
    f32bits,
    hand_model,
)
from creditcore.pack import (
    N_CAT,
    N_NUM,
    PackedModel,
    pack_classifier_pipeline,
    pack_drift,
    pack_isolation_forest,
)

# tiny models: <= 20 trees, depth <= 6
FAMILY_PARAMS = {
    "rf": {"n_estimators": 20, "max_depth": 6, "random_state": 0},
    "et": {"n_estimators": 12, "max_depth": 6, "random_state": 0},
    "gbt": {"n_estimators": 20, "max_depth": 3, "random_state": 0},
    "hgbt": {"n_estimators": 20, "max_depth": 4, "random_state": 0, "device": "cpu"},
}

# the three feature kinds of the oracle test: numeric, categorical, pair
NUMERIC = "credit_limit"
CATEGORICAL = "repayment_status_1"
PAIR = ("age", "sex")
ENTRIES = [NUMERIC, CATEGORICAL, PAIR]


def fit_pipe(train_df, algorithm: str, params: dict | None = None):
    from creditcore.models.forest import make_classifier_pipeline
    from creditcore.schema import FEATURES, TARGET

    pipe = make_classifier_pipeline(dict(params or FAMILY_PARAMS[algorithm]), algorithm=algorithm)
    pipe.fit(train_df[FEATURES], train_df[TARGET].values.ravel())
    return pipe


def pack_pipe(pipe, detectors) -> PackedModel:
    drift, outlier = detectors
    c = pack_classifier_pipeline(pipe)
    return PackedModel(**c, **pack_isolation_forest(outlier), **pack_drift(drift, c["vocabs"]))


def sample_frame(train_df, n: int = 64):
    """n rows of train_df with a NaN numeric and an unknown category, both in
    columns that no entry of ENTRIES targets."""
    from creditcore.schema import FEATURES

    df = train_df[FEATURES].sample(n, random_state=11).reset_index(drop=True).copy()
    df.loc[0, "bill_amount_3"] = np.nan
    df.loc[5, "payment_amount_2"] = np.nan
    df.loc[1, "education"] = "phd_never_seen"
    return df


def job(p0: int, b0: int, p1: int = -1, b1: int = 0) -> list[int]:
    return [p0, b0, p1, b1]


def num_job(col: int, value, col1: int | None = None, value1=None) -> list[int]:
    """Job overriding numeric column ``col`` (and optionally ``col1``)."""
    if col1 is None:
        return job(N_CAT + col, f32bits(value))
    return job(N_CAT + col, f32bits(value), N_CAT + col1, f32bits(value1))


def random_jobs(p: PackedModel, n: int, seed: int) -> np.ndarray:
    """n jobs over every player, one- and two-way, categorical codes from -1
    (unknown) to the vocabulary's end, numeric values around the medians."""
    rng = np.random.default_rng(seed)
    n_src = N_CAT + N_NUM
    scale = np.maximum(np.abs(p.medians), 1.0)

    def bits(player):
        if player < N_CAT:
            return int(rng.integers(-1, len(p.vocabs[player])))
        j = player - N_CAT
        return f32bits(p.medians[j] + scale[j] * rng.normal(0.0, 2.0))

    out = []
    for i in range(n):
        p0 = int(i % n_src)  # every player appears once n >= 23
        if rng.uniform() < 0.4:
            p1 = int((p0 + 1 + rng.integers(0, n_src - 1)) % n_src)
            out.append(job(p0, bits(p0), p1, bits(p1)))
        else:
            out.append(job(p0, bits(p0)))
    return np.asarray(out, dtype=np.int32)


def up(x) -> np.float32:
    return np.nextafter(np.float32(x), np.float32(np.inf))


def caterpillar_forest(cls_kind: int = 0, cls_bias: float = 0.0) -> PackedModel:
    """The 26-split caterpillar next to a single-leaf tree and a tree that
    splits on categorical column 0 alone (both of its one-hot features)."""
    cat = caterpillar_model().cls_nodes
    stump = np.array([[-1, f32bits(0.3125), 0, 0]], dtype=np.int32)
    two = np.array(
        [
            [0, f32bits(0.5), 1, 2],  # col 0 == "a"? right : left
            [1, f32bits(0.5), 3, 4],  # col 0 == "b"? right : left
            [-1, f32bits(0.75), 0, 0],
            [-1, f32bits(-0.25), 0, 0],  # neither: unknown
            [-1, f32bits(0.125), 0, 0],
        ],
        dtype=np.int32,
    )
    trees = [cat, stump, two]
    return hand_model(trees, [np.ones(len(t)) for t in trees], cls_kind=cls_kind, cls_bias=cls_bias)


def caterpillar_jobs() -> np.ndarray:
    """The edge jobs of the hand-built kernel test. Numeric columns 3 and 9
    carry two thresholds each on the caterpillar's path."""
    thr = {}
    for feat, t in CATERPILLAR_SPLITS:
        if feat >= N_ONEHOT:
            thr.setdefault(feat - N_ONEHOT, []).append(t)
    assert len(thr[3]) == 2 and len(thr[9]) == 2
    jobs = [job(0, 0), job(0, 1), job(0, -1)]  # categorical column 0: a, b, unknown
    for col in (3, 9):
        for t in thr[col]:
            jobs.append(num_job(col, t))  # equal to the threshold: goes left
            jobs.append(num_job(col, up(t)))  # the next f32 above: goes right
        jobs.append(num_job(col, 1e30))
        jobs.append(num_job(col, -1e30))
    jobs.append(job(0, 1, N_CAT + 3, f32bits(thr[3][0])))  # categorical x numeric
    jobs.append(job(N_CAT + 9, f32bits(up(thr[9][1])), 4, -1))  # numeric x categorical
    jobs.append(num_job(2, 0.5))  # the last row holds NaN in numeric column 2
    jobs.append(num_job(3, thr[3][1], 9, thr[9][0]))
    return np.asarray(jobs, dtype=np.int32)


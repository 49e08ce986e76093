"""GPU attributions — forest_contrib_kernel (csrc/creditcore_kernels.hip)
through ScoringEngine.explain_arrays vs cpu_ref.forest_contrib_cpu on the
same packed buffers. Run on a real MI355X (`pytest -m gpu`).

The 1e-9 bound is the project's GPU-vs-CPU forest bound: both sides
accumulate the same f32 values in f64; the GPU sums tree-chunks with atomics,
so only the summation order differs."""

from __future__ import annotations

import numpy as np
import pytest

from creditcore.engine import ScoringEngine
from creditcore.models.forest import make_classifier_pipeline
from creditcore.ops import cpu_ref
from creditcore.pack import (
    PackedModel,
    encode_batch,
    pack_classifier_pipeline,
    pack_drift,
    pack_isolation_forest,
)
from creditcore.schema import FEATURES, TARGET
from creditcore.train import fit_detectors

pytestmark = pytest.mark.gpu

N = 128  # forest_contrib_kernel's block size (CONTRIB_BLOCK)
ATOL = 1e-9


@pytest.fixture(scope="module")
def gpu_engine(packed):
    from creditcore.ops import gpu

    assert gpu.available(), (
        "HIP extension must be present on a GPU box (no silent CPU fallback)"
    )
    return ScoringEngine(packed, device="cuda", device_index=0)


@pytest.fixture(scope="module")
def encoded(packed, score_batch):
    return encode_batch(score_batch, packed.vocabs)


def _ref(packed, codes, nums):
    return cpu_ref.forest_contrib_cpu(packed, codes, cpu_ref.impute_nums(packed, nums))


def test_contrib_parity_score_batch(gpu_engine, packed, encoded):
    codes, nums = encoded
    out = gpu_engine.explain_arrays(codes, nums)
    ref = _ref(packed, codes, nums)
    assert out["contributions"].shape == ref.shape == (len(codes), 23)
    assert out["contributions"].dtype == np.float64
    err = np.abs(out["contributions"] - ref).max()
    print(f"contrib parity (score_batch) max |err| = {err:.3e}")
    np.testing.assert_allclose(out["contributions"], ref, rtol=0, atol=ATOL)
    assert out["base_value"] == packed.cls_base_value
    assert out["output_space"] == "probability"


@pytest.mark.parametrize("b", [1, 63, 64, 65, N - 1, N, N + 1, 1000])
def test_contrib_batch_size_sweep(gpu_engine, packed, b):
    """Row guard (b=1), a partly filled last block (N-1, N+1, 1000), exact
    blocks (N), sub-wave and wave edges (63..65); small batches also put many
    tree-chunks' atomics on the same row."""
    rng = np.random.default_rng(b)
    codes = np.stack(
        [rng.integers(-1, len(v), size=b) for v in packed.vocabs], axis=1
    ).astype(np.int16)
    nums = rng.normal(5000.0, 3000.0, size=(b, 14)).astype(np.float32)
    nums[rng.uniform(size=nums.shape) < 0.02] = np.nan
    got = gpu_engine.explain_arrays(codes, nums)["contributions"]
    ref = _ref(packed, codes, nums)
    err = np.abs(got - ref).max()
    print(f"contrib parity b={b} max |err| = {err:.3e}")
    np.testing.assert_allclose(got, ref, rtol=0, atol=ATOL)


def test_additivity_rf_gpu(gpu_engine, packed, encoded):
    codes, nums = encoded
    out = gpu_engine.explain_arrays(codes, nums)
    score = gpu_engine.score_arrays(codes, nums, with_drift=False)["predictions"]
    total = out["base_value"] + out["contributions"].sum(1)
    print(f"RF additivity on GPU max |err| = {np.abs(total - score).max():.3e}")
    np.testing.assert_allclose(total, score, rtol=0, atol=ATOL)
    np.testing.assert_allclose(out["predictions"], score, rtol=0, atol=ATOL)


def test_additivity_gbt_gpu(train_df, score_batch):
    pipe = make_classifier_pipeline(
        {"n_estimators": 60, "max_depth": 3, "random_state": 0}, algorithm="gbt"
    )
    pipe.fit(train_df[FEATURES], train_df[TARGET].values.ravel())
    drift, outlier = fit_detectors(train_df)
    c = pack_classifier_pipeline(pipe)
    gbt = PackedModel(**c, **pack_isolation_forest(outlier), **pack_drift(drift, c["vocabs"]))
    eng = ScoringEngine(gbt, device="cuda", device_index=0)
    codes, nums = encode_batch(score_batch, gbt.vocabs)
    out = eng.explain_arrays(codes, nums)
    assert out["output_space"] == "log_odds"
    np.testing.assert_allclose(
        out["contributions"], _ref(gbt, codes, nums), rtol=0, atol=ATOL
    )
    score = eng.score_arrays(codes, nums, with_drift=False)["predictions"]
    raw = out["base_value"] + out["contributions"].sum(1)
    proba = 1.0 / (1.0 + np.exp(-raw))
    print(f"GBT additivity on GPU max |err| = {np.abs(proba - score).max():.3e}")
    np.testing.assert_allclose(proba, score, rtol=0, atol=ATOL)
    np.testing.assert_allclose(out["predictions"], score, rtol=0, atol=ATOL)


def test_explain_leaves_session_alone(packed, encoded):
    """explain -> score -> explain on a fresh engine: the two explains agree
    (to the atomic-order bound), and the score equals one taken before any
    explain call — the op shares no state with the scoring session."""
    codes, nums = encoded
    eng = ScoringEngine(packed, device="cuda", device_index=0)
    before = eng.score_arrays(codes, nums)
    first = eng.explain_arrays(codes, nums)["contributions"]
    after = eng.score_arrays(codes, nums)
    second = eng.explain_arrays(codes, nums)["contributions"]
    np.testing.assert_allclose(first, second, rtol=0, atol=ATOL)
    np.testing.assert_allclose(
        after["predictions"], before["predictions"], rtol=0, atol=ATOL
    )
    np.testing.assert_array_equal(after["outliers"], before["outliers"])
    np.testing.assert_allclose(after["p_vals"], before["p_vals"], rtol=0, atol=1e-12)

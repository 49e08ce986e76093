"""GPU SHAP interaction values — forest_shap_inter_kernel
(csrc/creditcore_kernels.hip) through
ScoringEngine.explain_arrays(method="shap", interactions=True) vs
cpu_ref.forest_shap_interactions_cpu on the same path table. Run on a real
MI355X (`pytest -m gpu`).

The 1e-9 bound is the project's GPU-vs-CPU forest bound, for the reason given
in test_explain_gpu.py: both sides do the same f64 arithmetic on the same f32
inputs; only the order of the sums differs (and the kernel multiplies by a
stored quotient where the reference divides)."""

from __future__ import annotations

import numpy as np
import pytest

from _shap_models import caterpillar_model, caterpillar_rows, fit_packed
from creditcore.engine import ScoringEngine
from creditcore.ops import cpu_ref
from creditcore.pack import build_shap_paths, encode_batch

pytestmark = pytest.mark.gpu

R = 16  # forest_shap_inter_kernel's rows per block (SHAPI_ROWS)
BLOCK_TARGET = 2048  # forest_shap_interactions' default grid target
ATOL = 1e-9

FAMILIES = {
    "rf": ({"n_estimators": 25, "max_depth": 8, "random_state": 0}, "rf"),
    "gbt": ({"n_estimators": 60, "max_depth": 3, "random_state": 0}, "gbt"),
    "et": ({"n_estimators": 10, "max_depth": 12, "random_state": 0}, "et"),
}


@pytest.fixture(scope="module")
def detectors(train_df):
    from creditcore.train import fit_detectors

    return fit_detectors(train_df)


@pytest.fixture(scope="module")
def models(train_df, detectors):
    """family -> (packed, path table, GPU engine); trained once."""
    from creditcore.ops import gpu

    assert gpu.available(), (
        "HIP extension must be present on a GPU box (no silent CPU fallback)"
    )
    assert gpu.ext().SHAP_INTER_ROWS_PER_BLOCK == R
    out = {}
    for name, (params, algo) in FAMILIES.items():
        p = fit_packed(train_df, detectors, params, algo)
        out[name] = (p, build_shap_paths(p)[0], ScoringEngine(p, device="cuda", device_index=0))
    p = caterpillar_model()
    out["caterpillar"] = (p, build_shap_paths(p)[0], ScoringEngine(p, device="cuda", device_index=0))
    return out


def _ref(p, paths, codes, nums):
    return cpu_ref.forest_shap_interactions_cpu(
        p, codes, cpu_ref.impute_nums(p, nums), paths=paths
    )


def _path_chunks(b: int, n_leaves: int) -> int:
    """gridDim.y of forest_shap_interactions (csrc)."""
    row_blocks = -(-b // R)
    return max(1, min(-(-BLOCK_TARGET // row_blocks), n_leaves))


def _random_rows(p, b: int):
    rng = np.random.default_rng(b)
    codes = np.stack(
        [rng.integers(-1, len(v), size=b) for v in p.vocabs], axis=1
    ).astype(np.int16)
    nums = rng.normal(5000.0, 3000.0, size=(b, 14)).astype(np.float32)
    nums[rng.uniform(size=nums.shape) < 0.02] = np.nan
    return codes, nums


@pytest.mark.parametrize("family", ["rf", "gbt", "et"])
def test_interactions_parity_and_additivity(models, score_batch, monkeypatch, family):
    p, paths, eng = models[family]
    codes, nums = encode_batch(score_batch.iloc[:96], p.vocabs)
    # one launch over all 96 rows (6 row blocks)
    monkeypatch.setattr(ScoringEngine, "INTERACTION_LAUNCH_ROWS", 96)
    out = eng.explain_arrays(codes, nums, method="shap", interactions=True)
    got, ref = out["interactions"], _ref(p, paths, codes, nums)
    assert got.shape == ref.shape == (96, 23, 23) and got.dtype == np.float64
    chunks = _path_chunks(96, paths.n_leaves)
    if family != "gbt":  # the small GBT gets one chunk per leaf
        assert paths.n_leaves > chunks and paths.n_leaves % chunks != 0
    print(f"{family}: leaves={paths.n_leaves} chunks={chunks} "
          f"interaction parity max |err| = {np.abs(got - ref).max():.3e}")
    off = ref.copy()
    off[:, np.arange(23), np.arange(23)] = 0.0
    assert np.abs(off).max() > 1e-4
    np.testing.assert_allclose(got, ref, rtol=0, atol=ATOL)
    np.testing.assert_array_equal(got, got.transpose(0, 2, 1))
    np.testing.assert_allclose(got.sum(2), out["contributions"], rtol=0, atol=ATOL)
    score = eng.score_arrays(codes, nums, with_drift=False)["predictions"]
    raw = out["base_value"] + got.sum((1, 2))
    if family == "gbt":
        raw = 1.0 / (1.0 + np.exp(-raw))
    print(f"{family}: additivity on GPU max |err| = {np.abs(raw - score).max():.3e}")
    np.testing.assert_allclose(raw, score, rtol=0, atol=ATOL)


def test_interactions_caterpillar(models):
    """All 23 players on one path: 253 pairs dealt over the 16 threads of a
    row, the degree-21 integrand, both group slots of a thread (groups 16..22),
    players with two splits."""
    p, paths, eng = models["caterpillar"]
    codes, nums = caterpillar_rows()
    got = eng.explain_arrays(codes, nums, method="shap", interactions=True)["interactions"]
    ref = _ref(p, paths, codes, nums)
    print(f"caterpillar: interaction parity max |err| = {np.abs(got - ref).max():.3e}")
    assert (ref[0] != 0.0).all()  # row 0: every pair interacts
    np.testing.assert_allclose(got, ref, rtol=0, atol=ATOL)


@pytest.mark.parametrize("b", [1, R - 1, R, R + 1, 63, 64, 65, 2 * R + 3])
def test_interactions_batch_size_sweep(models, monkeypatch, b):
    """Row guard (b=1), partly filled last blocks (R-1, R+1, 63, 65, 2R+3),
    exact blocks (R, 64). Threads past the last row stay in the kernel's
    barriers on a clamped row and must not write."""
    p, paths, eng = models["rf"]
    codes, nums = _random_rows(p, b)
    monkeypatch.setattr(ScoringEngine, "INTERACTION_LAUNCH_ROWS", 128)  # one launch
    got = eng.explain_arrays(codes, nums, method="shap", interactions=True)["interactions"]
    ref = _ref(p, paths, codes, nums)
    print(f"interaction parity b={b} max |err| = {np.abs(got - ref).max():.3e}")
    assert got.shape == (b, 23, 23)
    np.testing.assert_allclose(got, ref, rtol=0, atol=ATOL)


def test_interactions_launch_slicing(models, monkeypatch):
    p, paths, eng = models["rf"]
    codes, nums = _random_rows(p, 2 * R + 3)
    monkeypatch.setattr(ScoringEngine, "INTERACTION_LAUNCH_ROWS", 128)
    whole = eng.explain_arrays(codes, nums, method="shap", interactions=True)
    monkeypatch.setattr(ScoringEngine, "INTERACTION_LAUNCH_ROWS", R)  # R + R + 3 rows
    sliced = eng.explain_arrays(codes, nums, method="shap", interactions=True)
    assert (whole["interactions"] != 0.0).any()
    np.testing.assert_allclose(
        sliced["interactions"], whole["interactions"], rtol=0, atol=ATOL
    )
    np.testing.assert_allclose(
        sliced["contributions"], whole["contributions"], rtol=0, atol=ATOL
    )


def test_interactions_leave_session_alone(models, score_batch):
    """explain(interactions) -> score -> explain(interactions) on a fresh
    engine: the two explains agree and the score equals one taken before any
    explain call (the bounds of test_shap_leaves_session_alone)."""
    p = models["rf"][0]
    codes, nums = encode_batch(score_batch.iloc[:40], p.vocabs)
    eng = ScoringEngine(p, device="cuda", device_index=0)
    before = eng.score_arrays(codes, nums)
    first = eng.explain_arrays(codes, nums, method="shap", interactions=True)["interactions"]
    after = eng.score_arrays(codes, nums)
    second = eng.explain_arrays(codes, nums, method="shap", interactions=True)["interactions"]
    np.testing.assert_allclose(first, second, rtol=0, atol=ATOL)
    np.testing.assert_allclose(
        after["predictions"], before["predictions"], rtol=0, atol=ATOL
    )
    np.testing.assert_array_equal(after["outliers"], before["outliers"])
    np.testing.assert_allclose(after["p_vals"], before["p_vals"], rtol=0, atol=1e-12)

"""GPU TreeSHAP — forest_shap_kernel (csrc/creditcore_kernels.hip) through
ScoringEngine.explain_arrays(method="shap") vs cpu_ref.forest_shap_cpu on the
same path table. Run on a real MI355X (`pytest -m gpu`).

The 1e-9 bound is the project's GPU-vs-CPU forest bound, for the reason given
in test_explain_gpu.py: both sides do the same f64 arithmetic on the same f32
inputs; only the order of the atomics and of the products differs (and the
kernel multiplies by a reciprocal where the reference divides)."""

from __future__ import annotations

import numpy as np
import pytest

from _shap_models import caterpillar_model, caterpillar_rows, fit_packed
from creditcore.engine import ScoringEngine
from creditcore.ops import cpu_ref
from creditcore.pack import build_shap_paths, encode_batch

pytestmark = pytest.mark.gpu

N = 128  # forest_shap_kernel's block size (CONTRIB_BLOCK)
BLOCK_TARGET = 2048  # forest_shap's default grid target
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
    out = {}
    for name, (params, algo) in FAMILIES.items():
        p = fit_packed(train_df, detectors, params, algo)
        out[name] = (p, build_shap_paths(p)[0], ScoringEngine(p, device="cuda", device_index=0))
    p = caterpillar_model()
    out["caterpillar"] = (p, build_shap_paths(p)[0], ScoringEngine(p, device="cuda", device_index=0))
    return out


def _ref(p, paths, codes, nums):
    return cpu_ref.forest_shap_cpu(p, codes, cpu_ref.impute_nums(p, nums), paths=paths)


def _path_chunks(b: int, n_leaves: int) -> int:
    """gridDim.y of forest_shap (csrc forest_shap())."""
    row_blocks = -(-b // N)
    return max(1, min(-(-BLOCK_TARGET // row_blocks), n_leaves))


@pytest.mark.parametrize("family", ["rf", "gbt", "et"])
def test_shap_parity_and_additivity(models, score_batch, family):
    p, paths, eng = models[family]
    codes, nums = encode_batch(score_batch.iloc[:96], p.vocabs)
    out = eng.explain_arrays(codes, nums, method="shap")
    got, ref = out["contributions"], _ref(p, paths, codes, nums)
    assert got.shape == ref.shape == (96, 23) and got.dtype == np.float64
    # the leaves do not divide evenly among the path chunks
    chunks = _path_chunks(96, paths.n_leaves)
    if family != "gbt":  # the small GBT gets one chunk per leaf
        assert paths.n_leaves > chunks and paths.n_leaves % chunks != 0
    print(f"{family}: leaves={paths.n_leaves} chunks={chunks} "
          f"shap parity max |err| = {np.abs(got - ref).max():.3e}")
    assert np.abs(ref).max() > 1e-4
    np.testing.assert_allclose(got, ref, rtol=0, atol=ATOL)
    assert out["base_value"] == build_shap_paths(p)[1]
    assert out["output_space"] == ("log_odds" if family == "gbt" else "probability")
    score = eng.score_arrays(codes, nums, with_drift=False)["predictions"]
    print(f"{family}: additivity on GPU max |err| = "
          f"{np.abs(out['predictions'] - score).max():.3e}")
    np.testing.assert_allclose(out["predictions"], score, rtol=0, atol=ATOL)
    raw = out["base_value"] + got.sum(1)
    if family == "gbt":
        raw = 1.0 / (1.0 + np.exp(-raw))
    np.testing.assert_allclose(raw, score, rtol=0, atol=ATOL)


def test_shap_caterpillar(models):
    """All 23 players on one path: the degree-22 integrand, 23 reciprocal
    groups in LDS, players with two splits."""
    p, paths, eng = models["caterpillar"]
    codes, nums = caterpillar_rows()
    got = eng.explain_arrays(codes, nums, method="shap")["contributions"]
    ref = _ref(p, paths, codes, nums)
    print(f"caterpillar: shap parity max |err| = {np.abs(got - ref).max():.3e}")
    assert (np.abs(ref[0]) > 0).all()  # row 0 credits every player
    np.testing.assert_allclose(got, ref, rtol=0, atol=ATOL)


@pytest.mark.parametrize("b", [1, 63, 64, 65, N - 1, N, N + 1, 300])
def test_shap_batch_size_sweep(models, b):
    """Row guard (b=1), a partly filled last block (N-1, N+1, 300), exact
    blocks (N), sub-wave and wave edges (63..65). Threads past the last row
    stay in the kernel's barriers and must not write."""
    p, paths, eng = models["rf"]
    rng = np.random.default_rng(b)
    codes = np.stack(
        [rng.integers(-1, len(v), size=b) for v in p.vocabs], axis=1
    ).astype(np.int16)
    nums = rng.normal(5000.0, 3000.0, size=(b, 14)).astype(np.float32)
    nums[rng.uniform(size=nums.shape) < 0.02] = np.nan
    got = eng.explain_arrays(codes, nums, method="shap")["contributions"]
    ref = _ref(p, paths, codes, nums)
    print(f"shap parity b={b} max |err| = {np.abs(got - ref).max():.3e}")
    np.testing.assert_allclose(got, ref, rtol=0, atol=ATOL)


def test_shap_leaves_session_alone(models, score_batch):
    """explain(shap) -> score -> explain(shap) on a fresh engine: the two
    explains agree (to the atomic-order bound) and the score equals one taken
    before any explain call."""
    p = models["rf"][0]
    codes, nums = encode_batch(score_batch.iloc[:200], p.vocabs)
    eng = ScoringEngine(p, device="cuda", device_index=0)
    before = eng.score_arrays(codes, nums)
    first = eng.explain_arrays(codes, nums, method="shap")["contributions"]
    after = eng.score_arrays(codes, nums)
    second = eng.explain_arrays(codes, nums, method="shap")["contributions"]
    saabas = eng.explain_arrays(codes, nums)["contributions"]
    np.testing.assert_allclose(first, second, rtol=0, atol=ATOL)
    # the bounds test_explain_gpu.py holds the session to (f64 atomics)
    np.testing.assert_allclose(
        after["predictions"], before["predictions"], rtol=0, atol=ATOL
    )
    np.testing.assert_array_equal(after["outliers"], before["outliers"])
    np.testing.assert_allclose(after["p_vals"], before["p_vals"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(
        saabas, cpu_ref.forest_contrib_cpu(p, codes, cpu_ref.impute_nums(p, nums)),
        rtol=0, atol=ATOL,
    )

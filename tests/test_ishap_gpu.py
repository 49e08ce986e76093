"""GPU interventional TreeSHAP — forest_ishap_kernel
(csrc/creditcore_kernels.hip) through
ScoringEngine.explain_arrays(method="interventional") vs
cpu_ref.forest_ishap_cpu on the same path table. Run on a real MI355X
(`pytest -m gpu`).

The 1e-9 bound is the project's GPU-vs-CPU forest bound: both sides do the
same f64 arithmetic (the same weight table, built by the same operations) on
the same f32 inputs; only the order of the sums and of the atomics differs."""

from __future__ import annotations

import numpy as np
import pytest

from _shap_models import N_SRC, caterpillar_model, caterpillar_rows, fit_packed
from creditcore.engine import ScoringEngine
from creditcore.ops import cpu_ref
from creditcore.pack import N_CAT, N_NUM, build_shap_paths, encode_batch
from test_ishap import _breaker_of, _caterpillar_pair_oracle

pytestmark = pytest.mark.gpu

N = 128  # forest_ishap_kernel's block size (CONTRIB_BLOCK)
ATOL = 1e-9
METHOD = "interventional"

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


def _ref(p, paths, codes, nums, bg_codes, bg_nums):
    return cpu_ref.forest_ishap_cpu(
        p,
        codes,
        cpu_ref.impute_nums(p, nums),
        bg_codes,
        cpu_ref.impute_nums(p, bg_nums),
        paths=paths,
    )


def _random_rows(p, n: int, seed: int):
    rng = np.random.default_rng(seed)
    codes = np.stack(
        [rng.integers(-1, len(v), size=n) for v in p.vocabs], axis=1
    ).astype(np.int16)
    nums = rng.normal(5000.0, 3000.0, size=(n, N_NUM)).astype(np.float32)
    nums[rng.uniform(size=nums.shape) < 0.02] = np.nan
    return codes, nums


@pytest.mark.parametrize("family", ["rf", "gbt", "et"])
def test_ishap_parity_and_additivity(models, score_batch, family):
    p, paths, eng = models[family]
    assert p.bg_codes.shape == (256, N_CAT) and p.bg_nums.shape == (256, N_NUM)
    codes, nums = encode_batch(score_batch.iloc[:96], p.vocabs)
    out = eng.explain_arrays(codes, nums, method=METHOD)
    got = out["contributions"]
    ref = _ref(p, paths, codes, nums, p.bg_codes, p.bg_nums)
    assert got.shape == ref.shape == (96, N_SRC) and got.dtype == np.float64
    print(f"{family}: leaves={paths.n_leaves} "
          f"ishap parity max |err| = {np.abs(got - ref).max():.3e}")
    assert np.abs(ref).max() > 1e-4
    np.testing.assert_allclose(got, ref, rtol=0, atol=ATOL)
    assert out["background_rows"] == 256
    assert out["output_space"] == ("log_odds" if family == "gbt" else "probability")
    # the base value is computed on the host: bit-equal to the CPU engine's
    cpu_out = ScoringEngine(p, device="cpu").explain_arrays(codes[:1], nums[:1], method=METHOD)
    assert out["base_value"] == cpu_out["base_value"]
    score = eng.score_arrays(codes, nums, with_drift=False)["predictions"]
    print(f"{family}: additivity on GPU max |err| = "
          f"{np.abs(out['predictions'] - score).max():.3e}")
    np.testing.assert_allclose(out["predictions"], score, rtol=0, atol=ATOL)


def test_ishap_caterpillar(models):
    """All 23 players on one path, players with two splits, and the corners
    of the weight table: the explained row differs from the background row
    in every player (nx = 23, nr = 0), then the roles swapped (0, 23)."""
    p, paths, eng = models["caterpillar"]
    codes, nums = caterpillar_rows()
    bc, bn = _breaker_of(codes[0], nums[0])
    fwd = eng.explain_arrays(codes, nums, method=METHOD, background=(bc[None], bn[None]))
    ref = _ref(p, paths, codes, nums, bc[None], bn[None])
    print(f"caterpillar (23, 0): parity max |err| = {np.abs(fwd['contributions'] - ref).max():.3e}")
    # row 0 against the breaker: the long leaf has all 23 players on x's side
    want, shapes = _caterpillar_pair_oracle(p, codes[0], nums[0], bc, bn)
    assert (N_SRC, 0) in shapes
    np.testing.assert_allclose(ref[0], want, rtol=0, atol=1e-12)
    np.testing.assert_allclose(fwd["contributions"], ref, rtol=0, atol=ATOL)
    rev = eng.explain_arrays(
        bc[None], bn[None], method=METHOD, background=(codes[:1], nums[:1])
    )
    ref = _ref(p, paths, bc[None], bn[None], codes[:1], nums[:1])
    print(f"caterpillar (0, 23): parity max |err| = {np.abs(rev['contributions'] - ref).max():.3e}")
    want, shapes = _caterpillar_pair_oracle(p, bc, bn, codes[0], nums[0])
    assert (0, N_SRC) in shapes
    np.testing.assert_allclose(ref[0], want, rtol=0, atol=1e-12)
    np.testing.assert_allclose(rev["contributions"], ref, rtol=0, atol=ATOL)
    # a mixed background over all rows
    bg = (np.concatenate([bc[None], codes]), np.concatenate([bn[None], nums]))
    mixed = eng.explain_arrays(codes, nums, method=METHOD, background=bg)
    np.testing.assert_allclose(
        mixed["contributions"], _ref(p, paths, codes, nums, *bg), rtol=0, atol=ATOL
    )
    np.testing.assert_allclose(
        mixed["predictions"],
        cpu_ref.score_forest_cpu(p, codes, cpu_ref.impute_nums(p, nums)),
        rtol=0,
        atol=ATOL,
    )


@pytest.mark.parametrize("b", [1, 63, 64, 65, N - 1, N, N + 1, 300])
def test_ishap_row_sweep(models, b):
    """Row guard (b=1), a partly filled last block (N-1, N+1, 300), exact
    blocks (N), sub-wave and wave edges (63..65), at R = 64. Threads past the
    last row stay in the kernel's barriers and must not write."""
    p, paths, eng = models["rf"]
    codes, nums = _random_rows(p, b, seed=b)
    bg = (p.bg_codes[:64], p.bg_nums[:64])
    got = eng.explain_arrays(codes, nums, method=METHOD, background=bg)["contributions"]
    ref = _ref(p, paths, codes, nums, *bg)
    print(f"ishap parity b={b} max |err| = {np.abs(got - ref).max():.3e}")
    assert got.shape == (b, N_SRC)
    np.testing.assert_allclose(got, ref, rtol=0, atol=ATOL)


@pytest.mark.parametrize("r", [1, 63, 64, 65, N - 1, N, N + 1, 257, 1024])
def test_ishap_background_sweep(models, r):
    """The cooperative mask pass: fewer background rows than threads, its
    stride and tail, and the full LDS mask capacity, at B = 65."""
    p, paths, eng = models["rf"]
    codes, nums = _random_rows(p, 65, seed=1000 + r)
    bg = _random_rows(p, r, seed=2000 + r)
    keep = min(r, 200)  # rows drawn like the sample itself keep live pairs common
    bg[0][:keep] = np.resize(p.bg_codes, (keep, N_CAT))
    bg[1][:keep] = np.resize(p.bg_nums, (keep, N_NUM))
    out = eng.explain_arrays(codes, nums, method=METHOD, background=bg)
    ref = _ref(p, paths, codes, nums, *bg)
    print(f"ishap parity r={r} max |err| = {np.abs(out['contributions'] - ref).max():.3e}")
    assert out["background_rows"] == r and np.abs(ref).max() > 1e-4
    np.testing.assert_allclose(out["contributions"], ref, rtol=0, atol=ATOL)


def test_ishap_too_many_background_rows_refused_on_the_host(models):
    p, _, eng = models["rf"]
    codes, nums = _random_rows(p, 4, seed=1)
    bg = _random_rows(p, 1025, seed=2)
    with pytest.raises(ValueError, match="1024"):
        eng.explain_arrays(codes, nums, method=METHOD, background=bg)
    import torch

    from creditcore.ops import gpu

    dev = torch.device("cuda", 0)
    eng.explain_arrays(codes, nums, method=METHOD, background=(bg[0][:4], bg[1][:4]))
    m = eng._shap_dev  # the path table, uploaded by the call above
    with pytest.raises(RuntimeError, match="background"):
        gpu.ext().forest_ishap(
            torch.from_numpy(codes).to(dev), torch.from_numpy(nums).to(dev),
            torch.from_numpy(bg[0]).to(dev), torch.from_numpy(bg[1]).to(dev),
            m["leaf_value"], m["leaf_off"], m["splits"], m["medians"], 0, p.cls_n_trees,
        )


def test_ishap_launch_splitting(models, monkeypatch):
    p, paths, eng = models["rf"]
    codes, nums = _random_rows(p, 300, seed=7)
    bg = (p.bg_codes[:64], p.bg_nums[:64])
    whole = eng.explain_arrays(codes, nums, method=METHOD, background=bg)["contributions"]
    monkeypatch.setattr(ScoringEngine, "ISHAP_MAX_PAIRS", 64 * 130 + 9)  # 130, 130, 40 rows
    split = eng.explain_arrays(codes, nums, method=METHOD, background=bg)["contributions"]
    print(f"launch splitting max |diff| = {np.abs(split - whole).max():.3e}")
    np.testing.assert_allclose(split, whole, rtol=0, atol=ATOL)
    np.testing.assert_allclose(split, _ref(p, paths, codes, nums, *bg), rtol=0, atol=ATOL)


def test_ishap_leaves_session_alone(models, score_batch):
    """explain -> score -> explain on a fresh engine: the two explains agree
    (to the atomic-order bound) and the score equals one taken before any
    explain call."""
    p = models["rf"][0]
    codes, nums = encode_batch(score_batch.iloc[:200], p.vocabs)
    eng = ScoringEngine(p, device="cuda", device_index=0)
    before = eng.score_arrays(codes, nums)
    first = eng.explain_arrays(codes, nums, method=METHOD)["contributions"]
    after = eng.score_arrays(codes, nums)
    second = eng.explain_arrays(codes, nums, method=METHOD)["contributions"]
    np.testing.assert_allclose(first, second, rtol=0, atol=ATOL)
    # the bounds test_explain_gpu.py holds the session to (f64 atomics)
    np.testing.assert_allclose(
        after["predictions"], before["predictions"], rtol=0, atol=ATOL
    )
    np.testing.assert_array_equal(after["outliers"], before["outliers"])
    np.testing.assert_allclose(after["p_vals"], before["p_vals"], rtol=0, atol=1e-12)

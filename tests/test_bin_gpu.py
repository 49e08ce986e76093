"""Device binning (hgbt.bin_features_gpu: bin_select / bin_assign in
csrc/creditcore_kernels.hip) against hgbt.bin_features on the same array, with
exact equality, and the two trainers fitted from device-born bins against the
same fits from host bins. Run on a real MI355X (`pytest -m gpu`)."""

from __future__ import annotations

import numpy as np
import pytest

from creditcore.models import hgbt
from creditcore.models.hgbt import HistGBTClassifier
from creditcore.models.hrf import HistForestClassifier

pytestmark = pytest.mark.gpu

KINDS = (
    "constant", "onehot", "two", "max_bins", "max_bins+1", "adjacent", "zeros",
    "denormal", "huge", "low_byte", "high_byte", "sparse_tail", "normal", "age",
)


def _column(kind: str, n: int, max_bins: int, rng) -> np.ndarray:
    """One f32 column of ``n`` rows of the given kind (module docstring of the
    issue: every mode and key-byte pattern the select has to tell apart)."""
    bits = lambda u: np.asarray(u, dtype=np.uint32).view(np.float32)  # noqa: E731
    pick = lambda values: rng.choice(np.asarray(values, dtype=np.float32), n)  # noqa: E731
    if kind == "constant":
        return np.full(n, 3.25, dtype=np.float32)
    if kind == "onehot":
        return pick([0.0, 1.0])
    if kind == "two":
        return pick([-1.0, 2.5])
    if kind == "max_bins":  # the last exact column ...
        return pick(np.arange(max_bins) * 0.37 - 5.0)
    if kind == "max_bins+1":  # ... and the first quantile one
        return pick(np.arange(max_bins + 1) * 0.37 - 5.0)
    if kind == "adjacent":  # midpoints round onto the upper neighbour
        return pick(bits(np.uint32(0x3F800000) + np.arange(40, dtype=np.uint32)))
    if kind == "zeros":
        return pick([-0.0, 0.0, -1e-3, 1e-3, -1e-30, 1e-30])
    if kind == "denormal":
        return pick(np.arange(-300, 301) * np.float32(1.4e-45))
    if kind == "huge":
        return pick([-3e38, 3e38, 0.0, 1.0])
    if kind == "low_byte":  # keys differ in their lowest byte only
        return pick(bits(np.uint32(0x40490F00) + np.arange(256, dtype=np.uint32)))
    if kind == "high_byte":  # ... and in their highest byte only (all finite)
        return pick(bits((np.arange(256, dtype=np.uint32) << 24) | np.uint32(0x00400000)))
    if kind == "sparse_tail":  # many ranks on one value; `< max` drops edges
        return np.where(rng.random(n) < 0.9, 0.0, rng.normal(size=n)).astype(np.float32)
    if kind == "normal":
        return rng.normal(size=n).astype(np.float32)
    return rng.integers(18, 74, size=n).astype(np.float32)  # age


def _matrix(n: int, n_feat: int, max_bins: int, first: int = 0) -> np.ndarray:
    rng = np.random.default_rng([n, n_feat, max_bins])
    cols = [_column(KINDS[(first + f) % len(KINDS)], n, max_bins, rng) for f in range(n_feat)]
    return np.ascontiguousarray(np.stack(cols, axis=1))


# all N at max_bins 256, all max_bins at N = 4099, and the feature counts (one
# above a column group) at N = 4099; F = 1 is the normal column, F = 3 starts
# at the sparse tail
CASES = (
    [(n, 51, 256, 0) for n in (1, 2, 63, 64, 65, 257, 4099, 200_003)]
    + [(4099, 51, b, 0) for b in (2, 3, 16, 255)]
    + [(4099, 1, 256, 12), (4099, 3, 256, 11), (4099, 65, 256, 0)]
)


@pytest.mark.parametrize("n, n_feat, max_bins, first", CASES)
def test_matches_host_binning(n, n_feat, max_bins, first, monkeypatch):
    from creditcore.ops import gpu

    assert n_feat != 65 or n_feat > gpu.ext().BIN_GROUP_COLS
    if n > 100_000:  # several launches over row slices, the last one ragged
        monkeypatch.setattr(hgbt, "BIN_LAUNCH_ROWS", 65_536)
    x = _matrix(n, n_feat, max_bins, first)
    ref_bins, ref_off, ref_thr = hgbt.bin_features(x, max_bins)
    bins, off, thr = hgbt.bin_features_gpu(x, max_bins, "cuda")
    assert bins.is_cuda and off.dtype == np.int32 and thr.dtype == np.float32
    np.testing.assert_array_equal(off, ref_off)
    np.testing.assert_array_equal(thr, ref_thr)
    np.testing.assert_array_equal(bins.cpu().numpy(), ref_bins)


@pytest.fixture(scope="module")
def credit():
    from creditcore.data import make_uci_shaped_frame
    from creditcore.models.forest import make_classifier_pipeline
    from creditcore.schema import FEATURES, TARGET

    df = make_uci_shaped_frame(n_rows=2000, seed=5)
    pre = make_classifier_pipeline({}, "rf").named_steps["preprocessor"]
    x = pre.fit_transform(df[FEATURES])
    x = x.toarray() if hasattr(x, "toarray") else x
    return np.ascontiguousarray(x, dtype=np.float32), df[TARGET].to_numpy().ravel()


@pytest.mark.parametrize("make", [
    lambda d: HistGBTClassifier(n_estimators=5, device="cuda", bin_device=d),
    lambda d: HistForestClassifier(n_estimators=5, random_state=3, device="cuda", bin_device=d),
    lambda d: HistForestClassifier(n_estimators=5, max_depth=14, deep_trees=True,
                                   random_state=3, device="cuda", bin_device=d),
], ids=["hgbt", "hrf", "hrf_deep14"])
def test_fits_identical_to_host_binning(make, credit):
    x, y = credit
    host, dev = make("cpu").fit(x, y), make("cuda").fit(x, y)
    fitted = [k for k, v in vars(host).items() if k.endswith("_") and isinstance(v, np.ndarray)]
    assert {"bin_thresholds_", "feature_", "threshold_", "value_"} <= set(fitted)
    for key in fitted:
        np.testing.assert_array_equal(getattr(dev, key), getattr(host, key), err_msg=key)

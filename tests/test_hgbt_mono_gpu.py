"""hgbt_split_mono (csrc/creditcore_kernels.hip) vs cpu_ref.hgbt_split_mono_cpu
with exact equality (the gain by its f64 bits), and a constrained GPU fit
replayed on the CPU, served and swept. Run on a real MI355X (`pytest -m gpu`)."""

from __future__ import annotations

import numpy as np
import pytest
from _hgbt_mono_cases import INF, S, hand_cases, run_case

from creditcore.models import hgbt
from creditcore.models.hgbt import verify_monotone
from creditcore.ops import cpu_ref

pytestmark = pytest.mark.gpu

MONO = {"credit_limit": -1, "age": 1, "payment_amount_1": -1}


@pytest.fixture(scope="module")
def ext():
    from creditcore.ops import gpu

    assert gpu.available(), (
        "HIP extension must be present on a GPU box (no silent CPU fallback)"
    )
    return gpu.ext()


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _gpu_split(ext):
    def split(hist, bin_off, lam, min_leaf, mono, bounds):
        return ext.hgbt_split_mono(
            _dev(hist), _dev(bin_off), lam, min_leaf, _dev(mono), _dev(bounds)
        ).cpu().numpy()

    return split


def _check(ext, hist, bin_off, lam, min_leaf, mono, bounds):
    mono = np.asarray(mono, dtype=np.int32)
    bounds = np.asarray(bounds, dtype=np.float64)
    got = _gpu_split(ext)(hist, bin_off, lam, min_leaf, mono, bounds)
    ref = cpu_ref.hgbt_split_mono_cpu(hist, bin_off, lam, min_leaf, mono, bounds)
    np.testing.assert_array_equal(got, ref)  # gain compared by its f64 bits
    return ref


def _level(n, n_bins, n_nodes, seed):
    """A level histogram of random rows (test_hgbt_gpu._problem's recipe)."""
    rng = np.random.default_rng(seed)
    bins = np.stack([rng.integers(0, nb, size=n) for nb in n_bins]).astype(np.uint8)
    bin_off = np.concatenate([[0], np.cumsum(n_bins)]).astype(np.int32)
    node = rng.integers(0, n_nodes, size=n).astype(np.int32)
    p = rng.random(n)
    y = rng.integers(0, 2, size=n)
    gq = np.rint((p - y) * (1 << S)).astype(np.int32)
    hq = np.rint(p * (1 - p) * (1 << S)).astype(np.int32)
    return cpu_ref.hgbt_hist_cpu(bins, bin_off, node, gq, hq, n_nodes), bin_off


def _bounds(rng, k):
    """Per-node bounds cycling through infinite, one-sided (both ways), tight
    around 0, and lo == hi; weights here are O(0.1)."""
    kinds = np.arange(k) % 5
    c = rng.normal(scale=0.05, size=k)
    lo = np.select([kinds == 0, kinds == 1, kinds == 2, kinds == 3], [-INF, -INF, c, c - 0.01], c)
    hi = np.select([kinds == 0, kinds == 1, kinds == 2, kinds == 3], [INF, c, INF, c + 0.01], c)
    return np.stack([lo, hi], axis=1)


def test_split_mono_random_levels(ext):
    rng = np.random.default_rng(7)
    n_split = n_none = 0
    for seed, n_bins, k in ((0, [2, 256, 7, 2, 100], 5), (1, [256], 1), (2, [2] * 9 + [255, 3], 33)):
        hist, bin_off = _level(4000, n_bins, k, seed)
        n_feat = len(n_bins)
        signs = [np.ones(n_feat), -np.ones(n_feat), rng.integers(-1, 2, size=n_feat)]
        for mono in signs:
            for bounds in (np.tile([-INF, INF], (k, 1)), _bounds(rng, k)):
                for lam, min_leaf in ((1.0, 5), (0.0, 1)):
                    ref = _check(ext, hist, bin_off, lam, min_leaf, mono, bounds)
                    n_split += int((ref[:, 1] >= 0).sum())
                    n_none += int((ref[:, 1] < 0).sum())
    assert n_split > 50 and n_none > 0


@pytest.mark.parametrize("name", sorted(hand_cases()))
def test_split_mono_hand_built(ext, name):
    """All rejected, second-best chosen, clamped sides, the zero-hessian side
    and the tie cases, against the brute force of the CPU file."""
    run_case(_gpu_split(ext), hand_cases()[name])


@pytest.mark.parametrize("sign", [1, -1])
def test_split_mono_one_full_256_bin_feature(ext, sign):
    """Every lane live with all four of its bins; gradients trend with the
    bin so that one sign accepts most candidates and the other rejects them."""
    rng = np.random.default_rng(11)
    n = 256 * 40
    bins = (np.arange(n) % 256).astype(np.uint8)[None, :]
    bin_off = np.asarray([0, 256], dtype=np.int32)
    trend = (bins[0].astype(np.float64) - 128.0) / 400.0
    p = np.clip(0.5 + trend + rng.normal(scale=0.05, size=n), 0.01, 0.99)
    y = rng.random(n) < 0.5
    gq = np.rint((p - y) * (1 << S)).astype(np.int32)
    hq = np.rint(p * (1 - p) * (1 << S)).astype(np.int32)
    hist = cpu_ref.hgbt_hist_cpu(bins, bin_off, np.zeros(n, dtype=np.int32), gq, hq, 1)
    assert (hist[0, 2] == 40).all()
    free = [[-INF, INF]]
    ref = _check(ext, hist, bin_off, 1.0, 1, [sign], free)
    # g rises with the bin, so the weight falls: only -1 admits the best cut
    plain = _check(ext, hist, bin_off, 1.0, 1, [0], free)
    assert plain[0, 1] == 0
    assert (ref[0, 2] == plain[0, 2]) == (sign < 0)
    # mirrored gradients swap the roles, so each sign sees live candidates
    for h in (hist, hist * np.asarray([-1, 1, 1])[None, :, None]):
        _check(ext, h, bin_off, 0.0, 1, [sign], [[-0.02, 0.03]])
        _check(ext, h, bin_off, 1.0, 41, [sign], [[0.0, INF]])
    mirrored = _check(ext, h, bin_off, 1.0, 1, [sign], free)
    assert (mirrored[0, 1] == 0) == (sign > 0)


def test_launcher_rejects_bad_arguments(ext):
    hist, bin_off = _level(500, [4, 3], 2, 3)
    ok = np.tile([-INF, INF], (2, 1))
    split = _gpu_split(ext)
    mono = np.zeros(2, dtype=np.int32)
    with pytest.raises(RuntimeError, match="mono"):
        split(hist, bin_off, 1.0, 1, np.zeros(3, dtype=np.int32), ok)
    with pytest.raises(RuntimeError, match="mono"):
        split(hist, bin_off, 1.0, 1, np.zeros(2, dtype=np.int64), ok)
    with pytest.raises(RuntimeError, match="bounds"):
        split(hist, bin_off, 1.0, 1, mono, ok[:1])
    with pytest.raises(RuntimeError, match="bounds"):
        split(hist, bin_off, 1.0, 1, mono, ok.astype(np.float32))
    with pytest.raises(RuntimeError, match="lo <= hi"):
        split(hist, bin_off, 1.0, 1, mono, np.asarray([[0.5, 0.25], [-INF, INF]]))
    with pytest.raises(RuntimeError, match="lo <= hi"):
        split(hist, bin_off, 1.0, 1, mono, np.asarray([[-INF, INF], [np.nan, 1.0]]))


@pytest.fixture(scope="module")
def replay():
    """One constrained GPU fit (test_hgbt_gpu.replay's shape) with the
    per-round int32 gradients recorded."""
    from creditcore.data import make_uci_shaped_frame
    from creditcore.models.forest import make_classifier_pipeline
    from creditcore.schema import FEATURES, TARGET

    df = make_uci_shaped_frame(n_rows=3000, seed=11)
    pipe = make_classifier_pipeline(
        {"n_estimators": 8, "max_depth": 5, "device": "cuda", "monotone": MONO},
        algorithm="hgbt",
    )
    grads = []
    pipe.named_steps["classifier"]._grad_hook = lambda r, g, h: grads.append((g, h))
    pipe.fit(df[FEATURES], df[TARGET].values.ravel())
    return df, pipe, grads


def test_replay_trees_bit_identical(replay):
    df, pipe, grads = replay
    from creditcore.schema import FEATURES, NUMERIC_FEATURES

    clf = pipe.named_steps["classifier"]
    assert clf.fit_device_ == "cuda" and len(grads) == 8
    mono = clf.monotone_cst_
    assert mono.dtype == np.int32 and np.abs(mono).sum() == 3
    assert mono[-len(NUMERIC_FEATURES)] == -1
    x = hgbt._to_dense_f32(pipe.named_steps["preprocessor"].transform(df[FEATURES]))
    bins, bin_off, bin_thr = hgbt.bin_features(x, clf.max_bins)
    backend = hgbt._CpuBackend(bins, bin_off)
    n_signed = 0
    for i, (gq, hq) in enumerate(grads):
        tree, _ = hgbt.grow_tree(
            backend, gq, hq, bin_off, bin_thr, clf.max_depth, clf.l2,
            clf.min_samples_leaf, clf.learning_rate, mono=mono,
        )
        got = clf.tree_arrays(i)
        for key, ref in tree.items():
            assert got[key].dtype == ref.dtype, key
            assert got[key].tobytes() == ref.tobytes(), (i, key)
        inner = tree["children_left"] >= 0
        n_signed += int((mono[tree["feature"][inner]] != 0).sum())
    assert n_signed > 0  # constrained columns were split on
    assert verify_monotone(pipe)


def test_first_tree_equals_cpu_fit(replay):
    """Round 0's gradients depend only on y and the prior."""
    df, pipe, _ = replay
    from sklearn.base import clone

    from creditcore.schema import FEATURES, TARGET

    cpu = clone(pipe).set_params(classifier__device="cpu", classifier__n_estimators=1)
    cpu.fit(df[FEATURES], df[TARGET].values.ravel())
    a = cpu.named_steps["classifier"].tree_arrays(0)
    b = pipe.named_steps["classifier"].tree_arrays(0)
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), key


def test_constrained_model_serves_monotone(replay, score_batch):
    from creditcore.engine import ScoringEngine
    from creditcore.pack import (
        PackedModel,
        encode_batch,
        pack_classifier_pipeline,
        pack_drift,
        pack_isolation_forest,
    )
    from creditcore.schema import FEATURES
    from creditcore.train import fit_detectors

    df, pipe, _ = replay
    drift, outlier = fit_detectors(df)
    c = pack_classifier_pipeline(pipe)
    packed = PackedModel(**c, **pack_isolation_forest(outlier), **pack_drift(drift, c["vocabs"]))
    eng = ScoringEngine(packed, device="cuda", device_index=0)
    codes, nums = encode_batch(score_batch, packed.vocabs)
    score = eng.score_arrays(codes, nums, with_drift=False)["predictions"]
    sk = pipe.predict_proba(score_batch[FEATURES])[:, 1]
    np.testing.assert_allclose(score, sk, rtol=0, atol=1e-9)

    # sweep one constrained feature over 64 values for 32 base rows
    base = score_batch.iloc[8:40].reset_index(drop=True)  # rows without NaN
    grid = np.quantile(df["credit_limit"].to_numpy(), np.linspace(0.0, 1.0, 64))
    sweep = base.loc[np.repeat(np.arange(32), 64)].reset_index(drop=True)
    sweep["credit_limit"] = np.tile(grid, 32)
    codes, nums = encode_batch(sweep, packed.vocabs)
    served = eng.score_arrays(codes, nums, with_drift=False)["predictions"].reshape(32, 64)
    raw = pipe.decision_function(sweep[FEATURES]).reshape(32, 64)
    assert (np.diff(raw, axis=1) <= 0.0).all()  # credit_limit = -1, exact
    assert (np.diff(raw, axis=1) < 0.0).any()
    # the allowance covers the device exp only
    assert np.diff(served, axis=1).max() <= 1e-12

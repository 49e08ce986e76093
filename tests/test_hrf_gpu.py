"""HistForest training kernels (hrf_hist / hrf_split / hrf_route in
csrc/creditcore_kernels.hip) vs the numpy primitives of ops/cpu_ref.py, with
exact equality: everything compared is an integer or comes from the same f64
formula evaluated in the same order (the proxy is compared by its f64 bits).
Run on a real MI355X (`pytest -m gpu`)."""

from __future__ import annotations

import math

import numpy as np
import pytest
from _hrf_cases import BIN_OFF6, assert_same_forest, candidate_cases, fit_hrf, hand_hist

from creditcore.models import hgbt, hrf
from creditcore.models.hgbt import plan_feature_groups
from creditcore.models.hrf import HistForestClassifier
from creditcore.ops import cpu_ref

pytestmark = pytest.mark.gpu

LDS_BYTES = hgbt.LDS_BUDGET_BYTES
LAYOUT = [2, 256, 7, 2, 100]


@pytest.fixture(scope="module")
def ext():
    from creditcore.ops import gpu

    assert gpu.available(), (
        "HIP extension must be present on a GPU box (no silent CPU fallback)"
    )
    assert gpu.ext().HRF_MAX_FEATS == hrf.MAX_FEATURES
    return gpu.ext()


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _problem(n, n_bins, slots, seed=0, leaf_frac=0.0, zero_frac=0.3):
    """Random level of a tree batch: bins u8[F, n], y u8[n], weights u8[TB, n]
    (a fraction 0), local slots i32[TB, n] in [0, slots[t]) (negative where
    the weight is 0, where a fraction sits in a leaf, and all over a tree
    without open slots) and slot_off."""
    rng = np.random.default_rng(seed)
    tb = len(slots)
    bins = np.stack([rng.integers(0, nb, size=n) for nb in n_bins]).astype(np.uint8)
    bin_off = np.concatenate([[0], np.cumsum(n_bins)]).astype(np.int32)
    y = rng.integers(0, 2, size=n).astype(np.uint8)
    w = rng.integers(1, 6, size=(tb, n)).astype(np.uint8)
    w[rng.random((tb, n)) < zero_frac] = 0
    node = np.stack(
        [rng.integers(0, max(k, 1), size=n) if k else np.full(n, -1) for k in slots]
    ).astype(np.int32)
    node[rng.random((tb, n)) < leaf_frac] = -3
    node[w == 0] = -1
    slot_off = np.concatenate([[0], np.cumsum(slots)]).astype(np.int32)
    return bins, bin_off, y, w, node, slot_off


def _check_hist(ext, prob, rows_per_block=None, max_feats=8):
    bins, bin_off, y, w, node, slot_off = prob
    rpb = int(ext.HRF_MAX_ROWS_PER_BLOCK) if rows_per_block is None else rows_per_block
    k_max = int(np.diff(slot_off).max())
    grp, entries = plan_feature_groups(np.diff(bin_off), k_max, LDS_BYTES, max_feats, planes=2)
    got = ext.hrf_hist(
        _dev(bins), _dev(bin_off), _dev(grp), _dev(y), _dev(w), _dev(node), _dev(slot_off),
        int(slot_off[-1]), int(bin_off[-1]), entries, rpb,
    ).cpu().numpy()
    ref = cpu_ref.hrf_hist_cpu(bins, bin_off, y, w, node, slot_off)
    np.testing.assert_array_equal(got, ref)
    return ref, entries


def _row_sweep(rpb):
    return [1, 63, 64, 65, 3 * rpb + 77]


@pytest.mark.parametrize("slots", [[3], [3, 0, 2]], ids=["tb1", "tb3"])
@pytest.mark.parametrize("rpb", [64, 256])
def test_hist_row_counts(ext, rpb, slots):
    for n in _row_sweep(rpb):
        prob = _problem(n, LAYOUT, slots, seed=n, zero_frac=0.3)
        ref, entries = _check_hist(ext, prob, rows_per_block=rpb)
        w = prob[3].astype(np.int64)
        live = [t for t, k in enumerate(slots) if k]
        # every feature sees every open row once, at its weight
        assert entries > 0 and ref[:, 1].sum() == 5 * w[live].sum()


def test_hist_shapes(ext):
    _check_hist(ext, _problem(500, [17], [2, 1], seed=1))
    # a 2-bin feature next to a 256-bin feature, bin 255 occupied
    prob = _problem(700, [2, 256], [1], seed=2, zero_frac=0.0)
    prob[0][1, :5] = 255
    ref, _ = _check_hist(ext, prob, max_feats=2)
    assert ref[0, 1, 2 + 255] >= 5
    # one feature group per feature and all features in one group
    for max_feats in (1, 4):
        _check_hist(ext, _problem(900, [2, 2, 256, 31], [2, 3], seed=3), max_feats=max_feats,
                    rows_per_block=256)


def test_hist_empty_slot_zero_weight_and_leaf_rows(ext):
    prob = _problem(800, [2, 64, 9], [4, 2], seed=4, leaf_frac=0.3, zero_frac=0.4)
    node, w = prob[4], prob[3]
    node[0][node[0] == 2] = 1  # slot 2 of tree 0 owns no row
    # zero weights whose slot was left valid, and weights on leaf rows: both skipped
    node[1, :50] = np.where(node[1, :50] == -3, -3, 0)
    w[1, :25] = 0
    ref, _ = _check_hist(ext, prob, rows_per_block=256)
    assert (ref[2] == 0).all() and ref[0].any() and ref[3].any()
    for t in range(2):
        live = node[t] >= 0
        a, b = prob[5][t], prob[5][t + 1]
        assert 0 < live.sum() < 800
        assert ref[a:b, 1, :2].sum() == w[t][live].astype(np.int64).sum()
        assert ref[a:b, 0, :2].sum() == (w[t][live].astype(np.int64) * prob[2][live]).sum()


def test_hist_int32_headroom(ext):
    """A full block of rows at weight 255 in one bin: the int32 LDS partial
    reaches HRF_MAX_ROWS_PER_BLOCK * 255, the largest value a block can sum."""
    rpb = int(ext.HRF_MAX_ROWS_PER_BLOCK)
    assert rpb * 255 < 2**31
    bins, bin_off, y, w, node, slot_off = _problem(rpb, [4, 2], [1], seed=6)
    bins[:], y[:], w[:], node[:] = 1, 1, 255, 0
    ref, entries = _check_hist(ext, (bins, bin_off, y, w, node, slot_off))
    assert entries > 0 and ref[0, 0, 1] == ref[0, 1, 1] == rpb * 255 == ref[0, 1, 5]


def test_hist_direct_global_path(ext):
    """64 open slots x a 256-bin feature: 64*2*256*4 B = 128 KiB is more than
    the slab budget, so the int64 global-atomic path runs; 32 slots (64 KiB)
    are the deepest level that still uses LDS."""
    prob = _problem(6000, [2, 256, 5], [64, 9], seed=7, leaf_frac=0.1)
    ref, entries = _check_hist(ext, prob, rows_per_block=1024)
    assert entries == 0 and (ref[:64, 1].sum(axis=1) > 0).all()
    ref, entries = _check_hist(ext, _problem(6000, [2, 256, 5], [32, 9], seed=8),
                               rows_per_block=1024)
    assert 0 < entries * 4 <= LDS_BYTES and entries == 32 * 2 * 256


def _check_split(ext, hist, bin_off, meta, m, min_leaf, seed):
    sd = seed - (1 << 64) if seed >= (1 << 63) else seed
    got = ext.hrf_split(_dev(hist), _dev(np.asarray(bin_off, dtype=np.int32)),
                        _dev(meta), m, min_leaf, sd).cpu().numpy()
    ref = cpu_ref.hrf_split_cpu(hist, bin_off, meta, m, min_leaf, seed)
    np.testing.assert_array_equal(got, ref)  # proxy compared by its f64 bits
    return ref


@pytest.mark.parametrize("n_feat", [1, 5, 11, 51])
def test_split_random_levels(ext, n_feat):
    rng = np.random.default_rng(n_feat)
    n_bins = [int(b) for b in rng.choice([2, 2, 3, 7, 100, 255, 256], size=n_feat)]
    slots = [5, 0, 4]
    bins, bin_off, y, w, node, slot_off = _problem(4000, n_bins, slots, seed=n_feat)
    hist = cpu_ref.hrf_hist_cpu(bins, bin_off, y, w, node, slot_off)
    meta = np.stack([np.repeat([7, 8, 499], slots), rng.integers(0, 4095, size=9)], axis=1)
    meta = meta.astype(np.int32)
    for m in sorted({1, max(1, math.isqrt(n_feat)), n_feat}):
        for seed in (0, 2**63 + 5):
            ref = _check_split(ext, hist, bin_off, meta, m, 5, seed)
            assert (ref[:, 1] >= 0).all() and (ref[:, 6] > 0).all()
    _check_split(ext, hist, bin_off, meta, 1, 1, 3)


def test_split_ties(ext):
    """Identical columns tie across features (lower rank wins), a symmetric
    histogram ties across bins (lowest bin wins)."""
    seed, meta, order, _ = candidate_cases()
    ref = _check_split(ext, hand_hist([4] * 6), BIN_OFF6, meta, 6, 1, seed)
    assert ref[0, 1] == order[0]
    rng = np.random.default_rng(3)
    col = rng.integers(0, 8, size=600).astype(np.uint8)
    bins = np.stack([col, col, col])
    bin_off = np.asarray([0, 8, 16, 24], dtype=np.int32)
    y = (col >= 4).astype(np.uint8)
    w = np.ones((1, 600), dtype=np.uint8)
    node = np.zeros((1, 600), dtype=np.int32)
    hist = cpu_ref.hrf_hist_cpu(bins, bin_off, y, w, node, np.asarray([0, 1], dtype=np.int32))
    for nd in range(4):
        m1 = np.asarray([[2, nd]], dtype=np.int32)
        ref = _check_split(ext, hist, bin_off, m1, 3, 1, 11)
        assert ref[0, 2] == 3 and ref[0, 3] == 0  # pure left side
    # bins 1 and 2 empty: "bin <= 0", "<= 1" and "<= 2" are the same split
    hist = np.zeros((1, 2, 4), dtype=np.int64)
    hist[0, :, 0], hist[0, :, 3] = [5, 40], [30, 40]
    ref = _check_split(ext, hist, [0, 4], meta, 1, 1, seed)
    assert list(ref[0, 1:5]) == [0, 0, 5, 40]


def test_split_candidate_rule_and_rejections(ext):
    seed, meta, order, cases = candidate_cases()
    for name, hist, want in cases:  # inside m, extension past m, no split
        ref = _check_split(ext, hist, BIN_OFF6, meta, 2, 1, seed)
        assert ref[0, 1] == want, name
    assert list(ref[0]) == [0, -1, 0, 0, 0, 48, 120]
    # min_samples_leaf rejects every bin: leaf records, totals still reported
    bins, bin_off, y, w, node, slot_off = _problem(300, [2, 50, 6], [2, 1], seed=9)
    hist = cpu_ref.hrf_hist_cpu(bins, bin_off, y, w, node, slot_off)
    meta3 = np.asarray([[0, 1], [0, 2], [1, 0]], dtype=np.int32)
    ref = _check_split(ext, hist, bin_off, meta3, 3, 10_000, 1)
    assert (ref[:, 1] == -1).all() and (ref[:, [0, 2, 3, 4]] == 0).all()
    assert (ref[:, 6] == hist[:, 1, :2].sum(axis=1)).all() and (ref[:, 6] > 0).all()


@pytest.mark.parametrize("rpb", [64, 256])
def test_route(ext, rpb):
    slots = [4, 0, 2]
    table = np.asarray(
        [[1, 100, 0, -5], [-1, 0, -2, -2], [0, 0, -7, 1], [2, 3, 2, 3],  # tree 0
         [1, 100, -9, 0], [-1, 0, -4, -4]],  # tree 2
        dtype=np.int32,
    )
    for n in _row_sweep(rpb):
        bins, _, _, _, node, slot_off = _problem(n, [2, 256, 7], slots, seed=n, leaf_frac=0.2)
        bins[1, ::3] = 100  # rows exactly in the split bin go left
        before = node.copy()
        d_node = _dev(node)
        ext.hrf_route(_dev(bins), _dev(table), d_node, _dev(slot_off))
        got = d_node.cpu().numpy()
        np.testing.assert_array_equal(got, cpu_ref.hrf_route_cpu(bins, table, before, slot_off))
        in0 = before[0] == 0
        assert (got[0][in0 & (bins[1] == 100)] == 0).all()
        assert (got[0][in0 & (bins[1] == 101)] == -5).all()
        assert (got[0][before[0] == 1] == -2).all()  # closed slot: leaf code
        assert (got[2][(before[2] == 0) & (bins[1] <= 100)] == -9).all()  # tree 2's own rows
        assert (got[2][before[2] == 1] == -4).all()
        assert (got[before < 0] == before[before < 0]).all()  # leaf rows stay
        assert (got[1] == before[1]).all()  # a tree without open slots


@pytest.fixture(scope="module")
def fits(train_df):
    params = {"n_estimators": 8, "max_depth": 5, "random_state": 3}
    cpu = fit_hrf(train_df, {**params, "device": "cpu"})
    gpu = fit_hrf(train_df, {**params, "device": "cuda"})
    return params, cpu, gpu


def test_gpu_fit_equals_cpu_fit(fits, train_df):
    params, cpu, gpu = fits
    a, b = cpu.named_steps["classifier"], gpu.named_steps["classifier"]
    assert a.fit_device_ == "cpu" and b.fit_device_ == "cuda" and b.n_trees_ == 8
    assert (np.diff(b.tree_offsets_) > 7).all()
    assert_same_forest(b, a)
    for tb in (1, 8):
        c = fit_hrf(train_df, {**params, "device": "cuda"}, tb).named_steps["classifier"]
        assert_same_forest(c, a)


def test_gpu_trained_model_serves(fits, train_df, score_batch):
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

    _, _, pipe = fits
    drift, outlier = fit_detectors(train_df)
    c = pack_classifier_pipeline(pipe)
    packed = PackedModel(**c, **pack_isolation_forest(outlier), **pack_drift(drift, c["vocabs"]))
    assert packed.cls_kind == 0
    eng = ScoringEngine(packed, device="cuda", device_index=0)
    codes, nums = encode_batch(score_batch, packed.vocabs)
    score = eng.score_arrays(codes, nums, with_drift=False)["predictions"]
    sk = pipe.predict_proba(score_batch[FEATURES])[:, 1]
    np.testing.assert_allclose(score, sk, rtol=0, atol=1e-9)
    out = eng.explain_arrays(codes, nums, method="shap")
    assert np.abs(out["contributions"]).max() > 1e-3
    total = out["base_value"] + out["contributions"].sum(1)
    np.testing.assert_allclose(total, score, rtol=0, atol=1e-9)
    np.testing.assert_allclose(out["predictions"], score, rtol=0, atol=1e-9)


def test_auto_without_extension_raises(monkeypatch):
    """A visible device and no extension: device="auto" must not fall back.
    The loader is patched; nothing runs on the GPU."""
    import torch

    from creditcore.ops import gpu

    assert torch.cuda.is_available()
    monkeypatch.setattr(gpu, "_ext", None)
    monkeypatch.setattr(gpu, "_err", ImportError("patched out"))
    x = np.random.default_rng(0).normal(size=(50, 2)).astype(np.float32)
    with pytest.raises(gpu.ExtensionMissing):
        HistForestClassifier(n_estimators=1, device="auto").fit(x, (x[:, 0] > 0).astype(int))

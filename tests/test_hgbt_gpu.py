"""HistGBT training kernels (hgbt_hist / hgbt_split / hgbt_route in
csrc/creditcore_kernels.hip) vs the numpy primitives of ops/cpu_ref.py, with
exact equality: everything compared is an integer or comes from the same f64
formula evaluated in the same order. Run on a real MI355X (`pytest -m gpu`)."""

from __future__ import annotations

import numpy as np
import pytest

from creditcore.models import hgbt
from creditcore.models.hgbt import HistGBTClassifier, plan_feature_groups
from creditcore.ops import cpu_ref

pytestmark = pytest.mark.gpu

S = cpu_ref.HGBT_SHIFT
LDS_BYTES = hgbt.LDS_BUDGET_BYTES


@pytest.fixture(scope="module")
def ext():
    from creditcore.ops import gpu

    assert gpu.available(), (
        "HIP extension must be present on a GPU box (no silent CPU fallback)"
    )
    assert gpu.ext().HGBT_SHIFT == S == hgbt.SHIFT
    return gpu.ext()


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _problem(n, n_bins, n_nodes, seed=0, leaf_frac=0.0):
    """Random bins u8[F, n] for the given per-feature bin counts, node ids in
    [0, n_nodes) (a fraction already marked leaf) and int32 gradients."""
    rng = np.random.default_rng(seed)
    bins = np.stack([rng.integers(0, nb, size=n) for nb in n_bins]).astype(np.uint8)
    bin_off = np.concatenate([[0], np.cumsum(n_bins)]).astype(np.int32)
    node = rng.integers(0, n_nodes, size=n).astype(np.int32)
    node[rng.random(n) < leaf_frac] = -3
    p = rng.random(n)
    y = rng.integers(0, 2, size=n)
    gq = np.rint((p - y) * (1 << S)).astype(np.int32)
    hq = np.rint(p * (1 - p) * (1 << S)).astype(np.int32)
    return bins, bin_off, node, gq, hq


def _gpu_hist(ext, bins, bin_off, node, gq, hq, n_nodes, rows_per_block=None, max_feats=8):
    rpb = int(ext.HGBT_MAX_ROWS_PER_BLOCK) if rows_per_block is None else rows_per_block
    grp, entries = plan_feature_groups(np.diff(bin_off), n_nodes, LDS_BYTES, max_feats)
    out = ext.hgbt_hist(
        _dev(bins), _dev(bin_off), _dev(grp), _dev(node), _dev(gq), _dev(hq),
        n_nodes, int(bin_off[-1]), entries, rpb,
    )
    return out.cpu().numpy(), entries


def _check_hist(ext, prob, n_nodes, **kw):
    bins, bin_off, node, gq, hq = prob
    got, entries = _gpu_hist(ext, bins, bin_off, node, gq, hq, n_nodes, **kw)
    ref = cpu_ref.hgbt_hist_cpu(bins, bin_off, node, gq, hq, n_nodes)
    np.testing.assert_array_equal(got, ref)
    return ref, entries


def _row_sweep(rpb):
    # wavefront edges, one block -1/0/+1, three blocks and a ragged tail
    return [1, 63, 64, 65, rpb - 1, rpb, rpb + 1, 3 * rpb + 77]


def test_hist_row_counts(ext):
    rpb = int(ext.HGBT_MAX_ROWS_PER_BLOCK)
    assert rpb * (1 << S) < 2**31 <= (rpb + 1) * (1 << S)
    for n in _row_sweep(rpb):
        ref, entries = _check_hist(ext, _problem(n, [2, 256, 7, 2, 100], 3, seed=n), 3)
        assert entries > 0 and ref[:, 2].sum() == 5 * n
    # a small rows_per_block: many blocks flushing into the same entries
    _check_hist(ext, _problem(1000, [2, 256, 7], 2, seed=5), 2, rows_per_block=64)


def test_hist_shapes(ext):
    # a single feature
    _check_hist(ext, _problem(500, [17], 2, seed=1), 2)
    # a 2-bin feature next to a 256-bin feature, bin 255 occupied
    prob = _problem(700, [2, 256], 1, seed=2)
    prob[0][1, :5] = 255
    ref, _ = _check_hist(ext, prob, 1, max_feats=2)
    assert ref[0, 2, 2 + 255] >= 5
    # one feature group per feature and all features in one group
    _check_hist(ext, _problem(900, [2, 2, 256, 31], 2, seed=3), 2, max_feats=1)
    _check_hist(ext, _problem(900, [2, 2, 256, 31], 2, seed=3), 2, max_feats=4)


def test_hist_empty_node_and_leaf_rows(ext):
    prob = _problem(800, [2, 64, 9], 4, seed=4, leaf_frac=0.3)
    prob[2][prob[2] == 2] = 1  # node 2 owns no row
    ref, _ = _check_hist(ext, prob, 4)
    assert ref[2].sum() == 0 and (ref[2] == 0).all()
    live = int((prob[2] >= 0).sum())
    assert 0 < live < 800 and ref[:, 2, :2].sum() == live  # leaf rows skipped


def test_hist_int32_headroom(ext):
    """One block's worth of rows, all at gq = +2^S in one bin: the int32 LDS
    partial reaches rows_per_block * 2^S, the largest value the bound allows."""
    rpb = int(ext.HGBT_MAX_ROWS_PER_BLOCK)
    bins, bin_off, node, gq, hq = _problem(rpb, [4, 2], 1, seed=6)
    bins[:] = 1
    node[:] = 0
    gq[:] = 1 << S
    hq[:] = 1 << (S - 2)
    ref, entries = _check_hist(ext, (bins, bin_off, node, gq, hq), 1)
    assert entries > 0 and ref[0, 0, 1] == rpb << S
    gq[:] = -(1 << S)
    ref, _ = _check_hist(ext, (bins, bin_off, node, gq, hq), 1)
    assert ref[0, 0, 1] == -(rpb << S)


def test_hist_direct_global_path(ext):
    """64 open nodes x a 256-bin feature: 64*3*256*4 B = 192 KiB is more than
    any LDS slab, so the int64 global-atomic path runs."""
    n_nodes = 64
    prob = _problem(5000, [2, 256, 5], n_nodes, seed=7, leaf_frac=0.1)
    ref, entries = _check_hist(ext, prob, n_nodes)
    assert entries == 0 and (ref[:, 2].sum(axis=1) > 0).all()
    # and the deepest LDS level next to it
    ref, entries = _check_hist(ext, _problem(5000, [2, 256, 5], 16, seed=8), 16)
    assert 0 < entries * 4 <= LDS_BYTES


def _check_split(ext, hist, bin_off, lam, min_leaf):
    got = ext.hgbt_split(_dev(hist), _dev(bin_off), lam, min_leaf).cpu().numpy()
    ref = cpu_ref.hgbt_split_cpu(hist, bin_off, lam, min_leaf)
    np.testing.assert_array_equal(got, ref)  # gain compared by its f64 bits
    return ref


def test_split_random_levels(ext):
    for seed, n_bins, k in ((0, [2, 256, 7, 2, 100], 5), (1, [256], 1), (2, [2] * 9 + [255, 3], 33)):
        bins, bin_off, node, gq, hq = _problem(4000, n_bins, k, seed=seed)
        hist = cpu_ref.hgbt_hist_cpu(bins, bin_off, node, gq, hq, k)
        ref = _check_split(ext, hist, bin_off, 1.0, 5)
        assert (ref[:, 1] >= 0).any()
        _check_split(ext, hist, bin_off, 0.0, 1)


def test_split_ties(ext):
    """Identical columns tie across features, a symmetric histogram ties
    across bins: lowest feature, then lowest bin."""
    rng = np.random.default_rng(3)
    n = 600
    col = rng.integers(0, 8, size=n).astype(np.uint8)
    bins = np.stack([col, col, col])
    bin_off = np.asarray([0, 8, 16, 24], dtype=np.int32)
    gq = ((col >= 4).astype(np.int32) * 2 - 1) * (1 << (S - 1))
    hq = np.full(n, 1 << (S - 2), dtype=np.int32)
    node = np.zeros(n, dtype=np.int32)
    hist = cpu_ref.hgbt_hist_cpu(bins, bin_off, node, gq, hq, 1)
    ref = _check_split(ext, hist, bin_off, 1.0, 1)
    assert ref[0, 1] == 0 and ref[0, 2] == 3
    # bins 1 and 2 empty: "bin <= 0", "<= 1" and "<= 2" are the same split
    hist = np.zeros((1, 3, 4), dtype=np.int64)
    hist[0, :, 0] = [-(40 << S), 10 << S, 40]
    hist[0, :, 3] = [40 << S, 10 << S, 40]
    ref = _check_split(ext, hist, np.asarray([0, 4], dtype=np.int32), 1.0, 1)
    assert ref[0, 1] == 0 and ref[0, 2] == 0


def test_split_rejections(ext):
    bins, bin_off, node, gq, hq = _problem(300, [2, 50, 6], 2, seed=9)
    hist = cpu_ref.hgbt_hist_cpu(bins, bin_off, node, gq, hq, 2)
    # min_samples_leaf rejects every bin
    ref = _check_split(ext, hist, bin_off, 1.0, 200)
    assert (ref[:, 1] == -1).all() and (ref[:, :6][:, [0, 2, 3, 4, 5]] == 0).all()
    assert (ref[:, 8] == np.bincount(node, minlength=2)).all()
    # all rows in one bin
    bins[:] = 1
    hist = cpu_ref.hgbt_hist_cpu(bins, bin_off, node, gq, hq, 2)
    ref = _check_split(ext, hist, bin_off, 1.0, 1)
    assert (ref[:, 1] == -1).all()


def test_route(ext):
    rpb = int(ext.HGBT_MAX_ROWS_PER_BLOCK)
    table = np.asarray(
        [[1, 100, 0, -5], [-1, 0, -2, -2], [0, 0, -7, 1], [2, 3, 2, 3]], dtype=np.int32
    )
    for n in _row_sweep(rpb):
        bins, _, node, _, _ = _problem(n, [2, 256, 7], 4, seed=n, leaf_frac=0.2)
        bins[1, ::3] = 100  # rows exactly in the split bin go left
        before = node.copy()
        d_node = _dev(node)
        ext.hgbt_route(_dev(bins), _dev(table), d_node)
        got = d_node.cpu().numpy()
        np.testing.assert_array_equal(got, cpu_ref.hgbt_route_cpu(bins, table, before))
        in0 = before == 0
        assert (got[in0 & (bins[1] == 100)] == 0).all()
        assert (got[in0 & (bins[1] == 101)] == -5).all()
        assert (got[before == 1] == -2).all()  # closed node: leaf encoding
        assert (got[before == -3] == -3).all()  # rows already in a leaf stay


@pytest.fixture(scope="module")
def replay():
    """One GPU fit with the per-round int32 gradients recorded."""
    from creditcore.data import make_uci_shaped_frame
    from creditcore.models.forest import make_classifier_pipeline
    from creditcore.schema import FEATURES, TARGET

    df = make_uci_shaped_frame(n_rows=3000, seed=11)
    pipe = make_classifier_pipeline(
        {"n_estimators": 8, "max_depth": 5, "device": "cuda"}, algorithm="hgbt"
    )
    grads = []
    pipe.named_steps["classifier"]._grad_hook = lambda r, g, h: grads.append((g, h))
    pipe.fit(df[FEATURES], df[TARGET].values.ravel())
    return df, pipe, grads


def test_replay_trees_bit_identical(replay):
    df, pipe, grads = replay
    from creditcore.schema import FEATURES

    clf = pipe.named_steps["classifier"]
    assert clf.fit_device_ == "cuda" and len(grads) == 8
    x = hgbt._to_dense_f32(pipe.named_steps["preprocessor"].transform(df[FEATURES]))
    bins, bin_off, bin_thr = hgbt.bin_features(x, clf.max_bins)
    backend = hgbt._CpuBackend(bins, bin_off)
    n_inner = 0
    for i, (gq, hq) in enumerate(grads):
        assert gq.dtype == hq.dtype == np.int32
        tree, _ = hgbt.grow_tree(
            backend, gq, hq, bin_off, bin_thr, clf.max_depth, clf.l2,
            clf.min_samples_leaf, clf.learning_rate,
        )
        got = clf.tree_arrays(i)
        for key, ref in tree.items():
            assert got[key].dtype == ref.dtype, key
            assert got[key].tobytes() == ref.tobytes(), (i, key)
        assert tree["children_left"][0] > 0  # the root did split
        n_inner += int((tree["children_left"] >= 0).sum())
    assert n_inner > 8 * 8


def test_first_tree_of_plain_fits_identical(replay):
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


def test_gpu_trained_model_serves(replay, score_batch):
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
    out = eng.explain_arrays(codes, nums, method="shap")
    assert np.abs(out["contributions"]).max() > 1e-3
    raw = out["base_value"] + out["contributions"].sum(1)
    np.testing.assert_allclose(1.0 / (1.0 + np.exp(-raw)), score, rtol=0, atol=1e-9)
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
        HistGBTClassifier(n_estimators=1, device="auto").fit(x, (x[:, 0] > 0).astype(int))

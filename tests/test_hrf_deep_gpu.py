"""Segmented levels of the HistForest trainer (hrf_seg_* in
csrc/creditcore_kernels.hip) against the numpy level primitives of
ops/cpu_ref.py, with exact equality. Run on a real MI355X (`pytest -m gpu`)."""

from __future__ import annotations

import numpy as np
import pytest
from _hrf_cases import assert_same_forest, spec_order
from _hrf_deep_cases import fit_deep, max_tree_depth

from creditcore.ops import cpu_ref

pytestmark = pytest.mark.gpu

SEED = 2**63 + 5
FIRST = 2  # the constant feature of the F = 9 layout


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


def _level(n_bins, chunk):
    """TB = 3, tree 1 without an open slot. Tree 0's slots hold 1 row, exactly
    one staging chunk, more than one chunk (some at weight 255) and 300 rows;
    tree 2's hold 40 and 3. The other rows sit in leaves (node < 0) or have
    weight 0, some of those with a slot left in ``node``; all interleaved."""
    rng = np.random.default_rng(len(n_bins))
    sizes = [[1, chunk, chunk + 77, 300], [], [40, 3]]
    n = 2 * chunk + 700
    bins = np.stack([rng.integers(0, nb, size=n) for nb in n_bins]).astype(np.uint8)
    y = rng.integers(0, 2, size=n).astype(np.uint8)
    w = rng.integers(1, 6, size=(3, n)).astype(np.uint8)
    node = np.full((3, n), -3, dtype=np.int32)
    for t, per_slot in enumerate(sizes):
        perm = rng.permutation(n)
        ends = np.cumsum(per_slot)
        for s, (a, b) in enumerate(zip(ends - per_slot, ends)):
            node[t, perm[a:b]] = s
        rest = perm[int(ends[-1]) if per_slot else 0:]
        w[t, rest[::2]] = 0
        node[t, rest[::4]] = 0  # weight 0 in an open slot: not an open row
    w[0, np.flatnonzero(node[0] == 2)[:9]] = 255
    slot_off = np.concatenate([[0], np.cumsum([len(s) for s in sizes])]).astype(np.int32)
    bin_off = np.concatenate([[0], np.cumsum(n_bins)]).astype(np.int32)
    return bins, bin_off, y, w, node, slot_off, np.concatenate(sizes).astype(int)


@pytest.mark.parametrize("m, min_leaf", [(None, 1), (1, 1), (1, 5), (None, 10**6)])
@pytest.mark.parametrize("n_bins", [[256, 2, 1, 7, 100, 2, 31, 255, 3], [256]], ids=["f9", "f1"])
def test_segmented_level_records(ext, n_bins, m, min_leaf):
    chunk = int(ext.HRF_SEG_CHUNK)
    bins, bin_off, y, w, node, slot_off, sizes = _level(n_bins, chunk)
    n_feat = len(n_bins)
    m = n_feat if m is None else m
    # slot 2 of tree 0 is node `nid`, where the constant feature ranks first
    nid = next(i for i in range(999) if spec_order(SEED, 7, i, n_feat)[0] == min(FIRST, n_feat - 1))
    meta = np.asarray([[7, 0], [7, 5], [7, nid], [7, 9], [499, 1], [499, 4094]], dtype=np.int32)
    hist = cpu_ref.hrf_hist_cpu(bins, bin_off, y, w, node, slot_off)
    ref = cpu_ref.hrf_split_cpu(hist, bin_off, meta, m, min_leaf, SEED)

    d_bins = _dev(bins)
    seg_off, rows = ext.hrf_seg_build(
        d_bins, _dev(y), _dev(w), _dev(node), _dev(slot_off), len(sizes), int(ref[:, 6].sum())
    )
    np.testing.assert_array_equal(np.diff(seg_off.cpu().numpy()), sizes)
    got = ext.hrf_seg_split(rows, seg_off, d_bins.t().contiguous(), _dev(bin_off), _dev(meta),
                            m, min_leaf, SEED - (1 << 64)).cpu().numpy()
    np.testing.assert_array_equal(got, ref)  # proxy compared by its f64 bits

    assert ref[2, 6] > 9 * 255 and ref[0, 1] == -1  # one row never splits
    if min_leaf > 1000:
        assert (ref[:, 1] == -1).all() and (ref[:, 6] > 0).all()
    elif n_feat > 1 and m == 1:  # rank 0 cannot split: the candidates extend past m
        assert ref[2, 1] >= 0 and ref[2, 1] != FIRST


@pytest.fixture(scope="module")
def cpu_forests():
    # every level dense: the plain level-wise algorithm, continued past level 12
    return {bootstrap: fit_deep("cpu", 16, bootstrap) for bootstrap in (True, False)}


@pytest.mark.parametrize("bootstrap", [True, False])
@pytest.mark.parametrize("dense_levels", [0, 3, 8, 12])
def test_deep_fit_equals_cpu_fit(cpu_forests, dense_levels, bootstrap):
    ref = cpu_forests[bootstrap]
    assert max_tree_depth(ref) > 12
    got = fit_deep("cuda", dense_levels, bootstrap)
    assert got.fit_device_ == "cuda"
    assert_same_forest(got, fit_deep("cpu", dense_levels, bootstrap))
    assert_same_forest(got, ref)

"""forest_anchor_kernel against cpu_ref.forest_anchor_cpu (every composite row
written out and walked on its own) and forest_whatif, bit for bit: a thread
adds exactly one leaf per tree to each mask's f64 sum, in tree order."""

from __future__ import annotations

import numpy as np
import pytest

from _pdp_cases import caterpillar_forest, caterpillar_rows, fit_pipe, pack_pipe
from _shap_models import CATERPILLAR_SPLITS, N_ONEHOT, f32bits, hand_model
from creditcore import anchors as an
from creditcore.engine import ScoringEngine
from creditcore.ops import cpu_ref
from creditcore.pack import N_CAT, N_NUM

pytestmark = pytest.mark.gpu

DEV = 0
N_SRC = N_CAT + N_NUM
FULL = (1 << N_SRC) - 1
CUT = 0.6875  # near the median sum of the three-tree forest's sample rows


@pytest.fixture(scope="module")
def ext():
    from creditcore.ops import gpu

    assert gpu.available(), "HIP extension must be present on a GPU box (no silent CPU fallback)"
    return gpu.ext()


def _forest(n_trees: int):
    """The caterpillar forest (26-split chain over all 23 players, one-node
    tree, categorical tree), cut or extended to n_trees by shifted chains."""
    base = caterpillar_forest()
    off = base.cls_tree_offsets
    trees = [base.cls_nodes[off[i] : off[i + 1]].copy() for i in range(3)]
    for i in range(3, n_trees):
        t = trees[0].copy()
        leaf = t[:, 0] < 0
        t[leaf, 1] = (t[leaf, 1].view(np.float32) + np.float32(i / 32)).view(np.int32)
        trees.append(t)
    trees = trees[:n_trees]
    return hand_model(trees, [np.ones(len(t)) for t in trees])


def _sample(s: int):
    """caterpillar_rows (12, the last with a NaN) resized to s rows."""
    codes, nums = caterpillar_rows()
    pick = np.arange(s) % len(codes)
    codes, nums = codes[pick].copy(), nums[pick].copy()
    nums[12:] += np.random.default_rng(s).normal(0.0, 1.5, size=nums[12:].shape).astype(np.float32)
    return codes, nums


def _launch(ext, p, codes, nums, bg_codes, bg_nums, sat, lists, cut, want_sums=True, chunk=64):
    import torch

    dev = torch.device("cuda", DEV)
    model = (p.cls_nodes, p.cls_tree_offsets, p.feat_col, p.feat_code, p.medians)
    off = np.concatenate([[0], np.cumsum([len(m) for m in lists])]).astype(np.int32)
    masks = np.concatenate(lists).astype(np.uint32)
    up = [torch.from_numpy(np.ascontiguousarray(a)).to(dev)
          for a in (codes, nums, bg_codes, bg_nums) + model + (sat.view(np.int32),)]
    counts, sums = ext.forest_anchor(
        *up, torch.from_numpy(masks.view(np.int32)), torch.from_numpy(off), float(cut), want_sums, chunk
    )
    assert counts.dtype == torch.int32 and tuple(counts.shape) == (len(masks),)
    assert tuple(sums.shape) == (len(masks) if want_sums else 0, len(bg_codes))
    return counts.cpu().numpy(), sums.cpu().numpy(), masks, off


def _check(ext, p, codes, nums, bg_codes, bg_nums, sat, lists, cut, chunk=64):
    """Kernel == forest_anchor_cpu; counts alone (the launcher's own chunk) ==
    counts with sums (jobs of ``chunk`` masks); every mask of one or two
    players == forest_whatif with row i's values, wherever sat replaces all."""
    import torch

    imp, bg_imp = cpu_ref.impute_nums(p, nums), cpu_ref.impute_nums(p, bg_nums)
    counts, sums, masks, off = _launch(
        ext, p, codes, nums, bg_codes, bg_nums, sat, lists, cut, chunk=chunk
    )
    want_c, want_s = cpu_ref.forest_anchor_cpu(
        p, codes, imp, bg_codes, bg_imp, sat, masks, off, cut, want_sums=True
    )
    np.testing.assert_array_equal(sums, want_s)
    np.testing.assert_array_equal(counts, want_c)
    alone = _launch(
        ext, p, codes, nums, bg_codes, bg_nums, sat, lists, cut, want_sums=False, chunk=0
    )[0]
    np.testing.assert_array_equal(alone, want_c)
    dev = torch.device("cuda", DEV)
    model = (p.cls_nodes, p.cls_tree_offsets, p.feat_col, p.feat_code, p.medians)
    row_of = np.repeat(np.arange(len(codes)), np.diff(off))
    jobs, at = [], []
    for m, (mask, i) in enumerate(zip(masks.tolist(), row_of)):
        pls = [pl for pl in range(N_SRC) if (mask >> pl) & 1]
        if 1 <= len(pls) <= 2:
            bits = [int(codes[i, pl]) if pl < N_CAT else f32bits(imp[i, pl - N_CAT]) for pl in pls]
            jobs.append([pls[0], bits[0]] + ([pls[1], bits[1]] if len(pls) == 2 else [-1, 0]))
            at.append(m)
    if jobs:
        whatif = ext.forest_whatif(
            *[torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (bg_codes, bg_nums) + model],
            torch.from_numpy(np.asarray(jobs, dtype=np.int32)),
        ).cpu().numpy()
        for k, m in enumerate(at):
            plain = (sat[row_of[m]] & masks[m]) == 0
            np.testing.assert_array_equal(sums[m, plain], whatif[k, plain])
    return counts, sums


def _lists(n: int, seed: int):
    """n masks (empty, full, singles, pairs, random), none, seven random."""
    rng = np.random.default_rng(seed)
    fixed = [0, FULL] + [1 << pl for pl in range(N_SRC)] + [(1 << 0) | (1 << 12), (1 << 18) | (1 << 3)]
    first = (fixed + rng.integers(0, FULL + 1, size=max(0, n - len(fixed))).tolist())[:n]
    return [np.array(first, dtype=np.uint32), np.empty(0, dtype=np.uint32),
            rng.integers(0, FULL + 1, size=7).astype(np.uint32)]


def _case(s: int):
    """Rows: one that follows the whole chain, the sample's NaN row changed
    elsewhere, and a copy of sample row 5 (its sat word there is full:
    nothing splits); sat from the sample's own quartile edges."""
    bg_codes, bg_nums = _sample(s)
    cat_codes, cat_nums = caterpillar_rows()
    codes = np.stack([cat_codes[0], cat_codes[11], bg_codes[5 % s]])
    nums = np.stack([cat_nums[0], cat_nums[11] + np.float32(0.5), bg_nums[5 % s]])
    assert np.isnan(nums[1]).any()
    return codes, nums, bg_codes, bg_nums


def _sat(p, codes, nums, bg_codes, bg_nums):
    imp, bg_imp = cpu_ref.impute_nums(p, nums), cpu_ref.impute_nums(p, bg_nums)
    edges = an.disc_edges(bg_imp, np.array([25.0, 50.0, 75.0]))
    return an.sat_table(codes, imp, bg_codes, bg_imp, edges)


@pytest.mark.parametrize("n_masks", [1, 64, 65, 92])
@pytest.mark.parametrize("s", [1, 63, 64, 65, 256])
def test_shapes(ext, s, n_masks):
    """Sample rows around the one-wave pass (one block each), masks around the
    64-mask chunk (one chunk, its edge, two chunks), lists of different
    lengths and an empty one in one launch."""
    assert ext.ANCHOR_CHUNK == 64
    p = _forest(3)
    codes, nums, bg_codes, bg_nums = _case(s)
    sat = _sat(p, codes, nums, bg_codes, bg_nums)
    assert sat[2, 5 % s] == FULL
    counts, sums = _check(ext, p, codes, nums, bg_codes, bg_nums, sat, _lists(n_masks, s), CUT)
    if s >= 63 and n_masks >= 64:
        assert len(np.unique(counts)) > 2  # the cut divides the sums
    # the copied sample row: every anchor leaves it as it is
    np.testing.assert_array_equal(sums[n_masks:, 5 % s], np.full(7, sums[0, 5 % s]))


@pytest.mark.parametrize("n_trees", [1, 2, 4, 5])
@pytest.mark.parametrize("chunk", [64, 7])
def test_tree_counts(ext, n_trees, chunk):
    p = _forest(n_trees)
    codes, nums, bg_codes, bg_nums = _case(65)
    sat = _sat(p, codes, nums, bg_codes, bg_nums)
    _check(ext, p, codes, nums, bg_codes, bg_nums, sat, _lists(65, n_trees), 0.75 * n_trees, chunk)


def test_chain_splits_on_every_player(ext):
    """The stack at its limit: the row follows the 26-split chain (column 0
    tested as two one-hot codes, numeric columns 3 and 9 twice), the sample
    row leaves it at the first test of every player, sat is empty, and mask k
    pins the first k players of the chain: at each of the 23 first tests both
    sides are alive, so 23 leaves wait on the stack while the walk goes on."""
    p = _forest(1)
    cat_codes, cat_nums = caterpillar_rows()
    codes, nums = cat_codes[:1], cat_nums[:1]
    order, b_codes, b_nums = [], codes.copy(), nums.copy()
    for feat, thr in CATERPILLAR_SPLITS:
        pl = feat // 2 if feat < N_ONEHOT else N_CAT + feat - N_ONEHOT
        if pl in order:
            continue
        order.append(pl)
        if pl < N_CAT:
            b_codes[0, pl] = 0 if codes[0, pl] != 0 else 1
        else:
            b_nums[0, pl - N_CAT] = thr + 10.0 if nums[0, pl - N_CAT] <= thr else thr - 10.0
    assert sorted(order) == list(range(N_SRC))
    prefix = np.cumsum([0] + [1 << pl for pl in order]).astype(np.uint32)  # 24 masks
    sat = np.zeros((1, 1), dtype=np.uint32)
    _, sums = _check(ext, p, codes, nums, b_codes, b_nums, sat, [prefix], 0.5)
    assert len(np.unique(sums)) == len(prefix)  # 24 different leaves


@pytest.fixture(scope="module")
def detectors(train_df):
    from creditcore.train import fit_detectors

    return fit_detectors(train_df)


@pytest.mark.parametrize("family", ["rf", "hgbt"])
def test_families_and_engine(ext, train_df, detectors, family, monkeypatch):
    from creditcore.counterfactual import raw_cut

    p = pack_pipe(fit_pipe(train_df, family), detectors)
    rng = np.random.default_rng(3)
    pick = rng.integers(0, len(p.bg_codes), size=6)
    codes, nums = p.bg_codes[pick].copy(), p.bg_nums[pick].copy()
    nums[rng.uniform(size=nums.shape) < 0.1] = np.nan
    codes[2, 4] = -1
    sat = _sat(p, codes, nums, p.bg_codes, p.bg_nums)
    lists = [rng.integers(0, FULL + 1, size=n).astype(np.uint32) for n in (92, 0, 23, 1, 64, 65)]
    lists[2] = np.array([1 << pl for pl in range(N_SRC)], dtype=np.uint32)
    counts, _ = _check(ext, p, codes, nums, p.bg_codes, p.bg_nums, sat, lists, raw_cut(p, 0.5))
    assert len(np.unique(counts)) > 1
    # the engine on CUDA equals the CPU engine, one launch per level or sliced
    gpu_eng = ScoringEngine(p, device="cuda", device_index=DEV)
    kw = {"precision_threshold": 0.9, "beam_size": 3, "max_anchor_size": 3}
    want = ScoringEngine(p, device="cpu").anchors(codes, nums, **kw)
    assert gpu_eng.anchors(codes, nums, **kw) == want
    monkeypatch.setattr(ScoringEngine, "ANCHOR_LAUNCH_PAIRS", 40 * len(p.bg_codes))
    assert gpu_eng.anchors(codes, nums, **kw) == want


def test_host_checks(ext):
    p = _forest(3)
    codes, nums, bg_codes, bg_nums = _case(12)
    sat = _sat(p, codes, nums, bg_codes, bg_nums)
    good = _lists(5, 0)
    for lists, table, match in (
        ([good[0]], sat, "mask_off must have"),
        (good[:2] + [np.array([1 << N_SRC], dtype=np.uint32)], sat, r"masks\[5\]"),
        (good, np.ascontiguousarray(sat[:, :-1]), "sat must be"),
    ):
        with pytest.raises(RuntimeError, match=match):
            _launch(ext, p, codes, nums, bg_codes, bg_nums, table, lists, 0.5)

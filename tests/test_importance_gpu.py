"""forest_permute_kernel against cpu_ref.forest_permute_cpu and
forest_whatif_cpu, bit for bit: one thread adds a row's f32 leaves to its f64
sums in tree order, as the reference does, and every compare on the way is the
same f32 compare on the same (imputed) donor value."""

from __future__ import annotations

import numpy as np
import pytest

from _pdp_cases import FAMILY_PARAMS, caterpillar_forest, caterpillar_rows, fit_pipe, pack_pipe
from _shap_models import N_ONEHOT, f32bits, hand_model
from creditcore import importance
from creditcore.engine import ScoringEngine
from creditcore.ops import cpu_ref
from creditcore.pack import N_CAT, N_NUM

pytestmark = pytest.mark.gpu

DEV = 0
UNTESTED = 13  # the numeric column _forest takes out of every tree


@pytest.fixture(scope="module")
def ext():
    from creditcore.ops import gpu

    assert gpu.available(), "HIP extension must be present on a GPU box (no silent CPU fallback)"
    return gpu.ext()


def _forest(n_trees: int = 3, cls_kind: int = 0, bias: float = 0.0):
    """The caterpillar forest (caterpillar, one-node tree, categorical tree)
    with the caterpillar's test of numeric column 13 moved to column 12, cut
    or extended to n_trees by caterpillars with shifted leaves."""
    base = caterpillar_forest(cls_kind, bias)
    off = base.cls_tree_offsets
    trees = [base.cls_nodes[off[i] : off[i + 1]].copy() for i in range(3)]
    trees[0][trees[0][:, 0] == N_ONEHOT + UNTESTED, 0] = N_ONEHOT + UNTESTED - 1
    for i in range(3, n_trees):
        t = trees[0].copy()
        leaf = t[:, 0] < 0
        t[leaf, 1] = (t[leaf, 1].view(np.float32) + np.float32(i / 32)).view(np.int32)
        trees.append(t)
    trees = trees[:n_trees]
    return hand_model(trees, [np.ones(len(t)) for t in trees], cls_kind=cls_kind, cls_bias=bias)


def _rows(r: int):
    """caterpillar_rows (12 rows, the last with a NaN in numeric column 2)
    resized to r rows, with random numerics past the first 12."""
    codes, nums = caterpillar_rows()
    pick = np.arange(r) % len(codes)
    codes, nums = codes[pick].copy(), nums[pick].copy()
    rng = np.random.default_rng(r)
    nums[12:] += rng.normal(0.0, 1.5, size=nums[12:].shape).astype(np.float32)
    return codes, nums


def _permute(ext, p, codes, nums, players, perm, **kw):
    import torch

    dev = torch.device("cuda", DEV)
    model = (p.cls_nodes, p.cls_tree_offsets, p.feat_col, p.feat_code, p.medians)
    out = ext.forest_permute(
        *[torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (codes, nums) + model],
        torch.from_numpy(np.ascontiguousarray(players)),
        torch.from_numpy(np.ascontiguousarray(perm)), **kw,
    )
    assert out.dtype == torch.float64 and tuple(out.shape) == (len(players), len(codes))
    return out.cpu().numpy()


def _check(ext, p, codes, nums, players, perm, picks, **kw):
    """Kernel == forest_permute_cpu, and at the picked (q, r) == the what-if
    of row r with the donor's value as the one override."""
    players = np.asarray(players, dtype=np.int32)
    perm = np.asarray(perm, dtype=np.int32)
    imp = cpu_ref.impute_nums(p, nums)
    got = _permute(ext, p, codes, nums, players, perm, **kw)
    np.testing.assert_array_equal(got, cpu_ref.forest_permute_cpu(p, codes, imp, players, perm))
    for q, r in picks:
        pl, d = int(players[q]), int(perm[q, r])
        bits = int(codes[d, pl]) if pl < N_CAT else f32bits(imp[d, pl - N_CAT])
        job = np.array([[pl, bits, -1, 0]], dtype=np.int32)
        assert got[q, r] == cpu_ref.forest_whatif_cpu(p, codes[r : r + 1], imp[r : r + 1], job)[0, 0]
    return got


def _table(r: int, runs, seed: int = 0):
    """(perm_player, perm) of random permutations: ``runs`` is [(player, n)]."""
    rng = np.random.default_rng(seed)
    players = np.repeat([pl for pl, _ in runs], [n for _, n in runs]).astype(np.int32)
    return players, np.stack([rng.permutation(r) for _ in players]).astype(np.int32)


@pytest.mark.parametrize("cls_kind, bias", [(0, 0.0), (1, -0.75)])
def test_hand_built_forest(ext, cls_kind, bias):
    p = _forest(3, cls_kind, bias)
    codes, nums = _rows(12)
    assert np.isnan(nums[11, 2]) and 1 in np.diff(p.cls_tree_offsets)
    ident, rev = np.arange(12), np.arange(12)[::-1]
    # column 3 (tested at -0.75 and again at 1.5): identity, reversal, random;
    # column 2: row 0 receives the NaN row's value; categorical column 0;
    # column 13, which no tree tests, five times (a full job and one of 1)
    players, perm = _table(12, [(N_CAT + 3, 3), (N_CAT + 2, 1), (0, 2), (N_CAT + UNTESTED, 5)])
    perm[0], perm[1], perm[3] = ident, rev, rev
    picks = [(1, 0), (1, 4), (2, 7), (3, 0), (3, 11), (4, 2), (5, 9), (8, 3)]
    got = _check(ext, p, codes, nums, players, perm, picks)
    base = cpu_ref.forest_raw_cpu(p, codes, cpu_ref.impute_nums(p, nums), tree_order=True)
    np.testing.assert_array_equal(got[0], base)
    assert (got[1:3] != base).any() and (got[4:6] != base).any()
    np.testing.assert_array_equal(got[6:], np.tile(base, (5, 1)))
    # the NaN donor gives the median: row 0 of table row 3 is the what-if at it
    job = np.array([[N_CAT + 2, f32bits(p.medians[2]), -1, 0]], dtype=np.int32)
    imp = cpu_ref.impute_nums(p, nums)
    assert got[3, 0] == cpu_ref.forest_whatif_cpu(p, codes[:1], imp[:1], job)[0, 0]


@pytest.mark.parametrize("block_target", [8192, 1])
@pytest.mark.parametrize("reps", [1, 4, 5])
@pytest.mark.parametrize("n_trees", [1, 4, 5])
@pytest.mark.parametrize("r", [1, 63, 64, 65, 130])
def test_shapes(ext, r, n_trees, reps, block_target):
    """Rows around the one-wave block (donors lie in other blocks), repeats
    around the PERM_ILP table rows of a job, block_target=1: one block per row
    block strides over all jobs."""
    assert ext.PERM_ROWS_PER_BLOCK == 64 and ext.PERM_ILP == importance.PERM_ILP == 4
    codes, nums = _rows(r)
    players, perm = _table(r, [(N_CAT + 3, reps), (0, reps), (N_CAT + 9, reps)], seed=r)
    picks = [(0, 0), (len(players) - 1, r - 1), (reps, r // 2)]
    _check(ext, _forest(n_trees), codes, nums, players, perm, picks, block_target=block_target)


@pytest.fixture(scope="module")
def detectors(train_df):
    from creditcore.train import fit_detectors

    return fit_detectors(train_df)


@pytest.mark.parametrize("family", list(FAMILY_PARAMS))
def test_families_and_engine(ext, train_df, detectors, family, monkeypatch):
    p = pack_pipe(fit_pipe(train_df, family), detectors)
    rng = np.random.default_rng(3)
    pick = rng.integers(0, len(p.bg_codes), size=130)
    codes, nums = p.bg_codes[pick].copy(), p.bg_nums[pick].copy()
    nums[rng.uniform(size=nums.shape) < 0.03] = np.nan
    players, perm = _table(130, [(pl, 2) for pl in range(N_CAT + N_NUM)], seed=5)
    got = _check(ext, p, codes, nums, players, perm, [(0, 0), (17, 64), (30, 129), (45, 77)])
    base = cpu_ref.forest_raw_cpu(p, codes, cpu_ref.impute_nums(p, nums), tree_order=True)
    assert (got != base).any()
    # the engine on CUDA equals the CPU engine, sliced in mid-feature or not
    labels = rng.integers(0, 2, size=130)
    gpu_eng = ScoringEngine(p, device="cuda", device_index=DEV)
    cpu_eng = ScoringEngine(p, device="cpu")
    for scoring in importance.SCORINGS:
        want = cpu_eng.permutation_importance((codes, nums), labels, scoring=scoring, seed=7)
        for pairs in (None, 130 * 3, 130 * 7 + 5):
            if pairs:
                monkeypatch.setattr(ScoringEngine, "PERM_LAUNCH_PAIRS", pairs)
            res = gpu_eng.permutation_importance((codes, nums), labels, scoring=scoring, seed=7)
            monkeypatch.undo()
            assert res["baseline_score"] == want["baseline_score"]
            for ra, rb in zip(res["results"], want["results"]):
                np.testing.assert_array_equal(ra["importances"], rb["importances"])


def test_host_checks(ext):
    p = _forest()
    codes, nums = _rows(12)
    players, perm = _table(12, [(N_CAT + 3, 2), (0, 1)])
    bad_player, bad_donor = players.copy(), perm.copy()
    bad_player[1], bad_donor[2, 5] = N_CAT + N_NUM, 12
    for bad, match in (
        ((players.astype(np.int64), perm), "perm_player"),
        ((players, perm.astype(np.int64)), "perm must"),
        ((bad_player, perm), r"perm_player\[1\]"),
        ((players, bad_donor), "perm row 2"),
        ((players, perm[:, :-1]), r"perm must be \[3, 12\]"),
    ):
        with pytest.raises(RuntimeError, match=match):
            _permute(ext, p, codes, nums, *bad)

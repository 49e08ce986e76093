"""forest_ale_kernel against cpu_ref.forest_ale_cpu and forest_whatif_cpu, bit
for bit: one thread adds a pair's f32 leaves to its f64 sums in tree order, as
the reference does, and every compare on the way is the same f32 compare."""

from __future__ import annotations

import numpy as np
import pytest

from _pdp_cases import FAMILY_PARAMS, caterpillar_forest, caterpillar_rows, fit_pipe, pack_pipe, up
from _shap_models import f32bits, hand_model
from creditcore import ale
from creditcore.engine import ScoringEngine
from creditcore.ops import cpu_ref
from creditcore.pack import N_CAT, N_NUM

pytestmark = pytest.mark.gpu

DEV = 0
# column 3 of the caterpillar is tested at -0.75 and, further down, at 1.5
T0, T1 = np.float32(-0.75), np.float32(1.5)
ENTRIES = [
    (3, [-3.0, 2.0]),  # Ke = 1; [lo, hi) holds both thresholds
    (3, [-2.0, T0, up(T0), 0.0, T1, up(T1), 2.5]),  # an edge on a threshold, one f32 above
    (9, [-2.5, -2.0, 0.75, 1.0]),  # its thresholds: 0.75 and -2.0
    (2, [-1.0, -0.7, -0.5, 0.0]),  # the last row holds NaN here: median -0.692
    (3, np.linspace(-3.0, 3.0, 101)),  # Ke = 100, the same column a third time
]


@pytest.fixture(scope="module")
def ext():
    from creditcore.ops import gpu

    assert gpu.available(), "HIP extension must be present on a GPU box (no silent CPU fallback)"
    return gpu.ext()


def _tables(entries):
    players = np.array([N_CAT + c for c, _ in entries], dtype=np.int32)
    off, z = ale.edge_table([np.asarray(e, dtype=np.float32) for _, e in entries])
    return players, off, z


def _ale(ext, p, codes, nums, players, off, z, **kw):
    import torch

    dev = torch.device("cuda", DEV)
    model = (p.cls_nodes, p.cls_tree_offsets, p.feat_col, p.feat_code, p.medians)
    interval, sums = ext.forest_ale(
        *[torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (codes, nums) + model],
        *[torch.from_numpy(np.ascontiguousarray(a)) for a in (players, off, z)], **kw,
    )
    assert interval.dtype == torch.int32 and sums.dtype == torch.float64
    assert tuple(sums.shape) == (len(players), len(codes), 2)
    return interval.cpu().numpy(), sums.cpu().numpy()


def _check(ext, p, codes, nums, entries, **kw):
    """Kernel == forest_ale_cpu, and its sums == forest_whatif_cpu at every
    edge, picked per row by an interval computed here."""
    players, off, z = _tables(entries)
    imp = cpu_ref.impute_nums(p, nums)
    interval, sums = _ale(ext, p, codes, nums, players, off, z, **kw)
    ref_interval, ref_sums = cpu_ref.forest_ale_cpu(p, codes, imp, players, off, z)
    np.testing.assert_array_equal(interval, ref_interval)
    np.testing.assert_array_equal(sums, ref_sums)
    rows = np.arange(len(codes))
    for e, (col, edges) in enumerate(entries):
        zz = np.asarray(edges, dtype=np.float32)
        k = np.clip(np.searchsorted(zz, imp[:, col], side="left"), 1, len(zz) - 1)
        jobs = np.array([[N_CAT + col, f32bits(v), -1, 0] for v in zz], dtype=np.int32)
        at_edges = cpu_ref.forest_whatif_cpu(p, codes, imp, jobs)  # [Ke + 1, R]
        np.testing.assert_array_equal(interval[e], k)
        np.testing.assert_array_equal(sums[e, :, 0], at_edges[k - 1, rows])
        np.testing.assert_array_equal(sums[e, :, 1], at_edges[k, rows])
    return interval, sums


def _rows(r: int):
    """caterpillar_rows plus rows on an edge, below z[0], above z[Ke] and one
    f32 above a threshold (ENTRIES[1]), resized to r rows with random numerics
    past the first 16."""
    codes, nums = caterpillar_rows()
    extra = np.repeat(nums[:1], 4, axis=0)
    extra[:, 3] = [T0, -5.0, 10.0, up(T0)]
    codes, nums = np.concatenate([codes, codes[:4]]), np.concatenate([nums, extra])
    rng = np.random.default_rng(r)
    pick = np.arange(r) % len(codes)
    codes, nums = codes[pick].copy(), nums[pick].copy()
    nums[16:] += rng.normal(0.0, 1.5, size=nums[16:].shape).astype(np.float32)
    return codes, nums


def _forest(n_trees: int, cls_kind: int = 0, bias: float = 0.0):
    """The caterpillar forest (3 trees) extended by caterpillars whose leaves
    are shifted, so that no two trees add the same values."""
    base = caterpillar_forest(cls_kind, bias)
    off = base.cls_tree_offsets
    trees = [base.cls_nodes[off[i] : off[i + 1]].copy() for i in range(3)]
    for i in range(3, n_trees):
        t = trees[0].copy()
        leaf = t[:, 0] < 0
        t[leaf, 1] = (t[leaf, 1].view(np.float32) + np.float32(i / 32)).view(np.int32)
        trees.append(t)
    trees = trees[:n_trees]
    return hand_model(trees, [np.ones(len(t)) for t in trees], cls_kind=cls_kind, cls_bias=bias)


@pytest.mark.parametrize("cls_kind, bias", [(0, 0.0), (1, -0.75)])
def test_hand_built_forest(ext, cls_kind, bias):
    p = caterpillar_forest(cls_kind, bias)
    codes, nums = _rows(16)
    assert np.isnan(nums[11, 2]) and 1 in np.diff(p.cls_tree_offsets)
    interval, sums = _check(ext, p, codes, nums, ENTRIES)
    # forks happen (both thresholds, one, at one f32's width) and do not (none)
    assert (sums[0, :, 0] != sums[0, :, 1]).any()
    k = interval[1]
    assert {1, 2, 3, 6} <= set(k.tolist())
    assert (sums[1, k == 2, 0] != sums[1, k == 2, 1]).any()  # (T0, up(T0)]
    assert (sums[1, k == 3, 0] == sums[1, k == 3, 1]).all()  # (up(T0), 0]
    # on an edge -> the interval it closes; outside -> clamped; NaN -> the median's
    assert k[12:16].tolist() == [1, 1, 6, 2] and interval[3, 11] == 2


@pytest.mark.parametrize("block_target", [8192, 1])
@pytest.mark.parametrize("n_trees", [1, 4, 5])
@pytest.mark.parametrize("r", [1, 63, 64, 65, 130])
def test_shapes(ext, r, n_trees, block_target):
    """Rows around the one-wave block, tree counts around the four trees in
    flight, entries of Ke = 1 to 100 in one launch (block_target=1: a single
    block strides over all of them)."""
    assert ext.ALE_ROWS_PER_BLOCK == 64
    codes, nums = _rows(r)
    _check(ext, _forest(n_trees), codes, nums, ENTRIES, block_target=block_target)


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
    imp = cpu_ref.impute_nums(p, nums)
    entries = [(c, ale.quantile_edges(imp[:, c], 20)) for c in range(N_NUM)]
    entries = [(c, z) for c, z in entries if len(z) > 1]
    _, sums = _check(ext, p, codes, nums, entries)
    assert (sums[:, :, 0] != sums[:, :, 1]).any()
    # the engine on CUDA equals the CPU engine, sliced or not
    from creditcore.schema import NUMERIC_FEATURES

    gpu_eng = ScoringEngine(p, device="cuda", device_index=DEV)
    cpu_eng = ScoringEngine(p, device="cpu")
    for smp in ((codes, nums), None):
        want = cpu_eng.accumulated_local_effects(list(NUMERIC_FEATURES), sample=smp, kind="both")
        for jobs in (None, 100, 3 * len(want["results"][0]["interval"]) + 5):
            if jobs:
                monkeypatch.setattr(ScoringEngine, "ALE_LAUNCH_JOBS", jobs)
            got = gpu_eng.accumulated_local_effects(list(NUMERIC_FEATURES), sample=smp, kind="both")
            monkeypatch.undo()
            for ra, rb in zip(got["results"], want["results"]):
                assert ra["edges"] == rb["edges"]
                for key in ("ale", "counts", "interval", "local_effect"):
                    np.testing.assert_array_equal(ra[key], rb[key])


def test_host_checks(ext):
    p = caterpillar_forest()
    codes, nums = _rows(16)
    players, off, z = _tables(ENTRIES[:2])
    for bad, match in (
        ((np.array([3, N_CAT + 3], np.int32), off, z), "numeric"),
        ((players, off[[0, 2, 1]].copy(), z), "edge_off"),  # unsorted
        ((players, off, z[::-1].copy()), "ascending"),
        ((players.astype(np.int64), off, z), "players"),
        ((players, off, z.astype(np.float64)), "edges"),
    ):
        with pytest.raises(RuntimeError, match=match):
            _ale(ext, p, codes, nums, *bad)

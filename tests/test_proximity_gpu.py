"""forest_leaf_kernel against a one-loop-per-(row, tree) walker,
forest_prox_topk_kernel against the definition (cpu_ref.forest_prox_topk_cpu)
on leaf tables drawn directly, and a GPU engine against a CPU engine. Counts
are integers: every comparison is exact."""

from __future__ import annotations

import numpy as np
import pytest

from _forest_cases import RAGGED_EVEN, RAGGED_ODD, edge_model, edge_rows, ragged_model, ragged_rows
from creditcore.ops import cpu_ref

pytestmark = pytest.mark.gpu


def naive_leaves(p, codes, nums) -> np.ndarray:
    """_forest_cases.naive_sums returning the node index of the leaf."""
    off = p.cls_tree_offsets.tolist()
    nodes, thr = p.cls_nodes.tolist(), p.cls_nodes[:, 1].view(np.float32).tolist()
    col, code = p.feat_col.tolist(), p.feat_code.tolist()
    x = np.where(np.isnan(nums), p.medians[None, :], nums).astype(np.float32).tolist()
    c = np.asarray(codes).tolist()
    out = np.zeros((len(x), len(off) - 1), dtype=np.int32)
    for r in range(len(x)):
        for t in range(len(off) - 1):
            k = off[t]
            while nodes[k][0] >= 0:
                f = nodes[k][0]
                v = x[r][col[f]] if code[f] < 0 else (1.0 if c[r][col[f]] == code[f] else 0.0)
                k = off[t] + (nodes[k][2] if v <= thr[k] else nodes[k][3])
            out[r, t] = k
    return out


@pytest.fixture(scope="module")
def leaf_cases():
    """name -> (model, codes, nums, naive leaves) of at most 65 rows."""
    cases = {}
    for name, p, (codes, nums) in (
        ("ragged_odd", ragged_model(RAGGED_ODD), ragged_rows()),
        ("ragged_even", ragged_model(RAGGED_EVEN), ragged_rows()),
        ("edges", edge_model(), edge_rows()),
    ):
        cases[name] = (p, codes[:65], nums[:65], naive_leaves(p, codes[:65], nums[:65]))
    return cases


@pytest.mark.parametrize("block_target", [1, 3, 2048])  # one chunk, ragged chunks, one group each
@pytest.mark.parametrize("rows", [1, 64, 65])
@pytest.mark.parametrize("name", ["ragged_odd", "ragged_even", "edges"])
def test_leaf_kernel_matches_naive_walker(leaf_cases, name, rows, block_target):
    import torch

    from creditcore.ops import gpu

    p, codes, nums, want = leaf_cases[name]
    rows = min(rows, len(codes))
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()  # noqa: E731
    got = gpu.ext().forest_leaves(
        dev(codes[:rows], np.int16), dev(nums[:rows], np.float32), dev(p.cls_nodes, np.int32),
        dev(p.cls_tree_offsets, np.int32), dev(p.feat_col, np.int32), dev(p.feat_code, np.int32),
        dev(p.medians, np.float32), block_target).cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got, want[:rows])
    imp = cpu_ref.impute_nums(p, nums[:rows])
    assert np.array_equal(cpu_ref.forest_leaves_cpu(p, codes[:rows], imp), want[:rows])


@pytest.mark.parametrize(
    "b,m,t,k,n_leaves,loo,launch_rows",
    [
        (3, 2, 1, 1, 2, False, 0),  # M = k + 1 at k = 1, T = 1
        (65, 33, 5, 32, 3, False, 0),  # M = k + 1 at k = 32, odd M: half a pair
        (7, 65, 5, 10, 1, False, 0),  # one leaf: every count is T, order is pure j
        (5, 257, 3, 32, 100000, False, 0),  # almost every count 0: the zero fill
        (4, 16384, 3, 32, 4, False, 0),  # the full counter array, 14-bit j, long lists
        (3, 65, 4096, 10, 2, False, 0),  # the tree cap: 4097 bins, 65 scan steps
        (65, 65, 9, 10, 4, True, 0),  # leave-one-out with duplicated rows
        (130, 130, 65, 32, 8, True, 64),  # ... over three launches, T past 64
        (65, 130, 257, 10, 16, False, 64),  # two launches over the batch rows
    ],
)
def test_prox_topk_kernel_matches_definition(b, m, t, k, n_leaves, loo, launch_rows):
    import torch

    from creditcore.ops import gpu

    rng = np.random.default_rng(1000 * m + t + k)
    base = (np.arange(t) * n_leaves).astype(np.int32)  # tree t owns its own node ids
    leaf_ref = rng.integers(0, n_leaves, (m, t)).astype(np.int32) + base
    leaf_ref[m // 2] = leaf_ref[0]  # duplicates: count T off the diagonal
    leaf_ref[m - 1] = leaf_ref[0]
    leaf_b = leaf_ref if loo else rng.integers(0, n_leaves, (b, t)).astype(np.int32) + base
    if not loo:
        leaf_b[0, ::2] = -1  # trees the leaf kernel skipped are never counted
    want_count, want_idx = cpu_ref.forest_prox_topk_cpu(leaf_b, leaf_ref, k, exclude_self=loo)
    ref_d = torch.from_numpy(leaf_ref).cuda()
    index = gpu.prox_index(ref_d, t * n_leaves)
    batch_d = ref_d if loo else torch.from_numpy(leaf_b).cuda()
    got = {lanes: gpu.forest_prox_topk(batch_d, index, k, loo, lanes, launch_rows)
           for lanes in (0, 1, 8, 64)}  # the index's own width and three fixed ones
    for count, idx in got.values():
        assert count.dtype == np.int32 and idx.dtype == np.int32 and count.shape == (len(leaf_b), k)
        assert np.array_equal(count, want_count) and np.array_equal(idx, want_idx)


@pytest.mark.parametrize("score", ["kth", "mean"])
def test_engine_gpu_vs_cpu(packed, score_batch, score):
    from creditcore.engine import ScoringEngine
    from creditcore.pack import encode_batch

    codes, nums = encode_batch(score_batch, packed.vocabs)
    want = ScoringEngine(packed, device="cpu").proximity(codes, nums, score=score)
    gpu_eng = ScoringEngine(packed, device="cuda")
    gpu_eng.PROX_LAUNCH_ROWS = 200  # three launches over the 512 rows
    got = gpu_eng.proximity(codes, nums, score=score)
    assert set(got) == set(want)
    for key, w in want.items():
        assert np.array_equal(got[key], w), key
        assert not isinstance(w, np.ndarray) or got[key].dtype == w.dtype, key
    assert 0 < want["is_outlier"].sum() < len(codes)

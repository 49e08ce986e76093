"""GPU partial dependence — forest_whatif_kernel (csrc/creditcore_kernels.hip)
against cpu_ref.forest_whatif_cpu. Run on a real MI355X (`pytest -m gpu`).

The comparison is exact (bit for bit), which is tighter than the project's
1e-9 bound on forest sums: the kernel uses no atomics, one thread owns every
tree of a (job, row) and adds the f32 leaves to its f64 sum in tree order, and
the reference adds the same values in the same order. Every compare on the
way is the same f32 compare."""

from __future__ import annotations

import numpy as np
import pytest

from _pdp_cases import (
    ENTRIES,
    FAMILY_PARAMS,
    caterpillar_forest,
    caterpillar_jobs,
    caterpillar_rows,
    fit_pipe,
    pack_pipe,
    random_jobs,
    sample_frame,
)
from creditcore.engine import ScoringEngine
from creditcore.ops import cpu_ref
from creditcore.pack import N_CAT, N_NUM, encode_batch

pytestmark = pytest.mark.gpu

DEV = 0


@pytest.fixture(scope="module")
def ext():
    from creditcore.ops import gpu

    assert gpu.available(), (
        "HIP extension must be present on a GPU box (no silent CPU fallback)"
    )
    return gpu.ext()


def _whatif(ext, p, codes, nums, jobs, **kw):
    import torch

    dev = torch.device("cuda", DEV)

    def up(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)

    out = ext.forest_whatif(
        up(codes, np.int16), up(nums, np.float32), up(p.cls_nodes, np.int32),
        up(p.cls_tree_offsets, np.int32), up(p.feat_col, np.int32), up(p.feat_code, np.int32),
        up(p.medians, np.float32),
        torch.from_numpy(np.ascontiguousarray(jobs, dtype=np.int32)), **kw,
    )
    assert out.dtype == torch.float64 and tuple(out.shape) == (len(jobs), len(codes))
    return out.cpu().numpy()


def _ref(p, codes, nums, jobs):
    return cpu_ref.forest_whatif_cpu(p, codes, cpu_ref.impute_nums(p, nums), jobs)


# ------------------------------------------------------- 7. hand-built forests


@pytest.mark.parametrize("cls_kind, bias", [(0, 0.0), (1, -0.75)])
def test_hand_built_forest(ext, cls_kind, bias):
    """The caterpillar (both one-hot features of column 0; two thresholds on
    numeric columns 3 and 9) next to a single-leaf tree: category codes 0, 1
    and -1, values on a threshold and one f32 above it, +-1e30, two-way jobs
    mixing a categorical and a numeric player, and a job on the column whose
    own value is NaN in the last row."""
    p = caterpillar_forest(cls_kind, bias)
    codes, nums = caterpillar_rows()
    assert np.isnan(nums[-1, 2]) and 1 in np.diff(p.cls_tree_offsets)
    jobs = caterpillar_jobs()
    got = _whatif(ext, p, codes, nums, jobs)
    ref = _ref(p, codes, nums, jobs)
    np.testing.assert_array_equal(got, ref)
    # the edges do what they are there for: a value on a threshold and the
    # next f32 above it end in different leaves for some row (the second
    # threshold of column 3 lies behind the first, which such a value fails)
    edge_pairs = [
        j for j in range(len(jobs) - 1)
        if jobs[j][0] == jobs[j + 1][0] >= N_CAT and jobs[j][2] == jobs[j + 1][2] == -1
        and abs(int(jobs[j][1]) - int(jobs[j + 1][1])) == 1
    ]
    assert len(edge_pairs) == 4
    assert sum(bool((ref[j] != ref[j + 1]).any()) for j in edge_pairs) == 3
    assert len({tuple(r) for r in ref[:3]}) == 3  # codes a, b, unknown all differ
    # the NaN cell takes the job's value, not the median
    k = len(jobs) - 2
    assert jobs[k][0] == N_CAT + 2
    x = cpu_ref.impute_nums(p, nums)
    x[:, 2] = 0.5
    np.testing.assert_array_equal(got[k], cpu_ref.forest_raw_cpu(p, codes, x, tree_order=True))
    # the engine finalises with the bias / the tree count
    eng = ScoringEngine(p, device="cuda", device_index=DEV)
    cpu = ScoringEngine(p, device="cpu")
    kw = dict(sample=(codes, nums), kind="both", grid={"bill_amount_2": [-1e30, 1.5, 1e30]})
    for response in ("probability",) + (("raw",) if cls_kind else ()):
        a = eng.partial_dependence(["sex", ("bill_amount_2", "sex")], response=response, **kw)
        b = cpu.partial_dependence(["sex", ("bill_amount_2", "sex")], response=response, **kw)
        for ra, rb in zip(a["results"], b["results"]):
            np.testing.assert_array_equal(ra["individual"], rb["individual"])
            np.testing.assert_array_equal(ra["average"], rb["average"])


def test_host_checks(ext):
    p = caterpillar_forest()
    codes, nums = caterpillar_rows()
    for bad, match in (
        ([[23, 0, -1, 0]], "player0"),
        ([[-1, 0, -1, 0]], "player0"),
        ([[3, 0, 23, 0]], "player1"),
        ([[3, 0, -2, 0]], "player1"),
        ([[3, 0, 3, 1]], "differ"),
        ([[3, 40000, -1, 0]], "int16"),
        (np.zeros((0, 4), dtype=np.int32), "at least one job"),
    ):
        with pytest.raises(RuntimeError, match=match):
            _whatif(ext, p, codes, nums, np.asarray(bad, dtype=np.int32).reshape(-1, 4))
    with pytest.raises(RuntimeError, match="at least one sample row"):
        _whatif(ext, p, codes[:0], nums[:0], caterpillar_jobs())
    import torch

    with pytest.raises(RuntimeError, match="host int32"):
        dev = torch.device("cuda", DEV)
        ext.forest_whatif(
            *[torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (
                codes, nums, p.cls_nodes, p.cls_tree_offsets, p.feat_col, p.feat_code, p.medians
            )],
            torch.from_numpy(caterpillar_jobs()).to(dev),
        )


# ------------------------------------------------------------------- 8. shapes


@pytest.fixture(scope="module")
def detectors(train_df):
    from creditcore.train import fit_detectors

    return fit_detectors(train_df)


@pytest.fixture(scope="module")
def trained(train_df, detectors):
    """20-tree rf (sklearn) and hgbt (trained on the GPU), packed."""
    hgbt = {**FAMILY_PARAMS["hgbt"], "device": "cuda"}
    pipes = {"rf": fit_pipe(train_df, "rf"), "hgbt": fit_pipe(train_df, "hgbt", hgbt)}
    assert pipes["hgbt"].named_steps["classifier"].fit_device_ == "cuda"
    return {k: pack_pipe(v, detectors) for k, v in pipes.items()}


def _rows(p, n: int, seed: int):
    """Rows resized from the packed sample, with NaNs and unknown categories."""
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, len(p.bg_codes), size=n)
    codes, nums = p.bg_codes[pick].copy(), p.bg_nums[pick].copy()
    nums[rng.uniform(size=nums.shape) < 0.03] = np.nan
    codes[rng.uniform(size=codes.shape) < 0.03] = -1
    return codes, nums


@pytest.mark.parametrize("family", ["rf", "hgbt"])
@pytest.mark.parametrize("r", [1, 255, 256, 257])
def test_row_shapes(ext, trained, family, r):
    """One row, a partly filled last wave, exact blocks and one row past
    them (the kernel stages 64 rows per block)."""
    p = trained[family]
    assert p.cls_n_trees == 20 and ext.WHATIF_ROWS_PER_BLOCK == 64
    codes, nums = _rows(p, r, seed=r)
    jobs = random_jobs(p, 33, seed=100 + r)
    got = _whatif(ext, p, codes, nums, jobs)
    ref = _ref(p, codes, nums, jobs)
    assert np.ptp(ref) > 1e-3
    np.testing.assert_array_equal(got, ref)


@pytest.mark.parametrize("family", ["rf", "hgbt"])
@pytest.mark.parametrize("j, block_target", [(1, 8192), (2, 8192), (33, 8192), (33, 8), (70, 3), (257, 1)])
def test_job_shapes(ext, trained, family, j, block_target):
    """One job, two, 33, and grids in which a block strides over several
    jobs: block_target caps the grid at ceil(block_target / row blocks) job
    chunks (3 row blocks here), down to one block walking all 257 jobs, each
    after restoring the columns the job before it overrode."""
    p = trained[family]
    codes, nums = _rows(p, 130, seed=j)
    jobs = random_jobs(p, j, seed=200 + j)
    got = _whatif(ext, p, codes, nums, jobs, block_target=block_target)
    np.testing.assert_array_equal(got, _ref(p, codes, nums, jobs))


# ------------------------------------------------------------------- 9. engine


def test_engine_equals_cpu_engine(trained, train_df, monkeypatch):
    df = sample_frame(train_df)
    for family, p in trained.items():
        gpu_eng = ScoringEngine(p, device="cuda", device_index=DEV)
        cpu_eng = ScoringEngine(p, device="cpu")
        sample = encode_batch(df, p.vocabs)
        responses = ("probability", "raw") if family == "hgbt" else ("probability",)
        for response in responses:
            for smp in (sample, None):  # the 64-row sample, then the packed 256 rows
                a = gpu_eng.partial_dependence(ENTRIES, sample=smp, kind="both", response=response)
                b = cpu_eng.partial_dependence(ENTRIES, sample=smp, kind="both", response=response)
                assert a["sample_rows"] == b["sample_rows"] == (64 if smp else 256)
                assert a["output_space"] == b["output_space"]
                for ra, rb in zip(a["results"], b["results"]):
                    assert ra["features"] == rb["features"]
                    assert ra["grid_values"] == rb["grid_values"]
                    np.testing.assert_array_equal(ra["individual"], rb["individual"])
                    np.testing.assert_array_equal(ra["average"], rb["average"])
        # slicing: one job per launch, then seven
        whole = gpu_eng.partial_dependence(ENTRIES, sample=sample, kind="both")
        for pairs in (2 * 64 - 1, 7 * 64 + 3):
            monkeypatch.setattr(ScoringEngine, "PDP_LAUNCH_PAIRS", pairs)
            part = gpu_eng.partial_dependence(ENTRIES, sample=sample, kind="both")
            monkeypatch.undo()
            for ra, rb in zip(whole["results"], part["results"]):
                np.testing.assert_array_equal(ra["individual"], rb["individual"])
                np.testing.assert_array_equal(ra["average"], rb["average"])


def test_monotone_ice_on_the_gpu(train_df, detectors):
    """The guarantee of test_pdp.test_monotone_ice_curves on a model trained
    and evaluated on the GPU: exact, since one thread adds a row's leaves in
    tree order."""
    params = {**FAMILY_PARAMS["hgbt"], "device": "cuda", "monotone": {"credit_limit": -1}}
    pipe = fit_pipe(train_df, "hgbt", params)
    assert pipe.named_steps["classifier"].fit_device_ == "cuda"
    p = pack_pipe(pipe, detectors)
    eng = ScoringEngine(p, device="cuda", device_index=DEV)
    for response in ("raw", "probability"):
        res = eng.partial_dependence(
            ["credit_limit"], kind="both", response=response, grid_resolution=50
        )["results"][0]
        ice = res["individual"]
        assert ice.shape == (256, 50)
        assert (np.diff(ice, axis=1) <= 0).all()
        assert (np.diff(res["average"]) <= 0).all()
        assert np.ptp(ice, axis=1).max() > 0


def test_session_untouched(trained, score_batch):
    """/score bytes before and after partial_dependence are identical: the
    what-if shares nothing with the scoring session. (The 20-tree sums of f32
    leaves are exact in f64, so the scorer's atomics cannot reorder them into
    different bits; the NaN rows of the batch are left out, JSON has no NaN.)"""
    import json

    p = trained["rf"]
    eng = ScoringEngine(p, device="cuda", device_index=DEV)
    body = json.dumps(score_batch.iloc[4:204].to_dict(orient="records")).encode()
    before = bytes(eng.score_json_bytes(body)["response_bytes"])
    out = eng.partial_dependence(ENTRIES, kind="both")
    after = bytes(eng.score_json_bytes(body)["response_bytes"])
    again = eng.partial_dependence(ENTRIES, kind="both")
    assert before == after and len(json.loads(after)["predictions"]) == 200
    for ra, rb in zip(out["results"], again["results"]):
        np.testing.assert_array_equal(ra["individual"], rb["individual"])
    assert N_CAT + N_NUM == 23

"""GPU counterfactuals: forest_sweep_kernel and forest_sweep_search_kernel
(csrc/creditcore_kernels.hip) against cpu_ref.forest_sweep_cpu. Run on a real
MI355X (`pytest -m gpu`).

The kernel is the ordered variant: every interval's f64 sum is built in tree
order by one thread, with plain stores and no atomics, and the reference adds
the same f32 leaves in the same order. So curves, records and raw sums
compare bit for bit, on fitted models as on the dyadic hand-built ones."""

from __future__ import annotations

import numpy as np
import pytest

from _cf_cases import (
    FAMILIES,
    FAMILY_PARAMS,
    NAN_COL,
    SWEEP_BLOCK,
    SWEEP_CHUNK,
    SWEEP_MAX_DEPTH,
    SWEEP_SEG_CAP,
    SWEPT,
    deep_forest,
    fit_pipe,
    hand_forest,
    hand_rows,
    ladder_forest,
    ladder_rows,
    pack_pipe,
    sample_frame,
)
from creditcore import counterfactual as cf
from creditcore.engine import ScoringEngine
from creditcore.ops import cpu_ref
from creditcore.pack import N_CAT, N_NUM, encode_batch
from creditcore.schema import FEATURES

pytestmark = pytest.mark.gpu

DEV = 0


@pytest.fixture(scope="module")
def ext():
    from creditcore.ops import gpu

    assert gpu.available(), (
        "HIP extension must be present on a GPU box (no silent CPU fallback)"
    )
    e = gpu.ext()
    assert (e.SWEEP_BLOCK, e.SWEEP_CHUNK, e.SWEEP_SEG_CAP, e.SWEEP_MAX_DEPTH) == (
        SWEEP_BLOCK, SWEEP_CHUNK, SWEEP_SEG_CAP, SWEEP_MAX_DEPTH,
    )
    assert e.SWEEP_MAX_DEPTH == cf.SWEEP_MAX_DEPTH
    return e


def _sweep(ext, p, codes, nums, jobs, cut, want_curves=True, tables=None):
    import torch

    from creditcore.ops import gpu

    dev = torch.device("cuda", DEV)
    t = tables or cf.build_tables(p)

    def up(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)

    forest = {
        "cls_nodes": up(p.cls_nodes, np.int32), "cls_off": up(p.cls_tree_offsets, np.int32),
        "feat_col": up(p.feat_col, np.int32), "feat_code": up(p.feat_code, np.int32),
        "medians": up(p.medians, np.float32),
    }
    sweep = {
        "node_rank": up(t.node_rank, np.int32), "thr": up(t.thr, np.float32),
        "thr_off": torch.from_numpy(t.thr_off), "max_depth": t.max_depth,
    }
    with torch.cuda.device(dev):
        return gpu.forest_sweep(
            up(codes, np.int16), up(nums, np.float32), forest, sweep, jobs, cut, want_curves
        )


def _ref(p, codes, nums, jobs, cut, tables=None):
    return cpu_ref.forest_sweep_cpu(p, codes, cpu_ref.impute_nums(p, nums), jobs, cut, tables)


def _same(got, ref, curves=True):
    np.testing.assert_array_equal(got[0], ref[0])
    np.testing.assert_array_equal(got[1], ref[1])
    if curves:
        assert len(got[2]) == len(ref[2])
        for a, b in zip(got[2], ref[2]):
            np.testing.assert_array_equal(a, b)
    else:
        assert got[2] is None


# --------------------------------------------------------- hand-built forests


@pytest.mark.parametrize("cls_kind, bias", [(0, 0.0), (1, -0.75)])
def test_hand_built_forest(ext, cls_kind, bias):
    """Nested and equal thresholds on one path (an empty half contributes
    nothing), a tree that never tests the column, a single-leaf tree, a
    shared threshold, thresholds one ulp apart, one-hot nodes above and below
    the swept nodes with row code -1; rows on a threshold, one ulp off it, at
    +-1e30, NaN in the swept column and NaN in another tested column. Every
    numeric column is swept, so K = 0 columns are in."""
    p = hand_forest(cls_kind, bias)
    codes, nums = hand_rows()
    t = cf.build_tables(p)
    assert len(t.thresholds[SWEPT]) == 5 and len(t.thresholds[0]) == 0
    assert np.isnan(nums[5, SWEPT]) and np.isnan(nums[6, NAN_COL]) and (codes[:, 0] == -1).any()
    jobs = cf.sweep_jobs(len(codes), list(range(N_NUM)))
    # the raw sums of the swept column lie in [1, 1.1]: a cut inside that
    # range (flips on both sides), one on a curve value and the 0.5 cut
    for cut in (1.04, 1.03125, cf.raw_cut(p, 0.5)):
        ref = _ref(p, codes, nums, jobs, cut, t)
        _same(_sweep(ext, p, codes, nums, jobs, cut, tables=t), ref)
        if cut == 1.04:
            swept = [j for j in range(len(jobs)) if jobs[j, 1] == SWEPT]
            assert all(np.ptp(ref[2][j]) > 0 for j in swept)
            assert (ref[0][swept, 1] >= 0).any() and (ref[0][swept, 2] >= 0).any()
    # the engine finalises with the bias / the tree count; the threshold
    # whose raw cut is 1.04
    threshold = 1.0 / (1.0 + np.exp(-(1.04 + bias))) if cls_kind else 1.04 / p.cls_n_trees
    gpu_eng = ScoringEngine(p, device="cuda", device_index=DEV)
    cpu_eng = ScoringEngine(p, device="cpu")
    for thr in (0.5, float(threshold)):
        a = gpu_eng.counterfactuals(codes, nums, threshold=thr, curves=True)
        _same_result(a, cpu_eng.counterfactuals(codes, nums, threshold=thr, curves=True))
    name = FEATURES[N_CAT + SWEPT]
    sides = [(r["counterfactuals"][name]["below"], r["counterfactuals"][name]["above"]) for r in a["rows"]]
    assert any(b is not None for b, _ in sides) and any(u is not None for _, u in sides)


def test_raw_sum_equal_to_the_cut(ext):
    """An interval whose raw sum equals the cut exactly is not class 1
    (``raw > cut``): with the cut on the curve's own value there the interval
    sides with the lower ones."""
    p = hand_forest()
    codes, nums = hand_rows()
    t = cf.build_tables(p)
    jobs = cf.sweep_jobs(len(codes), [SWEPT])
    curve = _ref(p, codes, nums, jobs, 0.0, t)[2][0]
    hit = 0
    for cut in np.unique(curve):
        ref = _ref(p, codes, nums, jobs, float(cut), t)
        _same(_sweep(ext, p, codes, nums, jobs, float(cut), tables=t), ref)
        hit += int((np.concatenate(ref[2]) == cut).sum())
    assert hit > 0


# ------------------------------------------------------------------ boundaries


@pytest.mark.parametrize("k", [SWEEP_CHUNK - 2, SWEEP_CHUNK - 1, SWEEP_CHUNK])
def test_chunk_boundaries(ext, k):
    """K + 1 one less than the chunk of intervals a block owns, equal to it
    and one more (a second chunk of a single interval); more than SWEEP_BLOCK
    trees (a second batch; a count that is no multiple of four), trees with
    more segments than the LDS list holds (each thread re-walks them) and a
    single-leaf tree. Columns 1.. have K = 0."""
    p = ladder_forest(k)
    t = cf.build_tables(p)
    seg = np.diff(p.cls_tree_offsets) // 2 + 1  # leaves per tree
    assert len(t.thresholds[0]) == k and p.cls_n_trees > SWEEP_BLOCK and p.cls_n_trees % 4
    assert (seg > SWEEP_SEG_CAP).any() and (seg <= SWEEP_SEG_CAP).any() and (seg == 1).any()
    codes, nums = ladder_rows(k)
    jobs = cf.sweep_jobs(3, [0, 1])
    cut = 0.125
    ref = _ref(p, codes, nums, jobs, cut, t)
    assert (ref[0][:, 1:] >= 0).any()
    _same(_sweep(ext, p, codes, nums, jobs, cut, tables=t), ref)
    _same(_sweep(ext, p, codes, nums, jobs, cut, want_curves=False, tables=t), ref, curves=False)


def test_stack_bound(ext):
    """A tree exactly as deep as the walk's stack, every push alive at once,
    sweeps; one level deeper is refused on the host before any launch."""
    p = deep_forest(SWEEP_MAX_DEPTH)
    t = cf.build_tables(p)
    assert t.max_depth == SWEEP_MAX_DEPTH
    codes, nums = ladder_rows(SWEEP_MAX_DEPTH)
    jobs = cf.sweep_jobs(3, [0])
    _same(_sweep(ext, p, codes, nums, jobs, 0.25, tables=t), _ref(p, codes, nums, jobs, 0.25, t))
    deeper = deep_forest(SWEEP_MAX_DEPTH + 1)
    assert cf.build_tables(deeper).max_depth == SWEEP_MAX_DEPTH + 1
    eng = ScoringEngine(deeper, device="cuda", device_index=DEV)
    with pytest.raises(ValueError, match="deepest tree"):
        eng.counterfactuals(codes, nums, features=["credit_limit"])
    assert eng._cf_dev is None  # nothing was uploaded, nothing launched
    with pytest.raises(RuntimeError, match="stack bound"):
        _sweep(ext, deeper, codes, nums, jobs, 0.25)  # the binding refuses too


def test_host_checks(ext):
    p = hand_forest()
    codes, nums = hand_rows()
    for bad, match in (
        ([[len(codes), 0]], "row out of range"),
        ([[-1, 0]], "row out of range"),
        ([[0, N_NUM]], "column out of range"),
        ([[0, -1]], "column out of range"),
        (np.zeros((0, 2), dtype=np.int32), "at least one job"),
    ):
        with pytest.raises(RuntimeError, match=match):
            _sweep(ext, p, codes, nums, np.asarray(bad, dtype=np.int32).reshape(-1, 2), 0.5)
    t = cf.build_tables(p)
    t.thr_off = t.thr_off.copy()
    t.thr_off[-1] += 1
    with pytest.raises(RuntimeError, match="thr_off"):
        _sweep(ext, p, codes, nums, [[0, 0]], 0.5, tables=t)


# --------------------------------------------------------------- fitted models


@pytest.fixture(scope="module")
def detectors(train_df):
    from creditcore.train import fit_detectors

    return fit_detectors(train_df)


@pytest.fixture(scope="module")
def trained(train_df, detectors):
    return {f: pack_pipe(fit_pipe(train_df, f), detectors) for f in FAMILIES}


@pytest.fixture(scope="module")
def rows(train_df, trained):
    return encode_batch(sample_frame(train_df), trained["rf"].vocabs)


@pytest.mark.parametrize("family", FAMILIES)
def test_fitted_models(ext, trained, rows, family):
    """64 rows x all 14 numeric columns of every family, at the central
    threshold and an off-centre one, with and without curves."""
    p = trained[family]
    assert p.cls_n_trees == FAMILY_PARAMS[family]["n_estimators"]
    codes, nums = rows
    t = cf.build_tables(p)
    jobs = cf.sweep_jobs(len(codes), list(range(N_NUM)))
    for threshold in (0.5, 0.3):
        cut = cf.raw_cut(p, threshold)
        ref = _ref(p, codes, nums, jobs, cut, t)
        _same(_sweep(ext, p, codes, nums, jobs, cut, tables=t), ref)
        _same(_sweep(ext, p, codes, nums, jobs, cut, want_curves=False, tables=t), ref, curves=False)
    assert (ref[0][:, 1:] >= 0).any()  # something flips at 0.3


@pytest.mark.parametrize("n_jobs", [1, SWEEP_BLOCK - 1, SWEEP_BLOCK + 1])
def test_job_counts(ext, trained, rows, n_jobs):
    p = trained["hgbt"]
    codes, nums = rows
    t = cf.build_tables(p)
    jobs = cf.sweep_jobs(len(codes), list(range(N_NUM)))[::3][:n_jobs]
    assert len(jobs) == n_jobs
    cut = cf.raw_cut(p, 0.4)
    _same(_sweep(ext, p, codes, nums, jobs, cut, tables=t), _ref(p, codes, nums, jobs, cut, t))


# ---------------------------------------------------------------------- engine


def _same_result(a, b):
    assert a["threshold"] == b["threshold"] and a["features"] == b["features"]
    assert len(a["rows"]) == len(b["rows"])
    for ra, rb in zip(a["rows"], b["rows"]):
        assert ra["probability"] == rb["probability"] and ra["decision"] == rb["decision"]
        assert list(ra["counterfactuals"]) == list(rb["counterfactuals"])
        for name, ea in ra["counterfactuals"].items():
            eb = rb["counterfactuals"][name]
            assert set(ea) == set(eb)
            for key in ea:
                if key in ("thresholds", "probabilities"):
                    np.testing.assert_array_equal(ea[key], eb[key])
                else:
                    assert ea[key] == eb[key] or (ea[key] != ea[key] and eb[key] != eb[key])


@pytest.mark.parametrize("family", ["rf", "hgbt"])
def test_engine_equals_cpu_engine(trained, rows, family, monkeypatch):
    p = trained[family]
    codes, nums = rows
    gpu_eng = ScoringEngine(p, device="cuda", device_index=DEV)
    cpu_eng = ScoringEngine(p, device="cpu")
    for kw in (
        {},
        {"threshold": 0.3, "curves": True},
        {"features": ["sex", "education"], "threshold": 0.3},
        {"features": ["age", "repayment_status_1"], "curves": True},
    ):
        a = gpu_eng.counterfactuals(codes, nums, **kw)
        _same_result(a, cpu_eng.counterfactuals(codes, nums, **kw))
        _same_result(a, gpu_eng.counterfactuals(codes, nums, **kw))  # lazy tables reused
    # CF_LAUNCH_JOBS + 1 jobs run as two launches and equal the one-launch call
    whole = gpu_eng.counterfactuals(codes, nums, threshold=0.3, curves=True)
    n_jobs = len(codes) * N_NUM
    calls = []
    real = gpu_eng._sweep_gpu

    def spy(*args):
        run = real(*args)

        def counted(jb):
            calls.append(len(jb))
            return run(jb)

        return counted

    monkeypatch.setattr(gpu_eng, "_sweep_gpu", spy)
    monkeypatch.setattr(ScoringEngine, "CF_LAUNCH_JOBS", n_jobs - 1)
    part = gpu_eng.counterfactuals(codes, nums, threshold=0.3, curves=True)
    assert calls == [n_jobs - 1, 1]
    _same_result(whole, part)


def test_session_untouched(trained, rows, score_batch):
    """/score bytes before and after counterfactuals are identical: the
    sweep shares nothing with the scoring session."""
    import json

    p = trained["rf"]
    eng = ScoringEngine(p, device="cuda", device_index=DEV)
    body = json.dumps(score_batch.iloc[4:204].to_dict(orient="records")).encode()
    before = bytes(eng.score_json_bytes(body)["response_bytes"])
    out = eng.counterfactuals(*rows, curves=True)
    after = bytes(eng.score_json_bytes(body)["response_bytes"])
    assert before == after and len(json.loads(after)["predictions"]) == 200
    _same_result(out, eng.counterfactuals(*rows, curves=True))

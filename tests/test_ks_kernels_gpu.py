"""Every K-S kernel variant of csrc/creditcore_kernels.hip against one f64
reference (models/drift.ks_2samp_d per column, rounded once to float32), on
tie-heavy inputs: the families of tests/_kernel_cases.py mixed over the
columns of one batch, uneven reference lengths, and batch sizes around every
loop, slice and kernel-switch edge. All variants evaluate |i/n - j/m| in f64
from the same integers, so they must agree bit for bit with each other and
with the reference.

Which test launches what:

| test                                   | kernel and launch path                        |
|----------------------------------------|-----------------------------------------------|
| test_direct_variants[b] "b256/lds0"    | ks_kernel_t<256>, ref in global (ks_stats)    |
| test_direct_variants[b] "b256/lds1"    | ks_kernel_t<256>, ref staged in LDS           |
| test_direct_variants[b] "b512/lds0"    | ks_kernel_t<512>, ref in global               |
| test_direct_variants[b] "b512/lds1"    | ks_kernel_t<512>, ref staged in LDS           |
| test_direct_variants[b] "scan"         | ks_scan_kernel (ks_stats_sorted)              |
| test_direct_variants[b<=256] "drift"   | ks_count_kernel_t<256> (drift_stats)          |
| test_direct_variants[b>256] "drift"    | ks_kernel_t<256> via drift_stats              |
| test_engine_variants[b<=256]           | ks_count_kernel_t<512> (ScoreSession.record)  |
| test_engine_variants[b>256]            | ks_count_mb_kernel_t<512> + reduce kernel     |
| test_engine_bitonic_branch             | session CREDITCORE_KS_BITONIC: ks_kernel_t<512>|
| test_ref_lds_refusal                   | host TORCH_CHECK only, nothing launched       |

Run on a real MI355X (`pytest -m gpu`); test_reference_matches_scipy needs
no GPU, nor does test_direct_cases_cover_families_and_lengths."""

from __future__ import annotations

import numpy as np
import pytest

from _kernel_cases import (
    FAMILIES,
    REF_LENS,
    generic_case,
    impute,
    ks_reference,
    most_tied_column,
    packed_case,
)

B_SMALL = [1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 127, 128, 129, 255, 256, 257,
           383, 511, 512, 513, 1000, 1024, 1025, 2049]
B_MAX = 16384  # MAX_DRIFT_ROWS: 64 KiB of batch LDS, g = 128 slices per column
F_ALL = (1, 3, 14, 65)
# engines: both sides of the 256 switch, 200 in (129, 255), mid-wave slices
B_ENGINE = [1, 5, 64, 65, 200, 255, 256, 257, 1025, 2049, B_MAX]


def test_reference_matches_scipy():
    """The reference itself: ks_2samp_d on the imputed f32 batch equals
    scipy.stats.ks_2samp(...).statistic to the last bit, on every family at
    the smallest sizes (reference lengths 1, 2, 37, ... by column)."""
    from scipy import stats

    for b in (1, 2, 3, 5, 257):
        for shift in range(len(FAMILIES)):
            case = generic_case(b, 3, seed=1000 * b + shift, shift=shift, len_shift=b + shift // 2)
            got = ks_reference(case)
            imp = impute(case["nums"], case["medians"]).astype(np.float64)
            off = case["rs_off"]
            for j, fam in enumerate(case["families"]):
                ref = case["ref_sorted"][off[j] : off[j + 1]].astype(np.float64)
                with np.errstate(divide="ignore"):  # p-value at n = m = 1
                    want = stats.ks_2samp(ref, imp[:, j], method="asymp").statistic
                assert got[j] == np.float32(want), (b, fam, got[j], want)
                if fam in ("below", "above"):
                    assert got[j] == 1.0


def _direct_cases(b):
    """The cases of test_direct_variants[b]: one per F. The family rotation
    moves with b and F, the reference-length rotation with the position of
    b in the sweep, so the two are independent."""
    k = (B_SMALL + [B_MAX]).index(b)
    for i, f in enumerate(F_ALL):
        yield generic_case(b, f, seed=97 * b + f, shift=b + 3 * i, len_shift=k + 2 * i)


def test_direct_cases_cover_families_and_lengths():
    """What the sweep of test_direct_variants feeds the kernels: every family
    meets every reference length it may have (so several), at single-column
    and many-column launches; few_values always has 3-5 distinct values with
    tie runs in the reference and the batch drawn from them (asserted in
    generic_case as it builds the column)."""
    seen: dict = {}
    for b in B_SMALL + [B_MAX]:
        for case in _direct_cases(b):
            for fam, n in zip(case["families"], case["ref_lens"]):
                seen.setdefault(fam, set()).add(n)
    assert set(seen) == set(FAMILIES)
    for fam, lens in seen.items():
        want = {37, 1000, 4097} if fam == "few_values" else set(REF_LENS)
        assert lens == want, (fam, sorted(lens))


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


def _direct_results(ext, case) -> dict:
    """Every stand-alone entry point on the same inputs -> {name: f32[F]}."""
    nums, med = _dev(case["nums"]), _dev(case["medians"])
    ref, off = _dev(case["ref_sorted"]), _dev(case["rs_off"])
    b, f = case["nums"].shape
    out = {}
    for block in (256, 512):
        for lds in (0, 1):
            out[f"b{block}/lds{lds}"] = ext.ks_stats(nums, med, ref, off, block, lds)
    xs = np.sort(impute(case["nums"], case["medians"]).T, axis=1)
    out["scan"] = ext.ks_stats_sorted(_dev(xs), ref, off)
    if f == 14:
        codes = _dev(np.zeros((b, 9), dtype=np.int16))
        cat_off = _dev(np.arange(10, dtype=np.int32) * 2)
        out["drift"] = ext.drift_stats(codes, nums, med, ref, off, cat_off, 18)[1]
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check(results: dict, want: np.ndarray, ctx):
    names = list(results)
    for k in names:
        assert results[k].dtype == np.float32
        # bit for bit with the f64 reference (measured on MI355X: 0 ulp)
        np.testing.assert_array_equal(results[k], want, err_msg=f"{k} {ctx}")
    for k in names[1:]:
        np.testing.assert_array_equal(results[k], results[names[0]], err_msg=f"{k} {ctx}")


@pytest.mark.gpu
@pytest.mark.parametrize("b", B_SMALL + [B_MAX])
def test_direct_variants(ext, b):
    """ks_stats (256/512 threads x ref in global/LDS), ks_stats_sorted and,
    at F = 14, drift_stats: equal to each other and to the reference,
    exactly (the kernels and numpy divide the same integers in IEEE f64 and
    round once to f32; nothing can contract)."""
    for case in _direct_cases(b):
        ctx = (b, case["families"], case["ref_lens"])
        _check(_direct_results(ext, case), ks_reference(case), ctx)


@pytest.mark.gpu
def test_ref_lds_refusal(ext):
    """A reference that does not fit LDS behind the batch is refused on the
    host (TORCH_CHECK in ks_stats) instead of launched."""
    n_ref = 41000  # 164 000 B > 160 KiB - 1 KiB, batch LDS aside
    case = generic_case(4, 1, seed=0)
    ref = np.sort(np.random.default_rng(0).normal(size=n_ref).astype(np.float32))
    off = np.array([0, n_ref], dtype=np.int64)
    args = (_dev(case["nums"]), _dev(case["medians"]), _dev(ref), _dev(off))
    for block in (256, 512):
        with pytest.raises(RuntimeError, match="ref too large for LDS"):
            ext.ks_stats(*args, block, 1)
    # the same inputs are fine with the reference left in global memory
    case["ref_sorted"], case["rs_off"] = ref, off
    got = ext.ks_stats(*args, 256, 0).cpu().numpy()
    np.testing.assert_array_equal(got, ks_reference(case))


@pytest.fixture(scope="module")
def engine(packed):
    from creditcore.engine import ScoringEngine

    return ScoringEngine(packed, device="cuda", device_index=0)


def _engine_ks(eng, packed, case):
    b = len(case["nums"])
    rng = np.random.default_rng(b)
    codes = np.stack(
        [rng.integers(-1, len(v), size=b) for v in packed.vocabs], axis=1
    ).astype(np.int16)
    return eng.score_arrays(codes, case["nums"], with_drift=True)["ks_d"]


@pytest.mark.gpu
@pytest.mark.parametrize("b", B_ENGINE)
def test_engine_variants(ext, engine, packed, b):
    """The session's K-S (counting kernel at b <= 256, multi-block counting
    plus reduce above) on batches built from the model's own reference
    values: equal to the reference and to the stand-alone sort kernel. The
    third rotation puts few_values on the model's most tied reference column
    (few distinct values, long tie runs on the reference side)."""
    tied = (-most_tied_column(packed)) % len(FAMILIES)
    assert packed_case(packed, 4, 0, shift=tied)["families"][most_tied_column(packed)] == "few_values"
    for shift in sorted({0, 5, tied}):
        case = packed_case(packed, b, seed=31 * b + shift, shift=shift)
        results = {"engine": _engine_ks(engine, packed, case)}
        results.update(_direct_results(ext, case))
        _check(results, ks_reference(case), (b, case["families"]))


@pytest.mark.gpu
def test_engine_bitonic_branch(ext, engine, packed, monkeypatch):
    """CREDITCORE_KS_BITONIC=1: ScoreSession.record() reads the variable with
    getenv every time it records (each new batch size, and every eager run of
    a size it does not capture), so a fresh engine built after setenv in the
    same process takes the ks_kernel_t<512> branch for b > 256. Compared
    with the default engine, which was recorded without the variable.

    The results cannot tell the two branches apart: both are bit-equal to the
    reference, which is the point. That the branch is taken rests on the
    getenv in record(), not on anything this test observes."""
    from creditcore.engine import ScoringEngine

    cases = [packed_case(packed, b, seed=7 * b, shift=b) for b in (257, 1025, 2049, B_MAX)]
    default = [_engine_ks(engine, packed, c) for c in cases]  # recorded first
    monkeypatch.setenv("CREDITCORE_KS_BITONIC", "1")
    bitonic_engine = ScoringEngine(packed, device="cuda", device_index=0)
    for case, dflt in zip(cases, default):
        got = _engine_ks(bitonic_engine, packed, case)
        ctx = (len(case["nums"]), case["families"])
        _check({"bitonic": got, "default": dflt}, ks_reference(case), ctx)

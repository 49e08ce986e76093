"""Input recipes and f64 references shared by the kernel-level drift tests
(test_ks_kernels_gpu.py, test_drift_hist_dense_gpu.py). No tests in here.

A K-S case is a batch ``nums`` f32[B, F] (NaN = missing), ``medians`` f32[F]
and per-column sorted references of uneven length, concatenated
(``ref_sorted`` / ``rs_off``). Every column follows one *family*, a recipe
that provokes ties inside the batch, between batch and reference, or none."""

from __future__ import annotations

import numpy as np

from creditcore.models.drift import ks_2samp_d

FAMILIES = (
    "few_values",  # (a) 3-5 distinct integers on both sides
    "const_on_ref",  # (b) constant equal to a reference value
    "const_between",  # (b) constant strictly between reference values
    "resampled",  # (c) every batch point ties a reference point
    "below",  # (d) wholly below the reference minimum, D = 1
    "above",  # (d) wholly above the reference maximum, D = 1
    "all_nan",  # (e) imputation makes the column constant
    "nan_tied_median",  # (e) 30 % NaN, median already present: a tie run
    "specials",  # (f) +-inf and +-0.0
    "normal",  # (g) continuous control
)
REF_LENS = (1, 2, 37, 1000, 4097)
# few_values needs room for 3-5 distinct values with tie runs in the reference
FEW_VALUES_REF_LENS = (37, 1000, 4097)

_SPECIALS = np.array([np.inf, -np.inf, -0.0, 0.0], dtype=np.float32)


def make_ref(rng, family: str, n: int) -> np.ndarray:
    """Sorted f32 reference column of length n for a generic case."""
    if family == "few_values":
        r = rng.integers(0, 4, size=n).astype(np.float32)
        r[:4] = np.arange(4)[: len(r)]  # all four values, whatever the draw
    else:
        r = rng.normal(0.0, 100.0, size=n).astype(np.float32)
        if family == "specials":
            k = min(n, 4)
            r[:k] = _SPECIALS[rng.permutation(4)[:k]]
    return np.sort(r)


def make_median(rng, family: str, ref: np.ndarray) -> np.float32:
    if family in ("all_nan", "nan_tied_median"):
        return np.float32(ref[len(ref) // 2])  # imputed values tie the ref
    if family == "specials":
        return np.float32(0.0)
    return np.float32(rng.normal(0.0, 100.0))


def make_col(rng, family: str, ref: np.ndarray, b: int, median) -> np.ndarray:
    """Batch column f32[b] of the family, given its sorted reference."""
    fin = ref[np.isfinite(ref)]
    if len(fin) == 0:
        fin = np.zeros(1, dtype=np.float32)
    lo, hi = float(fin[0]), float(fin[-1])
    if family == "few_values":
        u = np.unique(fin)
        vals = u[np.linspace(0, len(u) - 1, min(5, len(u))).astype(int)]
        col = rng.choice(vals, size=b)
        k = min(b, len(vals))
        col[rng.permutation(b)[:k]] = vals[:k]  # every value, if b allows
    elif family == "const_on_ref":
        col = np.full(b, fin[len(fin) // 2])
    elif family == "const_between":
        u = np.unique(fin)
        v = np.float32(hi + 1.0 + abs(hi))  # one distinct value: nothing between
        for i in range(len(u) // 2, len(u) - 1):
            mid = np.float32((float(u[i]) + float(u[i + 1])) / 2)
            if u[i] < mid < u[i + 1]:
                v = mid
                break
        col = np.full(b, v)
    elif family == "resampled":
        col = rng.choice(ref, size=b)
    elif family == "below":
        col = lo - (1.0 + np.abs(rng.normal(size=b))) * max(1.0, abs(lo))
    elif family == "above":
        col = hi + (1.0 + np.abs(rng.normal(size=b))) * max(1.0, abs(hi))
    elif family == "all_nan":
        col = np.full(b, np.nan)
    elif family == "nan_tied_median":
        col = rng.choice(ref, size=b).astype(np.float32)
        col[rng.uniform(size=b) < 0.3] = np.nan
        col[0::5] = np.nan
        col[1::4] = median  # present before imputation
    elif family == "specials":
        pool = np.concatenate([_SPECIALS, np.float32([lo, hi])])
        col = rng.choice(pool, size=b)
        k = min(b, 4)
        col[rng.permutation(b)[:k]] = _SPECIALS[:k]
    elif family == "normal":
        col = rng.normal(fin.mean(), fin.std() + 1.0, size=b)
    else:
        raise ValueError(family)
    return np.asarray(col, dtype=np.float32)


def column_families(f: int, shift: int) -> list[str]:
    """Families of the f columns; ``shift`` rotates them so that one-column
    cases still walk through all families as the shift varies."""
    return [FAMILIES[(j + shift) % len(FAMILIES)] for j in range(f)]


def ref_len(family: str, j: int, len_shift: int) -> int:
    """Reference length of column j. ``len_shift`` rotates the lengths
    independently of the family rotation, so that every family meets
    several lengths over a sweep."""
    lens = FEW_VALUES_REF_LENS if family == "few_values" else REF_LENS
    return lens[(j + len_shift) % len(lens)]


def generic_case(b: int, f: int, seed: int, shift: int = 0, len_shift: int = 0) -> dict:
    """K-S inputs with hand-made references of uneven length."""
    rng = np.random.default_rng(seed)
    fams = column_families(f, shift)
    refs, meds, cols = [], [], []
    for j, fam in enumerate(fams):
        ref = make_ref(rng, fam, ref_len(fam, j, len_shift))
        med = make_median(rng, fam, ref)
        col = make_col(rng, fam, ref, b, med)
        if fam == "few_values":  # ties on both sides and across the samples
            assert 3 <= len(np.unique(ref)) <= 5
            assert min(3, b) <= len(np.unique(col)) <= 5
            assert np.isin(col, ref).all() and len(ref) > len(np.unique(ref))
        refs.append(ref)
        meds.append(med)
        cols.append(col)
    return {
        "families": fams,
        "ref_lens": [len(r) for r in refs],
        "nums": np.ascontiguousarray(np.stack(cols, axis=1)),
        "medians": np.asarray(meds, dtype=np.float32),
        "ref_sorted": np.concatenate(refs),
        "rs_off": np.concatenate([[0], np.cumsum([len(r) for r in refs])]).astype(np.int64),
    }


def packed_case(packed, b: int, seed: int, shift: int = 0) -> dict:
    """The same families over a packed model's own reference and medians
    (what the engine's session holds): batches built from its values."""
    rng = np.random.default_rng(seed)
    off = packed.ref_sorted_offsets
    fams = column_families(len(off) - 1, shift)
    cols = []
    for j, fam in enumerate(fams):
        ref = packed.ref_sorted[off[j] : off[j + 1]]
        cols.append(make_col(rng, fam, ref, b, packed.medians[j]))
    return {
        "families": fams,
        "nums": np.ascontiguousarray(np.stack(cols, axis=1)),
        "medians": packed.medians,
        "ref_sorted": packed.ref_sorted,
        "rs_off": np.asarray(off, dtype=np.int64),
    }


def most_tied_column(packed) -> int:
    """The numeric column whose reference has the fewest distinct values."""
    off = packed.ref_sorted_offsets
    distinct = [len(np.unique(packed.ref_sorted[off[j] : off[j + 1]])) for j in range(len(off) - 1)]
    return int(np.argmin(distinct))


def impute(nums: np.ndarray, medians: np.ndarray) -> np.ndarray:
    return np.where(np.isnan(nums), medians[None, :], nums).astype(np.float32)


def ks_reference(case: dict) -> np.ndarray:
    """f32[F]: ks_2samp_d in f64 per column, rounded once to float32."""
    imp = impute(case["nums"], case["medians"])
    off = case["rs_off"]
    out = np.empty(imp.shape[1], dtype=np.float32)
    for j in range(imp.shape[1]):
        ref = case["ref_sorted"][off[j] : off[j + 1]].astype(np.float64)
        out[j] = np.float32(ks_2samp_d(ref, imp[:, j].astype(np.float64)))
    return out


def cat_hist_reference(codes: np.ndarray, cat_off: np.ndarray) -> np.ndarray:
    """Concatenated per-column histograms; code -1 counts in the last bin."""
    out = np.zeros(int(cat_off[-1]), dtype=np.int32)
    for c in range(codes.shape[1]):
        nb = int(cat_off[c + 1] - cat_off[c])
        col = codes[:, c].astype(np.int64)
        out[cat_off[c] : cat_off[c + 1]] = np.bincount(
            np.where(col < 0, nb - 1, col), minlength=nb
        )
    return out

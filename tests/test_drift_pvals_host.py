"""Host p-value epilogue (csrc drift_pvals_host: chi2_sf_int_dof, mtw_sf, smirnov_sf,
pelz_good_sf) vs scipy. On a machine where the extension is loaded,
cpu_ref.pvals_from_stats *is* this C code, so the engine parity tests compare
it with itself; here it faces scipy directly, on synthetic statistics.

Host C only: needs the built extension, no GPU."""

from __future__ import annotations

import numpy as np
import pytest
from scipy import stats

from creditcore.models.drift import chi2_from_counts, chi2_from_counts_many

# en = round(n_ref * n_batch / (n_ref + n_batch)); n_ref = n_batch = 2 en
EN_EXACT = (1, 2, 3, 10, 50, 139, 140)  # exact algorithm before and after
EN_BAND = (141, 200, 299)  # scipy's own regions: exact, Pelz-Good, Smirnov
# Pelz-Good; 320, 499, 500 sit on either side of where the exact corner ends
EN_SERIES = (300, 320, 499, 500, 1000, 8000)


@pytest.fixture(scope="module")
def ext():
    import torch  # noqa: F401  (loads libc10 for the extension)

    from creditcore.ops import gpu

    if not gpu.available():
        pytest.skip("extension not built")
    return gpu.ext()


def _d_grid(en: int) -> np.ndarray:
    """D in [0, 1] as float32: a uniform grid with both ends, the bulk of the
    null distribution (z = D sqrt(en) in [0.2, 3]), and values just below and
    above en D^2 = 18 (the mtw_sf cutoff)."""
    g = list(np.linspace(0.0, 1.0, 201))
    g += [z / np.sqrt(en) for z in np.linspace(0.2, 3.0, 57)]
    c = np.sqrt(18.0 / en)
    g += [c * (1 - 1e-3), c * (1 - 1e-6), c * (1 + 1e-6), c * (1 + 1e-3)]
    g = np.asarray(g, dtype=np.float32)
    g = np.unique(g[(g >= 0.0) & (g <= 1.0)])
    assert g[0] == 0.0 and g[-1] == 1.0
    if c < 1.0:
        d2 = en * g.astype(np.float64) ** 2
        assert (d2 < 18.0).any() and (d2 > 18.0).any()
        assert np.abs(d2 - 18.0).min() < 1e-4
    return g


def _ks_pvals(ext, en: int, d: np.ndarray) -> np.ndarray:
    one = np.ones(1, dtype=np.int32)
    off = np.array([0, 1], dtype=np.int32)
    out = np.asarray(ext.drift_pvals_host(one, d, one, off, 2 * en, 2 * en))
    assert out.shape == (1 + len(d),) and out[0] == 1.0  # one bin: k < 2
    return out[1:]


def _ks_max_err(ext, en: int) -> float:
    d = _d_grid(en)
    got = _ks_pvals(ext, en, d)
    assert got[0] == 1.0 and got[-1] == 0.0  # D = 0, D = 1
    assert ((got >= 0.0) & (got <= 1.0)).all()
    ref = stats.kstwo.sf(d.astype(np.float64), en)
    err = np.abs(got - ref)
    i = int(err.argmax())
    print(f"en={en}: max |p - kstwo.sf| = {err[i]:.3e} at D={d[i]:.6f}")
    return float(err[i])


@pytest.mark.parametrize("en", EN_EXACT)
def test_ks_pvalue_exact_small_en(ext, en):
    """en <= 140: mtw_sf is the exact matrix algorithm, as scipy's.

    Measured against scipy.stats.kstwo.sf on the D grid above, the largest
    absolute difference over all en listed is 1.12e-14 (at en = 140; 9.4e-15
    at 139, 4.9e-15 at 50, <= 1e-15 below). Asserted with a x4 margin for
    libm differences between machines: 4.5e-14."""
    assert _ks_max_err(ext, en) <= 4.5e-14


@pytest.mark.parametrize("en", EN_BAND)
def test_ks_pvalue_band_140_300(ext, en):
    """140 < en < 300, the band nobody had checked, against
    scipy.stats.kstwo.sf with the 3e-7 bound the project states for its K-S
    p-values.

    The C code used the Pelz-Good series for the whole band and missed the
    bound: 3.0e-6 at en = 141 (D = 0.045), 1.1e-6 at en = 200, 3.3e-7 at
    en = 299, all at small D (en D^1.5 <= 1.4) where kstwo.sf is exact, and
    5e-7 at en = 141 in the tail (en D^2 >= 2.2) where kstwo.sf is twice the
    Smirnov tail. Computing the whole band by the exact matrix method misses
    it as well (3.07e-6 at en = 141, D = 0.0463), because between those two
    regions kstwo.sf is itself the Pelz-Good series. drift_pvals_raw now
    follows scipy's selection region by region; measured after that:
    3.3e-16 at en = 141, 9.9e-16 at 200, 1.8e-15 at 299."""
    assert _ks_max_err(ext, en) <= 3e-7


@pytest.mark.parametrize("en", EN_SERIES)
def test_ks_pvalue_series_large_en(ext, en):
    """en >= 300: 3e-7 absolute, the bound of ks_asymp_pvalue_many's
    docstring. The bare series measured 3.24e-7 at en = 300 (D = 0.0231, in
    the corner en D^1.5 <= 1.4 where scipy too prefers its exact method), so
    below en = 500 that corner is computed exactly now. Measured after the
    change: 1.0e-7 at en = 300, 8.7e-8 at 320, 3.2e-8 at 499; at en = 500,
    the first without the exact corner, 1.19e-7 (in that corner, D = 0.0179);
    2.1e-8 at 1000, 2.9e-8 at 8000."""
    assert _ks_max_err(ext, en) <= 3e-7


def test_ks_pvalue_mirror_agrees(ext):
    """The numpy mirror (the path without the extension) keeps the same
    bound at en = 300 on the same grid."""
    from creditcore.models.drift import ks_asymp_pvalue_many

    d = _d_grid(300)
    got = ks_asymp_pvalue_many(d, 600, 600)
    ref = stats.kstwo.sf(d.astype(np.float64), 300)
    assert np.abs(got - ref).max() <= 3e-7
    np.testing.assert_allclose(_ks_pvals(ext, 300, d), got, atol=3e-7)


# ---------------------------------------------------------------- chi-square


def _chi2_columns():
    """(name, ref counts, batch counts) per categorical column."""
    rng = np.random.default_rng(5)
    cols = []
    for nb in range(1, 13):  # k = 1 .. 12: dof 0 .. 11, odd and even
        rc = rng.integers(1, 400, nb)
        # a batch from the reference's own proportions: p in the usual range
        cols.append((f"random{nb}", rc, rng.multinomial(150, rc / rc.sum())))
    # bins empty on both sides are dropped from k: 7 bins, k = 4 (dof 3)
    cols.append(("both_empty", [50, 0, 31, 0, 12, 0, 7], [9, 0, 2, 0, 8, 0, 3]))
    # a bin empty in the batch only stays (k = 5)
    cols.append(("batch_empty_bin", [50, 40, 31, 22, 12], [9, 0, 2, 5, 0]))
    # k = 2: Yates-corrected, plain and after dropping empty bins
    cols.append(("yates", [300, 120], [20, 31]))
    cols.append(("yates_after_drop", [0, 300, 0, 120], [0, 20, 0, 31]))
    # Yates clamps |o - e| - 0.5 at zero
    cols.append(("yates_clamped", [100, 100], [10, 10]))
    # k < 2: p = 1
    cols.append(("one_live_bin", [0, 17, 0], [0, 5, 0]))
    cols.append(("no_live_bin", [0, 0], [0, 0]))
    # an empty sample: p = 1
    cols.append(("empty_batch", [5, 6, 7], [0, 0, 0]))
    cols.append(("empty_ref", [0, 0, 0], [5, 6, 7]))
    # identical proportions: stat = 0, p = 1
    cols.append(("same_props", [30, 60, 90, 120], [10, 20, 30, 40]))
    cols.append(("same_props_k2", [30, 60], [10, 20]))
    # shifted: small p, and p that underflows to 0
    cols.append(("shifted", [400, 300, 200, 100], [10, 20, 30, 40]))
    cols.append(("gross_odd", [100000, 10, 10, 10], [10, 10, 10, 100000]))
    cols.append(("gross_even", [100000, 10, 10], [10, 10, 100000]))
    return [(n, np.asarray(r, np.int32), np.asarray(b, np.int32)) for n, r, b in cols]


def test_chi2_pvalues(ext):
    """chi2_sf_int_dof and the contingency statistic of drift_pvals_raw vs
    (1) scipy.stats.chi2_contingency through models/drift.chi2_from_counts
    and (2) scipy.stats.chi2.sf of the same statistic through
    chi2_from_counts_many.

    Measured largest relative difference over the columns above: 1.3e-15
    against (1) and 5.5e-15 against (2), the latter on the "shifted" column
    (p = 3.5e-20, where exp(-x/2) carries the rounding of x = 94). Asserted
    with a x4 margin on the larger one: 2.2e-14 relative. The columns whose p
    is exactly 1 or underflows to 0 must match exactly."""
    cols = _chi2_columns()
    rc = np.concatenate([c[1] for c in cols])
    bc = np.concatenate([c[2] for c in cols])
    off = np.concatenate([[0], np.cumsum([len(c[1]) for c in cols])]).astype(np.int32)
    got = np.asarray(
        ext.drift_pvals_host(bc, np.zeros(0, np.float32), rc, off, 1000, 1000)
    )
    assert got.shape == (len(cols),)
    ref1 = np.array([chi2_from_counts(r, b) for _, r, b in cols])
    ref2 = chi2_from_counts_many(rc, bc, off)

    by_name = {c[0]: i for i, c in enumerate(cols)}
    for name in ("random1", "one_live_bin", "no_live_bin", "empty_batch",
                 "empty_ref", "same_props", "same_props_k2", "yates_clamped"):
        assert got[by_name[name]] == 1.0, name
        assert ref1[by_name[name]] == 1.0, name
    for name in ("gross_odd", "gross_even"):
        assert got[by_name[name]] == 0.0 and ref1[by_name[name]] == 0.0, name
    assert 0.0 < got[by_name["shifted"]] < 1e-15

    for label, ref in (("chi2_contingency", ref1), ("chi2.sf", ref2)):
        live = ref > 0.0
        rel = np.abs(got[live] - ref[live]) / ref[live]
        i = int(rel.argmax())
        print(f"vs {label}: max rel err {rel[i]:.3e} "
              f"({np.asarray(cols, dtype=object)[live][i][0]}, p={ref[live][i]:.3e})")
        assert rel.max() <= 2.2e-14, label
        np.testing.assert_array_equal(got[~live], ref[~live])

"""The MMD kernel cases of _mmd_cases.py on the CPU: the independent reference
against cpu_ref, the exactness of the cluster problems, the f64 emulation of
the kernel's tiling on every case, every mutation of it seen by a committed
case, the shapes against the kernel's branch arithmetic, and
mmd.default_cols_per_block."""

from __future__ import annotations

import numpy as np
import pytest

import _mmd_cases as mc
from creditcore import mmd
from creditcore.ops import cpu_ref


def cluster_runs():
    """(case, row_begin, row_count or None) of every cluster comparison."""
    for case in mc.CLUSTER_CASES:
        yield case, 0, None
        for a, r in mc.slices_of(case.n):
            yield case, a, r


def cluster_sees(mutation) -> str | None:
    for case, a, r in cluster_runs():
        z, gamma, ind, want = mc.cluster_problem(case)
        got = mc.emulate_w(z, gamma, ind, case.cols, a, r, mutation=mutation)
        rows = slice(a, None if r is None else a + r)
        if not np.array_equal(got, want[rows].astype(np.float64)):
            return f"cluster {case.id} rows {a}+{r}"
    return None


def read_out_sees(mutation) -> str | None:
    for case in (*mc.READ_OUT_CASES[::-1], mc.ONE_HOT_CASE):
        z, gamma, ind, j_q = mc.read_out_problem(case)
        got = mc.emulate_w(z, gamma, ind, case.cols, mutation=mutation)
        want = mc.k_definition(z, gamma)[:, j_q]
        bound = mc.k_bound(z, gamma, exact_gram=case.dyadic)[:, j_q]
        if not (np.abs(got - want) <= bound).all():
            return f"read-out {case.id}"
    return None


@pytest.mark.parametrize("case", mc.CLUSTER_CASES, ids=lambda c: c.id)
def test_cluster_problem_is_exact(case):
    """K by definition is 1 inside a cluster and rounds to 0 in f32 across;
    the f64 reference is the integer count up to N exp(-512); every f32
    intermediate of the kernel is an integer below 2^24."""
    z, gamma, ind, want = mc.cluster_problem(case)
    assert gamma == 1.0 and ind.shape == (case.n, case.q) and set(np.unique(ind)) <= {0, 1}
    d2 = mc.d2_definition(z)
    assert set(np.unique(d2)) <= {0.0, 512.0}
    k = mc.k_definition(z, gamma)
    k32 = k.astype(np.float32)
    assert set(np.unique(k32)) <= {0.0, 1.0}
    assert np.array_equal(k32.astype(np.int64) @ ind.astype(np.int64), want)
    ref = k @ ind.astype(np.float64)
    assert np.abs(ref - want).max() <= case.n * np.exp(-512.0)
    assert np.array_equal(ref[want > 0], want[want > 0].astype(np.float64))
    assert np.array_equal(z, np.rint(z))
    assert 4 * mmd.squared_norms(z).max() < 2**24 and want.max() < 2**24
    # norms as the engine uploads them are exact
    assert np.array_equal(mmd.squared_norms(z).astype(np.float32), mmd.squared_norms(z))


def test_cluster_ids_are_not_periodic():
    """Moving j by 1, 4, 16 or 64, or exchanging g and r or reversing r inside
    a group of 16, changes the cluster of some row of every tile."""
    for c in (5, 7):
        cl = mc.cluster_ids(256, c)
        j = np.arange(256)
        for shift in (1, 4, 16, 64):
            assert (cl[shift:] != cl[:-shift]).any()
        js, g, r = j // 16, (j % 16) // 4, j % 4
        for other in (16 * js + 4 * r + g, 16 * js + 4 * g + 3 - r, 16 * js + g):
            for t in range(0, 256, 64):
                assert (cl[other][t : t + 64] != cl[t : t + 64]).any()


def test_cluster_coordinates_isolate_each_piece():
    """Pairs of clusters that differ only in the piece under test."""
    c132 = mc.cluster_coordinates(132, 7)
    assert sum(p >= 128 for p in c132) >= 2  # only the last chunk / its one float4
    assert sum(48 <= p < 64 for p in c132) >= 2  # only the last 16-wide step of chunk 0
    assert sum(64 <= p < 128 for p in c132) >= 2  # only the second chunk
    c68 = mc.cluster_coordinates(68, 7)
    assert sum(p >= 64 for p in c68) >= 2  # only the 4-wide second chunk
    assert mc.cluster_coordinates(5, 5)[0] == 4  # column d - 1 of the padded float4
    for case in mc.CLUSTER_CASES:
        assert len(set(mc.cluster_coordinates(case.d, case.c))) == case.c


def test_k_definition_agrees_with_cpu_ref():
    """Two algebras (pairwise differences, norm expansion) in f64. The norm
    expansion cancels: its error is a few f64 roundings of n_i + n_j times
    gamma, far below the f32 bound."""
    problems = [mc.cluster_problem(c)[:3] for c in mc.CLUSTER_CASES]
    problems += [mc.read_out_problem(c)[:3] for c in (*mc.READ_OUT_CASES, mc.ONE_HOT_CASE)]
    for z, gamma, ind in problems:
        want = mc.k_definition(z, gamma) @ ind.astype(np.float64)
        got = cpu_ref.mmd_perm_w_cpu(z, gamma, ind)
        n = mmd.squared_norms(z)
        tol = 2.0**-52 * (4 * z.shape[1] + 8) * gamma * 2 * n.max() * len(z)
        assert np.abs(got - want).max() <= tol + 1e-300


@pytest.mark.parametrize("case", mc.CLUSTER_CASES, ids=lambda c: c.id)
def test_emulation_is_exact_on_clusters(case):
    z, gamma, ind, want = mc.cluster_problem(case)
    full = mc.emulate_w(z, gamma, ind, case.cols)
    assert not np.isnan(full).any()  # every slab entry is written
    assert np.array_equal(full, want.astype(np.float64))
    for a, r in mc.slices_of(case.n):
        got = mc.emulate_w(z, gamma, ind, case.cols, a, r)
        assert np.array_equal(got, full[a : a + r])
    # the j < N mask alone is redundant with the indicator's zero padding
    assert np.array_equal(mc.emulate_w(z, gamma, ind, case.cols, mask_pad_j=False), full)


def test_emulation_is_within_bound_on_read_outs():
    for case in (*mc.READ_OUT_CASES, mc.ONE_HOT_CASE):
        z, gamma, ind, j_q = mc.read_out_problem(case)
        if case.dyadic:
            assert mc.dyadic_is_exact(z)
        got = mc.emulate_w(z, gamma, ind, case.cols)
        want = mc.k_definition(z, gamma)[:, j_q]
        bound = mc.k_bound(z, gamma, exact_gram=case.dyadic)[:, j_q]
        assert (np.abs(got - want) <= bound).all(), case.id
        assert (got[j_q, np.arange(len(j_q))] == 0.0).all()


@pytest.mark.parametrize("mutation", mc.MUTATIONS)
def test_mutation_is_seen(mutation):
    """Exact mismatch on a cluster case, or beyond the derived bound on a
    read-out case."""
    seen = cluster_sees(mutation) or read_out_sees(mutation)
    print(f"{mutation}: seen by {seen}")
    assert seen is not None


def test_cluster_cases_see_the_structural_mutations():
    """The mutations of masks, pairings, chunks, splits and slices are all
    caught exactly, without a tolerance. pad_j_unmasked alone falls to the
    read-out cases: a padding row adds k = exp(-gamma n_i), which is 0 in f32
    at the cluster problems' norms (n_i >= 256, gamma = 1)."""
    for mutation in mc.MUTATIONS:
        if mutation != "pad_j_unmasked":
            assert cluster_sees(mutation) is not None, mutation


def test_shapes_reach_the_kernel_branches():
    """Every branch of mmd_perm_kernel named by the shape arithmetic is taken
    by a committed case."""
    runs = []  # (N, Dp, cols, Q, row_begin, row_count)
    for case, a, r in cluster_runs():
        dp = -(-case.d // 4) * 4
        runs.append((case.n, dp, case.cols, case.q, a, case.n - a if r is None else r))
    for case in (*mc.READ_OUT_CASES, mc.ONE_HOT_CASE):
        dp = -(-case.d // 4) * 4
        runs.append((case.n, dp, case.cols, len(mc.read_out_columns(case.n)), 0, case.n))
    dps = {dp for _, dp, *_ in runs}
    assert {4, 8, 48, 64, 68, 80, 128, 132} <= dps
    assert max(dp for dp in dps if dp <= mc.DC) == 64  # the last zi_once value
    assert any(dp > mc.DC and dp % mc.DC == 4 for dp in dps)  # a chunk one float4 wide
    assert any(dp % mc.DC == 0 and dp > mc.DC for dp in dps)  # exact chunks
    assert any(dp % mc.STEP for dp in dps) and any(dp % mc.STEP == 0 for dp in dps)

    def tiles(n):
        return -(-n // mc.TILE)

    # multi-chunk path with several j tiles in a block and several splits
    assert any(dp > mc.DC and cols >= 2 * mc.TILE and n > cols and tiles(min(cols, n)) >= 2
               for n, dp, cols, *_ in runs)
    # zi_once path with several j tiles in a block (staged once, reused)
    assert any(dp <= mc.DC and cols >= 2 * mc.TILE and n > mc.TILE for n, dp, cols, *_ in runs)
    assert any(n % mc.TILE == 1 and n > mc.TILE for n, *_ in runs)  # one live row
    assert any(n % mc.TILE == 0 for n, *_ in runs)  # no padding at all
    assert any(cols > n and tiles(n) > 1 for n, _, cols, *_ in runs)
    assert any(n < mc.TILE for n, *_ in runs)
    qs = {q for _, _, _, q, _, _ in runs}
    assert {1, 16, 17, 256} <= qs  # below, on, one past a q tile; the maximum
    # slices: the guard my_i < row0 + rows decides (rows end inside a tile,
    # before N), from a row_begin other than 0
    for rc in (1, 63, 65):
        assert any(a > 0 and r == rc and a + r < n for n, _, _, _, a, r in runs)
    assert any(a > 0 and r % mc.TILE and a + r == n for n, _, _, _, a, r in runs) or any(
        a > 0 and n % mc.TILE and a + r < n for n, _, _, _, a, r in runs
    )
    assert max(n for n, *_ in runs) <= 331 and max(dps) <= 132


def test_one_hot_columns_cover_the_lanes():
    j = mc.read_out_columns(mc.ONE_HOT_CASE.n)
    n = mc.ONE_HOT_CASE.n
    assert len(j) <= 256 and len(set(j)) == len(j) and j.max() == n - 1
    for t in range(0, n, mc.TILE):
        assert t in j and min(t + mc.TILE, n) - 1 in j
    local = j[(j >= 64) & (j < 128)] - 64
    assert {(x // 16, (x % 16) // 4, x % 4) for x in local} == {
        (a, b, c) for a in range(4) for b in range(4) for c in range(4)
    }
    assert ((j >= n - n % mc.TILE) & (j < n)).sum() >= 2  # the ragged last tile


@pytest.mark.parametrize("n", [2, 64, 65, 4096, 32768])
def test_default_cols_per_block(n):
    cols = mmd.default_cols_per_block(n)
    assert cols > 0 and cols % mmd.MMD_TILE == 0
    blocks = -(-n // cols) * -(-n // mmd.MMD_TILE)
    assert 1 <= blocks <= 2 * 2048

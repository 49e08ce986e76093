"""The hand-built attribution cases of _attr_cases.py on the CPU: the exact
references against the subset brute force, cpu_ref against the references,
the cases against what they claim to contain, and every deliberately wrong
reference against the true one. test_attr_kernels_gpu.py runs the same cases
through the HIP kernels.

Bounds: 1e-12 is the project's "reference vs brute force" bound
(test_shap.py); a mutation counts as seen above 1e-6, a thousand times the
GPU bound of 1e-9."""

from __future__ import annotations

import numpy as np
import pytest

import _attr_cases as ac
from _shap_models import N_SRC
from creditcore.engine import _check_shap_paths
from creditcore.ops import cpu_ref
from creditcore.pack import (
    N_CAT,
    SHAP_CODE_SHIFT,
    SHAP_FIRST,
    SHAP_PLAYER_SHIFT,
    build_shap_paths,
)
from test_ishap import brute_force_ishap
from test_shap import brute_force_shap
from test_shap_interactions import brute_force_interactions

BRUTE = 1e-12
SEEN = 1e-6
BUILDS = [(f, k) for f in ac.FORESTS for k in ac.kinds_of(f)]


def _paths(forest: str, kind: int = 0):
    paths, base = build_shap_paths(ac.model(forest, kind))
    _check_shap_paths(paths)
    return paths, base


def _group_counts(paths) -> np.ndarray:
    first = (paths.splits[:, 3].view(np.uint32) & SHAP_FIRST) != 0
    rec_leaf = np.repeat(np.arange(paths.n_leaves), np.diff(paths.leaf_off))
    return np.bincount(rec_leaf[first], minlength=paths.n_leaves)


def _off_diagonal(m: np.ndarray) -> np.ndarray:
    out = m.copy()
    d = np.arange(N_SRC)
    out[:, d, d] = 0.0
    return out


# ------------------------------------------------- references vs brute force


@pytest.mark.parametrize("forest", ac.FORESTS)
def test_reference_equals_brute_force(forest):
    """On every tree with at most 9 players the closed forms in exact
    arithmetic equal the Shapley values, interaction indices and
    interventional values by subset enumeration."""
    c, p = ac.case(forest), ac.small_tree_model(forest)
    assert p.cls_n_trees >= (3 if forest == "transitions" else len(c.trees))
    codes, nums = c.codes[:33], c.nums[:33]
    want, want_base = brute_force_shap(p, codes, nums)
    got = ac.ref_shap(p, codes, nums)
    inter = brute_force_interactions(p, codes, nums)
    got_inter = ac.ref_inter(p, codes, nums)
    d = np.arange(N_SRC)
    errs = {
        "shap": np.abs(got - want).max(),
        "shap base": abs(ac.ref_shap_base(p) - want_base),
        "inter": np.abs(got_inter - _off_diagonal(inter)).max(),
        "inter diagonal": np.abs(got - got_inter.sum(2) - inter[:, d, d]).max(),
    }
    for r in ac.BG_ROWS:
        bg = c.bg_codes[:r], c.bg_nums[:r]
        want_i, want_ibase = brute_force_ishap(p, codes, nums, *bg)
        errs[f"ishap R={r}"] = np.abs(ac.ref_ishap(p, codes, nums, *bg) - want_i).max()
        errs[f"ishap base R={r}"] = abs(ac.ref_ishap_base(p, *bg) - want_ibase)
        assert np.abs(want_i).max() > 1e-3
    print(f"{forest}: " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert np.abs(want).max() > 1e-3
    assert forest == "stripes" or np.abs(_off_diagonal(inter)).max() > 1e-3
    assert max(errs.values()) <= BRUTE, errs


# ------------------------------------------------------ cpu_ref vs references


@pytest.mark.parametrize("forest,kind", BUILDS)
def test_cpu_ref_agrees_with_the_references(forest, kind):
    c, p = ac.case(forest), ac.model(forest, kind)
    paths, base = _paths(forest, kind)
    imp = cpu_ref.impute_nums(p, c.nums)
    errs = {}
    contrib = cpu_ref.forest_contrib_cpu(p, c.codes, imp)
    errs["contrib"] = np.abs(contrib - ac.reference(forest, kind, "contrib")).max()
    shap = cpu_ref.forest_shap_cpu(p, c.codes, imp, paths=paths)
    errs["shap"] = np.abs(shap - ac.reference(forest, kind, "shap")).max()
    errs["shap base"] = abs(base - ac.ref_shap_base(p))
    b = max(ac.ROWS["inter"])
    inter = cpu_ref.forest_shap_interactions_cpu(p, c.codes[:b], imp[:b], paths=paths)
    want = ac.reference(forest, kind, "inter")
    d = np.arange(N_SRC)
    errs["inter"] = np.abs(_off_diagonal(inter) - want).max()
    errs["inter diagonal"] = np.abs(inter[:, d, d] - (shap[:b] - want.sum(2))).max()
    for r in ac.BG_ROWS:
        bg = c.bg_codes[:r], cpu_ref.impute_nums(p, c.bg_nums[:r])
        got = cpu_ref.forest_ishap_cpu(p, c.codes, imp, *bg, paths=paths)
        errs[f"ishap R={r}"] = np.abs(got - ac.reference(forest, kind, "ishap", r)).max()
        ibase = cpu_ref.forest_ishap_base_cpu(p, *bg, paths=paths)
        errs[f"ishap base R={r}"] = abs(ibase - ac.ref_ishap_base(p, c.bg_codes[:r], c.bg_nums[:r]))
        if r == 1:  # row 0 is the background row: every player a dummy
            assert (got[0] == 0.0).all() and (ac.reference(forest, kind, "ishap", 1)[0] == 0.0).all()
    print(f"{forest}/{kind}: " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) <= BRUTE, errs
    # additivity of the references themselves (exact before their rounding)
    out = ac.naive_output(p, c.codes, c.nums)
    np.testing.assert_allclose(p.cls_base_value + ac.reference(forest, kind, "contrib").sum(1),
                               out, rtol=0, atol=BRUTE)  # fmt: skip
    np.testing.assert_allclose(ac.ref_shap_base(p) + ac.reference(forest, kind, "shap").sum(1),
                               out, rtol=0, atol=BRUTE)  # fmt: skip


# ------------------------------------------- the cases hold what they claim


def test_sizes_and_chunk_targets():
    for forest, kind in BUILDS:
        c, p = ac.case(forest), ac.model(forest, kind)
        assert p.cls_n_trees <= 40 and len(c.codes) == len(c.bg_codes) == 129
        assert p.cls_kind == kind and (p.cls_bias != 0.0) == (kind == 1)
        values = p.cls_nodes[p.cls_nodes[:, 0] < 0, 1].view(np.float32)
        assert (values > 0).any() and (values < 0).any() and (values == 0.0).any()
        n_leaves = _paths(forest, kind)[0].n_leaves
        for method in ac.METHODS:
            per_block = 16 if method == "inter" else 128
            n = p.cls_n_trees if method == "contrib" else n_leaves
            for b in ac.ROWS[method]:
                rb = -(-b // per_block)
                for want in (1, 2, 3, n - 1, n):
                    assert ac.launch_chunks(want * rb, rb, n) == want
    assert {-(-b // 16) for b in ac.ROWS["inter"]} == {1, 2, 3}
    assert {-(-b // 128) for b in ac.ROWS["shap"]} == {1, 2}


def test_transitions_forest():
    paths, _ = _paths("transitions")
    counts = _group_counts(paths).tolist()
    assert {0, 1, 2, 3, 16, 17, 23} <= set(counts) and max(counts) == 23
    back_to_back = set(zip(counts, counts[1:]))
    assert {(23, 1), (1, 17), (16, 0), (0, 23), (23, 0), (0, 1), (23, 17), (1, 0),
            (23, 23), (17, 17), (16, 16)} <= back_to_back  # fmt: skip
    # with two and three chunks a block still meets long paths next to short
    for chunks in (2, 3):
        seen = set()
        for c in range(chunks):
            seen |= set(zip(counts[c::chunks], counts[c::chunks][1:]))
        assert any(a >= 16 and b <= 1 for a, b in seen), chunks
        assert any(a <= 1 and b >= 16 for a, b in seen), chunks
    # one path folds three splits of a numeric column and both codes of a
    # categorical column into two players
    flags = paths.splits[:, 3].view(np.uint32).astype(np.int64)
    player = (flags >> SHAP_PLAYER_SHIFT) & 0xFF
    code = (flags >> SHAP_CODE_SHIFT) - 1
    folded = False
    for lo, hi in zip(paths.leaf_off[:-1], paths.leaf_off[1:]):
        pl, cd = player[lo:hi], code[lo:hi]
        folded |= (pl == N_CAT + 5).sum() == 3 and set(cd[pl == 2].tolist()) == {0, 1}
    assert folded
    # rows 0 and 1 follow the whole caterpillar, row 0 through an imputed NaN
    c, p = ac.case("transitions"), ac.model("transitions")
    assert np.isnan(c.nums[0, c.notes["nan_col"]])
    w = ac.Walk(p)
    deep = [lf for lf in w.leaves if len(lf.path) == 26]
    for row in w.rows(c.codes[:2], c.nums[:2]):
        followed = [all(w.right(f, t, row) == r for f, t, r, _ in lf.path) for lf in deep]
        assert sum(followed) == 4  # one leaf of each of the four caterpillars


def test_stripes_forest():
    paths, _ = _paths("stripes")
    depth = np.diff(paths.leaf_off)
    assert (depth[0::3] == 0).all() and (depth[1::3] == 1).all() and (depth[2::3] == 1).all()
    assert paths.n_leaves % 3 == 0  # chunk 0 of 3 sees leaves 0, 3, ...: root leaves only


def test_cover_forest():
    c, p = ac.case("cover"), ac.model("cover")
    paths, _ = _paths("cover")
    frac = paths.splits[:, 2].view(np.float32)
    assert (frac == 0.0).any() and (frac == 1.0).any() and (frac == np.float32(2.0**-20)).any()
    assert (frac == np.float32(1.0 - 2.0**-20)).any()
    flags = paths.splits[:, 3].view(np.uint32).astype(np.int64)
    player = (flags >> SHAP_PLAYER_SHIFT) & 0xFF
    assert not set(player.tolist()) & set(ac.COVER_UNSPLIT)
    assert set(player.tolist()) | set(ac.COVER_UNSPLIT) == set(range(N_SRC))
    x3, x4 = N_CAT + 3, N_CAT + 4
    for lo, hi in zip(paths.leaf_off[:-1], paths.leaf_off[1:]):
        assert not {x3, x4} <= set(player[lo:hi].tolist())
    # the zero-cover children of trees a and b: taken and not taken
    assert set((c.nums[1:5, 0] <= 0.0).tolist()) == {True, False}
    assert set((c.nums[1:5, 5] <= 0.0).tolist()) == {True, False}
    # exact zeros of the references (the GPU test asserts the same bit for bit)
    shap, inter = ac.reference("cover", 0, "shap"), ac.reference("cover", 0, "inter")
    assert (shap[:, list(ac.COVER_UNSPLIT)] == 0.0).all()
    assert (inter[:, x3, x4] == 0.0).all()
    imp = cpu_ref.impute_nums(p, c.nums)
    left0 = imp[:, 0] <= 0.0  # follows z = 1, off the z = 0 group: tree a gives 0
    assert (shap[left0][:, [N_CAT, N_CAT + 1]] == 0.0).all() and (shap[~left0, N_CAT] != 0.0).all()
    right5 = ~(imp[:, 5] <= 0.0)  # follows z = 1 of tree b
    assert (shap[right5, N_CAT + 5] == 0.0).all() and (shap[~right5, N_CAT + 5] != 0.0).all()


def _edges_hit(p, paths, codes, nums) -> set[str]:
    """Which compare edges some (row, split record) of the table sits on."""
    sp = paths.splits
    flags = sp[:, 3].view(np.uint32).astype(np.int64)
    recs = set(zip(((flags >> SHAP_PLAYER_SHIFT) & 0xFF).tolist(),
                   ((flags >> SHAP_CODE_SHIFT) - 1).tolist(),
                   sp[:, 1].view(np.float32).tolist()))  # fmt: skip
    up = lambda t: float(np.nextafter(np.float32(t), np.float32(np.inf)))  # noqa: E731
    down = lambda t: float(np.nextafter(np.float32(t), np.float32(-np.inf)))  # noqa: E731
    hit = set()
    for pl, code, thr in recs:
        if code >= 0:
            hit |= {f"cat_{code}_{have}" for have in set(codes[:, pl].tolist())}
            continue
        col = nums[:, pl - N_CAT]
        med = float(p.medians[pl - N_CAT])
        x = col[~np.isnan(col)].astype(np.float64)
        tests = {"eq": (x == thr).any(), "up": (x == up(thr)).any(), "down": (x == down(thr)).any(),
                 "pos_inf": (x == np.inf).any(), "neg_inf": (x == -np.inf).any(),
                 "nan_median_eq": np.isnan(col).any() and med == thr,
                 "nan_median_up": np.isnan(col).any() and med == up(thr)}  # fmt: skip
        if thr == 0.0:
            tests |= {"zero_neg": ((x == 0.0) & np.signbit(x)).any(),
                      "zero_pos": ((x == 0.0) & ~np.signbit(x)).any(),
                      "zero_tiny": (x == ac.TINY).any(), "zero_neg_tiny": (x == -ac.TINY).any()}  # fmt: skip
        hit |= {k for k, v in tests.items() if v}
    return hit


def test_threshold_forest():
    c, p = ac.case("threshold"), ac.model("threshold")
    paths, _ = _paths("threshold")
    assert int(_group_counts(paths).max()) <= 9  # the brute-force cap
    n = c.notes["n_edge"]
    assert _edges_hit(p, paths, c.codes[:n], c.nums[:n]) == set(ac.THRESHOLD_EDGES)
    assert _edges_hit(p, paths, c.bg_codes, c.bg_nums) == set(ac.THRESHOLD_EDGES)
    # numeric 0 and 1 meet their threshold on a left- and a right-going path
    flags = paths.splits[:, 3].view(np.uint32).astype(np.int64)
    player = (flags >> SHAP_PLAYER_SHIFT) & 0xFF
    for pl in (N_CAT, N_CAT + 1):
        assert set((flags[player == pl] & 1).tolist()) == {0, 1}
    # neighbours across an edge get different attributions from every method
    for method in ac.METHODS:
        ref = ac.reference("threshold", 0, method, 129 if method == "ishap" else 0)
        for a, b in c.notes["neighbours"]:
            if max(a, b) < len(ref):
                assert np.abs(ref[a] - ref[b]).max() > SEEN, (method, a, b)
    assert max(max(pair) for pair in c.notes["neighbours"]) < 129
    assert any(max(pair) < 33 for pair in c.notes["neighbours"])


@pytest.mark.parametrize("forest", ac.FORESTS)
def test_background_sets(forest):
    c, p = ac.case(forest), ac.model(forest)
    paths, _ = _paths(forest)
    ix = cpu_ref._IshapIndex(paths)
    rows = ix.masks(0, paths.n_leaves, c.codes, cpu_ref.impute_nums(p, c.nums))
    for r in ac.BG_ROWS:
        assert np.isnan(c.bg_nums[:r]).any() and (c.bg_codes[:r] == -1).any()
        np.testing.assert_array_equal(c.bg_codes[0], c.codes[0])
        np.testing.assert_array_equal(c.bg_nums[0].view(np.int32), c.nums[0].view(np.int32))
        bg = ix.masks(0, paths.n_leaves, c.bg_codes[:r], cpu_ref.impute_nums(p, c.bg_nums[:r]))
        for b in ac.ROWS["ishap"]:
            dead = (rows[:, :b, None] | bg[:, None, :]) != ix.full[:, None, None]
            live = ~dead & (rows[:, :b, None] != bg[:, None, :])
            # (row 0 against itself alone: dead off its own paths, dummies on them)
            assert dead.any() and (live.any() or (b == 1 and r == 1)), (r, b)


# --------------------------------------------------------- mutations are seen


def _mutant_and_reference(forest, kind, method, mutation, chunks):
    c, p = ac.case(forest), ac.model(forest, kind)
    b = 17
    args = (p, c.codes[:b], c.nums[:b])
    if method == "ishap":
        args += (c.bg_codes[:2], c.bg_nums[:2])
    fn = {"contrib": ac.ref_contrib, "shap": ac.ref_shap, "inter": ac.ref_inter,
          "ishap": ac.ref_ishap}[method]  # fmt: skip
    ref = ac.reference(forest, kind, method, 2 if method == "ishap" else 0)[:b]
    with np.errstate(invalid="ignore"):
        return fn(*args, mutation=mutation, chunks=chunks), ref


@pytest.mark.parametrize(
    "mutation,method", [(m, k) for m in ac.ATTR_MUTATIONS for k in ac.MUTATION_METHODS[m]]
)
def test_cases_see_mutation(mutation, method):
    """A reference with one deliberate error moves at least one committed
    case by more than 1e-6, for every method the error applies to: the cases
    would catch a kernel that made it. (The kernels are never run wrong.)"""
    seen = []
    for forest in ("threshold", "cover", "stripes", "transitions"):
        for chunks in (1, 2, 3) if mutation == "root_leaf_breaks" else (1,):
            bad, good = _mutant_and_reference(forest, 0, method, mutation, chunks)
            diff = float(np.nan_to_num(np.abs(bad - good), nan=np.inf).max())
            if diff > SEEN:
                seen.append(f"{forest}/chunks={chunks}: {diff:.2e}")
        if seen and forest != "threshold":
            break
    print(f"{mutation} on {method}: seen by {seen}")
    assert seen


def test_mutations_are_listed_once_and_leave_other_methods_alone():
    assert set(ac.MUTATION_METHODS) == set(ac.ATTR_MUTATIONS)
    assert len(set(ac.ATTR_MUTATIONS)) == len(ac.ATTR_MUTATIONS) >= 11
    for mutation in ac.ATTR_MUTATIONS:
        for method in set(ac.METHODS) - set(ac.MUTATION_METHODS[mutation]):
            bad, good = _mutant_and_reference("threshold", 0, method, mutation, 2)
            np.testing.assert_array_equal(bad, good, err_msg=f"{mutation} on {method}")

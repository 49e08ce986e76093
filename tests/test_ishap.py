"""Interventional TreeSHAP against a background sample: the sample in the
detector, the pack and the broadcast, the CPU reference (closed-form pair
rule over the path table), the engine's method="interventional" and
POST /explain?method=interventional.

The game: players are the 23 source columns (all one-hot features of a
categorical column are one player). For explained row x, background row r and
coalition S the hybrid row takes x on the columns of S and r elsewhere;
val(S) = mean_r f(hybrid), f the raw model output (probability, or log-odds
for gradient boosting). Tolerances: 1e-12 reference vs brute force (and vs
itself in another summation order), 1e-14 hand cases with exact fractions."""

from __future__ import annotations

import dataclasses
import itertools
import math
import multiprocessing as mp
import os
from fractions import Fraction

import numpy as np
import pytest

from _shap_models import (
    CATERPILLAR_SPLITS,
    N_ONEHOT,
    N_SRC,
    caterpillar_model,
    caterpillar_rows,
    f32bits,
    fit_packed,
    hand_model,
)
from creditcore.engine import ExplainTooLarge, ExplainUnavailable, ScoringEngine
from creditcore.ops import cpu_ref
from creditcore.pack import N_CAT, N_NUM, PackedModel, build_shap_paths, encode_batch
from creditcore.schema import FEATURES, SAMPLE_REQUEST

METHOD = "interventional"


def _ishap(packed, codes, nums, bg_codes, bg_nums, **kw):
    return cpu_ref.forest_ishap_cpu(
        packed,
        codes,
        cpu_ref.impute_nums(packed, nums),
        bg_codes,
        cpu_ref.impute_nums(packed, bg_nums),
        **kw,
    )


def _base(packed, bg_codes, bg_nums):
    return cpu_ref.forest_ishap_base_cpu(
        packed, bg_codes, cpu_ref.impute_nums(packed, bg_nums)
    )


def _raw_score(packed, codes, nums):
    """Model output in the attribution space (log-odds for GBT)."""
    p = cpu_ref.score_forest_cpu(packed, codes, cpu_ref.impute_nums(packed, nums))
    return np.log(p / (1.0 - p)) if packed.cls_kind == 1 else p


def _player(packed, feat) -> int:
    col = int(packed.feat_col[feat])
    return col if packed.feat_code[feat] >= 0 else N_CAT + col


# ------------------------------------------------------ brute-force oracle


def _tree_eval(packed, t, codes, nums_imp) -> np.ndarray:
    """Leaf value of tree t per row, walking the packed nodes (f32 compares,
    as the scorer); uses neither the path table nor the pair rule."""
    lo = int(packed.cls_tree_offsets[t])
    nodes = packed.cls_nodes[lo : int(packed.cls_tree_offsets[t + 1])]
    bits = nodes[:, 1].view(np.float32)
    cur = np.zeros(len(codes), dtype=np.int64)
    while True:
        feat = nodes[cur, 0]
        alive = np.flatnonzero(feat >= 0)
        if not len(alive):
            return bits[cur].astype(np.float64)
        f = feat[alive]
        col, code = packed.feat_col[f], packed.feat_code[f]
        x = np.where(
            code >= 0,
            (codes[alive, np.where(code >= 0, col, 0)] == code).astype(np.float32),
            nums_imp[alive, np.where(code >= 0, 0, col)],
        ).astype(np.float32)
        left = x <= bits[cur[alive]]
        cur[alive] = np.where(left, nodes[cur[alive], 2], nodes[cur[alive], 3])


def brute_force_ishap(packed, codes, nums, bg_codes, bg_nums):
    """Interventional Shapley values by subset enumeration over the players
    of each tree, scoring every hybrid row, and the base value (the empty
    coalition: the mean output over the background rows)."""
    x_imp = cpu_ref.impute_nums(packed, nums)
    r_imp = cpu_ref.impute_nums(packed, bg_nums)
    nb, nr = len(codes), len(bg_codes)
    # all (x, r) pairs, x-major
    xc, xn = np.repeat(codes, nr, axis=0), np.repeat(x_imp, nr, axis=0)
    rc, rn = np.tile(bg_codes, (nb, 1)), np.tile(r_imp, (nb, 1))
    phi = np.zeros((nb, N_SRC), dtype=np.float64)
    base = 0.0
    T = packed.cls_n_trees
    for t in range(T):
        lo, hi = packed.cls_tree_offsets[t], packed.cls_tree_offsets[t + 1]
        feats = packed.cls_nodes[lo:hi, 0]
        players = sorted({_player(packed, int(f)) for f in feats if f >= 0})
        m = len(players)
        assert m <= 9, "brute force is exponential in the players of a tree"
        value = {}
        for k in range(m + 1):
            for s in itertools.combinations(players, k):
                hc, hn = rc.copy(), rn.copy()
                for pl in s:
                    if pl < N_CAT:
                        hc[:, pl] = xc[:, pl]
                    else:
                        hn[:, pl - N_CAT] = xn[:, pl - N_CAT]
                leaf = _tree_eval(packed, t, hc, hn).reshape(nb, nr)
                value[frozenset(s)] = leaf.mean(axis=1)
        base += float(value[frozenset()][0])
        for i in players:
            rest = [q for q in players if q != i]
            for k in range(m):
                w = math.factorial(k) * math.factorial(m - 1 - k) / math.factorial(m)
                for s in itertools.combinations(rest, k):
                    s = frozenset(s)
                    phi[:, i] += w * (value[s | {i}] - value[s])
    if packed.cls_kind == 1:
        return phi, base + packed.cls_bias
    return phi / T, base / T


@pytest.fixture(scope="module")
def detectors(train_df):
    from creditcore.train import fit_detectors

    return fit_detectors(train_df)


SMALL = {
    "rf": ({"n_estimators": 8, "max_depth": 3, "random_state": 0}, "rf"),
    "et": ({"n_estimators": 8, "max_depth": 3, "random_state": 0}, "et"),
    "gbt": ({"n_estimators": 20, "max_depth": 3, "random_state": 0}, "gbt"),
}


@pytest.mark.parametrize("family", ["rf", "et", "gbt"])
def test_brute_force_oracle(train_df, detectors, score_batch, family):
    params, algo = SMALL[family]
    p = fit_packed(train_df, detectors, params, algo)
    assert p.cls_kind == (1 if family == "gbt" else 0)
    codes, nums = encode_batch(score_batch.iloc[:32], p.vocabs)  # NaN + unknown rows
    assert np.isnan(nums).any() and (codes < 0).any()
    bg_codes, bg_nums = encode_batch(score_batch.iloc[100:116], p.vocabs)
    bg_nums[5, 0] = np.nan
    want, want_base = brute_force_ishap(p, codes, nums, bg_codes, bg_nums)
    got = _ishap(p, codes, nums, bg_codes, bg_nums)
    base = _base(p, bg_codes, bg_nums)
    err = np.abs(got - want).max()
    print(f"{family}: brute force max |err| = {err:.3e}, base err = {abs(base - want_base):.3e}")
    assert np.abs(want).max() > 1e-4  # the oracle is not trivially zero
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    np.testing.assert_allclose(base, want_base, rtol=0, atol=1e-12)
    np.testing.assert_allclose(
        base + got.sum(1), _raw_score(p, codes, nums), rtol=0, atol=1e-12
    )


# --------------------------------------------------------------- hand cases


def _one_split(v_left: float, v_right: float):
    nodes = np.array(
        [
            [N_ONEHOT + 0, f32bits(0.0), 1, 2],
            [-1, f32bits(v_left), 0, 0],
            [-1, f32bits(v_right), 0, 0],
        ],
        dtype=np.int32,
    )
    return nodes, np.array([10.0, 4.0, 6.0])


def _and_tree(first: int, second: int):
    """leaf 1.0 iff numeric `first` > 0 and numeric `second` > 0; balanced."""
    nodes = np.array(
        [
            [N_ONEHOT + first, f32bits(0.0), 1, 2],
            [-1, f32bits(0.0), 0, 0],
            [N_ONEHOT + second, f32bits(0.0), 3, 4],
            [-1, f32bits(0.0), 0, 0],
            [-1, f32bits(1.0), 0, 0],
        ],
        dtype=np.int32,
    )
    return nodes, np.array([100.0, 50.0, 50.0, 25.0, 25.0])


def _rows(n, **cols):
    codes = np.zeros((n, N_CAT), dtype=np.int16)
    nums = np.zeros((n, N_NUM), dtype=np.float32)
    for j, v in cols.items():
        nums[:, int(j[1:])] = v
    return codes, nums


def test_single_split_is_value_difference():
    p = hand_model(*[[x] for x in _one_split(0.25, 0.75)])
    x = _rows(2, n0=[1.0, -1.0])  # right leaf, left leaf
    r = _rows(1, n0=[-1.0])  # left leaf
    phi = _ishap(p, *x, *r)
    want = np.zeros((2, N_SRC))
    want[0, N_CAT] = 0.75 - 0.25  # v_x - v_r
    np.testing.assert_allclose(phi, want, rtol=0, atol=1e-14)
    assert _base(p, *r) == 0.25
    assert (phi[1] == 0.0).all()  # same side as the background row


def test_and_tree_is_symmetric_in_both_split_orders():
    x = _rows(1, n0=[1.0], n1=[1.0])
    r = _rows(1, n0=[-1.0], n1=[-1.0])
    a, b = N_CAT + 0, N_CAT + 1
    saabas = []
    for first, second in ((0, 1), (1, 0)):
        p = hand_model(*[[t] for t in _and_tree(first, second)])
        phi = _ishap(p, *x, *r)
        np.testing.assert_allclose(phi[0, [a, b]], [0.5, 0.5], rtol=0, atol=1e-14)
        assert np.abs(np.delete(phi[0], [a, b])).max() == 0.0
        assert _base(p, *r) == 0.0
        saabas.append(cpu_ref.forest_contrib_cpu(p, x[0], cpu_ref.impute_nums(p, x[1]))[0, a])
    assert abs(saabas[0] - saabas[1]) > 0.2  # Saabas depends on the split order


def test_background_averaging_r1_and_r3():
    p = hand_model(*[[t] for t in _and_tree(0, 1)])
    x = _rows(4, n0=[1, 1, -1, -1], n1=[1, -1, 1, -1])
    bg = _rows(3, n0=[-1, 1, 1], n1=[-1, -1, 1])
    single = [
        _ishap(p, *x, bg[0][k : k + 1], bg[1][k : k + 1]) for k in range(3)
    ]
    # R = 1 against (-1, -1): row (1, 1) splits the whole 1.0 evenly
    np.testing.assert_allclose(single[0][0, N_CAT : N_CAT + 2], [0.5, 0.5], rtol=0, atol=1e-14)
    # R = 1 against (1, -1): only numeric 1 differs from row (1, 1)
    np.testing.assert_allclose(single[1][0, N_CAT : N_CAT + 2], [0.0, 1.0], rtol=0, atol=1e-14)
    all3 = _ishap(p, *x, *bg)
    np.testing.assert_allclose(all3, sum(single) / 3.0, rtol=0, atol=1e-14)
    np.testing.assert_allclose(all3[0, N_CAT : N_CAT + 2], [1 / 6, 1 / 2], rtol=0, atol=1e-14)
    base = _base(p, *bg)
    np.testing.assert_allclose(base, 1.0 / 3.0, rtol=0, atol=1e-14)
    np.testing.assert_allclose(base + all3.sum(1), _raw_score(p, *x), rtol=0, atol=1e-14)


def test_background_equal_to_the_row_gives_zeros():
    p = caterpillar_model()
    codes, nums = caterpillar_rows()
    for k in range(len(codes)):
        phi = _ishap(p, codes[k : k + 1], nums[k : k + 1], codes[k : k + 1], nums[k : k + 1])
        assert (phi == 0.0).all(), k


def test_root_leaf_forest():
    leaf = np.array([[-1, f32bits(0.6), 0, 0]], dtype=np.int32)
    p = hand_model([leaf, leaf.copy()], [[10.0], [3.0]])
    codes = np.zeros((4, N_CAT), dtype=np.int16)
    nums = np.ones((4, N_NUM), dtype=np.float32)
    bg = (np.ones((3, N_CAT), dtype=np.int16), np.zeros((3, N_NUM), dtype=np.float32))
    out = ScoringEngine(p, device="cpu").explain_arrays(codes, nums, method=METHOD, background=bg)
    assert (out["contributions"] == 0.0).all()
    assert out["base_value"] == np.float64(np.float32(0.6))
    np.testing.assert_array_equal(out["predictions"], np.float64(np.float32(0.6)))
    assert out["background_rows"] == 3


# -------------------------------------------------------------- caterpillar


def _breaker_of(codes0, nums0):
    """A row that breaks every player of the caterpillar's chain: it fails
    the first chain split of each of the 23 source columns."""
    c, x = codes0.copy(), nums0.copy()
    seen = set()
    for i, (feat, thr) in enumerate(CATERPILLAR_SPLITS):
        left = i % 3 != 1
        pl = feat // 2 if feat < N_ONEHOT else N_CAT + feat - N_ONEHOT
        if pl in seen:
            continue
        seen.add(pl)
        if feat < N_ONEHOT:
            # one-hot(code) <= 0.5 goes left: break "left" by having the
            # code, break "right" by not having it
            c[feat // 2] = feat % 2 if left else 1 - feat % 2
        else:
            x[feat - N_ONEHOT] = thr + 1.0 if left else thr - 1.0
    assert len(seen) == N_SRC
    return c, x


def _caterpillar_pair_oracle(p, xc, xn, rc, rn):
    """phi of one (x, r) pair on the caterpillar straight from its nodes: per
    leaf, a_p / b_p from the chain walk, then the pair rule with exact
    factorials (Fractions). No path table, no weight table. Also returns the
    (nx, nr) of every live leaf."""
    xi = cpu_ref.impute_nums(p, xn[None])[0]
    ri = cpu_ref.impute_nums(p, rn[None])[0]
    nodes = p.cls_nodes
    bits = nodes[:, 1].view(np.float32)

    def goes_left(feat, thr, c, x):
        col, code = int(p.feat_col[feat]), int(p.feat_code[feat])
        v = np.float32(c[col] == code) if code >= 0 else x[col]
        return bool(v <= thr)

    out = [Fraction(0)] * N_SRC
    shapes = []
    k = 0
    a, b = {}, {}  # per player along the chain so far
    while nodes[k, 0] >= 0:
        feat, left, right = int(nodes[k, 0]), int(nodes[k, 2]), int(nodes[k, 3])
        pl = _player(p, feat)
        x_left, r_left = goes_left(feat, bits[k], xc, xi), goes_left(feat, bits[k], rc, ri)
        kids = [(left, True), (right, False)]
        leaves = [(c, d) for c, d in kids if nodes[c, 0] < 0]
        for c, is_left in leaves:
            aa, bb = dict(a), dict(b)
            aa[pl] = aa.get(pl, True) and (x_left == is_left)
            bb[pl] = bb.get(pl, True) and (r_left == is_left)
            if not all(aa[q] or bb[q] for q in aa):
                continue
            xs = [q for q in aa if aa[q] and not bb[q]]
            rs = [q for q in aa if bb[q] and not aa[q]]
            nx, nr = len(xs), len(rs)
            if nx + nr == 0:
                continue
            shapes.append((nx, nr))
            v = Fraction(float(bits[c]))
            f = math.factorial
            for q in xs:
                out[q] += v * Fraction(f(nx - 1) * f(nr), f(nx + nr))
            for q in rs:
                out[q] -= v * Fraction(f(nr - 1) * f(nx), f(nx + nr))
        nxt = [(c, d) for c, d in kids if nodes[c, 0] >= 0]
        if not nxt:
            break
        c, is_left = nxt[0]
        a[pl] = a.get(pl, True) and (x_left == is_left)
        b[pl] = b.get(pl, True) and (r_left == is_left)
        k = c
    return np.array([float(v) for v in out]), shapes


def test_caterpillar_extreme_pairs():
    p = caterpillar_model()
    codes, nums = caterpillar_rows()
    bc, bn = _breaker_of(codes[0], nums[0])
    v_long = np.float64(np.float32(0.875))
    assert _raw_score(p, codes[:1], nums[:1])[0] == v_long  # row 0 follows the chain
    for (xc, xn, rc, rn), corner, sign in (
        ((codes[0], nums[0], bc, bn), (N_SRC, 0), +1.0),
        ((bc, bn, codes[0], nums[0]), (0, N_SRC), -1.0),
    ):
        want, shapes = _caterpillar_pair_oracle(p, xc, xn, rc, rn)
        assert corner in shapes  # the long leaf: all 23 players on one side
        got = _ishap(p, xc[None], xn[None], rc[None], rn[None])[0]
        print(f"caterpillar {corner}: max |err| = {np.abs(got - want).max():.3e}")
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
        # the long leaf hands every player +-v/23 (checked on its own in
        # test_long_leaf_gives_every_player_v_over_23); the rest comes from
        # the off-chain leaves, which the oracle also supplies
        base = _base(p, rc[None], rn[None])
        np.testing.assert_allclose(
            base + got.sum(), _raw_score(p, xc[None], xn[None])[0], rtol=0, atol=1e-12
        )
    # every remaining row against a mixed background, pair by pair
    bgc, bgn = np.stack([bc, codes[9], codes[3]]), np.stack([bn, nums[9], nums[3]])
    got = _ishap(p, codes, nums, bgc, bgn)
    want = np.zeros_like(got)
    for i in range(len(codes)):
        for k in range(3):
            want[i] += _caterpillar_pair_oracle(p, codes[i], nums[i], bgc[k], bgn[k])[0] / 3.0
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    np.testing.assert_allclose(
        _base(p, bgc, bgn) + got.sum(1), _raw_score(p, codes, nums), rtol=0, atol=1e-12
    )


def test_long_leaf_gives_every_player_v_over_23():
    """The chain leaf alone: with the off-chain leaves' values set to zero
    the extreme pairs credit exactly +-v/23 to each of the 23 columns."""
    p = caterpillar_model()
    nodes = p.cls_nodes.copy()
    off_chain = np.arange(1, len(nodes) - 1, 2)
    nodes[off_chain, 1] = f32bits(0.0)
    q = hand_model([nodes], [p.cls_node_cover])
    codes, nums = caterpillar_rows()
    bc, bn = _breaker_of(codes[0], nums[0])
    v = np.float64(np.float32(0.875))
    fwd = _ishap(q, codes[:1], nums[:1], bc[None], bn[None])[0]
    rev = _ishap(q, bc[None], bn[None], codes[:1], nums[:1])[0]
    np.testing.assert_allclose(fwd, np.full(N_SRC, v / N_SRC), rtol=0, atol=1e-14)
    np.testing.assert_allclose(rev, np.full(N_SRC, -v / N_SRC), rtol=0, atol=1e-14)


def test_weight_table():
    w = cpu_ref.ishap_weight_table()
    assert w.shape == (N_SRC + 1, N_SRC + 1) and (w[0] == 0.0).all()
    f = math.factorial
    for a in range(1, N_SRC + 1):
        for b in range(0, N_SRC + 1 - a):
            exact = Fraction(f(a - 1) * f(b), f(a + b))
            assert abs(Fraction(float(w[a, b])) - exact) <= exact * Fraction(1, 2**46), (a, b)
    assert w[N_SRC, 0] == 1.0 / N_SRC and w[1, 0] == 1.0 and w[1, 1] == 0.5


# -------------------------------------------------------------- dummy axiom


def test_unsplit_column_gets_exactly_zero():
    p = caterpillar_model()
    # drop the chain's tail: keep 12 chain splits
    nodes = p.cls_nodes[:25].copy()
    nodes[24] = [-1, f32bits(0.5), 0, 0]
    small = hand_model([nodes], [p.cls_node_cover[:25]])
    codes, nums = caterpillar_rows()
    bc, bn = _breaker_of(codes[0], nums[0])
    phi = _ishap(small, codes, nums, np.stack([bc, codes[10]]), np.stack([bn, nums[10]]))
    used = {_player(small, int(f)) for f in nodes[:, 0] if f >= 0}
    assert 0 < len(used) < N_SRC
    for c in range(N_SRC):
        if c in used:
            assert (phi[:, c] != 0.0).any(), c
        else:
            assert (phi[:, c] == 0.0).all(), c


def test_column_on_which_x_and_background_agree_gets_exactly_zero(packed, score_batch):
    codes, nums = encode_batch(score_batch.iloc[4:12], packed.vocabs)
    bg_codes, bg_nums = packed.bg_codes[:32].copy(), packed.bg_nums[:32].copy()
    before = _ishap(packed, codes, nums, bg_codes, bg_nums)
    cat, num = 3, 0  # repayment_status_1 and credit_limit: both split on
    assert (before[:, cat] != 0.0).any() and (before[:, N_CAT + num] != 0.0).any()
    codes[:, cat] = bg_codes[:, cat] = bg_codes[0, cat]
    nums[:, num] = bg_nums[:, num] = bg_nums[0, num]
    after = _ishap(packed, codes, nums, bg_codes, bg_nums)
    assert (after[:, cat] == 0.0).all() and (after[:, N_CAT + num] == 0.0).all()
    assert np.abs(after).max() > 1e-4


# --------------------------------------------------------------- additivity


def test_additivity_rf(packed, score_batch):
    codes, nums = encode_batch(score_batch.iloc[:8], packed.vocabs)
    out = ScoringEngine(packed, device="cpu").explain_arrays(codes, nums, method=METHOD)
    got = out["contributions"]
    assert got.shape == (8, N_SRC) and got.dtype == np.float64
    assert out["output_space"] == "probability" and out["background_rows"] == 256
    raw = out["base_value"] + got.sum(1)
    err = np.abs(raw - _raw_score(packed, codes, nums)).max()
    print(f"RF additivity max |err| = {err:.3e}")
    np.testing.assert_allclose(raw, _raw_score(packed, codes, nums), rtol=0, atol=1e-9)
    # the base value is the mean model output over the background rows
    np.testing.assert_allclose(
        out["base_value"],
        _raw_score(packed, packed.bg_codes, packed.bg_nums).mean(),
        rtol=0,
        atol=1e-9,
    )


def test_additivity_gbt_log_odds(train_df, detectors, score_batch):
    p = fit_packed(
        train_df, detectors, {"n_estimators": 60, "max_depth": 3, "random_state": 0}, "gbt"
    )
    codes, nums = encode_batch(score_batch.iloc[:16], p.vocabs)
    out = ScoringEngine(p, device="cpu").explain_arrays(codes, nums, method=METHOD)
    assert out["output_space"] == "log_odds"
    raw = out["base_value"] + out["contributions"].sum(1)
    np.testing.assert_allclose(raw, _raw_score(p, codes, nums), rtol=0, atol=1e-9)
    np.testing.assert_allclose(
        out["predictions"],
        cpu_ref.score_forest_cpu(p, codes, cpu_ref.impute_nums(p, nums)),
        rtol=0,
        atol=1e-9,
    )


# ----------------------------------------------------------------- plumbing


def test_pack_background_layout(packed, train_df, loaded_pyfunc):
    assert packed.bg_codes.shape == (256, 9) and packed.bg_codes.dtype == np.int16
    assert packed.bg_nums.shape == (256, 14) and packed.bg_nums.dtype == np.float32
    # reproducible from the seed: sorted draw without replacement, seed 0
    idx = np.sort(np.random.default_rng(0).choice(len(train_df), size=256, replace=False))
    rows = train_df[FEATURES].iloc[idx]
    det = loaded_pyfunc.python_model.drift
    assert det.background.shape == (256, len(FEATURES))
    assert (det.background == rows.values).all()
    want_codes, want_nums = encode_batch(rows.to_dict("records"), packed.vocabs)
    np.testing.assert_array_equal(packed.bg_codes, want_codes)
    np.testing.assert_array_equal(
        packed.bg_nums.view(np.int32), want_nums.astype(np.float32).view(np.int32)
    )


def test_detector_background_options(train_df):
    from creditcore.models.drift import TabularDriftDetector
    from creditcore.pack import pack_drift

    x = train_df[FEATURES].values[:300]
    plain = TabularDriftDetector(x)
    assert not hasattr(plain, "background")  # the default adds no attribute
    a = TabularDriftDetector(x, background_rows=40, background_seed=5)
    b = TabularDriftDetector(x, background_rows=40, background_seed=5)
    c = TabularDriftDetector(x, background_rows=40, background_seed=6)
    assert a.background.shape == (40, len(FEATURES))
    assert (a.background == b.background).all() and not (a.background == c.background).all()
    assert TabularDriftDetector(x, background_rows=1000).background.shape[0] == 300
    vocabs = [sorted(set(map(str, x[:, j]))) for j in range(N_CAT)]
    d = pack_drift(plain, vocabs)
    assert d["bg_codes"] is None and d["bg_nums"] is None
    d = pack_drift(a, vocabs)
    assert d["bg_codes"].shape == (40, N_CAT) and d["bg_nums"].shape == (40, N_NUM)


def test_save_load_roundtrip_and_old_npz(packed, tmp_path):
    path = str(tmp_path / "m.npz")
    packed.save(path)
    re = PackedModel.load(path)
    assert re.bg_codes.dtype == np.int16 and re.bg_nums.dtype == np.float32
    np.testing.assert_array_equal(re.bg_codes, packed.bg_codes)
    np.testing.assert_array_equal(re.bg_nums.view(np.int32), packed.bg_nums.view(np.int32))
    # a file written before the background sample existed
    z = np.load(path, allow_pickle=True)
    old_path = str(tmp_path / "old.npz")
    np.savez_compressed(
        old_path, **{k: z[k] for k in z.files if k not in ("bg_codes", "bg_nums")}
    )
    old = PackedModel.load(old_path)
    assert old.bg_codes is None and old.bg_nums is None
    eng, new = ScoringEngine(old, device="cpu"), ScoringEngine(packed, device="cpu")
    codes, nums = encode_batch(SAMPLE_REQUEST, old.vocabs)
    with pytest.raises(ExplainUnavailable, match="background"):
        eng.explain_arrays(codes, nums, method=METHOD)
    for method in ("saabas", "shap"):
        np.testing.assert_array_equal(
            eng.explain_arrays(codes, nums, method=method)["contributions"],
            new.explain_arrays(codes, nums, method=method)["contributions"],
        )
    # ... but an explicit background serves it
    bg = (packed.bg_codes[:8], packed.bg_nums[:8])
    np.testing.assert_array_equal(
        eng.explain_arrays(codes, nums, method=METHOD, background=bg)["contributions"],
        new.explain_arrays(codes, nums, method=METHOD, background=bg)["contributions"],
    )
    old.save(str(tmp_path / "again.npz"))
    again = np.load(str(tmp_path / "again.npz"), allow_pickle=True)
    assert "bg_codes" not in again and "bg_nums" not in again


def test_model_without_cover_still_explains(packed):
    coverless = dataclasses.replace(packed, cls_node_cover=None)
    codes, nums = encode_batch(SAMPLE_REQUEST * 2, packed.vocabs)
    bg = (packed.bg_codes[:16], packed.bg_nums[:16])
    a = ScoringEngine(coverless, device="cpu").explain_arrays(
        codes, nums, method=METHOD, background=bg
    )
    b = ScoringEngine(packed, device="cpu").explain_arrays(
        codes, nums, method=METHOD, background=bg
    )
    np.testing.assert_array_equal(a["contributions"], b["contributions"])
    assert a["base_value"] == b["base_value"]
    with pytest.raises(ExplainUnavailable):
        ScoringEngine(coverless, device="cpu").explain_arrays(codes, nums, method="shap")
    paths, base = build_shap_paths(coverless, require_cover=False)
    assert np.isnan(base) and paths.n_leaves == build_shap_paths(packed)[0].n_leaves


def test_engine_override_keys_and_caps(packed, score_batch, monkeypatch):
    eng = ScoringEngine(packed, device="cpu")
    codes, nums = encode_batch(score_batch.iloc[:8], packed.vocabs)
    own = eng.explain_arrays(codes, nums, method=METHOD)
    shap = eng.explain_arrays(codes, nums, method="shap")
    assert set(own) == set(shap) | {"background_rows"}
    assert own["background_rows"] == 256
    np.testing.assert_allclose(own["predictions"], shap["predictions"], rtol=0, atol=1e-9)
    assert not np.allclose(own["contributions"], shap["contributions"], atol=1e-4)
    # the override is honoured (and is not mistaken for the cached sample)
    bg = (packed.bg_codes[40:56], packed.bg_nums[40:56])
    over = eng.explain_arrays(codes, nums, method=METHOD, background=bg)
    assert over["background_rows"] == 16
    np.testing.assert_allclose(
        over["contributions"], _ishap(packed, codes, nums, *bg), rtol=0, atol=1e-14
    )
    assert over["base_value"] == _base(packed, *bg) != own["base_value"]
    again = eng.explain_arrays(codes, nums, method=METHOD)
    assert again["base_value"] == own["base_value"]
    np.testing.assert_array_equal(again["contributions"], own["contributions"])
    rec = eng.explain_records(SAMPLE_REQUEST * 2, method=METHOD, background=bg)
    assert rec["contributions"].shape == (2, N_SRC) and rec["background_rows"] == 16
    # refused inputs
    with pytest.raises(ValueError, match="method"):
        eng.explain_arrays(codes, nums, method="lime")
    with pytest.raises(ValueError, match="background"):
        eng.explain_arrays(codes, nums, method="shap", background=bg)
    assert ScoringEngine.ISHAP_MAX_BACKGROUND == 1024
    many = (np.zeros((1025, N_CAT), dtype=np.int16), np.zeros((1025, N_NUM), dtype=np.float32))
    with pytest.raises(ValueError, match="1024"):
        eng.explain_arrays(codes, nums, method=METHOD, background=many)
    with pytest.raises(ValueError, match="background"):
        eng.explain_arrays(codes, nums, method=METHOD, background=(many[0][:0], many[1][:0]))
    # the row cap is SHAP_MAX_ROWS
    monkeypatch.setattr(ScoringEngine, "SHAP_MAX_ROWS", 4)
    with pytest.raises(ExplainTooLarge):
        eng.explain_arrays(codes[:5], nums[:5], method=METHOD, background=bg)
    assert eng.explain_arrays(codes[:4], nums[:4], method=METHOD, background=bg)[
        "contributions"
    ].shape == (4, N_SRC)


def test_launch_split_by_pairs(packed, score_batch, monkeypatch):
    eng = ScoringEngine(packed, device="cpu")
    codes, nums = encode_batch(score_batch.iloc[:8], packed.vocabs)
    bg = (packed.bg_codes[:16], packed.bg_nums[:16])
    whole = eng.explain_arrays(codes, nums, method=METHOD, background=bg)
    sizes = []
    real = cpu_ref.forest_ishap_cpu

    def spy(p, c, *a, **kw):
        sizes.append(len(c))
        return real(p, c, *a, **kw)

    monkeypatch.setattr(cpu_ref, "forest_ishap_cpu", spy)
    monkeypatch.setattr(ScoringEngine, "ISHAP_MAX_PAIRS", 3 * 16 + 5)  # 3 rows per launch
    split = eng.explain_arrays(codes, nums, method=METHOD, background=bg)
    assert sizes == [3, 3, 2]
    np.testing.assert_allclose(
        split["contributions"], whole["contributions"], rtol=0, atol=1e-12
    )
    assert split["base_value"] == whole["base_value"]
    # a sample larger than the pair budget still makes progress row by row
    sizes.clear()
    monkeypatch.setattr(ScoringEngine, "ISHAP_MAX_PAIRS", 7)
    one = eng.explain_arrays(codes[:2], nums[:2], method=METHOD, background=bg)
    assert sizes == [1, 1]
    np.testing.assert_allclose(
        one["contributions"], whole["contributions"][:2], rtol=0, atol=1e-12
    )


def test_leaf_chunking_does_not_change_the_result(packed, score_batch):
    codes, nums = encode_batch(score_batch.iloc[:8], packed.vocabs)
    bg = (packed.bg_codes[:32], packed.bg_nums[:32])
    whole = _ishap(packed, codes, nums, *bg)
    tiny = _ishap(packed, codes, nums, *bg, max_bytes=1 << 16)
    np.testing.assert_allclose(tiny, whole, rtol=0, atol=1e-12)
    imp = cpu_ref.impute_nums(packed, bg[1])
    np.testing.assert_allclose(
        cpu_ref.forest_ishap_base_cpu(packed, bg[0], imp, max_bytes=1 << 12),
        cpu_ref.forest_ishap_base_cpu(packed, bg[0], imp),
        rtol=0,
        atol=1e-12,
    )


def _bcast_worker(rank: int, world: int, port: int, npz_path: str, q):
    try:
        import torch.distributed as dist

        from creditcore.parallel import broadcast_packed

        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        src = PackedModel.load(npz_path) if rank == 0 else None
        got = broadcast_packed(src, device="cpu", src=0)
        if got.bg_codes is None or got.bg_nums is None:
            q.put((rank, None))
        else:
            q.put(
                (
                    rank,
                    (
                        str(got.bg_codes.dtype),
                        got.bg_codes.tolist(),
                        str(got.bg_nums.dtype),
                        got.bg_nums.view(np.int32).tolist(),
                    ),
                )
            )
        dist.destroy_process_group()
    except Exception as e:  # surface worker failures to the parent
        q.put((rank, f"ERROR: {type(e).__name__}: {e}"))


def _bcast(npz_path: str, port: int) -> dict:
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_bcast_worker, args=(r, 2, port, npz_path, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = {}
    for _ in range(2):
        rank, a = q.get(timeout=180)
        assert not (isinstance(a, str) and a.startswith("ERROR")), a
        results[rank] = a
    for p in procs:
        p.join(timeout=60)
    return results


@pytest.mark.slow
def test_broadcast_carries_background(packed, tmp_path):
    path = str(tmp_path / "packed.npz")
    nums = packed.bg_nums.copy()
    nums[3, 2] = np.nan  # NaNs travel bit for bit
    dataclasses.replace(packed, bg_nums=nums).save(path)
    res = _bcast(path, 29547)
    cd, codes, nd, bits = res[1]
    assert cd == "int16" and nd == "float32"
    assert codes == packed.bg_codes.tolist()
    assert bits == nums.view(np.int32).tolist()  # bit-identical
    assert res[0] == res[1]
    old = str(tmp_path / "old.npz")
    dataclasses.replace(packed, bg_codes=None, bg_nums=None).save(old)
    res = _bcast(old, 29548)
    assert res[0] is None and res[1] is None


# --------------------------------------------------------------------- HTTP

DEFAULT_KEYS = {
    "output_space", "base_value", "features", "predictions", "contributions", "top_reasons",
}


@pytest.fixture(scope="module")
def client(model_dir):
    from fastapi.testclient import TestClient

    from creditcore.config import ServeConfig
    from creditcore.serve import create_app

    cfg = ServeConfig()
    cfg.model_directory = model_dir
    cfg.device = "cpu"
    with TestClient(create_app(cfg)) as c:
        yield c


def test_http_interventional(client, packed):
    r = client.post(f"/explain?method={METHOD}&top_k=4", json=SAMPLE_REQUEST)
    assert r.status_code == 200
    body = r.json()
    assert set(body) == DEFAULT_KEYS | {"method", "background_rows"}
    assert body["method"] == METHOD and body["background_rows"] == 256
    assert body["features"] == list(FEATURES) and body["output_space"] == "probability"
    row = body["contributions"][0]
    assert len(row) == 23
    assert body["base_value"] == _base(packed, packed.bg_codes, packed.bg_nums)
    total = body["base_value"] + sum(row)
    assert total == pytest.approx(body["predictions"][0], abs=1e-12)
    p = client.post("/predict", json=SAMPLE_REQUEST).json()["predictions"][0]
    assert p == pytest.approx(total, abs=1e-9)
    # top_reasons: the largest strictly positive values, descending
    want = sorted((j for j in range(23) if row[j] > 0.0), key=lambda j: (-row[j], j))[:4]
    assert [x["feature"] for x in body["top_reasons"][0]] == [FEATURES[j] for j in want]
    assert [x["contribution"] for x in body["top_reasons"][0]] == [row[j] for j in want]
    assert want


def test_http_other_methods_keep_their_keys(client):
    default = client.post("/explain", json=SAMPLE_REQUEST)
    assert default.status_code == 200 and set(default.json()) == DEFAULT_KEYS
    for method in ("saabas", "shap"):
        r = client.post(f"/explain?method={method}", json=SAMPLE_REQUEST)
        assert r.status_code == 200 and set(r.json()) == DEFAULT_KEYS | {"method"}
    bad = client.post("/explain?method=bogus", json=SAMPLE_REQUEST)
    assert bad.status_code == 422
    for method in ("saabas", "shap", METHOD):
        assert method in bad.json()["detail"]
    spec = client.get("/openapi.json").json()
    props = spec["components"]["schemas"]["ExplainOutput"]["properties"]
    assert "background_rows" in props and "method" in props


def test_http_interventional_errors(model_dir, packed, monkeypatch):
    """413 above the row cap and 501 for a model packed without a background
    sample, which still serves the other methods."""
    from fastapi.testclient import TestClient

    from creditcore import serve
    from creditcore.config import ServeConfig

    cfg = ServeConfig()
    cfg.model_directory = model_dir
    cfg.device = "cpu"
    with TestClient(serve.create_app(cfg)) as c:
        engines = serve.state["engines"]
        monkeypatch.setattr(ScoringEngine, "SHAP_MAX_ROWS", 2)
        assert c.post(f"/explain?method={METHOD}", json=SAMPLE_REQUEST * 3).status_code == 413
        assert c.post(f"/explain?method={METHOD}", json=SAMPLE_REQUEST * 2).status_code == 200
        assert c.post("/explain", json=SAMPLE_REQUEST * 3).status_code == 200
        monkeypatch.undo()

        bare = dataclasses.replace(packed, bg_codes=None, bg_nums=None)
        serve.state["engines"] = [ScoringEngine(bare, device="cpu")]
        try:
            r = c.post(f"/explain?method={METHOD}", json=SAMPLE_REQUEST)
            assert r.status_code == 501 and "background sample" in r.json()["detail"]
            assert c.post("/explain", json=SAMPLE_REQUEST).status_code == 200
            assert c.post("/explain?method=shap", json=SAMPLE_REQUEST).status_code == 200
        finally:
            serve.state["engines"] = engines

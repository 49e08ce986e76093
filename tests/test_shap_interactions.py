"""Exact SHAP interaction values for the classifier forest: the CPU reference
(cpu_ref.forest_shap_interactions_cpu), the engine's
explain_arrays(method="shap", interactions=True) and
POST /explain?method=shap&interactions=true.

Convention (the ``shap`` package's): per row a symmetric 23 x 23 matrix in
schema.FEATURES order; an off-diagonal entry is half of the pair's Shapley
interaction index of the path-dependent game of test_shap.py, the diagonal is
the feature's SHAP value minus its off-diagonal row sum."""

from __future__ import annotations

import dataclasses
import itertools
import math

import numpy as np
import pytest

from _shap_models import (
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
from creditcore.pack import N_CAT, N_NUM, build_shap_paths, encode_batch
from creditcore.schema import FEATURES, SAMPLE_REQUEST


def _inter(packed, codes, nums, **kw):
    return cpu_ref.forest_shap_interactions_cpu(
        packed, codes, cpu_ref.impute_nums(packed, nums), **kw
    )


def _shap(packed, codes, nums):
    return cpu_ref.forest_shap_cpu(packed, codes, cpu_ref.impute_nums(packed, nums))


def _raw_score(packed, codes, nums):
    """Model output in the attribution space (log-odds for GBT)."""
    p = cpu_ref.score_forest_cpu(packed, codes, cpu_ref.impute_nums(packed, nums))
    return np.log(p / (1.0 - p)) if packed.cls_kind == 1 else p


def _off_diagonal(m: np.ndarray) -> np.ndarray:
    out = m.copy()
    d = np.arange(N_SRC)
    out[:, d, d] = 0.0
    return out


# ------------------------------------------------------ brute-force oracle


def _tree_arrays(packed, t):
    lo, hi = packed.cls_tree_offsets[t], packed.cls_tree_offsets[t + 1]
    return packed.cls_nodes[lo:hi], packed.cls_node_cover[lo:hi].astype(np.float64)


def _frac(cover, child, parent) -> float:
    if cover[parent] <= 0.0:
        return 0.0
    return float(np.float32(cover[child] / cover[parent]))


def _player(packed, feat) -> int:
    col = int(packed.feat_col[feat])
    return col if packed.feat_code[feat] >= 0 else N_CAT + col


def _goes_left(packed, feat, thr_bits, codes, nums_imp) -> np.ndarray:
    col, code = int(packed.feat_col[feat]), int(packed.feat_code[feat])
    x = (codes[:, col] == code).astype(np.float32) if code >= 0 else nums_imp[:, col]
    return x <= np.int32(thr_bits).view(np.float32)


def _coalition_value(packed, nodes, cover, k, coalition, codes, nums_imp) -> np.ndarray:
    """Path-dependent expectation of the subtree at node k, per row."""
    feat, bits, left, right = (int(v) for v in nodes[k])
    if feat < 0:
        return np.full(len(codes), np.float64(np.int32(bits).view(np.float32)))
    vl = _coalition_value(packed, nodes, cover, left, coalition, codes, nums_imp)
    vr = _coalition_value(packed, nodes, cover, right, coalition, codes, nums_imp)
    if _player(packed, feat) in coalition:
        return np.where(_goes_left(packed, feat, bits, codes, nums_imp), vl, vr)
    return _frac(cover, left, k) * vl + _frac(cover, right, k) * vr


def brute_force_interactions(packed, codes, nums) -> np.ndarray:
    """The full matrix by subset enumeration over the players present in each
    tree: Shapley values, the Shapley interaction index of every pair, halves
    off the diagonal and the remainder on it. Uses neither the path table nor
    the quadrature."""
    nums_imp = cpu_ref.impute_nums(packed, nums)
    out = np.zeros((len(codes), N_SRC, N_SRC), dtype=np.float64)
    T = packed.cls_n_trees
    for t in range(T):
        nodes, cover = _tree_arrays(packed, t)
        players = sorted({_player(packed, int(f)) for f in nodes[:, 0] if f >= 0})
        m = len(players)
        assert m <= 9, "brute force is exponential in the players of a tree"
        value = {}
        for r in range(m + 1):
            for s in itertools.combinations(players, r):
                value[frozenset(s)] = _coalition_value(
                    packed, nodes, cover, 0, frozenset(s), codes, nums_imp
                )
        phi = {i: np.zeros(len(codes)) for i in players}
        for i in players:
            rest = [p for p in players if p != i]
            for r in range(m):
                w = math.factorial(r) * math.factorial(m - 1 - r) / math.factorial(m)
                for s in itertools.combinations(rest, r):
                    s = frozenset(s)
                    phi[i] += w * (value[s | {i}] - value[s])
        off = {i: np.zeros(len(codes)) for i in players}
        for i, j in itertools.combinations(players, 2):
            rest = [p for p in players if p not in (i, j)]
            idx = np.zeros(len(codes))
            for r in range(m - 1):
                w = math.factorial(r) * math.factorial(m - 2 - r) / math.factorial(m - 1)
                for s in itertools.combinations(rest, r):
                    s = frozenset(s)
                    idx += w * (value[s | {i, j}] - value[s | {i}] - value[s | {j}] + value[s])
            out[:, i, j] += 0.5 * idx
            out[:, j, i] += 0.5 * idx
            off[i] += 0.5 * idx
            off[j] += 0.5 * idx
        for i in players:
            out[:, i, i] += phi[i] - off[i]
    return out if packed.cls_kind == 1 else out / T


@pytest.fixture(scope="module")
def detectors(train_df):
    from creditcore.train import fit_detectors

    return fit_detectors(train_df)


SMALL = {
    "rf": ({"n_estimators": 8, "max_depth": 3, "random_state": 0}, "rf"),
    "et": ({"n_estimators": 8, "max_depth": 3, "random_state": 0}, "et"),
    "gbt": ({"n_estimators": 20, "max_depth": 3, "random_state": 0}, "gbt"),
}


@pytest.fixture(scope="module")
def small(train_df, detectors):
    return {k: fit_packed(train_df, detectors, *v) for k, v in SMALL.items()}


@pytest.mark.parametrize("family", ["rf", "et", "gbt"])
def test_brute_force_oracle(small, score_batch, family):
    p = small[family]
    codes, nums = encode_batch(score_batch.iloc[:32], p.vocabs)  # NaN + unknown rows
    assert np.isnan(nums).any() and (codes < 0).any()
    want = brute_force_interactions(p, codes, nums)
    got = _inter(p, codes, nums)
    assert got.shape == (32, N_SRC, N_SRC) and got.dtype == np.float64
    print(f"{family}: brute force max |err| = {np.abs(got - want).max():.3e}, "
          f"max |off-diagonal| = {np.abs(_off_diagonal(want)).max():.3e}")
    assert np.abs(_off_diagonal(want)).max() > 1e-4  # the oracle is not trivially zero
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)


# -------------------------------------------------- coefficient-form oracle


def _caterpillar_oracle(p, codes, nums):
    """Off-diagonal interaction values of the caterpillar straight from its
    nodes: per leaf, z_p/o_p from the chain walk, then the coefficients e_s of
    prod_{p != i,j} (z_p + o_p y) (np.convolve) times the exact weights
    s!(M-s-2)!/(2 (M-1)!): the integrand prod (z_p (1-t) + o_p t) is
    sum_s e_s t^s (1-t)^(M-2-s), and int t^s (1-t)^(M-2-s) dt is that Beta
    weight. (The same product written in powers of t alone, with
    coefficients of z_p + (o_p - z_p) y, would integrate with 1/(s+1)
    instead.) No quadrature, no path table."""
    nums_imp = cpu_ref.impute_nums(p, nums)
    nodes, cover = _tree_arrays(p, 0)
    out = np.zeros((len(codes), N_SRC, N_SRC), dtype=np.float64)
    for r in range(len(codes)):
        k = 0
        z, o = {}, {}  # per player, along the chain so far
        while True:
            feat, bits, left, right = (int(v) for v in nodes[k])
            pl = _player(p, feat)
            row_left = bool(_goes_left(p, feat, bits, codes[r : r + 1], nums_imp[r : r + 1])[0])
            for c in (c for c in (left, right) if nodes[c, 0] < 0):
                zz, oo = dict(z), dict(o)
                zz[pl] = zz.get(pl, 1.0) * _frac(cover, c, k)
                oo[pl] = oo.get(pl, 1) * int(row_left == (c == left))
                v = np.float64(np.int32(nodes[c, 1]).view(np.float32))
                m = len(zz)
                if m < 2:
                    continue
                w = [
                    math.factorial(s) * math.factorial(m - s - 2) / (2 * math.factorial(m - 1))
                    for s in range(m - 1)
                ]
                for i, j in itertools.combinations(sorted(zz), 2):
                    poly = np.ones(1)
                    for q in zz:
                        if q not in (i, j):
                            poly = np.convolve(poly, [zz[q], oo[q]])
                    val = v * (oo[i] - zz[i]) * (oo[j] - zz[j]) * float(np.dot(poly, w))
                    out[r, i, j] += val
                    out[r, j, i] += val
            nxt = [c for c in (left, right) if nodes[c, 0] >= 0]
            if not nxt:
                break
            c = nxt[0]
            z[pl] = z.get(pl, 1.0) * _frac(cover, c, k)
            o[pl] = o.get(pl, 1) * int(row_left == (c == left))
            k = c
    return out


def test_caterpillar_coefficient_oracle():
    p = caterpillar_model()
    codes, nums = caterpillar_rows()
    want = _caterpillar_oracle(p, codes, nums)
    got = _inter(p, codes, nums)
    print(f"caterpillar: coefficient form max |err| = "
          f"{np.abs(_off_diagonal(got) - want).max():.3e}")
    # row 0 follows the whole chain: all 253 pairs interact
    off = ~np.eye(N_SRC, dtype=bool)
    assert (want[0][off] != 0.0).all() and (got[0][off] != 0.0).all()
    np.testing.assert_allclose(_off_diagonal(got), want, rtol=0, atol=1e-12)
    d = np.arange(N_SRC)
    np.testing.assert_allclose(
        got[:, d, d], _shap(p, codes, nums) - want.sum(2), rtol=0, atol=1e-12
    )


# ---------------------------------------------------------------- structure


@pytest.mark.parametrize("family", ["rf", "et", "gbt"])
def test_structure(small, score_batch, family):
    p = small[family]
    codes, nums = encode_batch(score_batch.iloc[:32], p.vocabs)
    got = _inter(p, codes, nums)
    np.testing.assert_array_equal(got, got.transpose(0, 2, 1))  # bit for bit
    np.testing.assert_allclose(got.sum(2), _shap(p, codes, nums), rtol=0, atol=1e-12)
    _, base = build_shap_paths(p)
    np.testing.assert_allclose(
        base + got.sum((1, 2)), _raw_score(p, codes, nums), rtol=0, atol=1e-9
    )


# -------------------------------------------------------------- hand-built

# Hand-built cases compare a dozen-term f64 quadrature sum of O(1) values with
# exact fractions: a few ulp, bounded here by 1e-14 (as in test_shap.py).


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


def _four_rows():
    codes = np.zeros((4, N_CAT), dtype=np.int16)
    nums = np.zeros((4, N_NUM), dtype=np.float32)
    nums[:, 0] = [1, 1, -1, -1]
    nums[:, 1] = [1, -1, 1, -1]
    return codes, nums


def test_and_tree_by_hand():
    """f(empty) = 1/4, f({a}) = f({b}) = 1/2 or 0, f({a, b}) = 1 or 0: the
    interaction index is f(ab) - f(a) - f(b) + f(empty), half of it per side:
    (1,1): 1 - 1/2 - 1/2 + 1/4 = 1/4; (1,-1): 0 - 1/2 - 0 + 1/4 = -1/4;
    (-1,1): 0 - 0 - 1/2 + 1/4 = -1/4; (-1,-1): 1/4."""
    codes, nums = _four_rows()
    a, b = N_CAT + 0, N_CAT + 1
    for first, second in ((0, 1), (1, 0)):
        p = hand_model(*[[x] for x in _and_tree(first, second)])
        got = _inter(p, codes, nums)
        np.testing.assert_allclose(
            got[:, a, b], [0.125, -0.125, -0.125, 0.125], rtol=0, atol=1e-14
        )
        np.testing.assert_array_equal(got[:, a, b], got[:, b, a])
        # row (1, 1): phi = 3/8 each, so 1/4 stays on the diagonal
        np.testing.assert_allclose(got[0, a, a], 0.25, rtol=0, atol=1e-14)
        np.testing.assert_allclose(got[0, b, b], 0.25, rtol=0, atol=1e-14)
        rest = got.copy()
        rest[:, [a, a, b, b], [a, b, a, b]] = 0.0
        assert (rest == 0.0).all()


def test_unsplit_column_gets_exactly_zero():
    p = caterpillar_model()
    nodes = p.cls_nodes[:25].copy()  # keep 12 chain splits
    nodes[24] = [-1, f32bits(0.5), 0, 0]
    small = hand_model([nodes], [p.cls_node_cover[:25]])
    codes, nums = caterpillar_rows()
    got = _inter(small, codes, nums)
    used = {_player(small, int(f)) for f in nodes[:, 0] if f >= 0}
    assert 0 < len(used) < N_SRC
    for c in range(N_SRC):
        if c in used:
            assert (got[:, c, :] != 0.0).any(), c
        else:
            assert (got[:, c, :] == 0.0).all() and (got[:, :, c] == 0.0).all(), c


def test_players_that_never_share_a_path():
    """Root on numeric 0; its left child splits numeric 1, its right child
    numeric 2: players 1 and 2 meet on no path."""
    nodes = np.array(
        [
            [N_ONEHOT + 0, f32bits(0.0), 1, 2],
            [N_ONEHOT + 1, f32bits(0.0), 3, 4],
            [N_ONEHOT + 2, f32bits(0.0), 5, 6],
            [-1, f32bits(0.1), 0, 0],
            [-1, f32bits(0.9), 0, 0],
            [-1, f32bits(0.3), 0, 0],
            [-1, f32bits(0.6), 0, 0],
        ],
        dtype=np.int32,
    )
    cover = np.array([80.0, 30.0, 50.0, 10.0, 20.0, 35.0, 15.0])
    p = hand_model([nodes], [cover])
    rng = np.random.default_rng(3)
    codes = np.zeros((8, N_CAT), dtype=np.int16)
    nums = rng.normal(size=(8, N_NUM)).astype(np.float32)
    got = _inter(p, codes, nums)
    x0, x1, x2 = N_CAT, N_CAT + 1, N_CAT + 2
    assert (got[:, x1, x2] == 0.0).all() and (got[:, x2, x1] == 0.0).all()
    assert (got[:, x0, x1] != 0.0).all() and (got[:, x0, x2] != 0.0).all()
    np.testing.assert_allclose(
        got, brute_force_interactions(p, codes, nums), rtol=0, atol=1e-14
    )


def test_zero_cover_child():
    nodes, _ = _and_tree(0, 1)
    cover = np.array([100.0, 100.0, 0.0, 0.0, 0.0])  # nothing went right
    p = hand_model([nodes], [cover])
    codes = np.zeros((3, N_CAT), dtype=np.int16)
    nums = np.zeros((3, N_NUM), dtype=np.float32)
    nums[:, 0] = [1, 1, -1]
    nums[:, 1] = [1, -1, 1]
    got = _inter(p, codes, nums)
    assert np.isfinite(got).all()
    frac = build_shap_paths(p)[0].splits[:, 2].view(np.float32)
    assert (frac == 0.0).any()
    a, b = N_CAT, N_CAT + 1
    # row 2 is off a z = 0 player on both two-player paths: exact zeros
    assert (_off_diagonal(got)[2] == 0.0).all()
    # row 0: f(ab) = 1, every other coalition 0 -> index 1, half per side
    np.testing.assert_allclose(got[0, a, b], 0.5, rtol=0, atol=1e-14)
    np.testing.assert_allclose(
        got, brute_force_interactions(p, codes, nums), rtol=0, atol=1e-14
    )


def test_root_leaf_forest():
    leaf = np.array([[-1, f32bits(0.6), 0, 0]], dtype=np.int32)
    p = hand_model([leaf, leaf.copy()], [[10.0], [3.0]])
    codes = np.zeros((4, N_CAT), dtype=np.int16)
    nums = np.ones((4, N_NUM), dtype=np.float32)
    assert (_inter(p, codes, nums) == 0.0).all()
    out = ScoringEngine(p, device="cpu").explain_arrays(
        codes, nums, method="shap", interactions=True
    )
    assert out["interactions"].shape == (4, N_SRC, N_SRC)
    assert (out["interactions"] == 0.0).all()


def test_path_chunking_does_not_change_the_result(small, score_batch):
    p = small["rf"]
    codes, nums = encode_batch(score_batch.iloc[:8], p.vocabs)
    whole = _inter(p, codes, nums)
    tiny = _inter(p, codes, nums, max_bytes=1 << 14)
    assert (whole != 0.0).any()
    np.testing.assert_allclose(tiny, whole, rtol=0, atol=1e-12)


# ------------------------------------------------------------------- engine


def test_engine_keyword(packed, monkeypatch):
    eng = ScoringEngine(packed, device="cpu")
    codes, nums = encode_batch(SAMPLE_REQUEST * 5, packed.vocabs)
    nums[1:, 3] += np.arange(1, 5, dtype=np.float32) * 7000.0
    plain = eng.explain_arrays(codes, nums, method="shap")
    out = eng.explain_arrays(codes, nums, method="shap", interactions=True)
    assert set(out) == set(plain) | {"interactions"}
    assert "interactions" not in plain
    for k in plain:  # everything else is the method="shap" result
        np.testing.assert_array_equal(np.asarray(out[k]), np.asarray(plain[k]))
    m = out["interactions"]
    assert m.shape == (5, N_SRC, N_SRC) and m.dtype == np.float64
    np.testing.assert_array_equal(m, m.transpose(0, 2, 1))
    np.testing.assert_allclose(m.sum(2), out["contributions"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(m, _inter(packed, codes, nums), rtol=0, atol=1e-12)
    rec = eng.explain_records(SAMPLE_REQUEST, method="shap", interactions=True)
    np.testing.assert_allclose(rec["interactions"][0], m[0], rtol=0, atol=1e-12)

    for method in ("saabas", "interventional"):
        with pytest.raises(ValueError, match="interactions"):
            eng.explain_arrays(codes, nums, method=method, interactions=True)
    coverless = ScoringEngine(dataclasses.replace(packed, cls_node_cover=None), device="cpu")
    with pytest.raises(ExplainUnavailable):
        coverless.explain_arrays(codes, nums, method="shap", interactions=True)

    # slices of 2 + 2 + 1 rows
    monkeypatch.setattr(ScoringEngine, "INTERACTION_LAUNCH_ROWS", 2)
    sliced = eng.explain_arrays(codes, nums, method="shap", interactions=True)
    np.testing.assert_allclose(sliced["interactions"], m, rtol=0, atol=1e-12)

    assert ScoringEngine.INTERACTION_MAX_ROWS == 128
    monkeypatch.setattr(ScoringEngine, "INTERACTION_MAX_ROWS", 4)
    with pytest.raises(ExplainTooLarge):
        eng.explain_arrays(codes, nums, method="shap", interactions=True)
    assert eng.explain_arrays(codes, nums, method="shap")["contributions"].shape == (5, N_SRC)


# --------------------------------------------------------------------- HTTP

SHAP_KEYS = {
    "output_space", "base_value", "features", "predictions", "contributions",
    "top_reasons", "method",
}


def test_http_interactions(model_dir, packed, monkeypatch):
    from fastapi.testclient import TestClient

    from creditcore import serve
    from creditcore.config import ServeConfig

    cfg = ServeConfig()
    cfg.model_directory = model_dir
    cfg.device = "cpu"
    with TestClient(serve.create_app(cfg)) as c:
        r = c.post("/explain?method=shap&interactions=true", json=SAMPLE_REQUEST)
        assert r.status_code == 200
        body = r.json()
        assert set(body) == SHAP_KEYS | {"interactions"}
        m = np.asarray(body["interactions"])
        assert m.shape == (1, 23, 23) and body["features"] == list(FEATURES)
        np.testing.assert_allclose(m.sum(2), body["contributions"], rtol=0, atol=1e-12)
        pred = c.post("/predict", json=SAMPLE_REQUEST).json()["predictions"][0]
        assert body["base_value"] + m.sum() == pytest.approx(pred, abs=1e-9)

        plain = c.post("/explain?method=shap", json=SAMPLE_REQUEST)
        assert plain.status_code == 200 and set(plain.json()) == SHAP_KEYS
        off = c.post("/explain?method=shap&interactions=false", json=SAMPLE_REQUEST)
        assert off.status_code == 200 and set(off.json()) == SHAP_KEYS
        assert {k: v for k, v in body.items() if k != "interactions"} == plain.json()

        for q in ("interactions=true", "method=saabas&interactions=true",
                  "method=interventional&interactions=true"):
            assert c.post(f"/explain?{q}", json=SAMPLE_REQUEST).status_code == 422, q

        monkeypatch.setattr(ScoringEngine, "INTERACTION_MAX_ROWS", 2)
        url = "/explain?method=shap&interactions=true"
        assert c.post(url, json=SAMPLE_REQUEST * 3).status_code == 413
        assert c.post(url, json=SAMPLE_REQUEST * 2).status_code == 200
        assert c.post("/explain?method=shap", json=SAMPLE_REQUEST * 3).status_code == 200
        monkeypatch.undo()

        engines = serve.state["engines"]
        coverless = dataclasses.replace(packed, cls_node_cover=None)
        serve.state["engines"] = [ScoringEngine(coverless, device="cpu")]
        try:
            r = c.post(url, json=SAMPLE_REQUEST)
            assert r.status_code == 501 and "cover" in r.json()["detail"]
        finally:
            serve.state["engines"] = engines

        spec = c.get("/openapi.json").json()
        assert "interactions" in spec["components"]["schemas"]["ExplainOutput"]["properties"]

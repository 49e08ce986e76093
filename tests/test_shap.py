"""Exact path-dependent TreeSHAP for the classifier forest: per-node cover in
the pack, the flat path table, the CPU reference (closed-form Shapley integral
by 12-point Gauss-Legendre), the engine's method="shap" and
POST /explain?method=shap.

Players are the 23 source columns; all one-hot features of a categorical
column are one player. The game for a coalition S walks the tree, follows the
row at splits on columns in S and takes both children, weighted by
frac[child] = f32(cover[child] / cover[parent]), everywhere else."""

from __future__ import annotations

import dataclasses
import itertools
import math
import multiprocessing as mp
import os

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
from creditcore.pack import N_CAT, N_NUM, PackedModel, build_shap_paths, encode_batch
from creditcore.schema import FEATURES, SAMPLE_REQUEST


def _shap(packed, codes, nums):
    return cpu_ref.forest_shap_cpu(packed, codes, cpu_ref.impute_nums(packed, nums))


def _raw_score(packed, codes, nums):
    """Model output in the attribution space (log-odds for GBT)."""
    p = cpu_ref.score_forest_cpu(packed, codes, cpu_ref.impute_nums(packed, nums))
    return np.log(p / (1.0 - p)) if packed.cls_kind == 1 else p


# ------------------------------------------------------ brute-force oracle


def _tree_arrays(packed, t):
    lo, hi = packed.cls_tree_offsets[t], packed.cls_tree_offsets[t + 1]
    nodes = packed.cls_nodes[lo:hi]
    cover = packed.cls_node_cover[lo:hi].astype(np.float64)
    return nodes, cover


def _frac(cover, child, parent) -> float:
    if cover[parent] <= 0.0:
        return 0.0
    return float(np.float32(cover[child] / cover[parent]))


def _player(packed, feat) -> int:
    col = int(packed.feat_col[feat])
    return col if packed.feat_code[feat] >= 0 else N_CAT + col


def _goes_left(packed, feat, thr_bits, codes, nums_imp) -> np.ndarray:
    """Per row: the same f32 compare as the scorer."""
    col, code = int(packed.feat_col[feat]), int(packed.feat_code[feat])
    if code >= 0:
        x = (codes[:, col] == code).astype(np.float32)
    else:
        x = nums_imp[:, col]
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


def brute_force_shap(packed, codes, nums):
    """Shapley values by subset enumeration over the players present in each
    tree, and the base value (the empty coalition). Uses neither the path
    table nor the quadrature."""
    nums_imp = cpu_ref.impute_nums(packed, nums)
    phi = np.zeros((len(codes), N_SRC), dtype=np.float64)
    base = 0.0
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
        base += float(value[frozenset()][0])
        for i in players:
            rest = [p for p in players if p != i]
            for r in range(m):
                w = math.factorial(r) * math.factorial(m - 1 - r) / math.factorial(m)
                for s in itertools.combinations(rest, r):
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
    want, want_base = brute_force_shap(p, codes, nums)
    got = _shap(p, codes, nums)
    _, base = build_shap_paths(p)
    err = np.abs(got - want).max()
    print(f"{family}: brute force max |err| = {err:.3e}, base err = {abs(base - want_base):.3e}")
    assert np.abs(want).max() > 1e-4  # the oracle is not trivially zero
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    np.testing.assert_allclose(base, want_base, rtol=0, atol=1e-12)


# -------------------------------------------------- coefficient-form oracle


def _caterpillar_oracle(p, codes, nums):
    """SHAP of the caterpillar straight from its nodes: per leaf, z_p/o_p from
    the chain walk, then polynomial coefficients (np.convolve) times the exact
    Shapley weights k!(m-1-k)!/m!. No quadrature, no path table."""
    nums_imp = cpu_ref.impute_nums(p, nums)
    nodes, cover = _tree_arrays(p, 0)
    out = np.zeros((len(codes), N_SRC), dtype=np.float64)
    for r in range(len(codes)):
        k = 0
        z, o = {}, {}  # per player, along the chain so far
        while True:
            feat, bits, left, right = (int(v) for v in nodes[k])
            leaf_kids = [c for c in (left, right) if nodes[c, 0] < 0]
            pl = _player(p, feat)
            row_left = bool(_goes_left(p, feat, bits, codes[r : r + 1], nums_imp[r : r + 1])[0])
            for c in leaf_kids:
                zz, oo = dict(z), dict(o)
                zz[pl] = zz.get(pl, 1.0) * _frac(cover, c, k)
                oo[pl] = oo.get(pl, 1) * int(row_left == (c == left))
                v = np.float64(np.int32(nodes[c, 1]).view(np.float32))
                m = len(zz)
                for i in zz:
                    poly = np.ones(1)
                    for q in zz:
                        if q != i:
                            poly = np.convolve(poly, [zz[q], oo[q]])
                    w = [
                        math.factorial(j) * math.factorial(m - 1 - j) / math.factorial(m)
                        for j in range(m)
                    ]
                    out[r, i] += v * (oo[i] - zz[i]) * float(np.dot(poly, w))
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
    paths, base = build_shap_paths(p)
    # the long path carries all 23 players on 26 splits (degree-22 integrand)
    assert int(np.diff(paths.leaf_off).max()) == 26
    flags = paths.splits[:, 3].view(np.uint32)
    deepest = int(np.argmax(np.diff(paths.leaf_off)))
    run = flags[paths.leaf_off[deepest] : paths.leaf_off[deepest + 1]]
    assert int(((run & 2) != 0).sum()) == N_SRC
    assert sorted(set(((run >> 8) & 0xFF).tolist())) == list(range(N_SRC))
    # row 0 follows the whole chain, the next rows leave it at several depths
    score = _raw_score(p, codes, nums)
    assert score[0] == np.float64(np.float32(0.875))
    assert len(set(score[:8].tolist())) >= 6

    want = _caterpillar_oracle(p, codes, nums)
    got = _shap(p, codes, nums)
    err = np.abs(got - want).max()
    print(f"caterpillar: coefficient form max |err| = {err:.3e}")
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    np.testing.assert_allclose(base + got.sum(1), score, rtol=0, atol=1e-12)


# --------------------------------------------------------------- additivity


def test_additivity_rf(packed, score_batch):
    codes, nums = encode_batch(score_batch.iloc[:16], packed.vocabs)
    got = _shap(packed, codes, nums)
    assert got.shape == (16, N_SRC) and got.dtype == np.float64
    _, base = build_shap_paths(packed)
    err = np.abs(base + got.sum(1) - _raw_score(packed, codes, nums)).max()
    print(f"RF additivity max |err| = {err:.3e}")
    np.testing.assert_allclose(
        base + got.sum(1), _raw_score(packed, codes, nums), rtol=0, atol=1e-9
    )


def test_additivity_gbt_log_odds(train_df, detectors, score_batch):
    p = fit_packed(
        train_df, detectors, {"n_estimators": 60, "max_depth": 3, "random_state": 0}, "gbt"
    )
    codes, nums = encode_batch(score_batch.iloc[:16], p.vocabs)
    out = ScoringEngine(p, device="cpu").explain_arrays(codes, nums, method="shap")
    assert out["output_space"] == "log_odds"
    raw = out["base_value"] + out["contributions"].sum(1)
    np.testing.assert_allclose(raw, _raw_score(p, codes, nums), rtol=0, atol=1e-9)
    np.testing.assert_allclose(
        out["predictions"],
        cpu_ref.score_forest_cpu(p, codes, cpu_ref.impute_nums(p, nums)),
        rtol=0,
        atol=1e-9,
    )


# ----------------------------------------------------- axioms Saabas fails


# Hand-built cases below compare a dozen-term f64 quadrature sum of O(1)
# values with exact fractions: a few ulp, bounded here by 1e-14.


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


def test_symmetry_on_and_tree():
    codes = np.zeros((4, N_CAT), dtype=np.int16)
    nums = np.zeros((4, N_NUM), dtype=np.float32)
    nums[:, 0] = [1, 1, -1, -1]
    nums[:, 1] = [1, -1, 1, -1]
    a, b = N_CAT + 0, N_CAT + 1
    for first, second in ((0, 1), (1, 0)):
        p = hand_model(*[[x] for x in _and_tree(first, second)])
        shap = _shap(p, codes, nums)
        # both features matter equally for rows (1,1) and (-1,-1)
        np.testing.assert_allclose(shap[[0, 3], a], shap[[0, 3], b], rtol=0, atol=1e-14)
        np.testing.assert_allclose(shap[0, a], 0.375, rtol=0, atol=1e-14)
        saabas = cpu_ref.forest_contrib_cpu(p, codes, cpu_ref.impute_nums(p, nums))
        assert abs(saabas[0, a] - saabas[0, b]) > 0.2  # 0.25 vs 0.5 by split order
        _, base = build_shap_paths(p)
        assert base == 0.25
        np.testing.assert_allclose(
            base + shap.sum(1), _raw_score(p, codes, nums), rtol=0, atol=1e-14
        )


def test_unsplit_column_gets_exactly_zero():
    p = caterpillar_model()
    # drop the chain's tail: no split on numeric 13 ... keep 12 chain splits
    nodes = p.cls_nodes[:25].copy()
    nodes[24] = [-1, f32bits(0.5), 0, 0]
    small = hand_model([nodes], [p.cls_node_cover[:25]])
    codes, nums = caterpillar_rows()
    shap = _shap(small, codes, nums)
    used = {_player(small, int(f)) for f in nodes[:, 0] if f >= 0}
    assert 0 < len(used) < N_SRC
    for c in range(N_SRC):
        if c in used:
            assert (shap[:, c] != 0.0).any(), c
        else:
            assert (shap[:, c] == 0.0).all(), c


# --------------------------------------------------------------- edge cases


def test_zero_cover_child():
    nodes, cover = _and_tree(0, 1)
    cover = np.array([100.0, 100.0, 0.0, 0.0, 0.0])  # nothing went right
    p = hand_model([nodes], [cover])
    codes = np.zeros((3, N_CAT), dtype=np.int16)
    nums = np.zeros((3, N_NUM), dtype=np.float32)
    nums[:, 0] = [1, 1, -1]
    nums[:, 1] = [1, -1, 1]
    shap = _shap(p, codes, nums)
    paths, base = build_shap_paths(p)
    assert np.isfinite(shap).all() and base == 0.0
    frac = paths.splits[:, 2].view(np.float32)
    assert np.isfinite(frac).all() and (frac == 0.0).any()
    np.testing.assert_allclose(base + shap.sum(1), _raw_score(p, codes, nums), rtol=0, atol=1e-14)
    want, want_base = brute_force_shap(p, codes, nums)
    np.testing.assert_allclose(shap, want, rtol=0, atol=1e-14)
    assert shap[0, N_CAT] != 0.0


def test_bad_cover_is_refused():
    nodes, cover = _and_tree(0, 1)
    for bad in (-1.0, np.nan, np.inf):
        c = cover.copy()
        c[3] = bad
        p = hand_model([nodes], [cover])
        p.cls_node_cover = c.astype(np.float32)
        with pytest.raises(ValueError, match="cover"):
            build_shap_paths(p)


def test_root_leaf_forest():
    leaf = np.array([[-1, f32bits(0.6), 0, 0]], dtype=np.int32)
    p = hand_model([leaf, leaf.copy()], [[10.0], [3.0]])
    codes = np.zeros((4, N_CAT), dtype=np.int16)
    nums = np.ones((4, N_NUM), dtype=np.float32)
    out = ScoringEngine(p, device="cpu").explain_arrays(codes, nums, method="shap")
    assert (out["contributions"] == 0.0).all()
    assert out["base_value"] == np.float64(np.float32(0.6))
    np.testing.assert_array_equal(out["predictions"], np.float64(np.float32(0.6)))


def test_path_chunking_does_not_change_the_result(packed, score_batch):
    codes, nums = encode_batch(score_batch.iloc[:8], packed.vocabs)
    imp = cpu_ref.impute_nums(packed, nums)
    whole = cpu_ref.forest_shap_cpu(packed, codes, imp)
    tiny = cpu_ref.forest_shap_cpu(packed, codes, imp, max_bytes=1 << 16)
    np.testing.assert_allclose(tiny, whole, rtol=0, atol=1e-14)


# ----------------------------------------------------------------- plumbing


def test_pack_cover_layout(packed, loaded_pyfunc):
    c = packed.cls_node_cover
    assert c is not None and c.dtype == np.float32 and c.shape == (len(packed.cls_nodes),)
    clf = loaded_pyfunc.python_model.classifier.named_steps["classifier"]
    roots = c[packed.cls_tree_offsets[:-1]]
    want = [est.tree_.weighted_n_node_samples[0] for est in clf.estimators_]
    np.testing.assert_array_equal(roots, np.asarray(want, dtype=np.float32))
    # children partition their parent's cover
    split = np.flatnonzero(packed.cls_nodes[:, 0] >= 0)
    sizes = np.diff(packed.cls_tree_offsets)
    base = np.repeat(packed.cls_tree_offsets[:-1], sizes)
    kids = c[base[split] + packed.cls_nodes[split, 2]] + c[base[split] + packed.cls_nodes[split, 3]]
    np.testing.assert_allclose(kids, c[split], rtol=1e-6)


def test_path_table_layout(packed):
    paths, base = build_shap_paths(packed)
    leaves = int((packed.cls_nodes[:, 0] < 0).sum())
    assert paths.n_leaves == leaves and paths.leaf_off.shape == (leaves + 1,)
    assert paths.splits.dtype == np.int32 and paths.splits.shape[1] == 4
    assert paths.leaf_off[-1] == len(paths.splits)
    flags = paths.splits[:, 3].view(np.uint32)
    player = (flags >> 8) & 0xFF
    rec_leaf = np.repeat(np.arange(leaves), np.diff(paths.leaf_off))
    # grouped by player within each leaf, the first-of-player flag marks runs
    same = rec_leaf[1:] == rec_leaf[:-1]
    assert (player[1:][same] >= player[:-1][same]).all()
    first = (flags & 2) != 0
    np.testing.assert_array_equal(
        first[1:], ~same | (player[1:] != player[:-1])
    )
    assert 0.0 < base < 1.0


def test_save_load_roundtrip_and_old_npz(packed, tmp_path):
    path = str(tmp_path / "m.npz")
    packed.save(path)
    re = PackedModel.load(path)
    assert re.cls_node_cover.dtype == np.float32
    np.testing.assert_array_equal(
        re.cls_node_cover.view(np.int32), packed.cls_node_cover.view(np.int32)
    )
    # a file written before the cover existed
    z = np.load(path, allow_pickle=True)
    old_path = str(tmp_path / "old.npz")
    np.savez_compressed(old_path, **{k: z[k] for k in z.files if k != "cls_node_cover"})
    old = PackedModel.load(old_path)
    assert old.cls_node_cover is None and old.cls_node_value is not None
    eng = ScoringEngine(old, device="cpu")
    codes, nums = encode_batch(SAMPLE_REQUEST, old.vocabs)
    with pytest.raises(ExplainUnavailable):
        eng.explain_arrays(codes, nums, method="shap")
    with pytest.raises(ValueError, match="cls_node_cover"):
        _shap(old, codes, nums)
    saabas = eng.explain_arrays(codes, nums)
    np.testing.assert_array_equal(
        saabas["contributions"],
        ScoringEngine(packed, device="cpu").explain_arrays(codes, nums)["contributions"],
    )
    old.save(str(tmp_path / "again.npz"))
    assert "cls_node_cover" not in np.load(str(tmp_path / "again.npz"), allow_pickle=True)


def test_engine_methods_and_caps(packed, monkeypatch):
    eng = ScoringEngine(packed, device="cpu")
    out = eng.explain_records(SAMPLE_REQUEST * 3, method="shap")
    saabas = eng.explain_records(SAMPLE_REQUEST * 3)
    assert set(out) == set(saabas)
    assert out["output_space"] == "probability"
    assert out["contributions"].shape == (3, N_SRC)
    assert out["base_value"] == build_shap_paths(packed)[1]
    # close to, but not the same number as, the per-level-f32 Saabas base
    assert abs(out["base_value"] - saabas["base_value"]) < 1e-5
    np.testing.assert_allclose(out["predictions"], saabas["predictions"], rtol=0, atol=1e-9)
    assert not np.allclose(out["contributions"], saabas["contributions"], atol=1e-4)
    with pytest.raises(ValueError, match="method"):
        eng.explain_arrays(*encode_batch(SAMPLE_REQUEST, packed.vocabs), method="lime")
    assert 1 <= ScoringEngine.SHAP_MAX_ROWS <= 1024  # the issue's ceiling
    monkeypatch.setattr(ScoringEngine, "SHAP_MAX_ROWS", 4)
    big = (np.zeros((5, N_CAT), dtype=np.int16), np.zeros((5, N_NUM), dtype=np.float32))
    with pytest.raises(ExplainTooLarge):
        eng.explain_arrays(*big, method="shap")
    assert eng.explain_arrays(*big)["contributions"].shape == (5, N_SRC)  # saabas cap apart


def _bcast_worker(rank: int, world: int, port: int, npz_path: str, q):
    try:
        import torch.distributed as dist

        from creditcore.parallel import broadcast_packed

        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        src = PackedModel.load(npz_path) if rank == 0 else None
        got = broadcast_packed(src, device="cpu", src=0)
        nc = got.cls_node_cover
        q.put((rank, None if nc is None else (str(nc.dtype), nc.view(np.int32).tolist())))
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
def test_broadcast_carries_cover(packed, tmp_path):
    path = str(tmp_path / "packed.npz")
    packed.save(path)
    res = _bcast(path, 29541)
    dtype, bits = res[1]
    assert dtype == "float32"
    assert bits == packed.cls_node_cover.view(np.int32).tolist()  # bit-identical
    assert res[0] == res[1]
    old = str(tmp_path / "old.npz")
    dataclasses.replace(packed, cls_node_cover=None).save(old)
    res = _bcast(old, 29542)
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


def test_http_shap(client, packed):
    r = client.post("/explain?method=shap&top_k=4", json=SAMPLE_REQUEST)
    assert r.status_code == 200
    body = r.json()
    assert set(body) == DEFAULT_KEYS | {"method"}
    assert body["method"] == "shap" and body["features"] == list(FEATURES)
    row = body["contributions"][0]
    assert len(row) == 23
    assert body["base_value"] == build_shap_paths(packed)[1]
    total = body["base_value"] + sum(row)
    assert total == pytest.approx(body["predictions"][0], abs=1e-12)
    p = client.post("/predict", json=SAMPLE_REQUEST).json()["predictions"][0]
    assert p == pytest.approx(total, abs=1e-9)
    # top_reasons: the largest strictly positive SHAP values, descending
    want = sorted((j for j in range(23) if row[j] > 0.0), key=lambda j: (-row[j], j))[:4]
    assert [x["feature"] for x in body["top_reasons"][0]] == [FEATURES[j] for j in want]
    assert [x["contribution"] for x in body["top_reasons"][0]] == [row[j] for j in want]
    assert want


def test_http_method_values(client):
    default = client.post("/explain", json=SAMPLE_REQUEST)
    assert default.status_code == 200 and set(default.json()) == DEFAULT_KEYS
    named = client.post("/explain?method=saabas", json=SAMPLE_REQUEST)
    assert named.status_code == 200 and named.json()["method"] == "saabas"
    assert named.json()["contributions"] == default.json()["contributions"]
    assert client.post("/explain?method=bogus", json=SAMPLE_REQUEST).status_code == 422
    spec = client.get("/openapi.json").json()
    assert "method" in spec["components"]["schemas"]["ExplainOutput"]["properties"]


def test_http_shap_errors(model_dir, packed, tmp_path, monkeypatch):
    """413 above the SHAP row cap (the Saabas cap is untouched) and 501 for a
    model packed without cover, which still serves Saabas."""
    from fastapi.testclient import TestClient

    from creditcore import serve
    from creditcore.config import ServeConfig

    cfg = ServeConfig()
    cfg.model_directory = model_dir
    cfg.device = "cpu"
    with TestClient(serve.create_app(cfg)) as c:
        engines = serve.state["engines"]
        monkeypatch.setattr(ScoringEngine, "SHAP_MAX_ROWS", 2)
        assert c.post("/explain?method=shap", json=SAMPLE_REQUEST * 3).status_code == 413
        assert c.post("/explain?method=shap", json=SAMPLE_REQUEST * 2).status_code == 200
        assert c.post("/explain", json=SAMPLE_REQUEST * 3).status_code == 200
        monkeypatch.undo()

        coverless = dataclasses.replace(packed, cls_node_cover=None)
        serve.state["engines"] = [ScoringEngine(coverless, device="cpu")]
        try:
            r = c.post("/explain?method=shap", json=SAMPLE_REQUEST)
            assert r.status_code == 501 and "cover" in r.json()["detail"]
            assert c.post("/explain", json=SAMPLE_REQUEST).status_code == 200
        finally:
            serve.state["engines"] = engines

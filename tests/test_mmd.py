"""MMD permutation drift test on the CPU: the W-based statistics against the
definition, the p-value rules on a hand-checkable case, the engine and the
POST /drift/mmd route."""

from __future__ import annotations

import dataclasses

import numpy as np
import pytest

from creditcore import mmd
from creditcore.engine import ScoringEngine
from creditcore.ops import cpu_ref
from creditcore.pack import encode_batch

KEYS = {"mmd2", "p_val", "is_drift", "threshold", "distance_threshold", "gamma",
        "n", "n_ref", "n_permutations"}


@pytest.mark.parametrize("n,m,n_perm", [(5, 11, 3), (37, 20, 9), (12, 64, 17)])
def test_w_statistics_equal_definition(n, m, n_perm):
    """mmd2 from W = K . ind equals, for every permutation, the three block
    means of an explicit f64 K of the physically permuted pooled rows."""
    rng = np.random.default_rng(n * 100 + m)
    z = rng.normal(size=(n + m, 7)).astype(np.float32)
    z[:n] += 0.3
    gamma = mmd.median_gamma(z[n:])
    ind = mmd.indicator(n, m, n_perm, seed=5)
    got = mmd.statistics(cpu_ref.mmd_perm_w_cpu(z, gamma, ind, max_bytes=4096), ind, n, m)

    z64 = z.astype(np.float64)
    draws = np.random.default_rng(5)
    orders = [np.arange(n + m)] + [draws.permutation(n + m) for _ in range(n_perm)]
    for p, order in enumerate(orders):
        zz = z64[order]
        d2 = ((zz[:, None, :] - zz[None, :, :]) ** 2).sum(-1)
        k = np.exp(-gamma * d2)
        np.fill_diagonal(k, 0.0)
        want = (k[:n, :n].sum() / (n * (n - 1)) + k[n:, n:].sum() / (m * (m - 1))
                - 2.0 * k[:n, n:].mean())
        assert got[p] == pytest.approx(want, rel=1e-12, abs=1e-15), p


def test_decide_by_hand():
    """Observed 0.5 against permuted {0.1, 0.9, 0.5, 0.2}: two are >= it, so
    p = 3/5; at drift_p_val 0.5 the threshold is descending rank 2 (0.2)."""
    out = mmd.decide(np.array([0.5, 0.1, 0.9, 0.5, 0.2]), 0.5)
    assert out["p_val"] == 3 / 5 and out["is_drift"] == 0
    assert out["distance_threshold"] == 0.2 and out["threshold"] == 0.5
    out = mmd.decide(np.array([1.0, 0.1, 0.9, 0.5, 0.2]), 0.25)
    assert out["p_val"] == 1 / 5 and out["is_drift"] == 1
    assert out["distance_threshold"] == 0.5


def test_gamma_is_lower_median_of_pairs():
    z = np.array([[0.0], [1.0], [3.0], [7.0]], dtype=np.float32)
    # squared distances 1 4 9 16 36 49: the lower median of six is 9
    assert mmd.median_gamma(z) == 1.0 / 9.0
    with pytest.raises(ValueError):
        mmd.median_gamma(np.zeros((4, 2), dtype=np.float32))


def test_engine_reference_override_and_checks(packed, score_batch):
    eng = ScoringEngine(packed, device="cpu")
    codes, nums = encode_batch(score_batch.iloc[:40], packed.vocabs)
    out = eng.mmd_drift(codes, nums, n_permutations=20, seed=3)
    assert set(out) == KEYS
    assert (out["n"], out["n_ref"], out["n_permutations"]) == (40, 256, 20)
    assert out["threshold"] == packed.drift_p_val and 0 < out["p_val"] <= 1
    same = eng.mmd_drift(codes, nums, reference=(packed.bg_codes, packed.bg_nums),
                         n_permutations=20, seed=3)
    assert same == out
    shifted = nums + 2.0 * np.nanstd(packed.bg_nums, axis=0)
    drift = eng.mmd_drift(codes, shifted.astype(np.float32), n_permutations=20, seed=3)
    assert drift["p_val"] == 1 / 21 and drift["mmd2"] > out["mmd2"]
    with pytest.raises(ValueError):
        eng.mmd_drift(codes[:1], nums[:1])
    with pytest.raises(ValueError):
        eng.mmd_drift(codes, nums, n_permutations=mmd.MMD_MAX_PERMUTATIONS + 1)


def test_engine_refuses_non_finite_rows(packed, score_batch):
    """inf, -inf and an embedding that overflows f32 raise ValueError naming
    the side and leave the reference cache as it was; NaN is still imputed
    (the same assertions run on a GPU engine in test_mmd_kernels_gpu.py)."""
    from _mmd_cases import check_engine_refuses_non_finite

    codes, nums = encode_batch(score_batch.iloc[:40], packed.vocabs)
    check_engine_refuses_non_finite(ScoringEngine(packed, device="cpu"), packed, codes, nums)


def test_route_refuses_non_finite_rows(model_dir, score_batch):
    """A numeric that is infinite once it is f32, or that embeds past f32's
    range, is a 422 like mmd_drift's other ValueErrors, and the replica goes
    on serving."""
    from fastapi.testclient import TestClient

    from creditcore import serve
    from creditcore.config import ServeConfig

    cfg = ServeConfig()
    cfg.model_directory = model_dir
    cfg.device = "cpu"
    records = score_batch.iloc[4:36].to_dict(orient="records")
    with TestClient(serve.create_app(cfg)) as client:
        for value in (1e300, -1e300, 3.0e38):
            bad = [dict(r) for r in records]
            bad[7]["bill_amount_2"] = value
            r = client.post("/drift/mmd", json={"records": bad, "n_permutations": 10})
            assert r.status_code == 422 and "batch" in r.json()["detail"], r.text
        r = client.post("/drift/mmd", json={"records": records, "n_permutations": 10})
        assert r.status_code == 200 and np.isfinite(r.json()["mmd2"])


def test_route(model_dir, packed, score_batch):
    from fastapi.testclient import TestClient

    from creditcore import serve
    from creditcore.config import ServeConfig

    cfg = ServeConfig()
    cfg.model_directory = model_dir
    cfg.device = "cpu"
    records = score_batch.iloc[4:36].to_dict(orient="records")
    with TestClient(serve.create_app(cfg)) as client:
        r = client.post("/drift/mmd", json={"records": records, "n_permutations": 10})
        assert r.status_code == 200, r.text
        body = r.json()
        assert set(body) == KEYS and body["n"] == 32 and body["n_permutations"] == 10
        codes, nums = encode_batch(records, packed.vocabs)
        want = ScoringEngine(packed, device="cpu").mmd_drift(codes, nums, n_permutations=10)
        assert body["mmd2"] == want["mmd2"] and body["p_val"] == want["p_val"]
        assert client.post("/drift/mmd", json={"records": records[:1]}).status_code == 422
        assert client.post(
            "/drift/mmd", json={"records": records, "n_permutations": 0}
        ).status_code == 422
        assert client.post(
            "/drift/mmd", json={"records": records, "n_permutations": 255}
        ).status_code == 413
        big = {"records": records[:1] * (mmd.MMD_MAX_ROWS + 1)}
        assert client.post("/drift/mmd", json=big).status_code == 413
        engines = serve.state["engines"]
        bare = dataclasses.replace(packed, bg_codes=None, bg_nums=None)
        serve.state["engines"] = [ScoringEngine(bare, device="cpu")]
        try:
            r = client.post("/drift/mmd", json={"records": records})
            assert r.status_code == 501 and "background sample" in r.json()["detail"]
        finally:
            serve.state["engines"] = engines

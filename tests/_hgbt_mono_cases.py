"""Shared by test_hgbt_mono.py and test_hgbt_mono_gpu.py: hand-built level
histograms for the monotone-constrained split search, and a scalar brute
force of the rule (plain Python floats, one candidate at a time) that the
vectorised reference and the kernel are both checked against."""

from __future__ import annotations

import struct

import numpy as np

from creditcore.ops import cpu_ref

S = cpu_ref.HGBT_SHIFT
INF = float("inf")


def brute_force(hist, bin_off, lam, min_leaf, mono, bounds) -> np.ndarray:
    """The rule of models/hgbt.py's docstring, candidate by candidate."""
    sc = 1.0 / float(1 << S)
    n_nodes = hist.shape[0]
    out = np.zeros((n_nodes, cpu_ref.HGBT_REC), dtype=np.int64)
    for k in range(n_nodes):
        lo, hi = float(bounds[k][0]), float(bounds[k][1])
        a0, b0 = int(bin_off[0]), int(bin_off[1])
        G, H, C = (int(hist[k, p, a0:b0].sum()) for p in range(3))

        def side(g_int, h_int):
            g, d = g_int * sc, h_int * sc + lam
            if not d > 0.0:
                return None
            w = min(max(-g / d, lo), hi)
            return w, -((2.0 * g) * w + (d * w) * w)

        best = None  # (gain, feat, bin, GL, HL, CL)
        for f in range(len(bin_off) - 1):
            GL = HL = CL = 0
            for b in range(int(bin_off[f + 1]) - int(bin_off[f])):
                i = int(bin_off[f]) + b
                GL += int(hist[k, 0, i])
                HL += int(hist[k, 1, i])
                CL += int(hist[k, 2, i])
                if CL < min_leaf or C - CL < min_leaf:
                    continue
                left, right = side(GL, HL), side(G - GL, H - HL)
                if left is None or right is None:
                    continue
                parent = side(G, H)  # d_P = d_L + d_R - lam > 0 here
                gain = (left[1] + right[1]) - parent[1]
                if not gain > 0.0:
                    continue
                if mono[f] > 0 and not left[0] <= right[0]:
                    continue
                if mono[f] < 0 and not left[0] >= right[0]:
                    continue
                if best is None or gain > best[0]:  # first of equals: lowest (f, b)
                    best = (gain, f, b, GL, HL, CL)
        if best is None:
            out[k, 1] = -1
        else:
            out[k, 0] = struct.unpack("<q", struct.pack("<d", best[0]))[0]
            out[k, 1:6] = best[1:]
        out[k, 6:9] = (G, H, C)
    return out


def _hist(*features):
    """One node; every feature is a list of (g, h, count) bins, g and h in
    units of 1.0 (scaled to fixed point here)."""
    rows = [b for f in features for b in f]
    hist = np.zeros((1, 3, len(rows)), dtype=np.int64)
    for i, (g, h, c) in enumerate(rows):
        hist[0, :, i] = [int(g * (1 << S)), int(h * (1 << S)), c]
    off = np.concatenate([[0], np.cumsum([len(f) for f in features])]).astype(np.int32)
    return hist, off


def _case(hist, off, lam, min_leaf, mono, bounds, feat, bin_=None):
    return {
        "hist": hist, "bin_off": off, "lam": lam, "min_leaf": min_leaf,
        "mono": np.asarray(mono, dtype=np.int32),
        "bounds": np.asarray(bounds, dtype=np.float64).reshape(-1, 2),
        "feat": feat, "bin": bin_,
    }


def hand_cases() -> dict:
    """name -> case; ``feat`` / ``bin`` are the expected winner (-1: none)."""
    free = [[-INF, INF]]
    # feature 0 separates the gradients best, but its left side is the heavier
    # one (w_L = 40/11 > w_R): +1 rejects it. Feature 1 has the same totals.
    f0 = [(-40, 10, 40), (40, 10, 40)]
    f1 = [(-10, 5, 20), (-5, 5, 20), (15, 10, 40)]
    hist, off = _hist(f0, f1)
    cases = {
        "unconstrained_best": _case(hist, off, 1.0, 1, [0, 0], free, 0, 0),
        "second_best_chosen": _case(hist, off, 1.0, 1, [1, 0], free, 1, 1),
        "all_rejected": _case(hist, off, 1.0, 1, [1, 1], free, -1),
        "opposite_sign_accepts": _case(hist, off, 1.0, 1, [-1, -1], free, 0, 0),
        # w_R = -40/11 is clamped to -0.5, w_L = 40/11 stays
        "bounds_clamp_one_side": _case(hist, off, 1.0, 1, [0, 0], [[-0.5, 10.0]], 0, 0),
        # w = 0.25 on every side: the sides only pay l2 twice, gain = -l2 w^2
        # (exactly 0 with l2 = 0), so nothing splits
        "lo_equals_hi_l2_0": _case(hist, off, 0.0, 1, [0, 0], [[0.25, 0.25]], -1),
        "lo_equals_hi": _case(hist, off, 1.0, 1, [0, 0], [[0.25, 0.25]], -1),
    }
    # l2 = 0: feature 0's left side has no hessian (d_L = 0, -g/d = inf)
    z0 = [(-5, 0, 10), (5, 10, 10)]
    z1 = [(-4, 4, 8), (4, 6, 12)]
    hist, off = _hist(z0, z1)
    cases["zero_hessian_side"] = _case(hist, off, 0.0, 1, [0, -1], free, 1, 0)
    hist, off = _hist(z0)
    cases["zero_hessian_only"] = _case(hist, off, 0.0, 1, [-1], free, -1)

    # the two tie cases of test_hgbt_gpu.test_split_ties, with signs
    rng = np.random.default_rng(3)
    n = 600
    col = rng.integers(0, 8, size=n).astype(np.uint8)
    bins = np.stack([col, col, col])
    off = np.asarray([0, 8, 16, 24], dtype=np.int32)
    gq = ((col >= 4).astype(np.int32) * 2 - 1) * (1 << (S - 1))
    hq = np.full(n, 1 << (S - 2), dtype=np.int32)
    hist = cpu_ref.hgbt_hist_cpu(bins, off, np.zeros(n, dtype=np.int32), gq, hq, 1)
    cases["tie_features"] = _case(hist, off, 1.0, 1, [-1, -1, -1], free, 0, 3)
    cases["tie_features_first_barred"] = _case(hist, off, 1.0, 1, [1, -1, 0], free, 1, 3)
    # bins 1 and 2 empty: "bin <= 0", "<= 1" and "<= 2" are the same split
    hist, off = _hist([(-40, 10, 40), (0, 0, 0), (0, 0, 0), (40, 10, 40)])
    cases["tie_bins"] = _case(hist, off, 1.0, 1, [-1], free, 0, 0)
    return cases


def run_case(split_mono, case) -> np.ndarray:
    """``split_mono(hist, bin_off, lam, min_leaf, mono, bounds) -> records``
    on one case, checked word for word against the brute force."""
    args = [case[k] for k in ("hist", "bin_off", "lam", "min_leaf", "mono", "bounds")]
    got = split_mono(*args)
    np.testing.assert_array_equal(got, brute_force(*args))
    assert got[0, 1] == case["feat"]
    if case["feat"] < 0:
        assert (got[0, [0, 2, 3, 4, 5]] == 0).all()
    else:
        assert got[0, 2] == case["bin"]
    a, b = int(case["bin_off"][0]), int(case["bin_off"][1])
    np.testing.assert_array_equal(got[0, 6:9], case["hist"][0, :, a:b].sum(axis=1))
    return got

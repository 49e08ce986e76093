"""Micro-benchmark of the fused MMD permutation kernel (mmd_perm_kernel) on
rows embedded by the flagship model (bench.py's, fitted as bench/pdp_micro.py
fits it), P = 100 permutations.

    python bench/mmd_micro.py [--repeats N] [--sizes 1024,4096,16384] [--out FILE]

For n = m in --sizes (N = 2 n pooled rows), with device events (median of
--repeats after one warm-up each):

  (i)   one ext.mmd_perm_w call (operand padding, mmd_perm_kernel, the f64
        split sum): time, achieved FLOP/s with the operations computed from
        the shapes (2 N^2 (Dp + Qp), plus N^2 exponentials counted as one
        each), and the share of the f32 matrix peak;
  (ii)  the wall time of ScoringEngine.mmd_drift on the same rows (embedding,
        permutations, upload, kernel, statistics; gamma cached);
  (iii) the materialised torch formulation (Gram matrix, exp, matmul with the
        f32 indicator) on the same GPU where K is at most --torch-max-gib;
  (iv)  cpu_ref.mmd_perm_w_cpu (numpy, f64) at the smallest size, and the
        kernel's largest |W - W_ref| / N against it.

Last, the launch pair behind ScoringEngine.MMD_LAUNCH_ROWS: the kernel launch
at the caps (n = m = 16384) next to a forest_shap launch at SHAP_MAX_ROWS.

Needs a GPU."""

from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "bench"))

F32_MATRIX_PEAK = 157.3e12  # MI355X, FP32 matrix, FLOP/s (vendor data sheet)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sizes", default="1024,4096,16384")
    ap.add_argument("--permutations", type=int, default=100)
    ap.add_argument("--torch-max-gib", type=float, default=1.0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        print("mmd_micro: no GPU; nothing is measured", file=sys.stderr)
        return 2

    from pdp_micro import _flagship

    from creditcore import mmd
    from creditcore.data import make_request_batch
    from creditcore.engine import ScoringEngine
    from creditcore.ops import cpu_ref, gpu
    from creditcore.pack import encode_batch

    _, packed, _ = _flagship()
    eng = ScoringEngine(packed, device="cuda", device_index=0)
    dev = torch.device("cuda", 0)
    sizes = [int(s) for s in args.sizes.split(",")]
    n_perm = args.permutations
    top = max(sizes)
    b_codes, b_nums = encode_batch(make_request_batch(top, seed=11), packed.vocabs)
    r_codes, r_nums = encode_batch(make_request_batch(top, seed=12), packed.vocabs)

    def timed(fn) -> list[float]:
        fn()  # warm-up
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.repeats):
            t0 = torch.cuda.Event(enable_timing=True)
            t1 = torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            ms.append(t0.elapsed_time(t1))
        return ms

    lines = [
        f"device: {torch.cuda.get_device_name(0)}  repeats={args.repeats}  P={n_perm}  "
        f"D={packed.n_features_total}",
        "",
        f"{'n = m':>7}{'N':>7}{'cols/blk':>9}{'kernel ms':>11}{'TFLOP/s':>9}{'% peak':>8}"
        f"{'engine wall ms':>16}{'torch ms':>10}{'numpy ms':>10}",
    ]
    cap_ms = None
    for n in sizes:
        ref = (r_codes[:n], r_nums[:n])
        mu, sd = mmd.reference_scale(packed, ref[1])
        z_ref = mmd.embed(packed, ref[0], ref[1], mu, sd)
        z = np.concatenate([mmd.embed(packed, b_codes[:n], b_nums[:n], mu, sd), z_ref])
        gamma = mmd.median_gamma(z_ref)
        ind = mmd.indicator(n, n, n_perm, 0)
        big = 2 * n
        zp = mmd.pad_columns(z)
        dp, qp = zp.shape[1], -(-ind.shape[1] // 16) * 16
        cols = mmd.default_cols_per_block(big)
        z_d = torch.from_numpy(zp).to(dev)
        n_d = torch.from_numpy(mmd.squared_norms(z).astype(np.float32)).to(dev)
        i_d = torch.from_numpy(ind).to(dev)
        ms = float(np.median(timed(lambda: gpu.ext().mmd_perm_w(z_d, n_d, gamma, i_d, cols))))
        flops = 2.0 * big * big * (dp + qp) + float(big) * big
        if n == 16384:
            cap_ms = ms

        wall = []
        for _ in range(4):  # the first call computes and caches gamma
            t0 = time.perf_counter()
            eng.mmd_drift(b_codes[:n], b_nums[:n], reference=ref, n_permutations=n_perm)
            wall.append((time.perf_counter() - t0) * 1e3)

        torch_ms = "-"
        if 4.0 * big * big <= args.torch_max_gib * 2**30:
            i_f = i_d.float()

            def materialised():
                s = z_d @ z_d.T
                k = torch.exp(-gamma * (n_d[:, None] + n_d[None, :] - 2.0 * s).clamp_min_(0.0))
                k.fill_diagonal_(0.0)
                return k @ i_f

            torch_ms = f"{np.median(timed(materialised)):.2f}"
        numpy_ms = "-"
        if n == min(sizes):
            t0 = time.perf_counter()
            w_ref = cpu_ref.mmd_perm_w_cpu(z, gamma, ind)
            numpy_ms = f"{(time.perf_counter() - t0) * 1e3:.0f}"
            w = gpu.mmd_perm_w(z_d, n_d, gamma, i_d, cols)
            err = float(np.abs(w - w_ref).max() / big)
        lines.append(
            f"{n:>7}{big:>7}{cols:>9}{ms:>11.3f}{flops / ms / 1e9:>9.2f}"
            f"{100.0 * flops / (ms * 1e-3) / F32_MATRIX_PEAK:>8.1f}"
            f"{np.median(wall[1:]):>16.1f}{torch_ms:>10}{numpy_ms:>10}"
        )
    lines += ["", f"largest |W_gpu - W_ref| / N at n = m = {min(sizes)}: {err:.3e}"]

    if cap_ms is not None:
        cap = ScoringEngine.SHAP_MAX_ROWS
        codes, nums = encode_batch(make_request_batch(cap, seed=11), packed.vocabs)
        eng.explain_arrays(codes[:64], nums[:64], method="shap")  # uploads the tables
        sh = eng._shap_dev
        c_cap, x_cap = torch.from_numpy(codes).to(dev), torch.from_numpy(nums).to(dev)
        t_shap = float(np.median(timed(lambda: gpu.ext().forest_shap(
            c_cap, x_cap, sh["leaf_value"], sh["leaf_off"], sh["splits"], sh["medians"],
            int(packed.cls_kind), int(packed.cls_n_trees)))))
        ok = "within" if cap_ms <= 1.25 * t_shap else "OUTSIDE"
        lines += [
            f"launch pair: mmd_perm_w at the caps (n = m = 16384, N = 32768, one launch) "
            f"{cap_ms:.2f} ms; forest_shap B={cap} {t_shap:.2f} ms (bound "
            f"{1.25 * t_shap:.2f} ms) -> {ok} the rule",
        ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())

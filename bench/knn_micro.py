"""Micro-benchmark of the fused nearest-neighbour kernels (knn_topk_kernel,
knn_merge_kernel) on rows embedded by the flagship model (bench.py's, fitted
as bench/pdp_micro.py fits it).

    python bench/knn_micro.py [--repeats N] [--sizes 1024,4096,16384] [--ks 10,32] [--out FILE]

For B = M in --sizes and k in --ks, with device events (median of --repeats
after one warm-up each):

  (i)   one ext.knn_topk call (norm padding, both kernels): time, achieved
        FLOP/s of the distance GEMM counted from the shapes (2 B M Dp), and
        the share of the f32 matrix peak;
  (ii)  the wall time of ScoringEngine.knn_outliers on the same rows
        (embedding, upload, kernels, scores; the reference's leave-one-out
        pass cached);
  (iii) torch.cdist(...)**2 + torch.topk on the same tensors, which holds the
        B x M matrix;
  (iv)  cpu_ref.knn_topk_cpu (numpy, f64) at the smallest size, and whether
        the kernel's indices equal it where the f64 distances are not within
        the f32 bound of a tie.

Last, the launch pair behind ScoringEngine.KNN_LAUNCH_ROWS: the launch at the
caps (B = M = 16384, the largest k) next to a forest_shap launch at
SHAP_MAX_ROWS.

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
    ap.add_argument("--ks", default="10,32")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        print("knn_micro: no GPU; nothing is measured", file=sys.stderr)
        return 2

    from pdp_micro import _flagship

    from creditcore import knn, mmd
    from creditcore.data import make_request_batch
    from creditcore.engine import ScoringEngine
    from creditcore.ops import cpu_ref, gpu
    from creditcore.pack import encode_batch

    _, packed, _ = _flagship()
    eng = ScoringEngine(packed, device="cuda", device_index=0)
    dev = torch.device("cuda", 0)
    sizes = [int(s) for s in args.sizes.split(",")]
    ks = [int(s) for s in args.ks.split(",")]
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
        f"device: {torch.cuda.get_device_name(0)}  repeats={args.repeats}  "
        f"D={packed.n_features_total}",
        "",
        f"{'B = M':>7}{'k':>4}{'cols/blk':>9}{'kernels ms':>12}{'TFLOP/s':>9}{'% peak':>8}"
        f"{'engine wall ms':>16}{'cdist+topk ms':>15}{'numpy ms':>10}",
    ]
    cap_ms, agree = None, ""
    for n in sizes:
        ref = (r_codes[:n], r_nums[:n])
        mu, sd = mmd.reference_scale(packed, ref[1])
        z_ref = mmd.embed(packed, ref[0], ref[1], mu, sd)
        z_b = mmd.embed(packed, b_codes[:n], b_nums[:n], mu, sd)
        zr_d = torch.from_numpy(mmd.pad_columns(z_ref)).to(dev)
        zb_d = torch.from_numpy(mmd.pad_columns(z_b)).to(dev)
        nr_d = torch.from_numpy(mmd.squared_norms(z_ref).astype(np.float32)).to(dev)
        nb_d = torch.from_numpy(mmd.squared_norms(z_b).astype(np.float32)).to(dev)
        dp = int(zr_d.shape[1])
        cols = knn.default_cols_per_block(n, n)
        flops = 2.0 * n * n * dp
        for k in ks:
            ms = float(np.median(timed(
                lambda: gpu.ext().knn_topk(zb_d, zr_d, nb_d, nr_d, k, False, cols))))
            if n == 16384 and k == max(ks):
                cap_ms = ms

            wall = []
            for _ in range(4):  # the first call runs and caches the leave-one-out pass
                t0 = time.perf_counter()
                eng.knn_outliers(b_codes[:n], b_nums[:n], reference=ref, k=k)
                wall.append((time.perf_counter() - t0) * 1e3)

            torch_ms = float(np.median(timed(
                lambda: torch.topk(torch.cdist(zb_d, zr_d) ** 2, k, dim=1, largest=False))))
            numpy_ms = "-"
            if n == min(sizes):
                t0 = time.perf_counter()
                w_d2, w_idx = cpu_ref.knn_topk_cpu(z_b, z_ref, k)
                numpy_ms = f"{(time.perf_counter() - t0) * 1e3:.0f}"
                _, idx = gpu.knn_topk(zb_d, zr_d, nb_d, nr_d, k, False, cols)
                # rows whose k + 1 nearest f64 distances are apart by more than the bound
                d2x, _ = cpu_ref.knn_topk_cpu(z_b, z_ref, k + 1)
                bound = (2 * dp + 4) * 2.0**-24 * 2.0 * np.maximum(
                    mmd.squared_norms(z_b).max(), mmd.squared_norms(z_ref).max())
                sure = (np.diff(d2x, axis=1) > 2 * bound).all(axis=1)
                same = (idx[sure] == w_idx[sure]).all()
                agree += (f"k = {k}: indices equal the f64 reference on all {int(sure.sum())} of "
                          f"{n} rows without a near-tie: {bool(same)}\n")
            lines.append(
                f"{n:>7}{k:>4}{cols:>9}{ms:>12.3f}{flops / ms / 1e9:>9.2f}"
                f"{100.0 * flops / (ms * 1e-3) / F32_MATRIX_PEAK:>8.1f}"
                f"{np.median(wall[1:]):>16.1f}{torch_ms:>15.3f}{numpy_ms:>10}"
            )
    lines += ["", agree.rstrip()]

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
            f"launch pair: knn_topk at the caps (B = M = 16384, k = {max(ks)}, one launch) "
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

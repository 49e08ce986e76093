"""Micro-benchmark of the forest proximity kernels (forest_leaf_kernel,
forest_prox_topk_kernel) on two models over bench.py's frame: the flagship
random forest (500 trees, depth 16; short leaf lists) and a GPU-trained hgbt
(500 trees, depth 6; long leaf lists, the hard case).

    python bench/prox_micro.py [--repeats N] [--sizes 256,4096,16384] [--k 10] [--out FILE]

For each model and B = M in --sizes, with device events (median of --repeats
after one warm-up each):

  (i)   one ext.forest_leaves call on the batch and one ext.forest_prox_topk
        call (the index built before, not timed), separately; the latter with
        the index's own lanes_per_tree and with a whole wave per tree, and the
        number of co-memberships it walks per batch row;
  (ii)  the inverted index (torch sort / bincount / cumsum), once;
  (iii) the wall time of ScoringEngine.proximity on the same rows (upload,
        both kernels on the batch, scores; the reference side cached);
  (iv)  the same neighbours by the dense formulation in torch: a chunked
        (leaf_b[:, None] == leaf_r[None]).sum(-1) followed by topk, and
        whether its counts equal the kernel's;
  (v)   at the smallest size cpu_ref (numpy) and, for the random forest,
        scikit-learn apply + numpy.

Last, the launch pair behind ScoringEngine.PROX_LAUNCH_ROWS: on the model
that was slowest at the largest size, at k = 32, one forest_prox_topk launch
of a quarter, a half, three quarters and all of the batch rows (and of
PROX_LAUNCH_ROWS) next to a forest_shap launch at SHAP_MAX_ROWS.

Needs a GPU."""

from __future__ import annotations

import argparse
import dataclasses
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "bench"))

DENSE_BYTES = 1 << 30  # compares held at once by the dense formulation


def _hgbt(packed_rf):
    """The flagship pack with a 500 x depth 6 hgbt classifier, same frame."""
    import bench
    from creditcore.data import make_uci_shaped_frame
    from creditcore.models.forest import make_classifier_pipeline
    from creditcore.pack import pack_classifier_pipeline
    from creditcore.schema import FEATURES, TARGET

    df = make_uci_shaped_frame(n_rows=bench.TRAIN_ROWS, seed=2024)
    pipe = make_classifier_pipeline(
        {"n_estimators": 500, "max_depth": 6, "random_state": 2024}, "hgbt")
    pipe.fit(df[FEATURES], df[TARGET].values.ravel())
    return dataclasses.replace(packed_rf, **pack_classifier_pipeline(pipe))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sizes", default="256,4096,16384")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import pandas as pd
    import torch

    if not torch.cuda.is_available():
        print("prox_micro: no GPU; nothing is measured", file=sys.stderr)
        return 2

    from pdp_micro import _flagship

    from creditcore.data import make_request_batch
    from creditcore.engine import ScoringEngine
    from creditcore.ops import cpu_ref, gpu
    from creditcore.pack import encode_batch
    from creditcore.schema import FEATURES

    pipe, packed_rf, _ = _flagship()
    models = [("rf 500 x depth 16", packed_rf, pipe), ("hgbt 500 x depth 6", _hgbt(packed_rf), None)]
    dev = torch.device("cuda", 0)
    sizes = [int(s) for s in args.sizes.split(",")]
    k, top = args.k, max(sizes)
    batch_df = pd.DataFrame(make_request_batch(top, seed=11))
    ref_df = pd.DataFrame(make_request_batch(top, seed=12))
    b_codes, b_nums = encode_batch(batch_df, packed_rf.vocabs)
    r_codes, r_nums = encode_batch(ref_df, packed_rf.vocabs)

    def timed(fn) -> float:
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
        return float(np.median(ms))

    def dense(leaf_b, leaf_r):
        step = max(1, DENSE_BYTES // (leaf_r.shape[0] * leaf_r.shape[1]))
        parts = [
            torch.topk((leaf_b[a:a + step, None, :] == leaf_r[None]).sum(-1), k, dim=1)
            for a in range(0, leaf_b.shape[0], step)
        ]
        return torch.cat([p.values for p in parts]), torch.cat([p.indices for p in parts])

    lines = [f"device: {torch.cuda.get_device_name(0)}  repeats={args.repeats}  k={k}"]
    longest, worst, eng_rf = 0.0, None, None
    for name, packed, sk_pipe in models:
        eng = ScoringEngine(packed, device="cuda", device_index=0)
        eng_rf = eng_rf or eng
        with eng._explain_lock:
            m = eng._forest_dev()
        tabs = (m["cls_nodes"], m["cls_off"], m["feat_col"], m["feat_code"], m["medians"])
        lines += [
            "",
            f"{name}: {packed.cls_n_trees} trees, {len(packed.cls_nodes)} nodes",
            f"{'B = M':>7}{'leaf ms':>9}{'index ms':>10}{'lanes':>7}{'pairs/row':>11}{'prox ms':>9}"
            f"{'wave/tree ms':>14}{'engine wall ms':>16}{'dense torch ms':>16}{'same':>6}"
            f"{'numpy ms':>10}{'sklearn ms':>12}",
        ]
        for n in sizes:
            bc, bx = torch.from_numpy(b_codes[:n]).to(dev), torch.from_numpy(b_nums[:n]).to(dev)
            rc, rx = torch.from_numpy(r_codes[:n]).to(dev), torch.from_numpy(r_nums[:n]).to(dev)
            leaf_ms = timed(lambda: gpu.ext().forest_leaves(bc, bx, *tabs))
            leaf_b = gpu.ext().forest_leaves(bc, bx, *tabs)
            leaf_r = gpu.ext().forest_leaves(rc, rx, *tabs)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            index = gpu.prox_index(leaf_r, len(packed.cls_nodes))
            torch.cuda.synchronize()
            index_ms = (time.perf_counter() - t0) * 1e3
            start = index["leaf_start"].to(torch.int64)
            sizes_of = (start[1:] - start[:-1])[leaf_b.to(torch.int64)]  # [B, T] list lengths
            pairs = float(sizes_of.sum()) / n

            def prox(lanes):
                return gpu.ext().forest_prox_topk(
                    leaf_b, index["leaf_start"], index["leaf_rows"], n, k, False, lanes)

            prox_ms = timed(lambda: prox(index["lanes_per_tree"]))
            wave_ms = timed(lambda: prox(64))
            if n == top and prox_ms > longest:  # the launch pair's case
                longest, worst = prox_ms, (name, leaf_b, index)

            wall = []
            for _ in range(4):  # the first call builds and caches the reference side
                t0 = time.perf_counter()
                eng.proximity(b_codes[:n], b_nums[:n], reference=(r_codes[:n], r_nums[:n]), k=k)
                wall.append((time.perf_counter() - t0) * 1e3)

            dense_ms = timed(lambda: dense(leaf_b, leaf_r))
            same = bool((dense(leaf_b, leaf_r)[0] == prox(64)[0]).all())
            numpy_ms = sk_ms = "-"
            if n == min(sizes):
                imp_b = cpu_ref.impute_nums(packed, b_nums[:n])
                imp_r = cpu_ref.impute_nums(packed, r_nums[:n])
                t0 = time.perf_counter()
                cpu_ref.forest_prox_topk_cpu(
                    cpu_ref.forest_leaves_cpu(packed, b_codes[:n], imp_b),
                    cpu_ref.forest_leaves_cpu(packed, r_codes[:n], imp_r), k)
                numpy_ms = f"{(time.perf_counter() - t0) * 1e3:.0f}"
                if sk_pipe is not None:
                    t0 = time.perf_counter()
                    a = sk_pipe[-1].apply(sk_pipe[:-1].transform(batch_df[FEATURES].iloc[:n]))
                    r = sk_pipe[-1].apply(sk_pipe[:-1].transform(ref_df[FEATURES].iloc[:n]))
                    c = np.stack([(a[i][None] == r).sum(-1) for i in range(n)])
                    np.argsort(-c, axis=1, kind="stable")[:, :k]
                    sk_ms = f"{(time.perf_counter() - t0) * 1e3:.0f}"
            lines.append(
                f"{n:>7}{leaf_ms:>9.3f}{index_ms:>10.1f}{index['lanes_per_tree']:>7}{pairs:>11.0f}"
                f"{prox_ms:>9.3f}{wave_ms:>14.3f}{np.median(wall[1:]):>16.1f}{dense_ms:>16.3f}"
                f"{str(same):>6}{numpy_ms:>10}{sk_ms:>12}"
            )

    cap = ScoringEngine.SHAP_MAX_ROWS
    codes, nums = encode_batch(make_request_batch(cap, seed=11), packed_rf.vocabs)
    eng_rf.explain_arrays(codes[:64], nums[:64], method="shap")  # uploads the tables
    sh = eng_rf._shap_dev
    c_cap, x_cap = torch.from_numpy(codes).to(dev), torch.from_numpy(nums).to(dev)
    t_shap = timed(lambda: gpu.ext().forest_shap(
        c_cap, x_cap, sh["leaf_value"], sh["leaf_off"], sh["splits"], sh["medians"],
        int(packed_rf.cls_kind), int(packed_rf.cls_n_trees)))
    name, leaf_b, index = worst
    lines += [
        "",
        f"launch pair: forest_shap B={cap} {t_shap:.2f} ms (bound {1.25 * t_shap:.2f} ms); "
        f"forest_prox_topk on {name}, M = {top}, k = 32, one launch of",
    ]
    for rows in sorted({top // 4, top // 2, 3 * top // 4, top, ScoringEngine.PROX_LAUNCH_ROWS}):
        if rows <= top:
            ms = timed(lambda: gpu.ext().forest_prox_topk(
                leaf_b, index["leaf_start"], index["leaf_rows"], top, 32, False,
                index["lanes_per_tree"], 0, rows))
            ok = "within" if ms <= 1.25 * t_shap else "OUTSIDE"
            mark = "  <- PROX_LAUNCH_ROWS" if rows == ScoringEngine.PROX_LAUNCH_ROWS else ""
            lines.append(f"  {rows:>6} batch rows {ms:>8.2f} ms -> {ok} the rule{mark}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())

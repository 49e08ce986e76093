"""Micro-benchmark of the counterfactual sweep kernel on the flagship forest
(RF 500 trees x depth 16, fitted as bench/pdp_micro.py fits it).

    python bench/cf_micro.py [--repeats N] [--rows 256] [--brute-rows 32] [--out FILE]

Times, with device events (median of --repeats after one warm-up each):

  (i)   the sweep of --rows rows x all 14 numeric columns: one forest_sweep
        call (job-table upload, forest_sweep_kernel, forest_sweep_search_kernel)
        and the wall time of ScoringEngine.counterfactuals on the same rows;
  (ii)  the same curves by brute force through forest_whatif on the full
        threshold grid (one what-if job per interval), for --brute-rows rows,
        scaled to --rows; the curves of both are compared exactly;
  (iii) the longest single sweep launch the engine issues: CF_LAUNCH_JOBS jobs
        of a SHAP_MAX_ROWS-row call;
  (iv)  a forest_shap launch at ScoringEngine.SHAP_MAX_ROWS rows, the longest
        launch the engine issued before, which (iii) may not exceed.

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


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--brute-rows", type=int, default=32)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        print("cf_micro: no GPU; nothing is measured", file=sys.stderr)
        return 2

    from pdp_micro import _flagship

    from creditcore import counterfactual as cf
    from creditcore.data import make_request_batch
    from creditcore.engine import ScoringEngine
    from creditcore.ops import gpu
    from creditcore.pack import N_CAT, N_NUM, encode_batch
    from creditcore.schema import FEATURES

    pipe, packed, _ = _flagship()
    eng = ScoringEngine(packed, device="cuda", device_index=0)
    cap = ScoringEngine.SHAP_MAX_ROWS
    codes, nums = encode_batch(make_request_batch(cap, seed=11), packed.vocabs)
    n_trees = int(packed.cls_n_trees)
    numeric = list(FEATURES[N_CAT:])
    cols = list(range(N_NUM))
    cut = cf.raw_cut(packed, 0.5)
    r, rb = args.rows, args.brute_rows

    # one engine call per path uploads the tables
    eng.explain_arrays(codes[:64], nums[:64], method="shap")
    eng.counterfactuals(codes[:8], nums[:8], features=numeric)
    eng.partial_dependence(["sex"], sample=(codes[:8], nums[:8]))
    ext, m, sh, sw = eng._gpu["ext"], eng._explain_dev, eng._shap_dev, eng._cf_dev
    tables = eng._cf
    dev = torch.device("cuda", 0)
    c_cap = torch.from_numpy(codes).to(dev)
    x_cap = torch.from_numpy(nums).to(dev)
    k_of = [len(t) for t in tables.thresholds]

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

    def sweep_launch(jobs: np.ndarray):
        jt = torch.from_numpy(np.ascontiguousarray(jobs, dtype=np.int32))

        def go():
            return ext.forest_sweep(
                c_cap, x_cap, m["cls_nodes"], m["cls_off"], m["feat_col"], m["feat_code"],
                m["medians"], sw["node_rank"], sw["thr"], sw["thr_off"], jt, cut,
                int(sw["max_depth"]), False,
            )

        return go

    def shap_launch():
        return ext.forest_shap(
            c_cap, x_cap, sh["leaf_value"], sh["leaf_off"], sh["splits"], sh["medians"],
            int(packed.cls_kind), n_trees,
        )

    # brute force: every interval of a column as one what-if job on rb rows
    c_b, x_b = c_cap[:rb].contiguous(), x_cap[:rb].contiguous()
    step = max(1, ScoringEngine.PDP_LAUNCH_PAIRS // rb)
    brute_jobs = []
    for c in cols:
        values = cf.representatives(tables.thresholds[c])
        wj = np.zeros((len(values), 4), dtype=np.int32)
        wj[:, 0], wj[:, 1], wj[:, 2] = N_CAT + c, values.view(np.int32), -1
        brute_jobs += [torch.from_numpy(wj[s : s + step].copy()) for s in range(0, len(wj), step)]

    def brute():
        return [
            ext.forest_whatif(
                c_b, x_b, m["cls_nodes"], m["cls_off"], m["feat_col"], m["feat_code"],
                m["medians"], jt,
            )
            for jt in brute_jobs
        ]

    # the two compute the same curves, bit for bit
    jobs_b = cf.sweep_jobs(rb, cols)
    _, _, curves = gpu.forest_sweep(c_cap, x_cap, m, sw, jobs_b, cut, True)
    whatif = torch.cat(brute()).cpu().numpy()  # [sum (K+1), rb], column after column
    at, same = 0, True
    for ci, c in enumerate(cols):
        block = whatif[at : at + k_of[c] + 1]
        at += k_of[c] + 1
        for row in range(rb):
            same &= bool(np.array_equal(curves[row * len(cols) + ci], block[:, row]))

    lines = [
        f"model: {type(pipe.named_steps['classifier']).__name__} trees={n_trees} "
        f"nodes={len(packed.cls_nodes)} depth={tables.max_depth}",
        f"thresholds per numeric column K: {k_of} (sum {sum(k_of)})",
        f"device: {torch.cuda.get_device_name(0)}  repeats={args.repeats} "
        "(device events around one call incl. the job-table upload, after one warm-up)",
        f"sweep curves == brute-force curves on {rb} rows x {N_NUM} columns, bit for bit: {same}",
        "",
        f"{'launch':<58}{'median ms':>11}{'min ms':>10}{'max ms':>10}",
    ]

    def row(name: str, ms: list[float]) -> float:
        med = float(np.median(ms))
        lines.append(f"{name:<58}{med:>11.2f}{min(ms):>10.2f}{max(ms):>10.2f}")
        return med

    t_sweep = row(f"(i) forest_sweep {r} rows x {N_NUM} cols = {r * N_NUM} jobs",
                  timed(sweep_launch(cf.sweep_jobs(r, cols))))
    t_brute_b = row(f"(ii) forest_whatif brute, {rb} rows x {sum(k_of) + N_NUM} intervals",
                    timed(brute))
    t_brute = t_brute_b * r / rb
    launch_jobs = int(ScoringEngine.CF_LAUNCH_JOBS)
    t_long = row(f"(iii) forest_sweep CF_LAUNCH_JOBS = {launch_jobs} jobs of {cap} rows",
                 timed(sweep_launch(cf.sweep_jobs(cap, cols)[:launch_jobs])))
    t_shap = row(f"(iv) forest_shap B={cap}", timed(shap_launch))

    wall = []
    for _ in range(3):
        t0 = time.perf_counter()
        eng.counterfactuals(codes[:r], nums[:r], features=numeric)
        wall.append((time.perf_counter() - t0) * 1e3)
    lines += [
        "",
        f"(i) engine wall, counterfactuals({r} rows, 14 numeric features): "
        f"median {np.median(wall):.1f} ms (min {min(wall):.1f})",
        f"(ii) brute force scaled to {r} rows: {t_brute:.2f} ms = "
        f"{t_brute / t_sweep:.1f} x the sweep ({t_sweep:.2f} ms)",
        f"(iii) vs (iv): longest sweep launch {t_long:.2f} ms, forest_shap at its cap "
        f"{t_shap:.2f} ms -> {'within' if t_long <= t_shap else 'OUTSIDE'} the rule "
        "(a sweep launch may not exceed it)",
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

"""Per-kernel micro-benchmarks (hipEvent timing via torch.cuda.Event).

Sweeps launch configurations of the hot kernels on a real MI355X so the
session picks measured-best settings:

    python bench/kernel_micro.py            # K-S sweep + forest timing
    python bench/kernel_micro.py --shap-only   # the forest_shap section alone
"""

from __future__ import annotations

import json

import numpy as np

import os as _os
import sys as _sys
_sys.path.insert(0, _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))


def timed(fn, iters=50, warmup=10):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s = torch.cuda.Event(enable_timing=True)
    e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3  # µs


def timed_samples(fns: dict, rounds=15, iters=20, warmup=10) -> dict:
    """Interleaved rounds in one process: every round times each variant, so
    clock/thermal drift hits all of them alike. Returns per-variant
    {median, min, max} in µs over the rounds."""
    for fn in fns.values():
        timed(fn, iters=warmup, warmup=0)
    samples = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            samples[k].append(timed(fn, iters=iters, warmup=0))
    return {
        k: {
            "median_us": round(float(np.median(v)), 2),
            "min_us": round(min(v), 2),
            "max_us": round(max(v), 2),
        }
        for k, v in samples.items()
    }


def main():
    import torch

    from creditcore.ops import gpu
    from creditcore.pack import encode_batch
    from creditcore.data import make_request_batch

    import bench as flagship

    ext = gpu.ext()
    # the flagship bench model (500 trees x depth 16), from its cache
    p, _ = flagship._build_packed(flagship.bench_cache_dir())
    dev = torch.device("cuda", 0)

    medians = torch.from_numpy(p.medians).to(dev)
    ref = torch.from_numpy(p.ref_sorted).to(dev)
    rs_off = torch.from_numpy(p.ref_sorted_offsets).to(dev)

    shap_only = "--shap-only" in _sys.argv[1:]
    results = {}
    for b in () if shap_only else (1024, 4096, 16384):
        recs = make_request_batch(b, seed=b)
        codes, nums = encode_batch(recs, p.vocabs)
        d_nums = torch.from_numpy(nums).to(dev)
        for block in (256, 512):
            key = f"ks b={b} block={block}"
            try:
                us = timed(lambda: ext.ks_stats(d_nums, medians, ref, rs_off, block, 0))
                results[key] = round(us, 2)
            except Exception as exc:
                results[key] = f"error: {exc}"

    # forest via the functional pipeline (classifier + iforest + finalize)
    cls_nodes = torch.from_numpy(np.ascontiguousarray(p.cls_nodes)).to(dev)
    cls_off = torch.from_numpy(p.cls_tree_offsets).to(dev)
    if_nodes = torch.from_numpy(np.ascontiguousarray(p.if_nodes)).to(dev)
    if_off = torch.from_numpy(p.if_tree_offsets).to(dev)
    fc = torch.from_numpy(p.feat_col).to(dev)
    fk = torch.from_numpy(p.feat_code).to(dev)
    for b in () if shap_only else (1024, 16384):
        recs = make_request_batch(b, seed=b)
        codes, nums = encode_batch(recs, p.vocabs)
        d_codes = torch.from_numpy(codes).to(dev)
        d_nums = torch.from_numpy(nums).to(dev)
        us = timed(
            lambda: ext.score_forest_pipeline(
                d_codes, d_nums, cls_nodes, cls_off, fc, fk, medians,
                p.n_onehot, if_nodes, if_off,
                p.if_denom, p.if_offset, p.if_threshold,
            )
        )
        results[f"forest_pipeline b={b}"] = round(us, 2)
        # A/B: ILP depth x grid layout (classifier forest alone)
        # 0=1-tree, 1=ilp2, 2=ilp4, 3=ilp2+XCD-transposed grid, 4=ilp4+transposed
        for ilp in (0, 1, 2, 3, 4):
            us = timed(
                lambda: ext.forest_ilp_bench(
                    d_codes, d_nums, cls_nodes, cls_off, fc, fk, medians, ilp
                )
            )
            results[f"forest_cls b={b} ilp={ilp}"] = round(us, 2)
        a = ext.forest_ilp_bench(d_codes, d_nums, cls_nodes, cls_off, fc, fk, medians, 0)
        for v in (1, 2, 3, 4):
            c = ext.forest_ilp_bench(d_codes, d_nums, cls_nodes, cls_off, fc, fk, medians, v)
            results[f"forest_ilp_parity b={b} v={v}"] = float((a - c).abs().max().item())

    # attributions next to the scorer's classifier kernel at the same shape:
    # forest_contrib vs forest_kernel<false> (ilp=0, the kernel
    # score_forest_pipeline launches for the classifier), interleaved rounds
    if shap_only:
        pass
    elif p.cls_node_value is None:
        results["forest_contrib"] = "skipped: cached bench model predates node values"
    else:
        node_value = torch.from_numpy(p.cls_node_value).to(dev)
        b = 1024
        codes, nums = encode_batch(make_request_batch(b, seed=b), p.vocabs)
        d_codes = torch.from_numpy(codes).to(dev)
        d_nums = torch.from_numpy(nums).to(dev)
        def contrib(block_target=None):
            extra = () if block_target is None else (block_target,)
            return lambda: ext.forest_contrib(
                d_codes, d_nums, cls_nodes, node_value, cls_off, fc, fk,
                medians, p.cls_kind, *extra,
            )

        stats = timed_samples(
            {
                "forest_contrib": contrib(),
                # A/B of the grid size: fewer blocks = more trees per thread
                # = fewer atomics, against fewer waves in flight
                **{f"forest_contrib blocks={t}": contrib(t) for t in (2048, 1024, 256)},
                "forest_cls": lambda: ext.forest_ilp_bench(
                    d_codes, d_nums, cls_nodes, cls_off, fc, fk, medians, 0
                ),
                "forest_pipeline": lambda: ext.score_forest_pipeline(
                    d_codes, d_nums, cls_nodes, cls_off, fc, fk, medians,
                    p.n_onehot, if_nodes, if_off,
                    p.if_denom, p.if_offset, p.if_threshold,
                ),
            }
        )
        for k, v in stats.items():
            results[f"{k} b={b} samples"] = v
        results[f"forest_contrib/forest_cls b={b}"] = round(
            stats["forest_contrib"]["median_us"] / stats["forest_cls"]["median_us"], 3
        )

    # exact TreeSHAP next to the Saabas kernel on the same model: the path
    # table's size and build time, then forest_shap vs forest_contrib at a
    # full request (1024 rows) and at one row, interleaved rounds
    if p.cls_node_cover is None or p.cls_node_value is None:
        results["forest_shap"] = "skipped: cached bench model predates node cover"
    else:
        import time

        from creditcore.engine import _check_shap_paths
        from creditcore.pack import build_shap_paths

        t0 = time.perf_counter()
        paths, _ = build_shap_paths(p)
        t1 = time.perf_counter()
        _check_shap_paths(paths)
        t2 = time.perf_counter()
        results["forest_shap table"] = {
            "leaves": paths.n_leaves,
            "splits": int(len(paths.splits)),
            "mean_depth": round(len(paths.splits) / max(paths.n_leaves, 1), 2),
            "bytes": int(paths.splits.nbytes + paths.leaf_off.nbytes + paths.leaf_value.nbytes),
            "build_s": round(t1 - t0, 3),
            "check_s": round(t2 - t1, 3),
        }
        leaf_value = torch.from_numpy(paths.leaf_value).to(dev)
        leaf_off = torch.from_numpy(paths.leaf_off).to(dev)
        splits = torch.from_numpy(paths.splits).to(dev)
        node_value = torch.from_numpy(p.cls_node_value).to(dev)
        for b in (1024, 1):
            codes, nums = encode_batch(make_request_batch(b, seed=b + 7), p.vocabs)
            d_codes = torch.from_numpy(codes).to(dev)
            d_nums = torch.from_numpy(nums).to(dev)

            def shap(block_target=None, d_codes=d_codes, d_nums=d_nums):
                extra = () if block_target is None else (block_target,)
                return lambda: ext.forest_shap(
                    d_codes, d_nums, leaf_value, leaf_off, splits, medians,
                    p.cls_kind, p.cls_n_trees, *extra,
                )

            stats = timed_samples(
                {
                    "forest_shap": shap(),
                    **{f"forest_shap blocks={t}": shap(t) for t in (1024, 8192)},
                    "forest_contrib": lambda d_codes=d_codes, d_nums=d_nums: ext.forest_contrib(
                        d_codes, d_nums, cls_nodes, node_value, cls_off, fc, fk,
                        medians, p.cls_kind,
                    ),
                },
                rounds=5, iters=1, warmup=1,  # a launch is long; few suffice
            )
            for k, v in stats.items():
                results[f"{k} b={b} samples"] = v
            results[f"forest_shap/forest_contrib b={b}"] = round(
                stats["forest_shap"]["median_us"] / stats["forest_contrib"]["median_us"], 1
            )

    print(json.dumps(results, indent=2))


if __name__ == "__main__":
    main()

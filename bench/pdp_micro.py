"""Launch-length micro-benchmark of the partial-dependence what-if kernel on
the flagship forest (RF 500 trees x depth 16, trained as bench.py trains it).

    python bench/pdp_micro.py [--repeats N] [--out FILE] [--skip-sklearn]

Times single launches with device events (median of --repeats after one
warm-up launch per shape):

  forest_shap    at ScoringEngine.SHAP_MAX_ROWS rows — the launch length the
                 project already accepts on a shared GPU;
  forest_whatif  on the packed 256-row background sample over a sweep of
                 (job, row) pair counts, and at the largest single launch the
                 engine issues (PDP_LAUNCH_PAIRS // 256 jobs).

The rule that sizes ScoringEngine.PDP_LAUNCH_PAIRS: the longest what-if launch
is no longer than 1.25 x the forest_shap launch at its cap (the rule of
ISHAP_MAX_PAIRS). The script prints the largest swept pair count that meets
the rule and whether the constant as committed meets it.

It also records two wall times of the default request — the one-way curves of
all 23 features at grid_resolution 20 on the packed sample: the engine's
partial_dependence on the GPU, and scikit-learn's
partial_dependence(method="brute") on the same pipeline, sample and grids.
A recorded number for the README, not a gate. Needs a GPU."""

from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SWEEP = (4096, 16384, 65536, 131072, 262144, 524288, 1048576, 2097152)
NOISE = 1.25


def _flagship():
    """(pipeline, packed) of bench.py's model: same frame, parameters, seed."""
    import bench
    from creditcore import train as T
    from creditcore.data import make_uci_shaped_frame
    from creditcore.models.forest import make_classifier_pipeline
    from creditcore.pack import (
        PackedModel,
        pack_classifier_pipeline,
        pack_drift,
        pack_isolation_forest,
    )
    from creditcore.schema import FEATURES, TARGET

    seed = 2024
    df = make_uci_shaped_frame(n_rows=bench.TRAIN_ROWS, seed=seed)
    params = {k: v for k, v in bench.BENCH_MODEL.items() if k != "algo"}
    algo = bench.BENCH_MODEL.get("algo", "rf")
    pipe = make_classifier_pipeline({**params, "random_state": seed}, algo)
    pipe.fit(df[FEATURES], df[TARGET].values.ravel())
    drift, outlier = T.fit_detectors(df)
    c = pack_classifier_pipeline(pipe)
    packed = PackedModel(**c, **pack_isolation_forest(outlier), **pack_drift(drift, c["vocabs"]))
    return pipe, packed, drift


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--skip-sklearn", action="store_true")
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        print("pdp_micro: no GPU; launch lengths are not measured", file=sys.stderr)
        return 2

    import pandas as pd

    from creditcore.data import make_request_batch
    from creditcore.engine import ScoringEngine
    from creditcore.ops import cpu_ref
    from creditcore.pack import encode_batch
    from creditcore.schema import CATEGORICAL_FEATURES, FEATURES

    pipe, packed, drift = _flagship()
    eng = ScoringEngine(packed, device="cuda", device_index=0)
    cap = ScoringEngine.SHAP_MAX_ROWS
    codes, nums = encode_batch(make_request_batch(cap, seed=11), packed.vocabs)
    r = len(packed.bg_codes)
    n_trees = int(packed.cls_n_trees)

    # one engine call per path uploads the tables; the what-if is checked
    # against the CPU reference on a few jobs (exact: same order of sums)
    eng.explain_arrays(codes[:64], nums[:64], method="shap")
    first = eng.partial_dependence(["credit_limit", "sex"], kind="both", grid_resolution=4)
    ref = ScoringEngine(packed, device="cpu").partial_dependence(
        ["credit_limit", "sex"], kind="both", grid_resolution=4
    )
    err = max(
        float(np.abs(a["individual"] - b["individual"]).max())
        for a, b in zip(first["results"], ref["results"])
    )

    ext, m, sh = eng._gpu["ext"], eng._explain_dev, eng._shap_dev
    smp = eng._pdp_sample_dev
    dev = torch.device("cuda", 0)

    # job table of the sweep: every feature in turn, values from its own grid
    all_one_way = eng.partial_dependence(list(FEATURES))
    from creditcore import pdp

    imp = cpu_ref.impute_nums(packed, packed.bg_nums)
    axes = [pdp.build_axis(n, packed.vocabs, imp, 20, (0.05, 0.95), None) for n in FEATURES]
    base = np.concatenate([pdp.entry_jobs([a]) for a in axes])
    n_default = len(base)

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

    c_cap = torch.from_numpy(codes).to(dev)
    x_cap = torch.from_numpy(nums).to(dev)

    def shap_launch():
        return ext.forest_shap(
            c_cap, x_cap, sh["leaf_value"], sh["leaf_off"], sh["splits"], sh["medians"],
            int(packed.cls_kind), n_trees,
        )

    def whatif_launch(n_jobs: int):
        jobs = torch.from_numpy(np.ascontiguousarray(np.resize(base, (n_jobs, 4))))

        def go():
            return ext.forest_whatif(
                smp[0], smp[1], m["cls_nodes"], m["cls_off"], m["feat_col"], m["feat_code"],
                m["medians"], jobs,
            )

        return go

    lines = [
        f"model: {type(pipe.named_steps['classifier']).__name__} trees={n_trees} "
        f"nodes={len(packed.cls_nodes)}  sample rows R={r}",
        f"device: {torch.cuda.get_device_name(0)}  repeats={args.repeats} "
        "(device events, one launch each incl. the job-table upload, after one warm-up)",
        f"what-if vs the CPU reference (8 jobs x {r} rows): max |err| = {err:.2e}",
        f"default request: 23 one-way curves at grid_resolution 20 = {n_default} jobs "
        f"= {n_default * r} pairs",
        "",
        f"{'launch':<40}{'median ms':>11}{'min ms':>10}{'max ms':>10}",
    ]

    def row(name: str, ms: list[float]) -> float:
        med = float(np.median(ms))
        lines.append(f"{name:<40}{med:>11.2f}{min(ms):>10.2f}{max(ms):>10.2f}")
        return med

    t_shap = row(f"forest_shap   B={cap}", timed(shap_launch))
    bound = NOISE * t_shap
    largest = max(1, ScoringEngine.PDP_LAUNCH_PAIRS // r)
    fits, t_largest = 0, None
    for pairs in sorted(set(SWEEP) | {largest * r, n_default * r}):
        n_jobs = pairs // r
        t = row(f"forest_whatif J={n_jobs} R={r} ({n_jobs * r} pairs)", timed(whatif_launch(n_jobs)))
        if t <= bound:
            fits = max(fits, n_jobs * r)
        if n_jobs == largest:
            t_largest = t
        if t > 4.0 * bound:
            lines.append("(sweep stopped: launch above 4 x the bound)")
            break
    lines += [
        "",
        f"rule: longest forest_whatif launch <= {NOISE} x forest_shap at its cap = {bound:.2f} ms",
        f"largest swept pair count within the rule at R={r}: {fits}",
    ]
    if t_largest is not None:
        lines.append(
            f"ScoringEngine.PDP_LAUNCH_PAIRS = {ScoringEngine.PDP_LAUNCH_PAIRS}: largest single "
            f"launch J={largest}, {t_largest:.2f} ms = {t_largest / t_shap:.2f} x forest_shap "
            f"-> {'within' if t_largest <= bound else 'OUTSIDE'} the rule"
        )

    # wall time of the default request, engine (GPU) vs scikit-learn brute
    t0 = time.perf_counter()
    got = eng.partial_dependence(list(FEATURES))
    t_eng = time.perf_counter() - t0
    lines += ["", f"default request, engine on the GPU, wall: {t_eng * 1e3:.1f} ms"]
    if not args.skip_sklearn:
        from sklearn.inspection import partial_dependence

        x_df = pd.DataFrame(np.asarray(drift.background, dtype=object), columns=FEATURES)
        for c in FEATURES[len(CATEGORICAL_FEATURES):]:
            x_df[c] = x_df[c].astype(np.float64)
        t0 = time.perf_counter()
        worst = 0.0
        for res in got["results"]:
            name, grid = res["features"][0], res["grid_values"][0]
            ref = partial_dependence(
                pipe, x_df, features=[name],
                custom_values={name: np.asarray(grid, dtype=object if isinstance(grid[0], str) else None)},
                categorical_features=CATEGORICAL_FEATURES, method="brute", kind="average",
                response_method="predict_proba",
            )
            worst = max(worst, float(np.abs(ref["average"][0] - res["average"]).max()))
        t_sk = time.perf_counter() - t0
        lines += [
            f"default request, scikit-learn partial_dependence(method='brute'), wall: "
            f"{t_sk * 1e3:.1f} ms  ({t_sk / t_eng:.1f} x the engine)",
            f"max |engine - scikit-learn| over the 23 curves: {worst:.2e}",
        ]
    assert len(all_one_way["results"]) == len(FEATURES)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())

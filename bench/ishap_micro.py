"""Launch-length micro-benchmark of /explain's two Shapley kernels on the
flagship forest (RF 500 trees x depth 16, trained and cached as bench.py
trains it).

    python bench/ishap_micro.py [--repeats N] [--out FILE]

Times single launches with device events (median of --repeats after one
warm-up launch per shape):

  forest_shap   at ScoringEngine.SHAP_MAX_ROWS rows — the launch length the
                project already accepts on a shared GPU;
  forest_ishap  with the packed 256-row background at B = 1, 64, a sweep of
                row counts, and the largest single launch the engine issues
                (ISHAP_MAX_PAIRS // 256 rows).

The rule that sizes ScoringEngine.ISHAP_MAX_PAIRS: the longest interventional
launch is no longer than 1.25 x the forest_shap launch at its cap (the 1.25
covers run-to-run noise; NOTES.md records +-15-20 % on short windows). The
script prints the largest swept row count that meets the rule and whether the
constant as committed meets it. No speed claim is made; needs a GPU."""

from __future__ import annotations

import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SWEEP = (1, 4, 8, 16, 24, 32, 48, 64, 128, 256, 512, 1024)
NOISE = 1.25


def _flagship():
    import bench
    from creditcore.data import make_uci_shaped_frame
    from creditcore.models.drift import TabularDriftDetector
    from creditcore.pack import encode_background
    from creditcore.schema import FEATURES
    from creditcore.train import BACKGROUND_ROWS

    packed, path = bench._build_packed(bench.bench_cache_dir())
    if packed.bg_codes is None:
        # a cache file written before the background sample existed: draw
        # the sample the trainer would have drawn from the same frame
        df = make_uci_shaped_frame(n_rows=bench.TRAIN_ROWS, seed=2024)
        det = TabularDriftDetector(df[FEATURES].values, background_rows=BACKGROUND_ROWS)
        packed.bg_codes, packed.bg_nums = encode_background(det.background, packed.vocabs)
    return packed, path


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        print("ishap_micro: no GPU; launch lengths are not measured", file=sys.stderr)
        return 2

    from creditcore.data import make_request_batch
    from creditcore.engine import ScoringEngine
    from creditcore.pack import build_shap_paths, encode_batch

    packed, path = _flagship()
    eng = ScoringEngine(packed, device="cuda", device_index=0)
    cap = ScoringEngine.SHAP_MAX_ROWS
    codes, nums = encode_batch(make_request_batch(cap, seed=11), packed.vocabs)
    r = len(packed.bg_codes)
    paths = build_shap_paths(packed)[0]

    # one engine call per method uploads the tables and checks the results
    shap = eng.explain_arrays(codes[:64], nums[:64], method="shap")
    ish = eng.explain_arrays(codes[:64], nums[:64], method="interventional")
    score = eng.score_arrays(codes[:64], nums[:64], with_drift=False)["predictions"]
    add = max(
        float(np.abs(shap["predictions"] - score).max()),
        float(np.abs(ish["predictions"] - score).max()),
    )

    ext, m, bg = eng._gpu["ext"], eng._shap_dev, eng._ishap_dev
    dev = torch.device("cuda", 0)
    kind, n_trees = int(packed.cls_kind), int(packed.cls_n_trees)

    def timed(fn, b: int) -> list[float]:
        c = torch.from_numpy(codes[:b]).to(dev)
        x = torch.from_numpy(nums[:b]).to(dev)
        fn(c, x)  # warm-up
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.repeats):
            t0 = torch.cuda.Event(enable_timing=True)
            t1 = torch.cuda.Event(enable_timing=True)
            t0.record()
            fn(c, x)
            t1.record()
            t1.synchronize()
            ms.append(t0.elapsed_time(t1))
        return ms

    def shap_launch(c, x):
        return ext.forest_shap(
            c, x, m["leaf_value"], m["leaf_off"], m["splits"], m["medians"], kind, n_trees
        )

    def ishap_launch(c, x):
        return ext.forest_ishap(
            c, x, bg[0], bg[1], m["leaf_value"], m["leaf_off"], m["splits"],
            m["medians"], kind, n_trees,
        )

    lines = [
        f"model: {os.path.basename(path)}  trees={n_trees} leaves={paths.n_leaves} "
        f"records={len(paths.splits)}",
        f"device: {torch.cuda.get_device_name(0)}  repeats={args.repeats} "
        "(device events, one launch each, after one warm-up launch)",
        f"additivity of both methods vs the scorer at 64 rows: max |err| = {add:.2e}",
        "",
        f"{'launch':<34}{'median ms':>11}{'min ms':>10}{'max ms':>10}",
    ]

    def row(name: str, ms: list[float]) -> float:
        med = float(np.median(ms))
        lines.append(f"{name:<34}{med:>11.2f}{min(ms):>10.2f}{max(ms):>10.2f}")
        return med

    t_shap = row(f"forest_shap  B={cap}", timed(shap_launch, cap))
    largest = max(1, min(cap, ScoringEngine.ISHAP_MAX_PAIRS // r))
    fits = 0
    t_largest = None
    for b in sorted(set(SWEEP) | {largest}):
        t = row(f"forest_ishap B={b} R={r}", timed(ishap_launch, b))
        if t <= NOISE * t_shap:
            fits = b
        if b == largest:
            t_largest = t
    lines += [
        "",
        f"rule: longest forest_ishap launch <= {NOISE} x forest_shap at its cap "
        f"= {NOISE * t_shap:.2f} ms",
        f"largest swept B within the rule at R={r}: {fits}  (= {fits * r} pairs)",
        f"ScoringEngine.ISHAP_MAX_PAIRS = {ScoringEngine.ISHAP_MAX_PAIRS}: largest single "
        f"launch B={largest}, {t_largest:.2f} ms = {t_largest / t_shap:.2f} x forest_shap "
        f"-> {'within' if t_largest <= NOISE * t_shap else 'OUTSIDE'} the rule",
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

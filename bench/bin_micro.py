"""Launch length of device binning, held against the forest_shap launch.

    python bench/bin_micro.py [--out profiles/bench_results/bin_micro.txt]

The launch-length rule of this project (creditcore/engine.py,
PDP_LAUNCH_PAIRS): no launch longer than 1.25 x the forest_shap launch at
ScoringEngine.SHAP_MAX_ROWS on the flagship forest, measured in the same run.
hgbt.BIN_LAUNCH_ROWS caps the rows of one binning launch. This script times,
with device events, everything bin_features_gpu enqueues for a 51-column
matrix of R rows in one slice: the key transpose, four count and four plan
launches (ext.bin_select) and the assign launch (ext.bin_assign). The sum of
those ten launches bounds the longest of them, so R fits when the sum does.
"""

from __future__ import annotations

import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ROWS = (16_384, 800_000, 1 << 21, 1 << 22)
NOISE = 1.25


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        print("bin_micro: no GPU; nothing is measured", file=sys.stderr)
        return 2

    from pdp_micro import _flagship
    from train_micro import _matrix

    from creditcore.engine import ScoringEngine
    from creditcore.models import hgbt
    from creditcore.pack import encode_batch
    from creditcore.data import make_uci_shaped_frame
    from creditcore.schema import FEATURES

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

    lines = [f"{'launches':<58}{'median ms':>11}{'min ms':>10}{'max ms':>10}"]

    def row(name: str, ms: list[float]) -> float:
        med = float(np.median(ms))
        lines.append(f"{name:<58}{med:>11.2f}{min(ms):>10.2f}{max(ms):>10.2f}")
        return med

    _, packed, _ = _flagship()
    cap = ScoringEngine.SHAP_MAX_ROWS
    codes, nums = encode_batch(make_uci_shaped_frame(n_rows=cap, seed=11)[FEATURES], packed.vocabs)
    eng = ScoringEngine(packed, device="cuda", device_index=0)
    eng.explain_arrays(codes[:64], nums[:64], method="shap")  # uploads the path table
    sh, ext = eng._shap_dev, eng._gpu["ext"]
    dev = torch.device("cuda", 0)
    c_dev, x_dev = torch.from_numpy(codes).to(dev), torch.from_numpy(nums).to(dev)
    t_shap = row(f"forest_shap B={cap}", timed(lambda: ext.forest_shap(
        c_dev, x_dev, sh["leaf_value"], sh["leaf_off"], sh["splits"], sh["medians"],
        int(packed.cls_kind), int(packed.cls_n_trees))))
    bound = NOISE * t_shap

    base, _ = _matrix(200_000, 2024)
    fits = 0
    for r in ROWS:
        x = torch.from_numpy(np.ascontiguousarray(np.resize(base, (r, base.shape[1])))).to(dev)
        f = x.shape[1]
        bins = torch.empty((f, r), dtype=torch.uint8, device=dev)
        keys, _ = ext.bin_select(x, 0, f, 256, r)
        table = torch.zeros((f, int(ext.BIN_SLOTS)), dtype=torch.int32, device=dev)
        table[:, 0] = 255  # the longest search: 255 edges (their values do not matter)
        t_sel = row(f"bin_select R={r} F={f} (1 keys + 4 count + 4 plan)",
                    timed(lambda: ext.bin_select(x, 0, f, 256, r)))
        t_asg = row(f"bin_assign R={r} F={f}", timed(lambda: ext.bin_assign(keys, table, bins, 0, r)))
        if t_sel + t_asg <= bound:
            fits = max(fits, r)
        del x, bins, keys
    lines += [
        "",
        f"bound: {NOISE} x forest_shap = {bound:.2f} ms; the ten binning launches of one "
        f"slice together stay within it up to R = {fits} rows (largest measured)",
        f"hgbt.BIN_LAUNCH_ROWS = {int(hgbt.BIN_LAUNCH_ROWS)}: "
        + ("within" if int(hgbt.BIN_LAUNCH_ROWS) <= fits else "OUTSIDE") + " the rule",
    ]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

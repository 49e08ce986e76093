"""Launch-length micro-benchmark of the SHAP interaction kernel on the
flagship forest (RF 500 trees x depth 16, trained and cached as bench.py
trains it; the model of bench/ishap_micro.py).

    python bench/shap_inter_micro.py [--repeats N] [--out FILE]

Times single launches with device events (median of --repeats after one
warm-up launch per shape), all in one run:

  forest_shap               at ScoringEngine.SHAP_MAX_ROWS rows — the launch
                            length the project already accepts on a shared GPU;
  forest_shap_interactions  at multiples of the kernel's rows per block up to
                            ScoringEngine.INTERACTION_MAX_ROWS.

The rule that sizes ScoringEngine.INTERACTION_LAUNCH_ROWS is the one of
ISHAP_MAX_PAIRS: the largest row count tried whose launch is no longer than
1.25 x the forest_shap launch at its cap (the 1.25 covers run-to-run noise).
The script prints that row count and whether the constant as committed meets
the rule. No speed claim is made; needs a GPU."""

from __future__ import annotations

import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "bench"))

NOISE = 1.25


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        print("shap_inter_micro: no GPU; launch lengths are not measured", file=sys.stderr)
        return 2

    from ishap_micro import _flagship

    from creditcore.data import make_request_batch
    from creditcore.engine import ScoringEngine
    from creditcore.pack import build_shap_paths, encode_batch

    packed, path = _flagship()
    eng = ScoringEngine(packed, device="cuda", device_index=0)
    cap = ScoringEngine.SHAP_MAX_ROWS
    codes, nums = encode_batch(make_request_batch(cap, seed=11), packed.vocabs)
    paths = build_shap_paths(packed)[0]
    ext = eng._gpu["ext"]
    rpb = int(ext.SHAP_INTER_ROWS_PER_BLOCK)
    sweep = list(range(rpb, ScoringEngine.INTERACTION_MAX_ROWS + 1, rpb))

    # one engine call uploads the table and checks the result
    out = eng.explain_arrays(codes[:rpb], nums[:rpb], method="shap", interactions=True)
    score = eng.score_arrays(codes[:rpb], nums[:rpb], with_drift=False)["predictions"]
    inter = out["interactions"]
    add = float(np.abs(out["base_value"] + inter.sum((1, 2)) - score).max())
    rows = float(np.abs(inter.sum(2) - out["contributions"]).max())

    m = eng._shap_dev
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

    def inter_launch(c, x):
        return ext.forest_shap_interactions(
            c, x, m["leaf_value"], m["leaf_off"], m["splits"], m["medians"], kind, n_trees
        )

    groups = np.bincount(
        np.repeat(np.arange(paths.n_leaves), np.diff(paths.leaf_off)),
        weights=((paths.splits[:, 3] & 2) != 0).astype(np.float64),
        minlength=paths.n_leaves,
    )
    lines = [
        f"model: {os.path.basename(path)}  trees={n_trees} leaves={paths.n_leaves} "
        f"records={len(paths.splits)}",
        f"players per path: mean {groups.mean():.2f} max {int(groups.max())}; "
        f"pairs per path: mean {(groups * (groups - 1) / 2).mean():.1f}",
        f"device: {torch.cuda.get_device_name(0)}  repeats={args.repeats} "
        "(device events, one launch each, after one warm-up launch)",
        f"at {rpb} rows: base + matrix sum vs the scorer max |err| = {add:.2e}, "
        f"row sums vs SHAP values max |err| = {rows:.2e}",
        "",
        f"{'launch':<38}{'median ms':>11}{'min ms':>10}{'max ms':>10}",
    ]

    def row(name: str, ms: list[float]) -> float:
        med = float(np.median(ms))
        lines.append(f"{name:<38}{med:>11.2f}{min(ms):>10.2f}{max(ms):>10.2f}")
        return med

    t_shap = row(f"forest_shap              B={cap}", timed(shap_launch, cap))
    committed = int(ScoringEngine.INTERACTION_LAUNCH_ROWS)
    fits = 0
    t_committed = None
    for b in sorted(set(sweep) | {committed}):
        t = row(f"forest_shap_interactions B={b}", timed(inter_launch, b))
        if t <= NOISE * t_shap:
            fits = b
        if b == committed:
            t_committed = t
    lines += [
        "",
        f"rule: longest forest_shap_interactions launch <= {NOISE} x forest_shap at "
        f"its cap = {NOISE * t_shap:.2f} ms",
        f"largest row count tried within the rule: {fits}",
        f"ScoringEngine.INTERACTION_LAUNCH_ROWS = {committed}: {t_committed:.2f} ms = "
        f"{t_committed / t_shap:.2f} x forest_shap -> "
        f"{'within' if t_committed <= NOISE * t_shap else 'OUTSIDE'} the rule",
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

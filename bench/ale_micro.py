"""Micro-benchmark of accumulated local effects (forest_ale_kernel) on the
flagship forest (RF 500 trees x depth 16, fitted as bench/pdp_micro.py fits
it): all 14 numeric features, grid_resolution 20.

    python bench/ale_micro.py [--repeats N] [--out FILE]

Times, with device events for single launches (median of --repeats after one
warm-up launch per shape) and a host clock around whole engine calls:

  forest_shap  at ScoringEngine.SHAP_MAX_ROWS rows, the launch length the
               project already accepts on a shared GPU;
  forest_ale   one launch of all 14 entries at 256, 1024, 16384, 32768 and
               65536 rows (the call cap), and the engine call at 256, 1024
               and 65536 rows;
  the same curves at 1024 rows (PDP's cap) through
               partial_dependence(kind="both", grid=edges), with a check that
               each row's two ICE columns give the ALE local effects bit for
               bit;
  the numpy reference (device="cpu") at 256 rows.

The rule that sizes ScoringEngine.ALE_LAUNCH_JOBS (the rule of
PDP_LAUNCH_PAIRS): the longest forest_ale launch is no longer than 1.25 x the
forest_shap launch at its cap. The script prints the largest measured
(row, entry) pair count that meets it. Needs a GPU."""

from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "bench"))

LAUNCH_ROWS = (256, 1024, 16384, 32768, 65536)
ENGINE_ROWS = (256, 1024, 65536)
NOISE = 1.25
K = 20


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        print("ale_micro: no GPU; nothing is measured", file=sys.stderr)
        return 2

    from pdp_micro import _flagship

    from creditcore import ale
    from creditcore.data import make_request_batch
    from creditcore.engine import ScoringEngine
    from creditcore.ops import cpu_ref
    from creditcore.pack import N_CAT, encode_batch
    from creditcore.schema import NUMERIC_FEATURES

    pipe, packed, _ = _flagship()
    names = list(NUMERIC_FEATURES)
    eng = ScoringEngine(packed, device="cuda", device_index=0)
    cpu = ScoringEngine(packed, device="cpu")
    dev = torch.device("cuda", 0)
    n_trees = int(packed.cls_n_trees)
    codes, nums = encode_batch(make_request_batch(max(LAUNCH_ROWS), seed=11), packed.vocabs)

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

    def wall(fn):
        fn()  # warm-up: uploads, code objects
        t0 = time.perf_counter()
        out = fn()  # ends in a device-to-host copy, which synchronizes
        return out, (time.perf_counter() - t0) * 1e3

    lines = [
        f"model: {type(pipe.named_steps['classifier']).__name__} trees={n_trees} "
        f"nodes={len(packed.cls_nodes)}  entries: the {len(names)} numeric features, "
        f"grid_resolution {K}",
        f"device: {torch.cuda.get_device_name(0)}  repeats={args.repeats} (device events, one "
        "launch each incl. the edge-table upload, after one warm-up)",
        "",
        f"{'launch':<52}{'median ms':>11}{'min ms':>10}{'max ms':>10}",
    ]

    def row(name: str, ms: list[float]) -> float:
        med = float(np.median(ms))
        lines.append(f"{name:<52}{med:>11.2f}{min(ms):>10.2f}{max(ms):>10.2f}")
        return med

    cap = ScoringEngine.SHAP_MAX_ROWS
    eng.explain_arrays(codes[:64], nums[:64], method="shap")  # uploads the path table
    eng.accumulated_local_effects(names[:1])  # uploads the forest tables
    sh, m, ext = eng._shap_dev, eng._explain_dev, eng._gpu["ext"]
    c_dev, x_dev = torch.from_numpy(codes).to(dev), torch.from_numpy(nums).to(dev)
    t_shap = row(
        f"forest_shap B={cap}",
        timed(lambda: ext.forest_shap(
            c_dev[:cap], x_dev[:cap], sh["leaf_value"], sh["leaf_off"], sh["splits"],
            sh["medians"], int(packed.cls_kind), n_trees,
        )),
    )
    bound = NOISE * t_shap
    fits = 0
    for r in LAUNCH_ROWS:
        imp = cpu_ref.impute_nums(packed, nums[:r])
        edges = [ale.quantile_edges(imp[:, j], K) for j in range(len(names))]
        keep = [j for j, z in enumerate(edges) if len(z) > 1]
        off, z = ale.edge_table([edges[j] for j in keep])
        tabs = [torch.from_numpy(a) for a in (np.array([N_CAT + j for j in keep], np.int32), off, z)]
        t = row(
            f"forest_ale E={len(keep)} R={r} ({len(keep) * r} pairs)",
            timed(lambda: ext.forest_ale(
                c_dev[:r], x_dev[:r], m["cls_nodes"], m["cls_off"], m["feat_col"],
                m["feat_code"], m["medians"], *tabs,
            )),
        )
        if t <= bound:
            fits = max(fits, len(keep) * r)
    lines += [
        "",
        f"rule: longest forest_ale launch <= {NOISE} x forest_shap at its cap = {bound:.2f} ms",
        f"largest measured pair count within the rule: {fits} "
        f"(ScoringEngine.ALE_LAUNCH_JOBS = {ScoringEngine.ALE_LAUNCH_JOBS}; the caps allow "
        f"{ale.ALE_MAX_ROWS * ale.ALE_MAX_ENTRIES})",
        "",
        "whole calls, wall ms (host clock, second call):",
    ]
    for r in ENGINE_ROWS:
        smp = (codes[:r], nums[:r])
        got, t = wall(lambda: eng.accumulated_local_effects(names, sample=smp, kind="both"))
        lines.append(f"  accumulated_local_effects R={r} on the GPU: {t:.1f}")
        if r == 1024:
            grids = {res["feature"]: res["edges"] for res in got["results"]}
            ice, t_pdp = wall(lambda: eng.partial_dependence(
                names, sample=smp, kind="both", grid=grids))
            same = True
            for res, tab in zip(got["results"], ice["results"]):
                k, rows = res["interval"], np.arange(r)
                d = tab["individual"][rows, k] - tab["individual"][rows, k - 1]
                same &= bool(np.array_equal(d, res["local_effect"]))
            jobs = sum(len(g) for g in grids.values())
            lines.append(
                f"  the same curves through partial_dependence(kind='both', grid=edges) R={r} "
                f"({jobs} what-if jobs): {t_pdp:.1f}  ({t_pdp / t:.2f} x the ALE call); "
                f"local effects bit for bit: {same}"
            )
        if r == 256:
            ref, t_cpu = wall(lambda: cpu.accumulated_local_effects(names, sample=smp, kind="both"))
            same = all(
                np.array_equal(a["ale"], b["ale"]) and np.array_equal(a["interval"], b["interval"])
                for a, b in zip(got["results"], ref["results"])
            )
            lines.append(
                f"  numpy reference (device='cpu') R={r}: {t_cpu:.1f}  "
                f"({t_cpu / t:.1f} x the GPU call); curves bit for bit: {same}"
            )
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())

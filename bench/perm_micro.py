"""Micro-benchmark of permutation importance (forest_permute_kernel) on the
flagship forest (RF 500 trees x depth 16, fitted as bench/pdp_micro.py fits
it): all 23 features, 5 repeats, and on a boosted model (hgbt 500 x depth 6).

    python bench/perm_micro.py [--repeats N] [--out FILE] [--skip-sklearn]

Times, with device events around single launches (median of --repeats after
one warm-up launch per shape; a launch includes the launcher's host-side check
and upload of its tables) and a host clock around whole engine calls:

  forest_shap     at ScoringEngine.SHAP_MAX_ROWS rows, the launch length the
                  project already accepts on a shared GPU;
  forest_permute  all 115 table rows at 256, 16384 and 65536 sample rows, and
                  whole features (5 table rows each) at 65536 rows, for the
                  slicing constant;
  forest_whatif   at the same (job, row) pair count: one constant per job
                  instead of one donor per row;
  forest_permute  "ungrouped": the same table in repeat-major order, so that
                  no two adjacent rows share a player and every job holds one
                  repeat. Same sums, no shared base walk: the ratio is what
                  the sharing saves;
  the engine call (roc_auc) at the three sizes, and
  sklearn.inspection.permutation_importance(n_jobs=16) on the same pipeline at
  256 rows.

The rule that sizes ScoringEngine.PERM_LAUNCH_PAIRS (the rule of
PDP_LAUNCH_PAIRS): the longest forest_permute launch is no longer than 1.25 x
the forest_shap launch at its cap. The script prints the largest measured
(table row, sample row) pair count that meets it. Needs a GPU."""

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

ROWS = (256, 16384, 65536)
FEATURE_STEPS = (4, 8, 12, 16)  # whole features per launch at the row cap
BOOSTED_ROWS = 16384
REPS = 5
NOISE = 1.25


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--skip-sklearn", action="store_true")
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        print("perm_micro: no GPU; nothing is measured", file=sys.stderr)
        return 2

    from pdp_micro import _flagship

    from creditcore.data import make_uci_shaped_frame
    from creditcore.engine import ScoringEngine
    from creditcore.models.forest import make_classifier_pipeline
    from creditcore.pack import N_CAT, N_NUM, encode_batch, pack_classifier_pipeline
    from creditcore.schema import FEATURES, TARGET

    n_src = N_CAT + N_NUM
    pipe, packed, _ = _flagship()
    frame = make_uci_shaped_frame(n_rows=max(ROWS), seed=11)
    labels = frame[TARGET].to_numpy()
    codes, nums = encode_batch(frame[FEATURES], packed.vocabs)
    dev = torch.device("cuda", 0)
    c_dev, x_dev = torch.from_numpy(codes).to(dev), torch.from_numpy(nums).to(dev)
    rng = np.random.default_rng(0)

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

    lines = []

    def row(name: str, ms: list[float]) -> float:
        med = float(np.median(ms))
        lines.append(f"{name:<58}{med:>11.2f}{min(ms):>10.2f}{max(ms):>10.2f}")
        return med

    def tables(r: int, n_feat: int):
        """(perm_player, perm) feature-major, the same repeat-major, and the
        what-if jobs of as many (job, row) pairs."""
        feats = (np.arange(n_feat) * n_src // n_feat).astype(np.int32)  # spread over both kinds
        players = np.repeat(feats, REPS)
        perm = np.stack([rng.permutation(r) for _ in players]).astype(np.int32)
        order = np.arange(len(players)).reshape(n_feat, REPS).T.reshape(-1)
        jobs = np.zeros((len(players), 4), dtype=np.int32)
        jobs[:, 0], jobs[:, 2] = players, -1
        jobs[players >= N_CAT, 1] = packed.medians[players[players >= N_CAT] - N_CAT].view(np.int32)
        return [torch.from_numpy(np.ascontiguousarray(a)) for a in
                (players, perm, players[order], perm[order], jobs)]

    def launches(m, ext, r: int, n_feat: int, what: tuple) -> dict:
        pl, pm, pl_u, pm_u, jobs = tables(r, n_feat)
        model = (m["cls_nodes"], m["cls_off"], m["feat_col"], m["feat_code"], m["medians"])
        tag, out = f"Q={len(pl)} R={r} ({len(pl) * r} pairs)", {}
        if "permute" in what:
            out["permute"] = row(f"forest_permute {tag}", timed(
                lambda: ext.forest_permute(c_dev[:r], x_dev[:r], *model, pl, pm)))
        if "ungrouped" in what:
            out["ungrouped"] = row(f"forest_permute ungrouped {tag}", timed(
                lambda: ext.forest_permute(c_dev[:r], x_dev[:r], *model, pl_u, pm_u)))
        if "whatif" in what:
            out["whatif"] = row(f"forest_whatif J={len(pl)} R={r}", timed(
                lambda: ext.forest_whatif(c_dev[:r], x_dev[:r], *model, jobs)))
        return out

    eng = ScoringEngine(packed, device="cuda", device_index=0)
    cap = ScoringEngine.SHAP_MAX_ROWS
    eng.explain_arrays(codes[:64], nums[:64], method="shap")  # uploads the path table
    eng.permutation_importance((codes[:64], nums[:64]), labels[:64], scoring="accuracy")
    sh, m, ext = eng._shap_dev, eng._explain_dev, eng._gpu["ext"]
    lines += [
        f"model: {type(pipe.named_steps['classifier']).__name__} "
        f"trees={int(packed.cls_n_trees)} nodes={len(packed.cls_nodes)}  table: the {n_src} "
        f"features x {REPS} repeats, jobs of up to {ext.PERM_ILP} repeats",
        f"device: {torch.cuda.get_device_name(0)}  repeats={args.repeats} (device events around "
        "one launch each, incl. the launcher's table check and upload, after one warm-up)",
        "",
        f"{'launch':<58}{'median ms':>11}{'min ms':>10}{'max ms':>10}",
    ]
    t_shap = row(
        f"forest_shap B={cap}",
        timed(lambda: ext.forest_shap(
            c_dev[:cap], x_dev[:cap], sh["leaf_value"], sh["leaf_off"], sh["splits"],
            sh["medians"], int(packed.cls_kind), int(packed.cls_n_trees),
        )),
    )
    bound, fits, notes = NOISE * t_shap, 0, []
    for r in ROWS:
        t = launches(m, ext, r, n_src, ("permute", "ungrouped", "whatif"))
        notes.append(
            f"  R={r}: forest_permute / forest_whatif per pair {t['permute'] / t['whatif']:.2f}, "
            f"grouped / ungrouped {t['permute'] / t['ungrouped']:.2f}"
        )
        if t["permute"] <= bound:
            fits = max(fits, n_src * REPS * r)
    for f in FEATURE_STEPS:
        if launches(m, ext, max(ROWS), f, ("permute",))["permute"] <= bound:
            fits = max(fits, f * REPS * max(ROWS))
    lines += [
        "",
        f"rule: longest forest_permute launch <= {NOISE} x forest_shap at its cap = {bound:.2f} ms",
        f"largest measured pair count within the rule: {fits} "
        f"(ScoringEngine.PERM_LAUNCH_PAIRS = {ScoringEngine.PERM_LAUNCH_PAIRS})",
        "per pair, flagship forest:",
        *notes,
        "",
        "whole calls, wall ms (host clock, second call):",
    ]
    for r in ROWS:
        smp = (codes[:r], nums[:r])
        _, t = wall(lambda: eng.permutation_importance(smp, labels[:r], n_repeats=REPS))
        lines.append(f"  permutation_importance R={r} (roc_auc, {n_src} features) on the GPU: {t:.1f}")
    if not args.skip_sklearn:
        from sklearn.inspection import permutation_importance

        r = ROWS[0]
        t0 = time.perf_counter()
        permutation_importance(pipe, frame[FEATURES][:r], labels[:r], scoring="roc_auc",
                               n_repeats=REPS, random_state=0, n_jobs=16)
        lines.append(
            f"  sklearn.inspection.permutation_importance(n_jobs=16) R={r}: "
            f"{(time.perf_counter() - t0) * 1e3:.1f}"
        )

    # a boosted model: shallow trees, where a whole wave often never meets the column
    train = make_uci_shaped_frame(n_rows=20_000, seed=2024)
    gbt = make_classifier_pipeline(
        {"n_estimators": 500, "max_depth": 6, "random_state": 2024}, "hgbt")
    gbt.fit(train[FEATURES], train[TARGET].values.ravel())
    boosted = dataclasses.replace(packed, **pack_classifier_pipeline(gbt))
    eng_b = ScoringEngine(boosted, device="cuda", device_index=0)
    eng_b.permutation_importance((codes[:64], nums[:64]), labels[:64], scoring="accuracy")
    lines += ["", f"boosted model: hgbt trees={int(boosted.cls_n_trees)} "
              f"nodes={len(boosted.cls_nodes)}",
              f"{'launch':<58}{'median ms':>11}{'min ms':>10}{'max ms':>10}"]
    t = launches(eng_b._explain_dev, ext, BOOSTED_ROWS, n_src, ("permute", "ungrouped", "whatif"))
    lines.append(
        f"  forest_permute / forest_whatif per pair {t['permute'] / t['whatif']:.2f}, "
        f"grouped / ungrouped {t['permute'] / t['ungrouped']:.2f}"
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

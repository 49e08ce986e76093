"""Micro-benchmark of anchor rules (forest_anchor_kernel) on the flagship
forest (RF 500 x depth 16) and on a boosted model (hgbt 500 x depth 6), on the
packed 256-row background sample at ScoringEngine.anchors' defaults.

    python bench/anchor_micro.py --out profiles/bench_results/anchor_micro.txt

Per model and row count (1 / 64 / 1024 rows):

  engine    every search level as the engine launches it: one forest_anchor
            launch for all rows still searching, the launcher's own chunk
            (small jobs while the launch has few masks)
  chunk 64  the same launch with jobs of up to 64 masks of one row, all
            served by one walk of each tree
  chunk 1   the same launch with one mask per job, i.e. no sharing
  wall      the whole ScoringEngine.anchors call (host clock, second call)

and, for the rule that sizes ScoringEngine.ANCHOR_LAUNCH_PAIRS (the rule of
PDP_LAUNCH_PAIRS): level-1 launches (23 masks per row) at growing row counts
against 1.25 x the forest_shap launch at SHAP_MAX_ROWS measured in the same
run. No speed-up is claimed here; the file reports what was measured.
"""

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

ROWS = (1, 64, 1024)
RULE_ROWS = (16, 64, 128, 192, 256, 512, 1024)
NOISE = 1.25


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        print("anchor_micro: no GPU; nothing is measured", file=sys.stderr)
        return 2

    from pdp_micro import _flagship

    from creditcore import anchors as an
    from creditcore.counterfactual import raw_cut
    from creditcore.data import make_uci_shaped_frame
    from creditcore.engine import ScoringEngine
    from creditcore.models.forest import make_classifier_pipeline
    from creditcore.ops import cpu_ref
    from creditcore.pack import N_CAT, N_NUM, encode_batch, pack_classifier_pipeline
    from creditcore.schema import FEATURES, TARGET

    n_src = N_CAT + N_NUM
    pipe, packed, _ = _flagship()
    frame = make_uci_shaped_frame(n_rows=max(ROWS), seed=11)
    codes, nums = encode_batch(frame[FEATURES], packed.vocabs)
    dev = torch.device("cuda", 0)

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

    lines = []

    def row(name: str, ms: list[float]) -> float:
        med = float(np.median(ms))
        lines.append(f"{name:<62}{med:>11.2f}{min(ms):>10.2f}{max(ms):>10.2f}")
        return med

    def levels(eng, p, r: int):
        """The search of r rows at the defaults, level by level: per level
        the launch time shared and unshared."""
        ext, m = eng._gpu["ext"], eng._explain_dev
        model = (m["cls_nodes"], m["cls_off"], m["feat_col"], m["feat_code"], m["medians"])
        c, x = codes[:r], nums[:r]
        imp, bg_imp = cpu_ref.impute_nums(p, x), cpu_ref.impute_nums(p, p.bg_nums)
        sat = an.sat_table(c, imp, p.bg_codes, bg_imp, an.disc_edges(bg_imp, np.array([25.0, 50.0, 75.0])))
        cut = raw_cut(p, 0.5)
        s = len(bg_imp)
        up = [torch.from_numpy(np.ascontiguousarray(a)).to(dev)
              for a in (c, x, p.bg_codes, p.bg_nums, sat.view(np.int32))]
        level, total = [0], [0.0, 0.0, 0.0]

        def run(masks, mask_off):
            mk = torch.from_numpy(masks.view(np.int32))
            mo = torch.from_numpy(mask_off)

            def launch(chunk):
                return ext.forest_anchor(
                    up[0], up[1], up[2], up[3], *model, up[4], mk, mo, cut, False, chunk)

            tag = f"R={r} level {level[0]}: {len(masks)} masks x {s} = {len(masks) * s} pairs"
            for k, (name, chunk) in enumerate((("engine  ", 0), ("chunk 64", 64), ("chunk 1 ", 1))):
                total[k] += row(f"{name} {tag}", timed(lambda: launch(chunk)))
            level[0] += 1
            got, same = launch(0)[0].cpu().numpy(), launch(1)[0].cpu().numpy()
            assert (got == same).all(), "shared and unshared counts differ"
            return got

        own = cpu_ref.forest_raw_cpu(p, c, imp, tree_order=True) > cut
        found = an.search(run, sat, own, 0.95, 2, 6)
        met = sum(f[3] for f in found)
        return total, f"{met} of {r} rows met 0.95, mean size {np.mean([bin(f[0]).count('1') for f in found]):.2f}"

    def wall(eng, r: int) -> float:
        eng.anchors(codes[:r], nums[:r])  # warm-up: uploads, code objects
        t0 = time.perf_counter()
        eng.anchors(codes[:r], nums[:r])
        return (time.perf_counter() - t0) * 1e3

    def model_block(eng, p, rows):
        notes = []
        for r in rows:
            (a, b, c), found = levels(eng, p, r)
            notes.append(f"  R={r}: launches engine {a:.2f} ms, chunk 64 {b:.2f} ms, chunk 1 {c:.2f} ms, "
                         f"chunk 1 / engine {c / a:.2f}; anchors() wall {wall(eng, r):.1f} ms; {found}")
        return notes

    head = f"{'launch':<62}{'median ms':>11}{'min ms':>10}{'max ms':>10}"
    eng = ScoringEngine(packed, device="cuda", device_index=0)
    cap = ScoringEngine.SHAP_MAX_ROWS
    eng.explain_arrays(codes[:64], nums[:64], method="shap")  # uploads the path table
    eng.anchors(codes[:2], nums[:2])
    sh, ext = eng._shap_dev, eng._gpu["ext"]
    c_dev, x_dev = torch.from_numpy(codes).to(dev), torch.from_numpy(nums).to(dev)
    lines += [
        f"model: {type(pipe.named_steps['classifier']).__name__} "
        f"trees={int(packed.cls_n_trees)} nodes={len(packed.cls_nodes)}  sample: "
        f"{len(packed.bg_codes)} rows, defaults (0.95, beam 2, size 6, quartiles)",
        f"device: {torch.cuda.get_device_name(0)}  repeats={args.repeats} (device events around "
        "one launch each, incl. the launcher's table check and upload, after one warm-up)",
        "",
        head,
    ]
    t_shap = row(
        f"forest_shap B={cap}",
        timed(lambda: ext.forest_shap(
            c_dev[:cap], x_dev[:cap], sh["leaf_value"], sh["leaf_off"], sh["splits"],
            sh["medians"], int(packed.cls_kind), int(packed.cls_n_trees),
        )),
    )
    bound, fits = NOISE * t_shap, 0
    m = eng._explain_dev
    model = (m["cls_nodes"], m["cls_off"], m["feat_col"], m["feat_code"], m["medians"])
    s = len(packed.bg_codes)
    bg = [torch.from_numpy(a).to(dev) for a in (packed.bg_codes, packed.bg_nums)]
    singles = np.array([1 << pl for pl in range(n_src)], dtype=np.uint32)
    for r in RULE_ROWS:
        sat0 = torch.zeros((r, s), dtype=torch.int32, device=dev)  # nothing satisfied: most splits
        mk = torch.from_numpy(np.tile(singles, r).view(np.int32))
        off = torch.from_numpy((n_src * np.arange(r + 1)).astype(np.int32))
        t = row(f"forest_anchor level 1, R={r}: {r * n_src} masks x {s} = {r * n_src * s} pairs",
                timed(lambda: ext.forest_anchor(c_dev[:r], x_dev[:r], *bg, *model, sat0, mk, off, 0.0)))
        if t <= bound:
            fits = max(fits, r * n_src * s)
    lines += [
        "",
        f"rule: longest forest_anchor launch <= {NOISE} x forest_shap at its cap = {bound:.2f} ms",
        f"largest measured pair count within the rule: {fits} "
        f"(ScoringEngine.ANCHOR_LAUNCH_PAIRS = {ScoringEngine.ANCHOR_LAUNCH_PAIRS})",
        "",
        head,
    ]
    notes = model_block(eng, packed, ROWS)
    lines += ["", "per call, flagship forest:", *notes]

    train = make_uci_shaped_frame(n_rows=20_000, seed=2024)
    gbt = make_classifier_pipeline(
        {"n_estimators": 500, "max_depth": 6, "random_state": 2024}, "hgbt")
    gbt.fit(train[FEATURES], train[TARGET].values.ravel())
    boosted = dataclasses.replace(packed, **pack_classifier_pipeline(gbt))
    eng_b = ScoringEngine(boosted, device="cuda", device_index=0)
    eng_b.anchors(codes[:2], nums[:2])
    lines += ["", f"boosted model: hgbt trees={int(boosted.cls_n_trees)} "
              f"nodes={len(boosted.cls_nodes)}", head]
    notes = model_block(eng_b, boosted, ROWS)
    lines += ["", "per call, boosted model:", *notes]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Scoring engine — one model replica on one device.

The GPU path holds a C++ ScoreSession (csrc/creditcore_kernels.hip):
resident HBM model buffers, two private HIP streams, double-buffered pinned
staging, and one hipGraph per recurring request shape. A request is:

    host:   native JSON parse -> codes (int16), nums (f32)   [C, GIL-free]
    graph:  pinned H2D -> 2-tree-ILP forest kernels (classifier + isolation
            forest) -> finalize (re-zeros its accumulator rows) -> outs D2H,
            ∥ drift branch on stream 2 (categorical histogram + K-S) ->
            one packed drift D2H; no memset nodes
    host:   drift p-values (C: chi2 closed forms + MTW/Pelz-Good K-S sf)
            -> response JSON bytes (C, shortest-round-trip doubles)

Entry points by use: score_json_full (single C++ call, lowest latency),
submit_encoded_slot/finish_slot (double-buffered pipelining: step i's
epilogue overlaps step i+1's graph), score_arrays (array in/out for the
micro-batcher), score_records/score_json (dict/response-shaped outputs).

The CPU path (device="cpu") uses the same packed buffers via
creditcore.ops.cpu_ref — identical numerics (the HIP kernels are tested
against it). On a machine with a GPU the engine REFUSES to silently fall back
to CPU: the HIP extension must be present (ops/gpu.py).
"""

from __future__ import annotations

import threading
import time

import numpy as np

from .ops import cpu_ref
from .pack import N_CAT, N_NUM, PackedModel, encode_batch
from .schema import FEATURES


class ExplainUnavailable(RuntimeError):
    """The model was packed without per-node expected values
    (PackedModel.cls_node_value is None), so attributions cannot be computed."""


class ExplainTooLarge(ValueError):
    """An explain call exceeded ScoringEngine.EXPLAIN_MAX_ROWS."""


def _check_forest_tables(p: PackedModel) -> None:
    """Host-side bounds check of everything forest_contrib_kernel and
    forest_whatif_kernel index with model data (the kernels trust their
    tables): node features, child links, the one-hot/numeric source columns
    and, where the model carries one, the value array length."""
    nodes, off = p.cls_nodes, p.cls_tree_offsets
    n_feat = len(p.feat_col)
    ok = (
        nodes.ndim == 2
        and nodes.shape[1] == 4
        and (p.cls_node_value is None or len(p.cls_node_value) == len(nodes))
        and len(p.feat_code) == n_feat
        and len(p.medians) == N_NUM
        and len(off) >= 2
        and off[0] == 0
        and off[-1] == len(nodes)
        and bool((np.diff(off) > 0).all())
    )
    if ok:
        feat = nodes[:, 0]
        split = feat >= 0
        size = np.repeat(np.diff(off), np.diff(off))  # own tree's node count
        local = np.arange(len(nodes)) - np.repeat(off[:-1], np.diff(off))
        cat = p.feat_code >= 0
        ok = (
            bool((feat < n_feat).all())
            # BFS order: children come after their parent, so walks terminate
            and bool((nodes[split, 2:] > local[split, None]).all())
            and bool((nodes[split, 2:] < size[split, None]).all())
            and bool((p.feat_col >= 0).all())
            and bool((p.feat_col[cat] < N_CAT).all())
            and bool((p.feat_col[~cat] < N_NUM).all())
        )
    if not ok:
        raise ValueError("packed classifier forest is malformed; refusing to explain")


def _check_shap_paths(paths, n_players: int = N_CAT + N_NUM) -> None:
    """Host-side bounds check of everything forest_shap_kernel indexes with
    path-table data before the first upload: leaf offsets into the split
    records, the player (source column) of every record, at most 23 player
    groups per leaf (the kernel's LDS tables), and fractions in [0, 1]."""
    from .pack import SHAP_CODE_SHIFT, SHAP_FIRST, SHAP_PLAYER_SHIFT

    lv, off, sp = paths.leaf_value, paths.leaf_off, paths.splits
    ok = (
        lv.ndim == 1
        and lv.dtype == np.float32
        and off.dtype == np.int32
        and off.shape == (len(lv) + 1,)
        and sp.dtype == np.int32
        and sp.ndim == 2
        and sp.shape[1] == 4
        and off[0] == 0
        and off[-1] == len(sp)
        and bool((np.diff(off) >= 0).all())
        and bool(np.isfinite(lv).all())
    )
    if ok and len(sp):
        flags = sp[:, 3].view(np.uint32).astype(np.int64)
        player = (flags >> SHAP_PLAYER_SHIFT) & 0xFF
        numeric = (flags >> SHAP_CODE_SHIFT) == 0
        first = (flags & SHAP_FIRST) != 0
        frac = sp[:, 2].view(np.float32)
        starts = off[:-1][np.diff(off) > 0]
        rec_leaf = np.repeat(np.arange(len(lv)), np.diff(off))
        groups = np.bincount(rec_leaf[first], minlength=len(lv))
        ok = (
            bool((player < n_players).all())
            and bool((player[numeric] >= N_CAT).all())
            and bool((player[~numeric] < N_CAT).all())
            and bool(first[starts].all())  # every leaf's run opens a group
            and int(groups.max()) <= n_players
            and bool(((frac >= 0.0) & (frac <= 1.0)).all())
            and bool(np.isfinite(sp[:, 1].view(np.float32)).all())
        )
    if not ok:
        raise ValueError("SHAP path table is malformed; refusing to explain")


EXPLAIN_METHODS = ("saabas", "shap", "interventional")


class ScoringEngine:
    # K-S kernel LDS sort capacity (csrc MAX_DRIFT_ROWS) — the hardware
    # ceiling; the per-engine cap (config drift_max_batch) can only lower it
    HW_DRIFT_MAX_ROWS = 16384
    # per-call row cap of explain_arrays / explain_records / POST /explain
    EXPLAIN_MAX_ROWS = 16384
    # per-call row cap of method="shap": the cost is rows x leaves of the
    # forest (every path, not one per tree), and one launch has to stay
    # short on a shared GPU
    SHAP_MAX_ROWS = 1024
    # method="interventional" (row cap: SHAP_MAX_ROWS): most background rows
    # one call takes (the kernel's LDS mask capacity, csrc
    # ISHAP_MAX_BACKGROUND) ...
    ISHAP_MAX_BACKGROUND = 1024
    # ... and most (explained row, background row) pairs of one launch; a
    # call above it runs as several launches over row slices. Sized on the
    # flagship forest (RF 500 x depth 16, 1.08 M leaves) with the default
    # 256-row sample so that the longest interventional launch is no longer
    # than 1.25 x the method="shap" launch at SHAP_MAX_ROWS, the launch
    # length already accepted on a shared GPU: forest_shap at 1024 rows
    # 60.5 ms, forest_ishap at 16 rows x 256 = 4096 pairs 72.5 ms (24 rows:
    # 80.9 ms, over the 75.6 ms bound) on an MI355X,
    # profiles/bench_results/ishap_micro.txt. A larger background override
    # lengthens even a one-row launch (its floor grows with R).
    ISHAP_MAX_PAIRS = 4096
    # method="shap" with interactions=True: per-call row cap (a row of the
    # result is a 23 x 23 matrix, 529 numbers) ...
    INTERACTION_MAX_ROWS = 128
    # ... and most rows of one forest_shap_interactions launch; a call above
    # it runs as several launches over row slices. Sized like ISHAP_MAX_PAIRS:
    # the largest multiple of the kernel's rows per block (16), up to the
    # call cap, whose launch on the flagship forest is no longer than 1.25 x
    # the method="shap" launch at SHAP_MAX_ROWS measured in the same run:
    # forest_shap at 1024 rows 60.17 ms (bound 75.21 ms),
    # forest_shap_interactions at 128 rows 51.99 ms on an MI355X,
    # profiles/bench_results/shap_inter_micro.txt. Every row count up to the
    # call cap is within the bound, so today no call is sliced.
    INTERACTION_LAUNCH_ROWS = 128
    # partial_dependence: most (job, row) pairs of one forest_whatif launch
    # (a job is one grid point's column override, a pair one walk of the
    # whole forest); a call above it runs as several launches over job
    # slices. Sized like ISHAP_MAX_PAIRS: the largest measured pair count
    # whose launch on the flagship forest (RF 500 x depth 16) with the
    # 256-row sample is no longer than 1.25 x the method="shap" launch at
    # SHAP_MAX_ROWS measured in the same run: forest_shap at 1024 rows
    # 60.34 ms (bound 75.43 ms), forest_whatif at 8192 jobs x 256 rows =
    # 2,097,152 pairs 23.80 ms on an MI355X (the largest shape measured; the
    # default request, 81,152 pairs, 3.46 ms),
    # profiles/bench_results/pdp_micro.txt. The largest call the caps allow
    # (10.7 M pairs) runs as six launches.
    PDP_LAUNCH_PAIRS = 2097152
    # counterfactuals: most {row, numeric column} jobs of one forest_sweep
    # launch; a call above it runs as several launches over job slices. Held
    # against the method="shap" launch at SHAP_MAX_ROWS measured in the same
    # run, which a sweep launch may not exceed: forest_shap at 1024 rows
    # 60.35 ms, forest_sweep at 4096 jobs 16.28 ms on an MI355X with the
    # flagship forest (RF 500 x depth 16, 51k-62k thresholds per column;
    # bench/cf_micro.py, profiles/bench_results/cf_micro.txt). A launch holds
    # its jobs' curves on the device (8 B per interval: 1.7 GB at that
    # shape). The largest call the caps allow (1024 rows x 14 columns =
    # 14,336 jobs) runs as four launches.
    CF_LAUNCH_JOBS = 4096

    def __init__(
        self,
        packed: PackedModel,
        device: str = "cpu",
        device_index: int = 0,
        drift_max_rows: int | None = None,
    ):
        self.packed = packed
        self.device = device
        self.device_index = device_index
        self.n_features = N_CAT + N_NUM
        self.DRIFT_MAX_ROWS = min(
            drift_max_rows or self.HW_DRIFT_MAX_ROWS, self.HW_DRIFT_MAX_ROWS
        )
        self._gpu = None
        self._explain_lock = threading.Lock()
        self._explain_dev = None  # lazily uploaded device tensors (explain)
        self._shap = None  # lazily built (paths, base value) of method="shap"
        self._shap_dev = None  # lazily uploaded path table
        # method="interventional": lazily imputed packed background sample,
        # its base value, and its device copy
        self._ishap = None
        self._ishap_dev = None
        self._pdp_sample_dev = None  # partial_dependence: the packed sample
        # counterfactuals: lazily derived breakpoint tables, their device copy
        self._cf = None
        self._cf_dev = None
        if device == "cuda":
            self._init_gpu()

    # ------------------------------------------------------------------ GPU

    def _init_gpu(self, capacity: int = 16384):
        import torch

        from .ops import gpu

        ext = gpu.ext()  # raises loudly if the HIP extension is missing
        p = self.packed
        model = {
            "cls_nodes": torch.from_numpy(np.ascontiguousarray(p.cls_nodes)),
            "cls_tree_offsets": torch.from_numpy(p.cls_tree_offsets),
            "feat_col": torch.from_numpy(p.feat_col),
            "feat_code": torch.from_numpy(p.feat_code),
            "medians": torch.from_numpy(p.medians),
            "if_nodes": torch.from_numpy(np.ascontiguousarray(p.if_nodes)),
            "if_tree_offsets": torch.from_numpy(p.if_tree_offsets),
            "ref_sorted": torch.from_numpy(p.ref_sorted),
            "ref_sorted_offsets": torch.from_numpy(p.ref_sorted_offsets),
            "ref_cat_offsets": torch.from_numpy(p.ref_cat_offsets),
            "cls_kind": int(getattr(p, "cls_kind", 0)),
            "cls_bias": float(getattr(p, "cls_bias", 0.0)),
            "if_denom": float(p.if_denom),
            "if_offset": float(p.if_offset),
            "if_threshold": float(p.if_threshold),
        }
        sess = ext.ScoreSession(model, capacity, self.device_index)
        self._gpu = {"ext": ext, "model": model}
        self._set_session(sess)

    def _set_session(self, sess):
        g = self._gpu
        g["sess"] = sess
        # zero-copy numpy views of the session's pinned staging/outputs;
        # first index = slot (double-buffered for pipelined callers)
        g["np_codes"] = sess.pin_codes.numpy()
        g["np_nums"] = sess.pin_nums.numpy()
        g["np_outs"] = sess.pin_outs.numpy()
        g["np_hist"] = sess.pin_hist.numpy()
        g["np_ksd"] = sess.pin_ksd.numpy()

    def _ensure_capacity(self, b: int):
        g = self._gpu
        if b > g["sess"].capacity:
            cap = 1 << (b - 1).bit_length()
            self._set_session(g["ext"].ScoreSession(g["model"], cap, self.device_index))

    def _score_gpu(self, codes: np.ndarray, nums: np.ndarray, with_drift: bool = True) -> dict:
        g = self._gpu
        b = len(codes)
        self._ensure_capacity(b)
        # Drift is a batch-population statistic; cap its sample at the K-S
        # kernel's LDS sort capacity (predictions still cover every row).
        drift_now = with_drift and b <= self.DRIFT_MAX_ROWS
        # one C call: pinned staging memcpy (GIL released) + graph replay
        g["sess"].submit_arrays(codes, nums, 0, drift_now, True)
        flat = g["np_outs"][0].reshape(-1)  # b-packed: proba | iscore | outlier
        out = {
            "predictions": flat[:b].copy(),
            "instance_score": flat[b : 2 * b].copy(),
            "outliers": flat[2 * b : 3 * b].copy(),
        }
        if with_drift and not drift_now:
            # oversized batch: score a capped drift sample in a second pass
            db = self.DRIFT_MAX_ROWS
            g["sess"].score(db, True, True)
            drift_now, b = True, db
        if drift_now:
            hist = g["np_hist"][0].copy()
            ks_d = g["np_ksd"][0].copy()
            out["p_vals"] = cpu_ref.pvals_from_stats(self.packed, hist, ks_d, b)
            out["cat_hist"] = hist
            out["ks_d"] = ks_d
        return out

    # ------------------------------------------------------------------ API
    def score_arrays(self, codes: np.ndarray, nums: np.ndarray, with_drift: bool = True) -> dict:
        """Score an encoded batch; returns predictions/outliers/p_vals arrays."""
        if self.device == "cuda":
            return self._score_gpu(codes, nums, with_drift=with_drift)
        nums_imp = cpu_ref.impute_nums(self.packed, nums)
        proba = cpu_ref.score_forest_cpu(self.packed, codes, nums_imp)
        iscore, outliers = cpu_ref.score_iforest_cpu(self.packed, nums_imp)
        out = {"predictions": proba, "outliers": outliers, "instance_score": iscore}
        if with_drift:
            cat_hist, ks_d = cpu_ref.drift_stats_cpu(self.packed, codes, nums_imp)
            out["p_vals"] = cpu_ref.pvals_from_stats(self.packed, cat_hist, ks_d, len(codes))
            out["cat_hist"] = cat_hist
            out["ks_d"] = ks_d
        return out

    # ------------------------------------------------------- attributions
    def explain_arrays(
        self,
        codes: np.ndarray,
        nums: np.ndarray,
        method: str = "saabas",
        background=None,
        interactions: bool = False,
    ) -> dict:
        """Per-row attributions for the classifier: prediction-path (Saabas)
        contributions by default, exact path-dependent TreeSHAP values with
        ``method="shap"`` (same keys; ``base_value`` is then the SHAP base,
        the cover-weighted expectation of the model output, and the call is
        capped at SHAP_MAX_ROWS), interventional Shapley values against a
        background sample with ``method="interventional"`` (same keys plus
        ``background_rows``; ``base_value`` is then the mean model output
        over the background rows; same row cap). ``background`` is an
        optional encoded ``(codes, nums)`` pair that replaces the packed
        sample for that method. ``interactions=True`` (``method="shap"``
        only, capped at INTERACTION_MAX_ROWS) adds ``interactions``
        f64[B, 23, 23]: exact SHAP interaction values, symmetric, each
        off-diagonal entry half of the pair's interaction, the diagonal the
        feature's SHAP value minus its off-diagonal row sum, so that
        ``interactions.sum(2)`` is ``contributions``.

        Returns ``contributions`` f64[B, 23] in schema.FEATURES order,
        ``base_value``, ``output_space`` ("probability" for the averaging
        forests, "log_odds" for gradient boosting) and ``predictions``
        (base + row sum, through the sigmoid for log-odds) — the scoring
        kernels are not run. base_value + contributions.sum(1) is the model
        output by construction."""
        p = self.packed
        if method not in EXPLAIN_METHODS:
            raise ValueError(
                f"unknown explain method {method!r}; expected one of {EXPLAIN_METHODS}"
            )
        if interactions and method != "shap":
            raise ValueError("interactions=True applies to method='shap' only")
        if method == "interventional":
            return self._explain_ishap(codes, nums, background)
        if background is not None:
            raise ValueError("background= applies to method='interventional' only")
        if method == "shap":
            return self._explain_shap(codes, nums, interactions)
        if p.cls_node_value is None:
            raise ExplainUnavailable(
                "model was packed without per-node expected values; "
                "re-pack it from the trained pipeline to enable attributions"
            )
        b = len(codes)
        if b > self.EXPLAIN_MAX_ROWS:
            raise ExplainTooLarge(
                f"explain is capped at {self.EXPLAIN_MAX_ROWS} rows per call (got {b})"
            )
        codes = np.ascontiguousarray(codes, dtype=np.int16).reshape(b, N_CAT)
        nums = np.ascontiguousarray(nums, dtype=np.float32).reshape(b, N_NUM)
        if self.device == "cuda":
            contrib = self._explain_gpu(codes, nums)
        else:
            contrib = cpu_ref.forest_contrib_cpu(
                p, codes, cpu_ref.impute_nums(p, nums)
            )
        base = float(p.cls_base_value)
        raw = base + contrib.sum(axis=1)
        log_odds = int(getattr(p, "cls_kind", 0)) == 1
        return {
            "contributions": contrib,
            "base_value": base,
            "output_space": "log_odds" if log_odds else "probability",
            "predictions": 1.0 / (1.0 + np.exp(-raw)) if log_odds else raw,
        }

    def _explain_gpu(self, codes: np.ndarray, nums: np.ndarray) -> np.ndarray:
        import torch

        ext = self._gpu["ext"]
        dev = torch.device("cuda", self.device_index)
        # The lock covers the lazy upload and the call: concurrent explains on
        # one replica serialize; scoring is untouched (no shared state).
        with self._explain_lock:
            m = self._forest_dev()
            with torch.cuda.device(dev):
                out = ext.forest_contrib(
                    torch.from_numpy(codes).to(dev),
                    torch.from_numpy(nums).to(dev),
                    m["cls_nodes"],
                    m["cls_node_value"],
                    m["cls_off"],
                    m["feat_col"],
                    m["feat_code"],
                    m["medians"],
                    int(getattr(self.packed, "cls_kind", 0)),
                )
                return out.cpu().numpy()  # D2H copy synchronizes the stream

    def _forest_dev(self) -> dict:
        """The classifier forest tables on the device, bounds-checked and
        uploaded once; the caller holds _explain_lock."""
        import torch

        m = self._explain_dev
        if m is None:
            p = self.packed
            dev = torch.device("cuda", self.device_index)
            _check_forest_tables(p)
            # Own device copies of the model tensors — the session keeps
            # its buffers private, so cls_nodes sits in HBM twice
            # (16 B/node; accepted for an explain path that never
            # touches session state).
            tables = [
                ("cls_nodes", p.cls_nodes, np.int32),
                ("cls_off", p.cls_tree_offsets, np.int32),
                ("feat_col", p.feat_col, np.int32),
                ("feat_code", p.feat_code, np.int32),
                ("medians", p.medians, np.float32),
            ]
            if p.cls_node_value is not None:  # Saabas only
                tables.append(("cls_node_value", p.cls_node_value, np.float32))
            m = {
                k: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
                for k, a, dt in tables
            }
            self._explain_dev = m
        return m

    def _explain_shap(
        self, codes: np.ndarray, nums: np.ndarray, interactions: bool = False
    ) -> dict:
        p = self.packed
        if p.cls_node_cover is None:
            raise ExplainUnavailable(
                "model was packed without per-node cover; re-pack it from "
                "the trained pipeline to enable SHAP attributions"
            )
        b = len(codes)
        if interactions and b > self.INTERACTION_MAX_ROWS:
            raise ExplainTooLarge(
                f"explain with interactions is capped at "
                f"{self.INTERACTION_MAX_ROWS} rows per call (got {b})"
            )
        if b > self.SHAP_MAX_ROWS:
            raise ExplainTooLarge(
                f"explain with method='shap' is capped at {self.SHAP_MAX_ROWS} "
                f"rows per call (got {b})"
            )
        codes = np.ascontiguousarray(codes, dtype=np.int16).reshape(b, N_CAT)
        nums = np.ascontiguousarray(nums, dtype=np.float32).reshape(b, N_NUM)
        # The lock covers the lazy table build/upload and the call, as for
        # the Saabas tensors; nothing here is shared with the scoring session.
        with self._explain_lock:
            paths, base = self._path_table()
            if self.device == "cuda":
                contrib = self._shap_gpu(paths, codes, nums)
            else:
                contrib = cpu_ref.forest_shap_cpu(
                    p, codes, cpu_ref.impute_nums(p, nums), paths=paths
                )
            inter = self._shap_inter(paths, codes, nums) if interactions else None
        raw = base + contrib.sum(axis=1)
        log_odds = int(getattr(p, "cls_kind", 0)) == 1
        out = {
            "contributions": contrib,
            "base_value": base,
            "output_space": "log_odds" if log_odds else "probability",
            "predictions": 1.0 / (1.0 + np.exp(-raw)) if log_odds else raw,
        }
        if inter is not None:
            # the diagonal closes every row of the matrix onto the SHAP value
            d = np.arange(N_CAT + N_NUM)
            inter[:, d, d] = 0.0
            inter[:, d, d] = contrib - inter.sum(axis=2)
            out["interactions"] = inter
        return out

    def _shap_inter(self, paths, codes: np.ndarray, nums: np.ndarray) -> np.ndarray:
        """Off-diagonal SHAP interaction values f64[B, 23, 23] (the diagonal
        is the caller's), at most INTERACTION_LAUNCH_ROWS rows per launch;
        the caller holds _explain_lock."""
        p = self.packed
        if self.device == "cuda":
            import torch

            ext = self._gpu["ext"]
            dev = torch.device("cuda", self.device_index)
            m = self._path_table_dev(paths)

            def run(c: np.ndarray, x: np.ndarray) -> np.ndarray:
                with torch.cuda.device(dev):
                    out = ext.forest_shap_interactions(
                        torch.from_numpy(c).to(dev),
                        torch.from_numpy(x).to(dev),
                        m["leaf_value"],
                        m["leaf_off"],
                        m["splits"],
                        m["medians"],
                        int(getattr(p, "cls_kind", 0)),
                        int(p.cls_n_trees),
                    )
                    return out.cpu().numpy()  # D2H copy synchronizes the stream
        else:
            def run(c, x):
                return cpu_ref.forest_shap_interactions_cpu(
                    p, c, cpu_ref.impute_nums(p, x), paths=paths
                )
        step = max(1, int(self.INTERACTION_LAUNCH_ROWS))
        parts = [
            run(codes[s : s + step], nums[s : s + step])
            for s in range(0, len(codes), step)
        ]
        n_src = N_CAT + N_NUM
        if not parts:
            return np.zeros((0, n_src, n_src), dtype=np.float64)
        return np.concatenate(parts)

    def _path_table(self):
        """(path table, SHAP base value), built and bounds-checked once; the
        caller holds _explain_lock. A model without per-node cover gets the
        table too (fractions 1, base NaN): the interventional pair rule never
        reads them, and method="shap" refuses such a model before it gets
        here."""
        if self._shap is None:
            from .pack import build_shap_paths

            paths, base = build_shap_paths(self.packed, require_cover=False)
            _check_shap_paths(paths)
            self._shap = (paths, base)
        return self._shap

    def _path_table_dev(self, paths):
        """The path table on the device, uploaded once; the caller holds
        _explain_lock."""
        import torch

        dev = torch.device("cuda", self.device_index)
        m = self._shap_dev
        if m is None:
            m = {
                "leaf_value": torch.from_numpy(paths.leaf_value).to(dev),
                "leaf_off": torch.from_numpy(paths.leaf_off).to(dev),
                "splits": torch.from_numpy(np.ascontiguousarray(paths.splits)).to(dev),
                "medians": torch.from_numpy(
                    np.ascontiguousarray(self.packed.medians, dtype=np.float32)
                ).to(dev),
            }
            self._shap_dev = m
        return m

    def _explain_ishap(self, codes: np.ndarray, nums: np.ndarray, background) -> dict:
        p = self.packed
        own = background is None  # the packed sample: base value and upload cached
        if own:
            if p.bg_codes is None or p.bg_nums is None:
                raise ExplainUnavailable(
                    "model was packed without a background sample; re-train "
                    "and re-pack it (or pass background=) to enable "
                    "interventional attributions"
                )
            background = (p.bg_codes, p.bg_nums)
        bg_codes = np.ascontiguousarray(background[0], dtype=np.int16)
        bg_nums = np.ascontiguousarray(background[1], dtype=np.float32)
        r = len(bg_codes)
        if bg_codes.shape != (r, N_CAT) or bg_nums.shape != (r, N_NUM):
            raise ValueError(
                f"background must be (codes [R, {N_CAT}], nums [R, {N_NUM}])"
            )
        if not 1 <= r <= self.ISHAP_MAX_BACKGROUND:
            raise ValueError(
                f"the background sample must have 1..{self.ISHAP_MAX_BACKGROUND} "
                f"rows (got {r})"
            )
        b = len(codes)
        if b > self.SHAP_MAX_ROWS:
            raise ExplainTooLarge(
                f"explain with method='interventional' is capped at "
                f"{self.SHAP_MAX_ROWS} rows per call (got {b})"
            )
        codes = np.ascontiguousarray(codes, dtype=np.int16).reshape(b, N_CAT)
        nums = np.ascontiguousarray(nums, dtype=np.float32).reshape(b, N_NUM)
        # One launch covers at most ISHAP_MAX_PAIRS (row, background row)
        # pairs; a larger call goes slice by slice.
        step = max(1, int(self.ISHAP_MAX_PAIRS) // r)
        with self._explain_lock:
            paths, _ = self._path_table()
            if own and self._ishap is not None:
                bg_imp, base = self._ishap
            else:
                # host f64 from the path table: the same number on CPU and
                # GPU engines
                bg_imp = cpu_ref.impute_nums(p, bg_nums)
                base = cpu_ref.forest_ishap_base_cpu(p, bg_codes, bg_imp, paths=paths)
                if own:
                    self._ishap = (bg_imp, base)
            if self.device == "cuda":
                run = self._ishap_gpu(paths, bg_codes, bg_nums, own)
            else:
                def run(c, x):
                    return cpu_ref.forest_ishap_cpu(
                        p, c, cpu_ref.impute_nums(p, x), bg_codes, bg_imp, paths=paths
                    )
            parts = [
                run(codes[s : s + step], nums[s : s + step]) for s in range(0, b, step)
            ]
        contrib = (
            np.concatenate(parts) if parts else np.zeros((0, N_CAT + N_NUM), dtype=np.float64)
        )
        raw = base + contrib.sum(axis=1)
        log_odds = int(getattr(p, "cls_kind", 0)) == 1
        return {
            "contributions": contrib,
            "base_value": base,
            "output_space": "log_odds" if log_odds else "probability",
            "predictions": 1.0 / (1.0 + np.exp(-raw)) if log_odds else raw,
            "background_rows": r,
        }

    def _ishap_gpu(self, paths, bg_codes: np.ndarray, bg_nums: np.ndarray, own: bool):
        """One-launch runner of forest_ishap on the device (rows in, f64
        values out); the caller holds _explain_lock. The packed sample's
        device copy is kept; an override is uploaded per call."""
        import torch

        ext = self._gpu["ext"]
        dev = torch.device("cuda", self.device_index)
        m = self._path_table_dev(paths)
        bg = self._ishap_dev if own else None
        if bg is None:
            bg = (torch.from_numpy(bg_codes).to(dev), torch.from_numpy(bg_nums).to(dev))
            if own:
                self._ishap_dev = bg

        def run(c: np.ndarray, x: np.ndarray) -> np.ndarray:
            with torch.cuda.device(dev):
                out = ext.forest_ishap(
                    torch.from_numpy(c).to(dev),
                    torch.from_numpy(x).to(dev),
                    bg[0],
                    bg[1],
                    m["leaf_value"],
                    m["leaf_off"],
                    m["splits"],
                    m["medians"],
                    int(getattr(self.packed, "cls_kind", 0)),
                    int(self.packed.cls_n_trees),
                )
                return out.cpu().numpy()  # D2H copy synchronizes the stream

        return run

    def _shap_gpu(self, paths, codes: np.ndarray, nums: np.ndarray) -> np.ndarray:
        """forest_shap on the device; the caller holds _explain_lock."""
        import torch

        ext = self._gpu["ext"]
        dev = torch.device("cuda", self.device_index)
        m = self._path_table_dev(paths)
        with torch.cuda.device(dev):
            out = ext.forest_shap(
                torch.from_numpy(codes).to(dev),
                torch.from_numpy(nums).to(dev),
                m["leaf_value"],
                m["leaf_off"],
                m["splits"],
                m["medians"],
                int(getattr(self.packed, "cls_kind", 0)),
                int(self.packed.cls_n_trees),
            )
            return out.cpu().numpy()  # D2H copy synchronizes the stream

    # ------------------------------------------------- partial dependence
    def partial_dependence(
        self,
        features,
        sample=None,
        grid_resolution: int = 20,
        percentiles=(0.05, 0.95),
        grid: dict | None = None,
        kind: str = "average",
        response: str = "probability",
    ) -> dict:
        """Partial dependence (and, with ``kind="both"``, the per-row ICE
        curves) of the classifier output on one feature or a pair: every row
        of a sample is scored with the feature set to each grid value in
        turn, and the outputs are averaged over the rows.

        ``features`` lists feature names (one-way) and pairs of distinct
        names (two-way). ``sample`` is an encoded ``(codes, nums)`` pair and
        defaults to the packed background sample. Grids follow the rule of
        creditcore/pdp.py (scikit-learn's, f32-rounded; categoricals take the
        whole vocabulary) unless ``grid={name: values}`` gives them.
        ``response="raw"`` (gradient boosting only) returns log-odds, not
        probabilities; a probability is taken per (row, grid point) before
        the rows are averaged, as scikit-learn's predict_proba PDP does.

        Returns ``{"results": [...], "sample_rows", "output_space"}``; each
        result holds ``features``, ``grid_values`` (one list per axis),
        ``average`` f64[G] or f64[G0, G1] and, with ``kind="both"``,
        ``individual`` f64[R, G] or f64[R, G0, G1]. The scoring session is not
        touched. Caps (creditcore/pdp.py) raise ExplainTooLarge."""
        from . import pdp

        p = self.packed
        if kind not in pdp.PDP_KINDS:
            raise ValueError(f"kind must be one of {pdp.PDP_KINDS} (got {kind!r})")
        if response not in pdp.PDP_RESPONSES:
            raise ValueError(f"response must be one of {pdp.PDP_RESPONSES} (got {response!r})")
        cls_kind = int(getattr(p, "cls_kind", 0))
        if response == "raw" and cls_kind != 1:
            raise ValueError("response='raw' applies to the log-odds (boosted) families only")
        own = sample is None  # the packed sample: its device copy is kept
        try:
            entries = pdp.parse_features(features)
            res, pct = pdp.check_grid_args(grid_resolution, percentiles)
            overrides = pdp.check_grid_override(grid)
            if own:
                if p.bg_codes is None or p.bg_nums is None:
                    raise ExplainUnavailable(
                        "model was packed without a background sample; re-train "
                        "and re-pack it (or pass sample=) to enable partial dependence"
                    )
                sample = (p.bg_codes, p.bg_nums)
            codes = np.ascontiguousarray(sample[0], dtype=np.int16)
            nums = np.ascontiguousarray(sample[1], dtype=np.float32)
            r = len(codes)
            if codes.shape != (r, N_CAT) or nums.shape != (r, N_NUM):
                raise ValueError(f"sample must be (codes [R, {N_CAT}], nums [R, {N_NUM}])")
            if r < 1:
                raise ValueError("the sample must have at least one row")
            if r > pdp.PDP_MAX_ROWS:
                raise pdp.PdpTooLarge(
                    f"the sample is capped at {pdp.PDP_MAX_ROWS} rows (got {r})"
                )
            nums_imp = cpu_ref.impute_nums(p, nums)
            axes: dict = {}
            for names in entries:
                for n in names:
                    if n not in axes:
                        axes[n] = pdp.build_axis(
                            n, p.vocabs, nums_imp, res, pct, overrides.get(n)
                        )
            tables = [pdp.entry_jobs([axes[n] for n in names]) for names in entries]
        except pdp.PdpTooLarge as e:
            raise ExplainTooLarge(str(e)) from None
        jobs = np.ascontiguousarray(np.concatenate(tables), dtype=np.int32)
        # One launch covers at most PDP_LAUNCH_PAIRS (job, row) pairs; a
        # larger call goes job slice by job slice.
        step = max(1, int(self.PDP_LAUNCH_PAIRS) // r)
        with self._explain_lock:
            if self.device == "cuda":
                run = self._whatif_gpu(codes, nums, own)
            else:
                def run(jb):
                    return cpu_ref.forest_whatif_cpu(p, codes, nums_imp, jb)
            raw = np.concatenate(
                [run(jobs[s : s + step]) for s in range(0, len(jobs), step)]
            )
        vals = pdp.finalize(raw, cls_kind, float(p.cls_bias), int(p.cls_n_trees), response)
        results, at = [], 0
        for names, table in zip(entries, tables):
            shape = [len(axes[n].bits) for n in names]
            v = vals[at : at + len(table)]  # [G, R], axis 0 of a pair major
            at += len(table)
            out = {
                "features": list(names),
                "grid_values": [list(axes[n].values) for n in names],
                "average": v.mean(axis=1).reshape(shape),
            }
            if kind == "both":
                out["individual"] = np.ascontiguousarray(v.T).reshape([r] + shape)
            results.append(out)
        return {
            "results": results,
            "sample_rows": r,
            "output_space": "log_odds" if response == "raw" else "probability",
        }

    def _whatif_gpu(self, codes: np.ndarray, nums: np.ndarray, own: bool):
        """One-launch runner of forest_whatif on the device (job table in, raw
        f64[J, R] sums out); the caller holds _explain_lock. Uses the
        lazily uploaded forest tables of _explain_gpu; the packed sample's
        device copy is kept, another sample is uploaded per call."""
        import torch

        ext = self._gpu["ext"]
        dev = torch.device("cuda", self.device_index)
        m = self._forest_dev()
        smp = self._pdp_sample_dev if own else None
        if smp is None:
            smp = (torch.from_numpy(codes).to(dev), torch.from_numpy(nums).to(dev))
            if own:
                self._pdp_sample_dev = smp

        def run(jb: np.ndarray) -> np.ndarray:
            with torch.cuda.device(dev):
                out = ext.forest_whatif(
                    smp[0],
                    smp[1],
                    m["cls_nodes"],
                    m["cls_off"],
                    m["feat_col"],
                    m["feat_code"],
                    m["medians"],
                    torch.from_numpy(np.ascontiguousarray(jb, dtype=np.int32)),
                )
                return out.cpu().numpy()  # D2H copy synchronizes the stream

        return run

    # ---------------------------------------------------- counterfactuals
    def counterfactuals(
        self,
        codes: np.ndarray,
        nums: np.ndarray,
        features=None,
        threshold: float = 0.5,
        curves: bool = False,
    ) -> dict:
        """The smallest change to ONE feature that flips the classifier's
        decision ``probability > threshold`` of each row, every other feature
        held fixed. Exact with respect to the packed f32 thresholds: for a
        numeric feature the model output is piecewise constant, its
        breakpoints are the thresholds the forest tests on the column
        (creditcore/counterfactual.py), and the whole curve over those K + 1
        intervals is computed (forest_sweep_kernel; cpu_ref.forest_sweep_cpu
        with device="cpu") and searched for the nearest flip on each side. A
        categorical feature is tried code by code over its vocabulary through
        the what-if kernel of partial_dependence.

        ``features`` defaults to all 23 names. Returns ``{"threshold",
        "features", "rows"}``; a row holds ``probability``, ``decision`` (0/1)
        and ``counterfactuals``, one entry per feature. Numeric: ``value``
        (the imputed own value), ``below`` / ``above``, each None or
        ``{value, delta, probability}`` with ``value`` the closest f32 whose
        decision differs (above: the next f32 after the flipping interval's
        lower threshold; below: its upper threshold). With ``curves=True``
        also ``thresholds`` (K) and ``probabilities`` (K + 1). Categorical:
        ``value`` (the own category, None if unknown) and ``flips``, the
        ``{category, probability}`` of every other known category whose
        decision differs, in vocabulary order. The decision is taken in raw
        space (``raw > cut``, counterfactual.raw_cut). The scoring session is
        not touched. Caps (creditcore/counterfactual.py) raise
        ExplainTooLarge."""
        from . import counterfactual as cf
        from . import pdp

        p = self.packed
        names = cf.parse_features(features)
        thr = cf.check_threshold(threshold)
        codes = np.ascontiguousarray(codes, dtype=np.int16)
        nums = np.ascontiguousarray(nums, dtype=np.float32)
        r = len(codes)
        if codes.shape != (r, N_CAT) or nums.shape != (r, N_NUM):
            raise ValueError(f"rows must be (codes [R, {N_CAT}], nums [R, {N_NUM}])")
        if r < 1:
            raise ValueError("counterfactuals needs at least one row")
        if r > cf.CF_MAX_ROWS:
            raise ExplainTooLarge(
                f"counterfactuals is capped at {cf.CF_MAX_ROWS} rows per call (got {r})"
            )
        players = [FEATURES.index(n) for n in names]
        num_cols = [pl - N_CAT for pl in players if pl >= N_CAT]
        cat_players = [pl for pl in players if pl < N_CAT]
        cls_kind = int(getattr(p, "cls_kind", 0))
        cut = cf.raw_cut(p, thr)
        nums_imp = cpu_ref.impute_nums(p, nums)
        # the row's own raw sum is entry k0 of any of its curves: a call
        # without a numeric feature sweeps column 0 for it
        sweep_cols = num_cols or [0]
        jobs = cf.sweep_jobs(r, sweep_cols)
        step = max(1, int(self.CF_LAUNCH_JOBS))
        with self._explain_lock:
            tables = self._cf_tables()
            if curves:
                points = r * sum(len(tables.thresholds[c]) + 1 for c in num_cols)
                if points > cf.CF_MAX_CURVE_POINTS:
                    raise ExplainTooLarge(
                        f"curves=True would return {points} curve points; the cap is "
                        f"{cf.CF_MAX_CURVE_POINTS} per call (fewer rows or features)"
                    )
            want = bool(curves and num_cols)
            if self.device == "cuda":
                cf.check_depth(tables)
                sweep = self._sweep_gpu(codes, nums, cut, want)
                whatif = self._whatif_gpu(codes, nums, False) if cat_players else None
            else:
                def sweep(jb):
                    rec, raw, cv = cpu_ref.forest_sweep_cpu(p, codes, nums_imp, jb, cut, tables)
                    return rec, raw, cv if want else None

                def whatif(jb):
                    return cpu_ref.forest_whatif_cpu(p, codes, nums_imp, jb)
            parts = [sweep(jobs[s : s + step]) for s in range(0, len(jobs), step)]
            rec = np.concatenate([a for a, _, _ in parts]).reshape(r, len(sweep_cols), 3)
            raw = np.concatenate([b for _, b, _ in parts]).reshape(r, len(sweep_cols), 3)
            curve_of = [c for _, _, cv in parts for c in cv] if want else None
            cat_raw = None
            if cat_players:
                wj = cf.category_jobs(p.vocabs, cat_players)
                if len(wj):
                    wstep = max(1, int(self.PDP_LAUNCH_PAIRS) // r)
                    cat_raw = np.concatenate(
                        [whatif(wj[s : s + wstep]) for s in range(0, len(wj), wstep)]
                    )  # [G, R]

        def prob(x):
            return pdp.finalize(
                np.asarray(x, dtype=np.float64), cls_kind, float(p.cls_bias),
                int(p.cls_n_trees), "probability",
            )

        own_raw = raw[:, 0, 0]
        own_dec = own_raw > cut
        own_prob = prob(own_raw)
        side_prob = prob(raw)
        cat_prob = prob(cat_raw) if cat_raw is not None else None
        cat_at = {}
        at = 0
        for pl in cat_players:
            cat_at[pl] = at
            at += len(p.vocabs[pl])
        rows = []
        for i in range(r):
            entries = {}
            for name, pl in zip(names, players):
                if pl < N_CAT:
                    vocab = p.vocabs[pl]
                    own = int(codes[i, pl])
                    flips = []
                    for code in range(len(vocab)):
                        g = cat_at[pl] + code
                        if code != own and bool(cat_raw[g, i] > cut) != bool(own_dec[i]):
                            flips.append(
                                {"category": vocab[code], "probability": float(cat_prob[g, i])}
                            )
                    entries[name] = {
                        "value": vocab[own] if 0 <= own < len(vocab) else None,
                        "flips": flips,
                    }
                    continue
                c = pl - N_CAT
                s = num_cols.index(c)
                t = tables.thresholds[c]
                own = float(nums_imp[i, c])
                _, kb, ka = (int(k) for k in rec[i, s])
                entry = {
                    "value": own,
                    "below": cf.side_entry(t, kb, False, own, side_prob[i, s, 1]) if kb >= 0 else None,
                    "above": cf.side_entry(t, ka, True, own, side_prob[i, s, 2]) if ka >= 0 else None,
                }
                if curves:
                    entry["thresholds"] = t.astype(np.float64)
                    entry["probabilities"] = prob(curve_of[i * len(num_cols) + s])
                entries[name] = entry
            rows.append(
                {
                    "probability": float(own_prob[i]),
                    "decision": int(own_dec[i]),
                    "counterfactuals": entries,
                }
            )
        return {"threshold": thr, "features": names, "rows": rows}

    def _cf_tables(self):
        """The breakpoint tables of counterfactuals, derived once from the
        packed forest; the caller holds _explain_lock."""
        from . import counterfactual as cf

        if self._cf is None:
            _check_forest_tables(self.packed)
            self._cf = cf.build_tables(self.packed)
        return self._cf

    def _sweep_gpu(self, codes: np.ndarray, nums: np.ndarray, cut: float, want_curves: bool):
        """One-launch runner of forest_sweep on the device ({row, column} job
        table in; records, raw sums and, when asked, curves out); the caller
        holds _explain_lock. Breakpoint tables are uploaded once, next to
        the forest tables of _forest_dev."""
        import torch

        from .ops import gpu

        dev = torch.device("cuda", self.device_index)
        m = self._forest_dev()
        t = self._cf_tables()
        if self._cf_dev is None:
            self._cf_dev = {
                "node_rank": torch.from_numpy(t.node_rank).to(dev),
                "thr": torch.from_numpy(t.thr).to(dev),
                "thr_off": torch.from_numpy(t.thr_off),  # host: the binding checks it
                "max_depth": t.max_depth,
            }
        sw = self._cf_dev
        rows = (torch.from_numpy(codes).to(dev), torch.from_numpy(nums).to(dev))

        def run(jb: np.ndarray):
            with torch.cuda.device(dev):
                return gpu.forest_sweep(rows[0], rows[1], m, sw, jb, cut, want_curves)

        return run

    def counterfactual_records(self, records, **kw) -> dict:
        """counterfactuals on a request body (list of dicts / DataFrame)."""
        codes, nums = encode_batch(records, self.packed.vocabs)
        return self.counterfactuals(codes, nums, **kw)

    def explain_records(
        self,
        records,
        method: str = "saabas",
        background=None,
        interactions: bool = False,
    ) -> dict:
        """explain_arrays on a request body (list of dicts / DataFrame)."""
        codes, nums = encode_batch(records, self.packed.vocabs)
        return self.explain_arrays(
            codes, nums, method=method, background=background, interactions=interactions
        )

    def encode_json_body(self, body: bytes) -> tuple:
        """Parse a raw /score JSON body into (codes, nums) with the native C
        parser (GIL released during the parse); raises ValueError on
        malformed/ill-typed bodies (callers fall back to pydantic for proper
        422 semantics)."""
        from .ops import gpu
        from .pack import CATEGORICAL_FEATURES, MISSING_CATEGORY, NUMERIC_FEATURES

        if gpu.available():
            codes, nums = self._ensure_json_encoder().encode(body)
            return np.asarray(codes), np.asarray(nums)
        import json

        recs = json.loads(body)
        if not isinstance(recs, list) or not all(isinstance(r, dict) for r in recs):
            raise ValueError("body must be a JSON array of records")
        # Strictness parity with the native parser: nulls and ill-typed
        # values raise ValueError so callers fall back to pydantic for the
        # reference's 422/coercion semantics; absent fields take the schema
        # defaults (pydantic default semantics, reference app/model.py:8-34
        # — encode_batch alone would fill missing categoricals with
        # MISSING_CATEGORY instead).
        cat = set(CATEGORICAL_FEATURES)
        num = set(NUMERIC_FEATURES)
        for r in recs:
            for k, v in r.items():
                if k in cat:
                    if not isinstance(v, str):
                        raise ValueError(f"field {k}: expected string")
                elif k in num:
                    if isinstance(v, bool) or not isinstance(v, (int, float)):
                        raise ValueError(f"field {k}: expected number")
        from .schema import LoanApplicant

        defaults = LoanApplicant().__dict__
        recs = [{**defaults, **r} for r in recs]
        return encode_batch(recs, self.packed.vocabs)

    def _ensure_json_encoder(self):
        enc = getattr(self, "_json_encoder", None)
        if enc is None:
            from .ops import gpu
            from .pack import CATEGORICAL_FEATURES, MISSING_CATEGORY, NUMERIC_FEATURES

            dc, dn = self.default_rows()
            enc = gpu.ext().JsonEncoder(
                self.packed.vocabs,
                CATEGORICAL_FEATURES,
                NUMERIC_FEATURES,
                MISSING_CATEGORY,
                dc,
                dn,
            )
            self._json_encoder = enc
        return enc

    def score_json(self, body: bytes) -> dict:
        """Score a raw /score JSON request body (wire-format fast path)."""
        codes, nums = self.encode_json_body(body)
        return self._score_encoded(codes, nums)

    def score_json_full(self, body: bytes) -> dict:
        """Fully-native request: one C++ call parses the wire JSON, stages,
        replays the graph, converts drift p-values and serializes the
        response — no Python object pass. Falls back to the staged path for
        oversized batches or on CPU."""
        if self.device != "cuda":
            return self.score_json_bytes(body)
        g = self._gpu
        try:
            resp, rows = g["sess"].score_json_full(
                body,
                self._ensure_json_encoder(),
                self.packed.ref_cat_counts,
                self.packed.ref_cat_offsets,
                int(self.packed.ref_sorted_offsets[1] - self.packed.ref_sorted_offsets[0]),
                FEATURES,
                self.DRIFT_MAX_ROWS,
            )
        except RuntimeError:
            # batch larger than the resident session capacity: grow + retry
            # through the staged path
            return self.score_json_bytes(body)
        return {
            "response_bytes": resp,
            "rows": int(rows),
            "cat_hist": g["np_hist"][0].copy(),
        }

    def default_rows(self) -> tuple:
        """Encoded schema-default record (absent request fields take these
        values — pydantic default semantics, reference app/model.py:8-34)."""
        if getattr(self, "_default_rows", None) is None:
            from .schema import LoanApplicant

            dc, dn = encode_batch([LoanApplicant().__dict__], self.packed.vocabs)
            self._default_rows = (
                np.ascontiguousarray(dc[0]),
                np.ascontiguousarray(dn[0]),
            )
        return self._default_rows

    def score_json_bytes(self, body: bytes) -> dict:
        """Wire-format in, wire-format out: parse the JSON request with the
        C parser, score through the session graph, and serialize the
        response JSON in C — the full /score answer with no Python object
        pass. Returns {"response_bytes", "rows"}."""
        codes, nums = self.encode_json_body(body)
        return self.score_encoded_bytes(codes, nums)

    def score_encoded_bytes(self, codes: np.ndarray, nums: np.ndarray) -> dict:
        b = len(codes)
        if self.device != "cuda" or b == 0:
            import json

            out = self._score_encoded(codes, nums)
            return {
                "response_bytes": json.dumps(out["response"]).encode(),
                "rows": b,
            }
        g = self._gpu
        self._ensure_capacity(b)
        nb = b
        if b <= self.DRIFT_MAX_ROWS:
            g["sess"].submit_arrays(codes, nums, 0, True, True)
        else:
            g["np_codes"][0][:b] = codes
            g["np_nums"][0][:b] = nums
            # Oversized batch: drift is a batch-population statistic, so run
            # the capped-sample drift pass FIRST (only with_drift passes
            # write the pinned drift blob), then the full batch without
            # drift — pin_outs then holds the b-packed layout
            # build_response_json reads. The reverse order overwrote the
            # b-packed outputs with a cap-packed second pass and corrupted
            # rows >= cap (round-1 advisor finding).
            g["sess"].score(self.DRIFT_MAX_ROWS, True, True)
            g["sess"].score(b, False, True)
            nb = self.DRIFT_MAX_ROWS
        pvals = cpu_ref.pvals_from_stats(self.packed, g["np_hist"][0], g["np_ksd"][0], nb)
        resp = g["ext"].build_response_json(
            g["sess"].pin_outs, b, np.ascontiguousarray(pvals), FEATURES
        )
        return {
            "response_bytes": resp,
            "rows": b,
            # for node-global drift aggregation by the serving layer
            "cat_hist": g["np_hist"][0].copy(),
        }

    # -------------------------------------------------- pipelined slot API
    def submit_encoded_slot(self, codes: np.ndarray, nums: np.ndarray, slot: int) -> int:
        """Stage + launch (no sync) into a pinned slot; pair with
        finish_slot. Slot i%2 lets step i's epilogue overlap step i+1's
        graph. Falls back to capacity growth like the sync path."""
        g = self._gpu
        b = len(codes)
        self._ensure_capacity(b)
        assert b <= self.DRIFT_MAX_ROWS, "pipelined path caps at DRIFT_MAX_ROWS"
        g["sess"].submit_arrays(codes, nums, slot & 1, True, False)
        return b

    def finish_slot(self, slot: int, b: int) -> dict:
        """Wait for the slot's graph; C epilogue: drift p-values +
        response serialization from the slot's pinned buffers."""
        g = self._gpu
        s = slot & 1
        n_ref = int(self.packed.ref_sorted_offsets[1] - self.packed.ref_sorted_offsets[0])
        resp = g["sess"].response_epilogue(
            s, b, self.packed.ref_cat_counts, self.packed.ref_cat_offsets,
            n_ref, FEATURES,
        )
        return {
            "response_bytes": resp,
            "rows": b,
            "cat_hist": g["np_hist"][s].copy(),
        }

    def score_records(self, records) -> dict:
        """Score a request body (list of dicts / DataFrame); returns the
        reference response shape (02-register cell-9)."""
        codes, nums = encode_batch(records, self.packed.vocabs)
        return self._score_encoded(codes, nums)

    def _score_encoded(self, codes: np.ndarray, nums: np.ndarray) -> dict:
        t0 = time.perf_counter()
        raw = self.score_arrays(codes, nums)
        latency_ms = (time.perf_counter() - t0) * 1e3
        # (1 - p_val) computed in float32, like the reference's
        # (1 - drift_results["data"]["p_val"]).tolist() on the float32
        # p_val array (02-register cell-9); .tolist() is C-speed.
        one_minus = (
            np.float32(1.0) - np.asarray(raw["p_vals"], dtype=np.float32)
        ).astype(np.float64)
        resp = {
            "predictions": np.asarray(raw["predictions"]).tolist(),
            "outliers": np.asarray(raw["outliers"]).tolist(),
            "feature_drift_batch": dict(zip(FEATURES, one_minus.tolist())),
        }
        return {"response": resp, "latency_ms": latency_ms, "rows": len(codes)}


def load_engine(
    model_directory: str,
    device: str = "auto",
    device_index: int = 0,
    drift_max_rows: int | None = None,
) -> ScoringEngine:
    """Load a model into a ScoringEngine. Accepts a pyfunc model dir, a
    packed .npz, or a registry URI (``models:/<name>/<version|latest>`` —
    the reference's MLflow registry addressing, 02-register cell-15)."""
    import os

    from . import pack as packmod
    from .config import ServeConfig
    from .registry import resolve_model_uri

    if device == "auto":
        device = ServeConfig().resolve_device()
    model_directory = resolve_model_uri(model_directory)
    if model_directory.endswith(".npz") and os.path.isfile(model_directory):
        packed = PackedModel.load(model_directory)
    else:
        packed = packmod.pack_pyfunc_dir(model_directory)
    return ScoringEngine(
        packed,
        device=device,
        device_index=device_index,
        drift_max_rows=drift_max_rows,
    )

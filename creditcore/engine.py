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
    # accumulated_local_effects: most (row, entry) pairs of one forest_ale
    # launch (a pair is one dual walk of the whole forest, between one and
    # two plain walks); a call above it runs as several launches over entry
    # and row slices. Sized like PDP_LAUNCH_PAIRS: the largest measured pair
    # count whose launch on the flagship forest (RF 500 x depth 16, all 14
    # numeric features at grid_resolution 20) is no longer than 1.25 x the
    # method="shap" launch at SHAP_MAX_ROWS measured in the same run:
    # forest_shap at 1024 rows 60.26 ms (bound 75.32 ms), forest_ale at
    # 65,536 rows x 14 entries = 917,504 pairs 27.62 ms on an MI355X (256
    # rows: 5.78 ms, 16,384 rows: 7.31 ms), bench/ale_micro.py,
    # profiles/bench_results/ale_micro.txt. That is the largest call the caps
    # allow (ALE_MAX_ROWS x N_NUM), so today no call is sliced.
    ALE_LAUNCH_JOBS = 917504
    # permutation_importance: most (table row, sample row) pairs of one
    # forest_permute launch (a table row is one permutation of one column, a
    # pair at most one walk of the whole forest); a call above it runs as
    # several launches over table-row slices cut at job boundaries. Sized
    # like PDP_LAUNCH_PAIRS: the largest measured pair count whose launch on
    # the flagship forest (RF 500 x depth 16, whole features of 5 repeats at
    # 65,536 rows) is no longer than 1.25 x the method="shap" launch at
    # SHAP_MAX_ROWS measured in the same run: forest_shap at 1024 rows
    # 60.22 ms (bound 75.28 ms), forest_permute at 60 table rows x 65,536
    # rows = 3,932,160 pairs 71.14 ms (80 table rows: 95.18 ms, over the
    # bound) on an MI355X, bench/perm_micro.py,
    # profiles/bench_results/perm_micro.txt. The default call at the row cap
    # (23 features x 5 repeats and the baseline row, 7.6 M pairs) runs as two
    # launches, the largest the caps allow (48.3 M pairs) as thirteen.
    PERM_LAUNCH_PAIRS = 3932160
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
    # anchors: most (mask, sample row) pairs of one forest_anchor launch (a
    # mask is one candidate anchor of one row, a pair one composite row's sum
    # over the whole forest, shared with the other masks of its chunk); a
    # search level above it runs as several launches over row ranges. Sized
    # like PDP_LAUNCH_PAIRS: the largest measured pair count whose launch on
    # the flagship forest (RF 500 x depth 16, level-1 candidate lists, 23
    # masks per row, on the 256-row sample) is no longer than 1.25 x the
    # method="shap" launch at SHAP_MAX_ROWS measured in the same run:
    # forest_shap at 1024 rows 60.09 ms (bound 75.11 ms), forest_anchor at
    # 64 rows x 23 masks x 256 = 376,832 pairs 62.04 ms (128 rows:
    # 113.25 ms, over the bound) on an MI355X,
    # bench/anchor_micro.py, profiles/bench_results/anchor_micro.txt. A level
    # of the largest call the caps allow (1024 rows x 92 masks x 1024 sample
    # rows, 96 M pairs) runs as 256 launches.
    ANCHOR_LAUNCH_PAIRS = 376832
    # mmd_drift: most pooled rows i (64-row tiles) of one mmd_perm launch; a
    # call above it runs as several launches over row slices. Sized like
    # ISHAP_MAX_PAIRS: the launch at the caps (n = m = 16384, N = 32768
    # pooled rows, flagship D, P = 100) may take no longer than 1.25 x the
    # method="shap" launch at SHAP_MAX_ROWS measured in the same run
    # (bench/mmd_micro.py, profiles/bench_results/mmd_micro.txt): forest_shap
    # at 1024 rows 60.03 ms (bound 75.04 ms), mmd_perm_w at N = 32768 as one
    # launch 4.36 ms on an MI355X. The caps allow no larger call, so today no
    # call is sliced.
    MMD_LAUNCH_ROWS = 32768
    # knn_outliers: most batch rows (64-row tiles) of one knn_topk launch; a
    # call above it runs as several launches over row slices. Same rule: the
    # launch at the caps (B = M = 16384, flagship D, k = 32) may take no
    # longer than 1.25 x the method="shap" launch at SHAP_MAX_ROWS measured
    # in the same run (bench/knn_micro.py,
    # profiles/bench_results/knn_micro.txt): forest_shap at 1024 rows
    # 59.78 ms (bound 74.73 ms), knn_topk at B = M = 16384, k = 32 as one
    # launch 2.70 ms on an MI355X. The caps allow no larger call, so today no
    # call is sliced.
    KNN_LAUNCH_ROWS = 16384
    # proximity: most batch rows (one block each) of one forest_prox_topk
    # launch; a call above it runs as several launches over row slices. Same
    # rule: the longest launch the engine issues may take no longer than
    # 1.25 x the method="shap" launch at SHAP_MAX_ROWS measured in the same
    # run (bench/prox_micro.py, profiles/bench_results/prox_micro.txt):
    # forest_shap at 1024 rows 60.39 ms (bound 75.48 ms), forest_prox_topk at
    # B = M = 16384, k = 32 as one launch 29.89 ms on an MI355X on the slower
    # of the two models measured (hgbt 500 x depth 6, 3.1 M co-memberships
    # per row; the flagship RF 500 x depth 16 2.71 ms). The caps allow no
    # larger call, so today no call is sliced. The time follows the length of
    # the leaf lists, so a shallower forest than depth 6 would take longer.
    PROX_LAUNCH_ROWS = 16384

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
        # mmd_drift: (key, mu, sd, z_ref, gamma) of the last reference sample
        self._mmd_ref = None
        # knn_outliers: the last (reference, k) seen: its embedding, device
        # copy and leave-one-out neighbour distances
        self._knn_ref = None
        # proximity: the last (reference, k) seen: its leaf table, inverted
        # index and leave-one-out counts
        self._prox_ref = None
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

    # ------------------------------------------- accumulated local effects
    def accumulated_local_effects(
        self,
        features,
        sample=None,
        grid_resolution: int = 20,
        grid: dict | None = None,
        kind: str = "average",
        response: str = "probability",
    ) -> dict:
        """Accumulated local effects (ALE) of the classifier output on numeric
        features: every row of a sample is moved only across the grid
        interval its own value lies in, the differences are averaged per
        interval and accumulated, and the curve is centred (creditcore/ale.py
        states the estimator in full). Unlike partial dependence, no row is
        scored away from the values it was observed with, which matters for
        strongly correlated columns.

        ``features`` lists numeric feature names (a categorical name is a
        ValueError). ``sample`` is an encoded ``(codes, nums)`` pair and
        defaults to the packed background sample. Edges are the sample
        quantiles at ``grid_resolution`` equal steps unless ``grid={name:
        edges}`` gives them (rows outside clamp into the first or last
        interval). ``response="raw"`` (gradient boosting only) works in
        log-odds.

        Returns ``{"results": [...], "sample_rows", "output_space"}``; each
        result holds ``feature``, ``edges`` (Ke + 1 floats), ``ale`` f64[Ke +
        1], ``counts`` i64[Ke] and, with ``kind="both"``, the per-row
        ``interval`` i32[R] (1..Ke) and ``local_effect`` f64[R]. A constant
        column has one edge, ``ale = [0.0]`` and ``counts = [R]``. The
        scoring session is not touched. Caps (creditcore/ale.py) raise
        ExplainTooLarge."""
        from . import ale

        p = self.packed
        if kind not in ale.ALE_KINDS:
            raise ValueError(f"kind must be one of {ale.ALE_KINDS} (got {kind!r})")
        if response not in ale.ALE_RESPONSES:
            raise ValueError(f"response must be one of {ale.ALE_RESPONSES} (got {response!r})")
        cls_kind = int(getattr(p, "cls_kind", 0))
        if response == "raw" and cls_kind != 1:
            raise ValueError("response='raw' applies to the log-odds (boosted) families only")
        own = sample is None  # the packed sample: its device copy is kept
        try:
            names = ale.parse_features(features)
            res, overrides = ale.check_args(grid_resolution, grid)
            if own:
                if p.bg_codes is None or p.bg_nums is None:
                    raise ExplainUnavailable(
                        "model was packed without a background sample; re-train and "
                        "re-pack it (or pass sample=) to enable accumulated local effects"
                    )
                sample = (p.bg_codes, p.bg_nums)
            codes = np.ascontiguousarray(sample[0], dtype=np.int16)
            nums = np.ascontiguousarray(sample[1], dtype=np.float32)
            r = len(codes)
            if codes.shape != (r, N_CAT) or nums.shape != (r, N_NUM):
                raise ValueError(f"sample must be (codes [R, {N_CAT}], nums [R, {N_NUM}])")
            if r < 1:
                raise ValueError("the sample must have at least one row")
            if r > ale.ALE_MAX_ROWS:
                raise ale.AleTooLarge(
                    f"the sample is capped at {ale.ALE_MAX_ROWS} rows (got {r})"
                )
            nums_imp = cpu_ref.impute_nums(p, nums)
            edges_of = {}
            for n in names:
                if n not in edges_of:
                    edges_of[n] = (
                        ale.override_edges(n, overrides[n])
                        if n in overrides
                        else ale.quantile_edges(nums_imp[:, FEATURES.index(n) - N_CAT], res)
                    )
        except ale.AleTooLarge as e:
            raise ExplainTooLarge(str(e)) from None
        # constant columns (one edge) are answered here, not by the kernel
        sent = [i for i, n in enumerate(names) if len(edges_of[n]) > 1]
        players = np.array([FEATURES.index(names[i]) for i in sent], dtype=np.int32)
        interval = np.empty((len(sent), r), dtype=np.int32)
        sums = np.empty((len(sent), r, 2), dtype=np.float64)
        # One launch covers at most ALE_LAUNCH_JOBS (row, entry) pairs: whole
        # entries over a row slice, as many as fit.
        rows_step = max(1, min(r, int(self.ALE_LAUNCH_JOBS)))
        ent_step = max(1, int(self.ALE_LAUNCH_JOBS) // rows_step)
        with self._explain_lock:
            if sent:
                if self.device == "cuda":
                    run = self._ale_gpu(codes, nums, own)
                else:
                    def run(a, b, pl, off, z):
                        return cpu_ref.forest_ale_cpu(p, codes[a:b], nums_imp[a:b], pl, off, z)
            for e in range(0, len(sent), ent_step):
                off, z = ale.edge_table([edges_of[names[i]] for i in sent[e : e + ent_step]])
                for a in range(0, r, rows_step):
                    b = min(a + rows_step, r)
                    interval[e : e + ent_step, a:b], sums[e : e + ent_step, a:b] = run(
                        a, b, players[e : e + ent_step], off, z
                    )
        results, slot = [], {i: s for s, i in enumerate(sent)}
        for i, n in enumerate(names):
            z = edges_of[n]
            out = {"feature": n, "edges": [float(v) for v in z]}
            if i in slot:
                s = slot[i]
                curve, counts, local = ale.finish(
                    interval[s], sums[s], len(z) - 1, cls_kind, float(p.cls_bias),
                    int(p.cls_n_trees), response,
                )
                rows_k = interval[s]
            else:
                curve, counts = np.zeros(1), np.array([r], dtype=np.int64)
                local, rows_k = np.zeros(r), np.zeros(r, dtype=np.int32)
            out["ale"], out["counts"] = curve, counts
            if kind == "both":
                out["interval"], out["local_effect"] = rows_k.copy(), local
            results.append(out)
        return {
            "results": results,
            "sample_rows": r,
            "output_space": "log_odds" if response == "raw" else "probability",
        }

    def _ale_gpu(self, codes: np.ndarray, nums: np.ndarray, own: bool):
        """One-launch runner of forest_ale on the device (row slice and edge
        table in, numpy (interval, sums) out); the caller holds
        _explain_lock. Tables and sample as _whatif_gpu keeps them."""
        import torch

        ext = self._gpu["ext"]
        dev = torch.device("cuda", self.device_index)
        m = self._forest_dev()
        smp = self._pdp_sample_dev if own else None
        if smp is None:
            smp = (torch.from_numpy(codes).to(dev), torch.from_numpy(nums).to(dev))
            if own:
                self._pdp_sample_dev = smp

        def run(a: int, b: int, players: np.ndarray, edge_off: np.ndarray, edges: np.ndarray):
            with torch.cuda.device(dev):
                interval, sums = ext.forest_ale(
                    smp[0][a:b],
                    smp[1][a:b],
                    m["cls_nodes"],
                    m["cls_off"],
                    m["feat_col"],
                    m["feat_code"],
                    m["medians"],
                    torch.from_numpy(np.ascontiguousarray(players, dtype=np.int32)),
                    torch.from_numpy(np.ascontiguousarray(edge_off, dtype=np.int32)),
                    torch.from_numpy(np.ascontiguousarray(edges, dtype=np.float32)),
                )
                return interval.cpu().numpy(), sums.cpu().numpy()  # D2H copies synchronize

        return run

    # ---------------------------------------------- permutation importance
    def permutation_importance(
        self,
        sample,
        labels,
        features=None,
        n_repeats: int = 5,
        scoring: str = "roc_auc",
        seed: int = 0,
        threshold: float = 0.5,
        permutations=None,
    ) -> dict:
        """Permutation feature importance of the classifier on a labelled
        sample (the estimator of sklearn.inspection.permutation_importance):
        how much a score of the model on ``labels`` drops when ONE column of
        the sample is shuffled among its rows, ``n_repeats`` shuffles per
        feature (creditcore/importance.py).

        ``sample`` is an encoded ``(codes, nums)`` pair of up to 65,536 rows,
        ``labels`` one 0/1 per row. ``features`` defaults to all 23 names.
        ``scoring`` is one of importance.SCORINGS (``threshold`` is the
        decision cut of "accuracy"). The shuffles are drawn from
        ``np.random.default_rng(seed)`` in (feature, repeat) order unless
        ``permutations`` i[n_features, n_repeats, R] gives them.

        Returns ``{"baseline_score", "results", "sample_rows", "scoring",
        "n_repeats"}``; a result holds ``feature``, ``importances``
        f64[n_repeats] (baseline minus permuted score), ``importances_mean``
        and ``importances_std`` (ddof 0). The scoring session is not touched.
        Caps (creditcore/importance.py) raise ExplainTooLarge."""
        from . import importance as imp
        from .pdp import finalize

        p = self.packed
        try:
            names = imp.parse_features(features)
            reps = imp.check_args(n_repeats, scoring)
            thr = imp.check_threshold(threshold)
            codes = np.ascontiguousarray(sample[0], dtype=np.int16)
            nums = np.ascontiguousarray(sample[1], dtype=np.float32)
            r = len(codes)
            if codes.shape != (r, N_CAT) or nums.shape != (r, N_NUM):
                raise ValueError(f"sample must be (codes [R, {N_CAT}], nums [R, {N_NUM}])")
            if r > imp.IMPORTANCE_MAX_ROWS:
                raise imp.ImportanceTooLarge(
                    f"the sample is capped at {imp.IMPORTANCE_MAX_ROWS} rows (got {r})"
                )
            y = imp.check_labels(labels, r, scoring)
            take = imp.permutation_source(permutations, seed, len(names), reps, r)
        except imp.ImportanceTooLarge as e:
            raise ExplainTooLarge(str(e)) from None
        # Table row 0 is the identity on the first feature's column (the
        # baseline: the same code path gives the unpermuted sums), then
        # n_repeats rows per feature.
        players = np.array([FEATURES.index(n) for n in names], dtype=np.int32)
        perm_player = np.concatenate([players[:1], np.repeat(players, reps)])
        scores = np.empty(len(perm_player), dtype=np.float64)
        cls_kind, n_trees = int(getattr(p, "cls_kind", 0)), int(p.cls_n_trees)
        with self._explain_lock:
            if self.device == "cuda":
                run = self._permute_gpu(codes, nums)
            else:
                nums_imp = cpu_ref.impute_nums(p, nums)

                def run(pl, pm):
                    return cpu_ref.forest_permute_cpu(p, codes, nums_imp, pl, pm)
            for a, b in imp.launch_slices(perm_player, r, self.PERM_LAUNCH_PAIRS, imp.PERM_ILP):
                perm = take(b - a) if a else np.concatenate(
                    [np.arange(r, dtype=np.int32)[None, :], take(b - 1)]
                )
                raw = run(perm_player[a:b], np.ascontiguousarray(perm, dtype=np.int32))
                prob = finalize(raw, cls_kind, float(p.cls_bias), n_trees, "probability")
                scores[a:b] = [imp.score(scoring, y, row, thr) for row in prob]
        drops = (scores[0] - scores[1:]).reshape(len(names), reps)
        return {
            "baseline_score": float(scores[0]),
            "results": [
                {
                    "feature": n,
                    "importances": d,
                    "importances_mean": float(d.mean()),
                    "importances_std": float(d.std()),
                }
                for n, d in zip(names, drops)
            ],
            "sample_rows": r,
            "scoring": scoring,
            "n_repeats": reps,
        }

    def _permute_gpu(self, codes: np.ndarray, nums: np.ndarray):
        """One-launch runner of forest_permute on the device (a slice of the
        permutation table in, numpy f64[Q, R] sums out); the caller holds
        _explain_lock. The sample is uploaded here, once per call."""
        import torch

        ext = self._gpu["ext"]
        dev = torch.device("cuda", self.device_index)
        m = self._forest_dev()
        smp = (torch.from_numpy(codes).to(dev), torch.from_numpy(nums).to(dev))

        def run(perm_player: np.ndarray, perm: np.ndarray):
            with torch.cuda.device(dev):
                out = ext.forest_permute(
                    smp[0],
                    smp[1],
                    m["cls_nodes"],
                    m["cls_off"],
                    m["feat_col"],
                    m["feat_code"],
                    m["medians"],
                    torch.from_numpy(np.ascontiguousarray(perm_player, dtype=np.int32)),
                    torch.from_numpy(perm),
                )
                return out.cpu().numpy()  # the D2H copy synchronizes

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

    # -------------------------------------------------------------- anchors
    def anchors(
        self,
        codes: np.ndarray,
        nums: np.ndarray,
        sample=None,
        precision_threshold: float = 0.95,
        beam_size: int = 2,
        max_anchor_size: int = 6,
        disc_perc=(25, 50, 75),
        threshold: float = 0.5,
    ) -> dict:
        """Anchor rules (alibi's ``AnchorTabular``): per row a small set of
        predicates on its own features, ``feature == category`` or ``lo <
        value <= hi`` (the row's interval among the sample column's
        ``disc_perc`` quantile edges), under which the classifier keeps the
        row's decision ``probability > threshold`` for at least
        ``precision_threshold`` of the sample rows, whatever their other
        features are. creditcore/anchors.py holds the definition: precision
        and coverage are exact on the sample, and a deterministic beam search
        (``beam_size`` at most 4, anchors of at most ``max_anchor_size``
        predicates) returns the widest anchor that reaches the threshold.

        ``sample`` defaults to the pack's background sample
        (ExplainUnavailable without one); ``(codes, nums)`` of up to 1,024
        rows overrides it. Each search level is one forest_anchor launch for
        all rows still searching (cpu_ref.forest_anchor_cpu on a CPU engine),
        cut at ANCHOR_LAUNCH_PAIRS. Returns ``{"rows", "precision_threshold",
        "beam_size", "sample_rows"}``; a row holds ``anchor`` (one entry per
        predicate: ``feature`` and ``category``, or ``low`` / ``high`` with
        None for an open end), ``names``, ``precision``, ``coverage``, ``met``
        (False: ``max_anchor_size`` ended the search, the best-precision
        anchor of the last level is returned), ``decision`` and
        ``probability``. The scoring session is not touched. Caps
        (creditcore/anchors.py) raise ExplainTooLarge."""
        from . import anchors as an
        from . import counterfactual as cf
        from .pdp import finalize

        p = self.packed
        try:
            prec, beam, max_size, perc = an.check_args(
                precision_threshold, beam_size, max_anchor_size, disc_perc
            )
        except an.AnchorTooLarge as e:
            raise ExplainTooLarge(str(e)) from None
        thr = cf.check_threshold(threshold)
        codes = np.ascontiguousarray(codes, dtype=np.int16)
        nums = np.ascontiguousarray(nums, dtype=np.float32)
        r = len(codes)
        if codes.shape != (r, N_CAT) or nums.shape != (r, N_NUM):
            raise ValueError(f"rows must be (codes [R, {N_CAT}], nums [R, {N_NUM}])")
        if r < 1:
            raise ValueError("anchors needs at least one row")
        if r > an.ANCHOR_MAX_ROWS:
            raise ExplainTooLarge(f"anchors is capped at {an.ANCHOR_MAX_ROWS} rows per call (got {r})")
        if sample is None:
            if p.bg_codes is None or p.bg_nums is None:
                raise ExplainUnavailable(
                    "model was packed without a background sample; re-train and "
                    "re-pack, or pass sample=(codes, nums)"
                )
            sample = (p.bg_codes, p.bg_nums)
        bg_codes = np.ascontiguousarray(sample[0], dtype=np.int16)
        bg_nums = np.ascontiguousarray(sample[1], dtype=np.float32)
        s = len(bg_codes)
        if bg_codes.shape != (s, N_CAT) or bg_nums.shape != (s, N_NUM) or s < 1:
            raise ValueError(f"sample must be (codes [S, {N_CAT}], nums [S, {N_NUM}]), S >= 1")
        if s > an.ANCHOR_MAX_SAMPLE:
            raise ExplainTooLarge(f"the sample is capped at {an.ANCHOR_MAX_SAMPLE} rows (got {s})")
        cut = cf.raw_cut(p, thr)
        nums_imp = cpu_ref.impute_nums(p, nums)
        bg_imp = cpu_ref.impute_nums(p, bg_nums)
        edges = an.disc_edges(bg_imp, perc)
        sat = an.sat_table(codes, nums_imp, bg_codes, bg_imp, edges)
        # the rows' own decisions: the scorer's tree-order sums, on the host
        # for both engines (R walks of the forest against R x S x masks)
        own_raw = cpu_ref.forest_raw_cpu(p, codes, nums_imp, tree_order=True)
        with self._explain_lock:
            if self.device == "cuda":
                launch = self._anchor_gpu(codes, nums, bg_codes, bg_nums, sat, cut)
            else:
                def launch(a, b, masks, off):
                    return cpu_ref.forest_anchor_cpu(
                        p, codes[a:b], nums_imp[a:b], bg_codes, bg_imp, sat[a:b], masks, off, cut
                    )[0]

            def run(masks: np.ndarray, mask_off: np.ndarray) -> np.ndarray:
                parts = [
                    launch(a, b, masks[mask_off[a] : mask_off[b]], mask_off[a : b + 1] - mask_off[a])
                    for a, b in an.launch_slices(mask_off, s, int(self.ANCHOR_LAUNCH_PAIRS))
                ]
                return np.concatenate(parts)

            found = an.search(run, sat, own_raw > cut, prec, beam, max_size)
        prob = finalize(
            own_raw, int(getattr(p, "cls_kind", 0)), float(p.cls_bias), int(p.cls_n_trees),
            "probability",
        )
        rows = []
        for i, (mask, hits, covered, met) in enumerate(found):
            entries, names = an.describe(mask, codes[i], nums_imp[i], edges, p.vocabs)
            rows.append(
                {
                    "anchor": entries,
                    "names": names,
                    "precision": hits / s,
                    "coverage": covered / s,
                    "met": met,
                    "decision": int(own_raw[i] > cut),
                    "probability": float(prob[i]),
                }
            )
        return {
            "rows": rows,
            "precision_threshold": prec,
            "beam_size": beam,
            "sample_rows": s,
        }

    def _anchor_gpu(self, codes, nums, bg_codes, bg_nums, sat: np.ndarray, cut: float):
        """One-launch runner of forest_anchor on the device (a row range and
        its candidate lists in, numpy counts out); the caller holds
        _explain_lock. Rows, sample and the sat table are uploaded here, once
        per call; a level uploads only its masks."""
        import torch

        ext = self._gpu["ext"]
        dev = torch.device("cuda", self.device_index)
        m = self._forest_dev()
        up = [
            torch.from_numpy(a).to(dev)
            for a in (codes, nums, bg_codes, bg_nums, np.ascontiguousarray(sat).view(np.int32))
        ]

        def run(a: int, b: int, masks: np.ndarray, mask_off: np.ndarray) -> np.ndarray:
            with torch.cuda.device(dev):
                counts, _ = ext.forest_anchor(
                    up[0][a:b],
                    up[1][a:b],
                    up[2],
                    up[3],
                    m["cls_nodes"],
                    m["cls_off"],
                    m["feat_col"],
                    m["feat_code"],
                    m["medians"],
                    up[4][a:b],
                    torch.from_numpy(np.ascontiguousarray(masks, dtype=np.uint32).view(np.int32)),
                    torch.from_numpy(np.ascontiguousarray(mask_off, dtype=np.int32)),
                    float(cut),
                )
                return counts.cpu().numpy()  # the D2H copy synchronizes

        return run

    def anchors_records(self, records, sample=None, **kw) -> dict:
        """anchors on a request body (list of dicts / DataFrame); ``sample``
        likewise, encoded with the same vocabulary."""
        codes, nums = encode_batch(records, self.packed.vocabs)
        if sample is not None:
            sample = encode_batch(sample, self.packed.vocabs)
        return self.anchors(codes, nums, sample=sample, **kw)

    # ------------------------------------------------------------ MMD drift
    def mmd_drift(
        self,
        codes: np.ndarray,
        nums: np.ndarray,
        reference=None,
        n_permutations: int = 100,
        seed: int = 0,
        cols_per_block: int | None = None,
    ) -> dict:
        """Multivariate drift of a batch against a reference sample: the
        unbiased MMD^2 of whole embedded rows under one RBF kernel (median
        heuristic on the reference), with a permutation p-value
        (creditcore/mmd.py holds the exact statistic). Independent of the
        classifier; one test, so the pack's ``drift_p_val`` is used with no
        Bonferroni correction.

        ``reference`` defaults to the pack's background sample
        (ExplainUnavailable without one); ``(codes, nums)`` overrides it. The
        heavy product W = K . ind runs in mmd_perm_kernel on a GPU engine and
        in cpu_ref.mmd_perm_w_cpu on a CPU engine; everything else is shared
        host code. Returns ``mmd2``, ``p_val``, ``is_drift``, ``threshold``
        (the pack's drift_p_val), ``distance_threshold``, ``gamma``, ``n``,
        ``n_ref``, ``n_permutations``. The scoring session is not touched.
        Caps (creditcore/mmd.py) raise ExplainTooLarge; an infinite numeric,
        or rows whose embedding or squared norm is not finite in f32, raise
        ValueError naming the side (NaN numerics are imputed)."""
        from . import mmd

        p = self.packed
        n_perm = mmd.check_permutations(n_permutations)
        codes, nums = mmd.check_rows(codes, nums, "batch")
        if len(codes) > mmd.MMD_MAX_ROWS:
            raise ExplainTooLarge(
                f"mmd_drift is capped at {mmd.MMD_MAX_ROWS} batch rows (got {len(codes)})"
            )
        if reference is None:
            if p.bg_codes is None or p.bg_nums is None:
                raise ExplainUnavailable(
                    "model was packed without a background sample; re-train and "
                    "re-pack, or pass reference=(codes, nums)"
                )
            reference = (p.bg_codes, p.bg_nums)
        ref_codes, ref_nums = mmd.check_rows(reference[0], reference[1], "reference")
        if len(ref_codes) > mmd.MMD_MAX_REFERENCE:
            raise ExplainTooLarge(
                f"mmd_drift is capped at {mmd.MMD_MAX_REFERENCE} reference rows "
                f"(got {len(ref_codes)})"
            )
        n, m = len(codes), len(ref_codes)
        with self._explain_lock:
            mu, sd, z_ref, gamma = self._mmd_reference(ref_codes, ref_nums)
            z_batch = mmd.check_embedding(mmd.embed(p, codes, nums, mu, sd), "batch")
            z = np.concatenate([z_batch, z_ref])
            ind = mmd.indicator(n, m, n_perm, int(seed))
            w = self._mmd_w(z, gamma, ind, cols_per_block)
        out = mmd.decide(mmd.statistics(w, ind, n, m), float(p.drift_p_val))
        out.update(gamma=gamma, n=n, n_ref=m, n_permutations=n_perm)
        return out

    def _mmd_reference(self, ref_codes: np.ndarray, ref_nums: np.ndarray):
        """(mu, sd, z_ref, gamma) of a reference sample, kept for the last
        sample seen; the caller holds _explain_lock."""
        import hashlib

        from . import mmd

        key = hashlib.sha1(ref_codes.tobytes() + ref_nums.tobytes()).digest()
        if self._mmd_ref is None or self._mmd_ref[0] != key:
            mu, sd = mmd.reference_scale(self.packed, ref_nums)
            z_ref = mmd.embed(self.packed, ref_codes, ref_nums, mu, sd)
            mmd.check_embedding(z_ref, "reference")  # before it can be cached
            self._mmd_ref = (key, mu, sd, z_ref, mmd.median_gamma(z_ref))
        return self._mmd_ref[1:]

    def _mmd_w(self, z: np.ndarray, gamma: float, ind: np.ndarray, cols_per_block=None):
        """W = K . ind f64[N, Q] on this engine's device."""
        from . import mmd

        if self.device != "cuda":
            return cpu_ref.mmd_perm_w_cpu(z, gamma, ind)
        import torch

        from .ops import gpu

        dev = torch.device("cuda", self.device_index)
        norms = mmd.squared_norms(z).astype(np.float32)
        cols = int(cols_per_block or mmd.default_cols_per_block(len(z)))
        with torch.cuda.device(dev):
            return gpu.mmd_perm_w(
                torch.from_numpy(mmd.pad_columns(z)).to(dev),
                torch.from_numpy(norms).to(dev),
                gamma,
                torch.from_numpy(ind).to(dev),
                cols,
                launch_rows=int(self.MMD_LAUNCH_ROWS),
            )

    def mmd_drift_records(self, records, reference=None, **kw) -> dict:
        """mmd_drift on a request body (list of dicts / DataFrame);
        ``reference`` likewise, encoded with the same vocabulary."""
        codes, nums = encode_batch(records, self.packed.vocabs)
        if reference is not None:
            reference = encode_batch(reference, self.packed.vocabs)
        return self.mmd_drift(codes, nums, reference=reference, **kw)

    # ------------------------------------------------- nearest-neighbour outliers
    def knn_outliers(
        self,
        codes: np.ndarray,
        nums: np.ndarray,
        reference=None,
        k: int = 10,
        score: str = "kth",
        fpr: float = 0.05,
        neighbors: bool = False,
        cols_per_block: int | None = None,
    ) -> dict:
        """Nearest-neighbour outlier scores of a batch against a reference
        sample (alibi-detect's ``KNN``; creditcore/knn.py holds the
        definition): ``instance_score`` is the distance to the k-th nearest
        reference row in the MMD embedding (``score="mean"``: the mean of the
        k distances), ``threshold`` the ``1 - fpr`` quantile of the
        reference's own leave-one-out scores, ``is_outlier`` their comparison.
        Independent of the classifier and of the isolation forest behind
        /predict's ``outliers`` field.

        ``reference`` defaults to the pack's background sample
        (ExplainUnavailable without one); ``(codes, nums)`` overrides it. The
        neighbour search runs in knn_topk_kernel on a GPU engine and in
        cpu_ref.knn_topk_cpu on a CPU engine; everything else is shared host
        code. Returns ``instance_score`` f64[B], ``is_outlier`` i8[B],
        ``threshold``, ``k``, ``score``, ``fpr``, ``n``, ``n_ref`` and, with
        ``neighbors=True``, ``neighbor_index`` i32[B, k] (row numbers of the
        reference sample, nearest first, ties to the lower row) and
        ``neighbor_distance`` f64[B, k]. The scoring session is not touched.
        Caps (creditcore/knn.py) raise ExplainTooLarge; bad arguments and
        rows that do not embed to finite f32 values raise ValueError."""
        from . import knn, mmd

        p = self.packed
        codes, nums = mmd.check_rows(codes, nums, "batch", 1, "knn_outliers")
        if len(codes) > knn.KNN_MAX_ROWS:
            raise ExplainTooLarge(
                f"knn_outliers is capped at {knn.KNN_MAX_ROWS} batch rows (got {len(codes)})"
            )
        if reference is None:
            if p.bg_codes is None or p.bg_nums is None:
                raise ExplainUnavailable(
                    "model was packed without a background sample; re-train and "
                    "re-pack, or pass reference=(codes, nums)"
                )
            reference = (p.bg_codes, p.bg_nums)
        ref_codes, ref_nums = mmd.check_rows(
            reference[0], reference[1], "reference", 2, "knn_outliers"
        )
        if len(ref_codes) > knn.KNN_MAX_REFERENCE:
            raise ExplainTooLarge(
                f"knn_outliers is capped at {knn.KNN_MAX_REFERENCE} reference rows "
                f"(got {len(ref_codes)})"
            )
        k, score, fpr = knn.check_args(k, score, fpr, len(ref_codes))
        with self._explain_lock:
            ref = self._knn_reference(ref_codes, ref_nums, k, cols_per_block)
            z_batch = mmd.check_embedding(
                mmd.embed(p, codes, nums, ref["mu"], ref["sd"]), "batch"
            )
            d2, idx = self._knn_topk(z_batch, ref, k, False, cols_per_block)
        return knn.result(d2, idx, ref["loo_d2"], k, score, fpr, bool(neighbors))

    def _knn_reference(self, ref_codes, ref_nums, k: int, cols_per_block=None) -> dict:
        """Embedding, device copy and leave-one-out neighbour distances of a
        reference sample, kept for the last (sample, k) seen; the caller
        holds _explain_lock."""
        import hashlib

        from . import mmd

        key = (hashlib.sha1(ref_codes.tobytes() + ref_nums.tobytes()).digest(), k)
        if self._knn_ref is None or self._knn_ref["key"] != key:
            mu, sd = mmd.reference_scale(self.packed, ref_nums)
            z_ref = mmd.embed(self.packed, ref_codes, ref_nums, mu, sd)
            mmd.check_embedding(z_ref, "reference")  # before it can be cached
            ref = {"key": key, "mu": mu, "sd": sd, "z": z_ref}
            if self.device == "cuda":
                ref["dev"] = self._knn_upload(z_ref)
            ref["loo_d2"], _ = self._knn_topk(z_ref, ref, k, True, cols_per_block)
            self._knn_ref = ref
        return self._knn_ref

    def _knn_upload(self, z: np.ndarray):
        """(z padded to the kernel's float4 columns, squared norms) on this
        engine's device; the norms are f64 sums rounded once to f32."""
        import torch

        from . import mmd

        dev = torch.device("cuda", self.device_index)
        return (
            torch.from_numpy(mmd.pad_columns(z)).to(dev),
            torch.from_numpy(mmd.squared_norms(z).astype(np.float32)).to(dev),
        )

    def _knn_topk(self, z_batch, ref: dict, k: int, exclude_self: bool, cols_per_block=None):
        """(d2 f64[B, k], idx i32[B, k]) of z_batch against the reference on
        this engine's device; with exclude_self z_batch is the reference."""
        if self.device != "cuda":
            return cpu_ref.knn_topk_cpu(z_batch, ref["z"], k, exclude_self)
        import torch

        from .ops import gpu

        zr, nr = ref["dev"]
        zb, nb = (zr, nr) if exclude_self else self._knn_upload(z_batch)
        with torch.cuda.device(torch.device("cuda", self.device_index)):
            d2, idx = gpu.knn_topk(
                zb, zr, nb, nr, k, exclude_self,
                cols_per_block=int(cols_per_block or 0),
                launch_rows=int(self.KNN_LAUNCH_ROWS),
            )
        return d2.astype(np.float64), idx

    def knn_outliers_records(self, records, reference=None, **kw) -> dict:
        """knn_outliers on a request body (list of dicts / DataFrame);
        ``reference`` likewise, encoded with the same vocabulary."""
        codes, nums = encode_batch(records, self.packed.vocabs)
        if reference is not None:
            reference = encode_batch(reference, self.packed.vocabs)
        return self.knn_outliers(codes, nums, reference=reference, **kw)

    # ------------------------------------------------------- forest proximity
    def proximity(
        self,
        codes: np.ndarray,
        nums: np.ndarray,
        reference=None,
        k: int = 10,
        score: str = "kth",
        fpr: float = 0.05,
        neighbors: bool = True,
    ) -> dict:
        """Breiman's forest proximity of a batch against a reference sample
        (creditcore/proximity.py holds the definition): the proximity of two
        rows is the share of the classifier's trees in which they end in the
        same leaf. Per batch row the k reference rows of highest proximity,
        ``instance_score`` = 1 - the proximity of the k-th (``score="mean"``:
        1 - the mean of the k), ``threshold`` the ``1 - fpr`` quantile of the
        reference's own leave-one-out scores, ``is_outlier`` their comparison.

        ``reference`` defaults to the pack's background sample
        (ExplainUnavailable without one); ``(codes, nums)`` overrides it.
        Leaves and neighbours come from forest_leaf_kernel and
        forest_prox_topk_kernel on a GPU engine, from cpu_ref.forest_leaves_cpu
        and cpu_ref.forest_prox_topk_cpu on a CPU engine; both are integer, so
        the engines agree exactly. Returns ``instance_score`` f64[B],
        ``is_outlier`` i8[B], ``threshold``, ``k``, ``score``, ``fpr``, ``n``,
        ``n_ref``, ``n_trees`` and, with ``neighbors``, ``neighbor_index``
        i32[B, k] (row numbers of the reference sample, closest first, ties
        to the lower row) and ``neighbor_proximity`` f64[B, k]. The scoring
        session is not touched. Caps (creditcore/proximity.py) raise
        ExplainTooLarge; bad arguments raise ValueError."""
        from . import proximity as px

        p = self.packed
        codes, nums = px.check_rows(codes, nums, "batch", 1)
        if len(codes) > px.PROX_MAX_ROWS:
            raise ExplainTooLarge(
                f"proximity is capped at {px.PROX_MAX_ROWS} batch rows (got {len(codes)})"
            )
        if p.cls_n_trees > px.PROX_MAX_TREES:
            raise ExplainTooLarge(
                f"proximity is capped at {px.PROX_MAX_TREES} trees (the model has {p.cls_n_trees})"
            )
        if reference is None:
            if p.bg_codes is None or p.bg_nums is None:
                raise ExplainUnavailable(
                    "model was packed without a background sample; re-train and "
                    "re-pack, or pass reference=(codes, nums)"
                )
            reference = (p.bg_codes, p.bg_nums)
        ref_codes, ref_nums = px.check_rows(reference[0], reference[1], "reference", 2)
        if len(ref_codes) > px.PROX_MAX_REFERENCE:
            raise ExplainTooLarge(
                f"proximity is capped at {px.PROX_MAX_REFERENCE} reference rows "
                f"(got {len(ref_codes)})"
            )
        k, score, fpr = px.check_args(k, score, fpr, len(ref_codes))
        with self._explain_lock:
            ref = self._prox_reference(ref_codes, ref_nums, k)
            count, idx = self._prox_topk(self._prox_leaves(codes, nums), ref, k, False)
        return px.result(
            count, idx, ref["loo_count"], p.cls_n_trees, k, score, fpr, bool(neighbors)
        )

    def _prox_reference(self, ref_codes, ref_nums, k: int) -> dict:
        """Leaf table, inverted index (GPU) and leave-one-out counts of a
        reference sample, kept for the last (sample, k) seen; the caller
        holds _explain_lock."""
        import hashlib

        key = (hashlib.sha1(ref_codes.tobytes() + ref_nums.tobytes()).digest(), k)
        if self._prox_ref is None or self._prox_ref["key"] != key:
            leaf = self._prox_leaves(ref_codes, ref_nums)
            ref = {"key": key, "leaf": leaf}
            if self.device == "cuda":
                from .ops import gpu

                ref["index"] = gpu.prox_index(leaf, len(self.packed.cls_nodes))
            ref["loo_count"], _ = self._prox_topk(leaf, ref, k, True)
            self._prox_ref = ref
        return self._prox_ref

    def _prox_leaves(self, codes: np.ndarray, nums: np.ndarray):
        """leaf[R, T] of the rows on this engine's device (numpy on a CPU
        engine, a device tensor on a GPU engine); the caller holds
        _explain_lock."""
        if self.device != "cuda":
            return cpu_ref.forest_leaves_cpu(
                self.packed, codes, cpu_ref.impute_nums(self.packed, nums)
            )
        import torch

        from .ops import gpu

        dev = torch.device("cuda", self.device_index)
        m = self._forest_dev()
        with torch.cuda.device(dev):
            return gpu.forest_leaves(
                torch.from_numpy(codes).to(dev), torch.from_numpy(nums).to(dev), m
            )

    def _prox_topk(self, leaf_batch, ref: dict, k: int, exclude_self: bool):
        """(count i32[B, k], idx i32[B, k]) of the batch's leaf table against
        the reference on this engine's device."""
        if self.device != "cuda":
            return cpu_ref.forest_prox_topk_cpu(leaf_batch, ref["leaf"], k, exclude_self)
        import torch

        from .ops import gpu

        with torch.cuda.device(torch.device("cuda", self.device_index)):
            return gpu.forest_prox_topk(
                leaf_batch, ref["index"], k, exclude_self,
                launch_rows=int(self.PROX_LAUNCH_ROWS),
            )

    def proximity_records(self, records, reference=None, **kw) -> dict:
        """proximity on a request body (list of dicts / DataFrame);
        ``reference`` likewise, encoded with the same vocabulary."""
        codes, nums = encode_batch(records, self.packed.vocabs)
        if reference is not None:
            reference = encode_batch(reference, self.packed.vocabs)
        return self.proximity(codes, nums, reference=reference, **kw)

    def permutation_importance_records(self, records, labels, **kw) -> dict:
        """permutation_importance on a request body (list of dicts /
        DataFrame) and its labels."""
        return self.permutation_importance(
            encode_batch(records, self.packed.vocabs), labels, **kw
        )

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

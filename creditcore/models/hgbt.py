"""Histogram gradient-boosted trees trained on the MI355X.

``HistGBTClassifier`` is a LightGBM / XGBoost-``hist`` style trainer for
binary log-loss with second-order (Newton) leaves. Trees grow level by level
from three primitives,

    hist   per-(open node, bin) sums of the quantised gradients
    split  best (gain, feature, bin) per open node
    route  rows move to their child node or leaf

which run as HIP kernels (csrc/creditcore_kernels.hip, hgbt_*_kernel) on
``device="cuda"`` and as the numpy references of ops/cpu_ref.py on
``device="cpu"``. The two are specified to build identical trees from
identical integer inputs:

- Features are binned once on the host into u8 bins from f32 edges,
  ``bin(x) = #{edges < x}``, so "bin <= b goes left" is exactly
  ``x <= edges[b]`` for every f32 x and ``edges[b]`` is the packed threshold.
  Columns with at most ``max_bins`` distinct values get the midpoints
  between them as edges (a one-hot column: 2 bins, edge 0.5), the others
  ``max_bins`` quantile bins. The layout is ragged: feature f owns bins
  ``bin_off[f]:bin_off[f+1]``.
- Gradients g = p - y and hessians h = p(1 - p) are quantised to int32 fixed
  point, rint(g * 2^20). Histogram sums are int64 and therefore independent
  of the order atomics land in.
- gain = GL^2/(HL+l2) + GR^2/(HR+l2) - G^2/(H+l2) in f64 from the integer
  sums, one fixed operation order, no FMA contraction. A split needs
  ``min_samples_leaf`` rows on both sides and gain > 0; ties go to the
  highest gain, then the lowest feature, then the lowest bin.
- leaf = -G/(H+l2) * learning_rate in f64, rounded to f32; it is computed on
  the host from the integer sums for both devices.

Monotone constraints (``monotone_cst``: a sign in {-1, 0, +1} per encoded
column) use the bounds propagation of XGBoost-hist, LightGBM "basic" and
sklearn. Every open node carries f64 leaf-weight bounds [lo, hi], the root
[-inf, +inf]. With g = G 2^-20 and d = H 2^-20 + l2,

- a side takes w = min(max(-g/d, lo), hi) and scores s = -((2g)w + (dw)w);
  gain = (s_L + s_R) - s_P with left, right and parent all clamped to the
  node's bounds (one fixed operation order, no FMA contraction);
- a split also needs d_L > 0, d_R > 0 and, on a +1 column, w_L <= w_R
  (w_L >= w_R on a -1 column); ties break as above;
- with mid = (w_L + w_R)/2 the children of a +1 split get [lo, mid] (left)
  and [mid, hi] (right), of a -1 split [mid, hi] and [lo, mid]; a split on an
  unconstrained column hands [lo, hi] to both. The bounds are computed on the
  host from the split record's integer sums for both devices;
- leaf = clamp(-g/d, lo, hi) * learning_rate in f64, rounded to f32. Rounding
  and a positive rate keep the order, so every leaf under the lower child is
  <= every leaf under the upper one exactly and the f64 sum over the trees is
  monotone in the column.

The search runs in hgbt_split_mono_kernel / cpu_ref.hgbt_split_mono_cpu.
Without a non-zero sign the plain kernel and formula above run, so
unconstrained models do not change. ``verify_monotone`` checks a fitted model.

Limits: binary targets, ``max_depth <= 12``, ``max_bins <= 256``, no row or
column subsampling, no native categorical splits (one-hot columns are
ordinary 2-bin features, which a sign may not order usefully), no
missing-value direction (the pipeline imputes first). ``random_state`` is
accepted for pipeline compatibility; training is deterministic without it.

The fitted state is plain numpy (sklearn-``tree_``-like flat arrays for all
trees plus ``tree_offsets_``), so the estimator pickles without tensors and
``pack.pack_classifier_pipeline`` turns it into the node-SoA the serving
kernels read (``cls_kind = 1``).
"""

from __future__ import annotations

import numpy as np
from sklearn.base import BaseEstimator, ClassifierMixin

MAX_DEPTH = 12
MAX_BINS = 256
SHIFT = 20  # fractional bits of the fixed-point gradients (cpu_ref.HGBT_SHIFT)
LDS_BUDGET_BYTES = 64 * 1024  # per-block histogram slab; 2 blocks per CU
TARGET_BLOCKS = 1024  # histogram grid size aimed at when rows are few


def _to_dense_f32(x) -> np.ndarray:
    """The serving kernels see f32 features: train on exactly those."""
    if hasattr(x, "toarray"):  # scipy sparse from the ColumnTransformer
        x = x.toarray()
    x = np.asarray(x)
    if x.ndim != 2:
        raise ValueError("expected a 2-D feature matrix")
    return np.ascontiguousarray(x, dtype=np.float32)


def _column_edges(col: np.ndarray, max_bins: int) -> np.ndarray:
    """f32 bin edges of one column (ascending, at most max_bins - 1)."""
    lo, hi = col.min(), col.max()
    if lo == hi:
        return np.zeros(0, dtype=np.float32)
    if np.all((col == lo) | (col == hi)):  # binary (one-hot) fast path
        distinct = np.asarray([lo, hi], dtype=np.float32)
        srt = None
    else:
        srt = np.sort(col)
        distinct = srt[np.concatenate([[True], srt[1:] != srt[:-1]])]
    if len(distinct) <= max_bins:
        a, b = distinct[:-1], distinct[1:]
        mid = ((a.astype(np.float64) + b.astype(np.float64)) * 0.5).astype(np.float32)
        # adjacent floats: the rounded midpoint may land on b; a itself splits
        return np.where(mid >= b, a, mid).astype(np.float32)
    n = len(srt)
    pos = (np.arange(1, max_bins, dtype=np.int64) * n) // max_bins
    cand = np.unique(srt[pos])
    return cand[cand < hi].astype(np.float32)


def bin_features(x: np.ndarray, max_bins: int = MAX_BINS):
    """Bin a dense f32 matrix [N, F].

    Returns (bins u8[F, N] feature-major, bin_off i32[F+1],
    bin_threshold f32[total_bins]); ``bin_threshold[bin_off[f] + b]`` is the
    f32 edge e with {bin <= b} == {x <= e} (+inf for a feature's last bin)."""
    n, n_feat = x.shape
    bins = np.empty((n_feat, n), dtype=np.uint8)
    bin_off = np.zeros(n_feat + 1, dtype=np.int32)
    thr = []
    for f in range(n_feat):
        col = np.ascontiguousarray(x[:, f])
        edges = _column_edges(col, max_bins)
        bins[f] = np.searchsorted(edges, col, side="left")
        bin_off[f + 1] = bin_off[f] + len(edges) + 1
        thr.append(edges)
        thr.append(np.asarray([np.inf], dtype=np.float32))
    return bins, bin_off, np.concatenate(thr).astype(np.float32)


class _CpuBackend:
    """The three level primitives as numpy references (ops/cpu_ref.py)."""

    def __init__(self, bins: np.ndarray, bin_off: np.ndarray):
        from ..ops import cpu_ref

        self._ref = cpu_ref
        self.bins, self.bin_off = bins, bin_off
        self.n_rows = bins.shape[1]

    def new_nodes(self):
        return np.zeros(self.n_rows, dtype=np.int32)

    def hist(self, node, gq, hq, n_nodes):
        return self._ref.hgbt_hist_cpu(self.bins, self.bin_off, node, gq, hq, n_nodes)

    def split(self, hist, lam, min_leaf) -> np.ndarray:
        return self._ref.hgbt_split_cpu(hist, self.bin_off, lam, min_leaf)

    def split_mono(self, hist, lam, min_leaf, mono, bounds) -> np.ndarray:
        return self._ref.hgbt_split_mono_cpu(hist, self.bin_off, lam, min_leaf, mono, bounds)

    def route(self, node, table):
        return self._ref.hgbt_route_cpu(self.bins, table, node)


def plan_feature_groups(
    n_bins: np.ndarray, n_nodes: int, lds_bytes: int, max_feats: int, planes: int = 3
) -> tuple[np.ndarray, int]:
    """Feature groups of one histogram launch (grid.y) and the int32 entry
    count of the largest group's LDS slab, n_nodes * planes * group bins
    (3 planes here; models/hrf.py plans its 2-plane histogram with this too).

    Consecutive features are packed while the slab stays within ``lds_bytes``
    and the group within ``max_feats`` features. A level whose single widest
    feature does not fit gets slab 0: the direct-global path."""
    per_bin = int(planes) * int(n_nodes)
    cap = lds_bytes // 4
    fits = per_bin * int(n_bins.max()) <= cap
    off, cur_bins, cur_feats, widest = [0], 0, 0, 0
    for f, nb in enumerate(int(b) for b in n_bins):
        full = cur_feats >= max_feats or (fits and per_bin * (cur_bins + nb) > cap)
        if cur_feats and full:
            off.append(f)
            cur_bins = cur_feats = 0
        cur_bins += nb
        cur_feats += 1
        widest = max(widest, cur_bins)
    off.append(len(n_bins))
    return np.asarray(off, dtype=np.int32), (per_bin * widest if fits else 0)


class _GpuBackend:
    """The three level primitives as HIP kernels over torch tensors."""

    def __init__(self, bins: np.ndarray, bin_off: np.ndarray, ext, device):
        import torch

        self._torch, self._ext, self.device = torch, ext, device
        self.n_rows = bins.shape[1]
        self.n_bins = np.diff(bin_off)
        self.total_bins = int(bin_off[-1])
        self.bins = torch.from_numpy(bins).to(device)
        self.bin_off = torch.from_numpy(bin_off).to(device)
        self.rows_per_block = int(ext.HGBT_MAX_ROWS_PER_BLOCK)
        self.lds_bytes = LDS_BUDGET_BYTES
        self._groups: dict = {}
        self._mono = None

    def new_nodes(self):
        return self._torch.zeros(self.n_rows, dtype=self._torch.int32, device=self.device)

    def _plan(self, n_nodes: int):
        plan = self._groups.get(n_nodes)
        if plan is None:
            row_blocks = max(1, -(-self.n_rows // self.rows_per_block))
            want = max(1, -(-TARGET_BLOCKS // row_blocks))
            max_feats = max(1, -(-len(self.n_bins) // want))
            off, entries = plan_feature_groups(
                self.n_bins, n_nodes, self.lds_bytes, max_feats
            )
            plan = (self._torch.from_numpy(off).to(self.device), entries)
            self._groups[n_nodes] = plan
        return plan

    def hist(self, node, gq, hq, n_nodes):
        grp_off, entries = self._plan(n_nodes)
        return self._ext.hgbt_hist(
            self.bins, self.bin_off, grp_off, node, gq, hq,
            n_nodes, self.total_bins, entries, self.rows_per_block,
        )

    def split(self, hist, lam, min_leaf) -> np.ndarray:
        # the only per-level traffic back to the host: <= 2^depth records
        return self._ext.hgbt_split(hist, self.bin_off, lam, min_leaf).cpu().numpy()

    def split_mono(self, hist, lam, min_leaf, mono, bounds) -> np.ndarray:
        if self._mono is None or self._mono[0] is not mono:  # one upload per fit
            self._mono = (mono, self._torch.from_numpy(mono).to(self.device))
        return self._ext.hgbt_split_mono(
            hist, self.bin_off, lam, min_leaf, self._mono[1],
            self._torch.from_numpy(bounds).to(self.device),
        ).cpu().numpy()

    def route(self, node, table):
        self._ext.hgbt_route(self.bins, self._torch.from_numpy(table).to(self.device), node)
        return node


def _leaf_values(g_sum: np.ndarray, h_sum: np.ndarray, lam: float, lr: float) -> np.ndarray:
    """Newton leaf -G/(H+l2) * lr in f64 from the integer sums, then f32."""
    sc = 1.0 / float(1 << SHIFT)
    g = g_sum.astype(np.float64) * sc
    den = h_sum.astype(np.float64) * sc + lam
    v = np.zeros(len(g), dtype=np.float64)
    np.divide(-g, den, out=v, where=den > 0.0)
    return (v * lr).astype(np.float32)


def _bounded_weights(g_sum, h_sum, lam: float, lo, hi) -> np.ndarray:
    """clamp(-G/(H+l2), lo, hi) in f64 from the integer sums: the weight the
    constrained split search gives a side (0 before the clamp when the
    denominator is not positive, like ``_leaf_values``)."""
    from ..ops.cpu_ref import hgbt_mono_weight

    sc = 1.0 / float(1 << SHIFT)
    g = g_sum.astype(np.float64) * sc
    den = h_sum.astype(np.float64) * sc + lam
    ok = den > 0.0
    w = hgbt_mono_weight(np.where(ok, g, 0.0), np.where(ok, den, 1.0), lo, hi)
    return np.asarray(w, dtype=np.float64)


def _child_bounds(sign, w_l, w_r, lo, hi) -> np.ndarray:
    """f64[n, 2, 2] bounds of the (left, right) children of n splits: a signed
    split cuts the parent's [lo, hi] at mid = (w_L + w_R)/2, an unsigned one
    hands it down."""
    mid = (w_l + w_r) / 2.0
    out = np.empty((len(mid), 2, 2), dtype=np.float64)
    out[:, 0, 0] = np.where(sign < 0, mid, lo)
    out[:, 0, 1] = np.where(sign > 0, mid, hi)
    out[:, 1, 0] = np.where(sign > 0, mid, lo)
    out[:, 1, 1] = np.where(sign < 0, mid, hi)
    return out


def grow_tree(
    backend,
    gq,
    hq,
    bin_off: np.ndarray,
    bin_threshold: np.ndarray,
    max_depth: int,
    lam: float,
    min_leaf: int,
    lr: float,
    mono: np.ndarray | None = None,
):
    """Grow one tree level by level on ``backend`` from the int32 gradients.

    ``mono`` (i32 per column, at least one non-zero sign) switches to the
    constrained split search and carries a [lo, hi] weight-bounds row for
    every open slot alongside ``active``; ``None`` is the plain trainer.

    Returns (tree, node): ``tree`` holds sklearn-style flat arrays
    (children_left/right, feature, threshold f32, value f32, cover i64) in
    creation order, which is breadth-first; ``node`` is the backend's per-row
    id array, every entry now -(leaf node + 1)."""
    cap = 2 ** (max_depth + 1) - 1
    cl = np.full(cap, -1, dtype=np.int32)
    cr = np.full(cap, -1, dtype=np.int32)
    feature = np.full(cap, -2, dtype=np.int32)
    threshold = np.full(cap, -2.0, dtype=np.float32)
    value = np.zeros(cap, dtype=np.float32)
    cover = np.zeros(cap, dtype=np.int64)
    n_used = 1
    node = backend.new_nodes()
    active = np.zeros(1, dtype=np.int64)  # tree node id of every open slot
    bounds = np.asarray([[-np.inf, np.inf]])  # [lo, hi] of every open slot (mono)
    for depth in range(max_depth):
        k = len(active)
        hist = backend.hist(node, gq, hq, k)
        if mono is None:
            rec = backend.split(hist, lam, min_leaf)
        else:
            rec = backend.split_mono(hist, lam, min_leaf, mono, bounds)
        feat, bin_ = rec[:, 1], rec[:, 2]
        g_l, h_l, c_l = rec[:, 3], rec[:, 4], rec[:, 5]
        g_t, h_t, c_t = rec[:, 6], rec[:, 7], rec[:, 8]
        if depth == 0:  # children get their sums from the parent's record
            cover[0] = c_t[0]
            if mono is None:
                value[0] = _leaf_values(g_t, h_t, lam, lr)[0]
            else:
                w = _bounded_weights(g_t, h_t, lam, bounds[:, 0], bounds[:, 1])
                value[0] = (w * lr).astype(np.float32)[0]
        split = feat >= 0
        ns = int(split.sum())
        table = np.zeros((k, 4), dtype=np.int32)
        closed = -(active[~split] + 1)
        table[~split, 0] = -1
        table[~split, 2] = closed
        table[~split, 3] = closed
        if ns:
            parent = active[split]
            left = n_used + 2 * np.arange(ns, dtype=np.int64)
            n_used += 2 * ns
            cl[parent], cr[parent] = left, left + 1
            feature[parent] = feat[split]
            threshold[parent] = bin_threshold[bin_off[feat[split]] + bin_[split]]
            child = np.stack([left, left + 1], axis=1).ravel()
            c_g = np.stack([g_l[split], (g_t - g_l)[split]], axis=1).ravel()
            c_h = np.stack([h_l[split], (h_t - h_l)[split]], axis=1).ravel()
            c_c = np.stack([c_l[split], (c_t - c_l)[split]], axis=1).ravel()
            cover[child] = c_c
            if mono is None:
                value[child] = _leaf_values(c_g, c_h, lam, lr)
            else:
                lo, hi = bounds[split, 0], bounds[split, 1]
                w_l = _bounded_weights(c_g[0::2], c_h[0::2], lam, lo, hi)
                w_r = _bounded_weights(c_g[1::2], c_h[1::2], lam, lo, hi)
                c_b = _child_bounds(mono[feat[split]], w_l, w_r, lo, hi).reshape(-1, 2)
                w = _bounded_weights(c_g, c_h, lam, c_b[:, 0], c_b[:, 1])
                value[child] = (w * lr).astype(np.float32)
            # a child stays open while it may still split
            is_open = (c_c >= 2 * min_leaf) if depth + 1 < max_depth else np.zeros(
                2 * ns, dtype=bool
            )
            code = np.where(is_open, np.cumsum(is_open) - 1, -(child + 1))
            table[split, 0] = feat[split]
            table[split, 1] = bin_[split]
            table[split, 2] = code[0::2]
            table[split, 3] = code[1::2]
            active = child[is_open]
            if mono is not None:
                bounds = np.ascontiguousarray(c_b[is_open])
        else:
            active = np.zeros(0, dtype=np.int64)
        node = backend.route(node, table)
        if not len(active):
            break
    tree = {
        "children_left": cl[:n_used].copy(),
        "children_right": cr[:n_used].copy(),
        "feature": feature[:n_used].copy(),
        "threshold": threshold[:n_used].copy(),
        "value": value[:n_used].copy(),
        "cover": cover[:n_used].copy(),
    }
    return tree, node


_TREE_KEYS = ("children_left", "children_right", "feature", "threshold", "value", "cover")


class HistGBTClassifier(ClassifierMixin, BaseEstimator):
    """Histogram gradient-boosted trees, binary log-loss (module docstring).

    ``device``: "cuda" trains with the HIP kernels, "cpu" with the numpy
    references, "auto" takes the GPU when one is visible; with a visible GPU
    and no extension it raises ``ExtensionMissing`` and never falls back."""

    def __init__(
        self,
        n_estimators=100,
        max_depth=6,
        learning_rate=0.1,
        max_bins=MAX_BINS,
        l2=1.0,
        min_samples_leaf=20,
        random_state=None,
        device="auto",
        monotone_cst=None,
    ):
        self.n_estimators = n_estimators
        self.max_depth = max_depth
        self.learning_rate = learning_rate
        self.max_bins = max_bins
        self.l2 = l2
        self.min_samples_leaf = min_samples_leaf
        self.random_state = random_state
        self.device = device
        self.monotone_cst = monotone_cst

    # -- training ----------------------------------------------------------
    def _check_params(self):
        if not 1 <= int(self.max_depth) <= MAX_DEPTH:
            raise ValueError(f"max_depth must be in [1, {MAX_DEPTH}]")
        if not 2 <= int(self.max_bins) <= MAX_BINS:
            raise ValueError(f"max_bins must be in [2, {MAX_BINS}]")
        if int(self.n_estimators) < 1:
            raise ValueError("n_estimators must be >= 1")
        if int(self.min_samples_leaf) < 1:
            raise ValueError("min_samples_leaf must be >= 1")
        if not float(self.l2) >= 0.0:
            raise ValueError("l2 must be >= 0")
        if self.device not in ("auto", "cpu", "cuda"):
            raise ValueError("device must be 'auto', 'cpu' or 'cuda'")

    def _resolve_monotone(self, n_feat: int) -> np.ndarray:
        """``monotone_cst`` as an i32 sign per encoded column: a sequence of
        length n_feat, or {column index: sign} with negative indices counting
        from the end (the pipeline's one-hot width is unknown before fit)."""
        cst = self.monotone_cst
        out = np.zeros(n_feat, dtype=np.int32)
        if cst is None:
            return out
        if isinstance(cst, dict):
            items = list(cst.items())
        else:
            if len(cst) != n_feat:
                raise ValueError(
                    f"monotone_cst has {len(cst)} entries for {n_feat} features"
                )
            items = list(enumerate(cst))
        for idx, sign in items:
            if isinstance(idx, (bool, np.bool_)) or int(idx) != idx:
                raise ValueError(f"monotone_cst column index {idx!r} is not an integer")
            if not -n_feat <= int(idx) < n_feat:
                raise ValueError(
                    f"monotone_cst column index {idx} out of range for {n_feat} features"
                )
            if sign not in (-1, 0, 1):
                raise ValueError(f"monotone_cst values must be -1, 0 or 1, got {sign!r}")
            out[int(idx)] = int(sign)
        return out

    def _resolve_device(self) -> str:
        if self.device == "cpu":
            return "cpu"
        import torch

        from ..ops import gpu

        if torch.cuda.is_available():
            gpu.ext()  # a GPU box without the extension is an error
            return "cuda"
        if self.device == "cuda":
            raise RuntimeError("device='cuda' requested but no GPU is visible")
        return "cpu"

    def fit(self, X, y):
        self._check_params()
        x = _to_dense_f32(X)
        if not np.isfinite(x).all():
            raise ValueError("HistGBTClassifier needs finite features (impute first)")
        y = np.asarray(y).ravel()
        if len(y) != len(x):
            raise ValueError("X and y have different lengths")
        self.classes_ = np.unique(y)
        if len(self.classes_) != 2:
            raise ValueError("HistGBTClassifier supports binary targets only")
        y01 = (y == self.classes_[1]).astype(np.float64)
        p1 = float(np.clip(y01.mean(), 1e-12, 1.0 - 1e-12))
        self.init_raw_ = float(np.log(p1 / (1.0 - p1)))
        self.n_features_in_ = x.shape[1]
        self.monotone_cst_ = self._resolve_monotone(x.shape[1])

        bins, bin_off, bin_thr = bin_features(x, int(self.max_bins))
        self.bin_offsets_ = bin_off
        self.bin_thresholds_ = bin_thr
        device = self._resolve_device()
        self.fit_device_ = device
        if device == "cuda":
            trees = self._boost_gpu(bins, bin_off, bin_thr, y01)
        else:
            trees = self._boost_cpu(bins, bin_off, bin_thr, y01)

        sizes = [len(t["feature"]) for t in trees]
        self.tree_offsets_ = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        for key in _TREE_KEYS:
            setattr(self, key + "_", np.concatenate([t[key] for t in trees]))
        return self

    def _grow(self, backend, gq, hq, bin_off, bin_thr):
        return grow_tree(
            backend, gq, hq, bin_off, bin_thr,
            int(self.max_depth), float(self.l2), int(self.min_samples_leaf),
            float(self.learning_rate),
            # the plain path stays as it is without a non-zero sign: the
            # bounded score rounds differently from g^2/d even when idle
            mono=self.monotone_cst_ if self.monotone_cst_.any() else None,
        )

    def _boost_cpu(self, bins, bin_off, bin_thr, y01):
        backend = _CpuBackend(bins, bin_off)
        hook = getattr(self, "_grad_hook", None)
        raw = np.full(len(y01), self.init_raw_, dtype=np.float64)
        scale = float(1 << SHIFT)
        trees = []
        for rnd in range(int(self.n_estimators)):
            p = 1.0 / (1.0 + np.exp(-raw))
            gq = np.rint((p - y01) * scale).astype(np.int32)
            hq = np.rint(p * (1.0 - p) * scale).astype(np.int32)
            if hook is not None:
                hook(rnd, gq.copy(), hq.copy())
            tree, node = self._grow(backend, gq, hq, bin_off, bin_thr)
            raw += tree["value"][-(node.astype(np.int64) + 1)].astype(np.float64)
            trees.append(tree)
        return trees

    def _boost_gpu(self, bins, bin_off, bin_thr, y01):
        import torch

        from ..ops import gpu

        dev = torch.device("cuda", torch.cuda.current_device())
        backend = _GpuBackend(bins, bin_off, gpu.ext(), dev)
        hook = getattr(self, "_grad_hook", None)
        y_d = torch.from_numpy(y01).to(dev)
        raw = torch.full_like(y_d, self.init_raw_)
        scale = float(1 << SHIFT)
        trees = []
        for rnd in range(int(self.n_estimators)):
            p = torch.sigmoid(raw)
            gq = torch.round((p - y_d) * scale).to(torch.int32)
            hq = torch.round(p * (1.0 - p) * scale).to(torch.int32)
            if hook is not None:
                hook(rnd, gq.cpu().numpy(), hq.cpu().numpy())
            tree, node = self._grow(backend, gq, hq, bin_off, bin_thr)
            value = torch.from_numpy(tree["value"]).to(dev).to(torch.float64)
            raw += value[-(node.to(torch.int64) + 1)]
            trees.append(tree)
        return trees

    # -- fitted model ------------------------------------------------------
    @property
    def n_trees_(self) -> int:
        return len(self.tree_offsets_) - 1

    def tree_arrays(self, i: int) -> dict:
        """Flat arrays of tree i (views): children_left/right, feature,
        threshold, value, cover."""
        a, b = int(self.tree_offsets_[i]), int(self.tree_offsets_[i + 1])
        return {key: getattr(self, key + "_")[a:b] for key in _TREE_KEYS}

    def decision_function(self, X) -> np.ndarray:
        """Raw log-odds: init_raw_ plus the f32 leaves summed in f64, with
        the f32 compare ``x <= threshold`` the serving kernels use."""
        x = _to_dense_f32(X)
        n = len(x)
        out = np.full(n, self.init_raw_, dtype=np.float64)
        off = self.tree_offsets_
        roots = off[:-1]
        chunk = max(1, (4 << 20) // max(1, self.n_trees_))
        for a in range(0, n, chunk):
            xs = x[a : a + chunk]
            m = len(xs)
            cur = np.repeat(roots, m)
            base = cur.copy()
            rows = np.tile(np.arange(m, dtype=np.int64), self.n_trees_)
            alive = np.arange(len(cur), dtype=np.int64)
            while len(alive):
                nidx = cur[alive]
                inner = self.children_left_[nidx] >= 0
                alive, nidx = alive[inner], nidx[inner]
                if not len(alive):
                    break
                go_left = xs[rows[alive], self.feature_[nidx]] <= self.threshold_[nidx]
                nxt = np.where(go_left, self.children_left_[nidx], self.children_right_[nidx])
                cur[alive] = base[alive] + nxt
            leaf = self.value_[cur].astype(np.float64).reshape(self.n_trees_, m)
            # tree order, like the per-row accumulation of the packed scorer
            for t in range(self.n_trees_):
                out[a : a + m] += leaf[t]
        return out

    def predict_proba(self, X) -> np.ndarray:
        p1 = 1.0 / (1.0 + np.exp(-self.decision_function(X)))
        return np.stack([1.0 - p1, p1], axis=1)

    def predict(self, X) -> np.ndarray:
        return self.classes_[(self.decision_function(X) > 0.0).astype(np.int64)]


def verify_monotone(estimator, monotone_cst=None) -> bool:
    """Structural check of a fitted model against its constraints.

    True when, at every split on a constrained column, the largest leaf value
    under the lower child does not exceed the smallest under the upper one
    (lower = left for +1, right for -1). That makes every tree, and so their
    f64 sum, monotone in the column. ``estimator`` is a fitted
    ``HistGBTClassifier`` or a pipeline ending in one; ``monotone_cst``
    (a sign per encoded column) overrides the fitted ``monotone_cst_``, e.g.
    to ask whether an unconstrained model happens to comply."""
    clf = estimator
    if hasattr(estimator, "named_steps"):
        clf = estimator.named_steps["classifier"]
    sign = clf.monotone_cst_ if monotone_cst is None else np.asarray(monotone_cst)
    if len(sign) != clf.n_features_in_:
        raise ValueError("monotone_cst must have one sign per encoded column")
    for i in range(clf.n_trees_):
        t = clf.tree_arrays(i)
        left, right, feat = t["children_left"], t["children_right"], t["feature"]
        lo = t["value"].copy()  # smallest / largest leaf of every subtree
        hi = t["value"].copy()
        # children follow their parent in creation order: one reverse sweep
        for n in range(len(left) - 1, -1, -1):
            a, b = left[n], right[n]
            if a < 0:
                continue
            s = sign[feat[n]]
            if (s > 0 and hi[a] > lo[b]) or (s < 0 and hi[b] > lo[a]):
                return False
            lo[n], hi[n] = min(lo[a], lo[b]), max(hi[a], hi[b])
    return True

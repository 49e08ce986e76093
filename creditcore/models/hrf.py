"""Histogram random forest trained on the MI355X, many trees per launch.

``HistForestClassifier`` is a bagged forest of Gini trees over the u8 bins of
models/hgbt.py. A forest's trees are independent, so a batch of ``TB`` trees
grows level by level in the same launches, from three primitives over the
batch's flat list of open slots,

    hist   per-(open slot, bin) integer sums {sum w*y, sum w}
    split  the slot's split among its sampled candidate features
    route  rows move to their child slot or leaf

which run as HIP kernels (csrc/creditcore_kernels.hip, hrf_*_kernel) on
``device="cuda"`` and as the numpy references of ops/cpu_ref.py on
``device="cpu"``. Nothing between the trees is floating point, so the two
devices are specified to build byte-identical forests:

- Binning is ``hgbt.bin_features``: "bin <= b goes left" is ``x <= edge`` and
  the f32 edge is the packed threshold.
- Bagging: tree t weighs row i by its bootstrap count,
  ``bincount(default_rng([random_state, t]).integers(0, N, N))``, drawn on
  the host (u8; ``random_state=None`` counts as 0). ``bootstrap=False``: all
  ones. A row of weight k counts as k rows everywhere: histograms,
  ``min_samples_leaf``, cover and leaf value. sklearn's forest applies
  ``min_samples_leaf`` to the number of distinct samples instead; this
  trainer counts the duplicates, as classic bagging with copied rows would.
- Criterion: Gini, through the proxy PL^2/WL + PR^2/WR - P^2/W (P positives,
  W weight) in f64 from the integer sums, one operation order, no FMA. A
  split needs ``min_samples_leaf`` weight on both sides and proxy > 0; ties
  within a feature go to the lowest bin. ``criterion="entropy"`` is not
  offered: a device log cannot be held bit-identical to numpy's.
- Features per node: feature f of node ``node_id`` (breadth-first creation
  order) of tree t has the key ``cpu_ref.hrf_feature_keys``; features are
  ranked by (key, f). The candidates are the first max(max_features, r* + 1)
  ranks, r* being the lowest rank with a valid split (sklearn's rule of
  drawing past ``max_features`` until something can split); the node takes
  the candidate with the highest proxy, ties to the lower rank, and becomes a
  leaf when no feature can split.
- Leaf value P/W in f64 from the integer sums, rounded to f32, on the host;
  cover is W. A child stays open while W >= 2*min_samples_leaf, 0 < P < W
  and depth remains.

Limits: binary targets, ``max_depth <= 12``, ``max_bins <= 256``, at most
1024 features (the split kernel's per-feature tables live in LDS), no OOB
score, no class weights, no missing-value direction (the pipeline imputes).

The fitted state is plain numpy, as in models/hgbt.py, and
``pack.pack_classifier_pipeline`` packs it as a leaf-mean forest
(``cls_kind = 0``).
"""

from __future__ import annotations

import math

import numpy as np
from sklearn.base import BaseEstimator, ClassifierMixin

from .hgbt import (
    LDS_BUDGET_BYTES,
    MAX_BINS,
    MAX_DEPTH,
    TARGET_BLOCKS,
    _TREE_KEYS,
    _to_dense_f32,
    bin_features,
    plan_feature_groups,
)

MAX_FEATURES = 1024  # hrf_split_kernel's LDS tables (ext.HRF_MAX_FEATS)
# level histogram of one tree batch, worst case; it sets the batch size
HIST_BUDGET_BYTES = 1 << 30
_CPU_SPLIT_CHUNK = 256  # slots per hrf_split_cpu call (bounds its temporaries)


def bootstrap_weights(random_state, tree: int, n_rows: int, bootstrap: bool = True) -> np.ndarray:
    """u8[n_rows] row weights of tree ``tree``: its bootstrap counts."""
    if not bootstrap:
        return np.ones(n_rows, dtype=np.uint8)
    seed = 0 if random_state is None else int(random_state)
    draw = np.random.default_rng([seed, int(tree)]).integers(0, n_rows, n_rows)
    w = np.bincount(draw, minlength=n_rows)
    if w.max(initial=0) > 255:
        raise ValueError("a bootstrap count above 255 does not fit the u8 weights")
    return w.astype(np.uint8)


def resolve_max_features(max_features, n_feat: int) -> int:
    if max_features is None:
        return n_feat
    if isinstance(max_features, str):
        if max_features == "sqrt":
            return max(1, math.isqrt(n_feat))
        raise ValueError("max_features must be 'sqrt', an integer or None")
    if isinstance(max_features, (bool, float)) or int(max_features) != max_features:
        raise ValueError("max_features must be 'sqrt', an integer or None")
    if not 1 <= int(max_features) <= n_feat:
        raise ValueError(f"max_features must be in [1, {n_feat}]")
    return int(max_features)


def tree_batch_size(n_trees: int, n_rows: int, total_bins: int, max_depth: int, min_leaf: int) -> int:
    """Trees per batch from HIST_BUDGET_BYTES. A level has at most
    2^(max_depth-1) open slots per tree, and at most N / (2*min_leaf): every
    open slot holds 2*min_leaf of the tree's total weight N."""
    slots = max(1, min(2 ** (max_depth - 1), n_rows // (2 * min_leaf)))
    per_tree = slots * 2 * total_bins * 8
    return int(max(1, min(n_trees, HIST_BUDGET_BYTES // per_tree)))


class _CpuBackend:
    """The three level primitives as numpy references (ops/cpu_ref.py)."""

    def __init__(self, bins: np.ndarray, bin_off: np.ndarray, y: np.ndarray):
        from ..ops import cpu_ref

        self._ref = cpu_ref
        self.bins, self.bin_off, self.y = bins, bin_off, y

    def start(self, w: np.ndarray, node: np.ndarray):
        self.w = w
        return node

    def hist(self, node, slot_off, k_max):
        return self._ref.hrf_hist_cpu(self.bins, self.bin_off, self.y, self.w, node, slot_off)

    def split(self, hist, slot_meta, m, min_leaf, seed) -> np.ndarray:
        step = _CPU_SPLIT_CHUNK
        return np.concatenate([
            self._ref.hrf_split_cpu(
                hist[a : a + step], self.bin_off, slot_meta[a : a + step], m, min_leaf, seed
            )
            for a in range(0, len(hist), step)
        ])

    def route(self, node, table, slot_off):
        return self._ref.hrf_route_cpu(self.bins, table, node, slot_off)


class _GpuBackend:
    """The three level primitives as HIP kernels over torch tensors."""

    def __init__(self, bins: np.ndarray, bin_off: np.ndarray, y: np.ndarray, ext, device):
        import torch

        self._torch, self._ext, self.device = torch, ext, device
        self.n_rows = bins.shape[1]
        self.n_bins = np.diff(bin_off)
        self.total_bins = int(bin_off[-1])
        self.bins = self._dev(bins)
        self.bin_off = self._dev(bin_off)
        self.y = self._dev(y)
        self.rows_per_block = int(ext.HRF_MAX_ROWS_PER_BLOCK)
        self.lds_bytes = LDS_BUDGET_BYTES
        self._groups: dict = {}

    def _dev(self, a: np.ndarray):
        return self._torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

    def start(self, w: np.ndarray, node: np.ndarray):
        self.w = self._dev(w)
        self.n_batch = len(w)
        return self._dev(node)

    def _plan(self, k_max: int):
        key = (k_max, self.n_batch)
        plan = self._groups.get(key)
        if plan is None:
            row_blocks = max(1, -(-self.n_rows // self.rows_per_block)) * self.n_batch
            want = max(1, -(-TARGET_BLOCKS // row_blocks))
            max_feats = max(1, -(-len(self.n_bins) // want))
            off, entries = plan_feature_groups(
                self.n_bins, k_max, self.lds_bytes, max_feats, planes=2
            )
            plan = (self._dev(off), entries)
            self._groups[key] = plan
        return plan

    def hist(self, node, slot_off, k_max):
        grp_off, entries = self._plan(k_max)
        self._slot_off = self._dev(slot_off)
        return self._ext.hrf_hist(
            self.bins, self.bin_off, grp_off, self.y, self.w, node, self._slot_off,
            int(slot_off[-1]), self.total_bins, entries, self.rows_per_block,
        )

    def split(self, hist, slot_meta, m, min_leaf, seed) -> np.ndarray:
        # the only per-level traffic back to the host: one record per open slot
        seed = seed - (1 << 64) if seed >= (1 << 63) else seed
        return self._ext.hrf_split(
            hist, self.bin_off, self._dev(slot_meta), m, min_leaf, seed
        ).cpu().numpy()

    def route(self, node, table, slot_off):
        self._ext.hrf_route(self.bins, self._dev(table), node, self._slot_off)
        return node


def _excl_cumsum(counts: np.ndarray) -> np.ndarray:
    return np.cumsum(counts) - counts


def grow_forest_batch(
    backend,
    tree_ids: np.ndarray,
    w: np.ndarray,
    y: np.ndarray,
    bin_off: np.ndarray,
    bin_threshold: np.ndarray,
    max_depth: int,
    max_features: int,
    min_leaf: int,
    seed: int,
) -> list[dict]:
    """Grow the trees ``tree_ids`` (global indices) together, level by level,
    from their row weights ``w`` u8[TB, N] and the targets ``y`` u8[N].

    A level is a flat list of open slots, sorted by tree and, within a tree,
    by node id; a node's id is its place in the tree's breadth-first creation
    order, so it does not depend on which trees share the batch. Returns one
    dict of sklearn-style flat arrays per tree (hgbt.grow_tree's layout)."""
    tb = len(tree_ids)
    cap = 2 ** (max_depth + 1) - 1
    cl = np.full((tb, cap), -1, dtype=np.int32)
    cr = np.full((tb, cap), -1, dtype=np.int32)
    feature = np.full((tb, cap), -2, dtype=np.int32)
    threshold = np.full((tb, cap), -2.0, dtype=np.float32)
    value = np.zeros((tb, cap), dtype=np.float32)
    cover = np.zeros((tb, cap), dtype=np.int64)
    n_used = np.ones(tb, dtype=np.int64)

    def is_open(p_sum, w_sum, depth):
        if depth >= max_depth:
            return np.zeros(len(w_sum), dtype=bool)
        return (w_sum >= 2 * min_leaf) & (p_sum > 0) & (p_sum < w_sum)

    # the root's sums come from the weights; every other node's from its
    # parent's split record
    w_root = w.sum(axis=1, dtype=np.int64)
    p_root = w[:, y.astype(bool)].sum(axis=1, dtype=np.int64)
    cover[:, 0] = w_root
    value[:, 0] = (p_root / np.maximum(w_root, 1)).astype(np.float32)
    root_open = is_open(p_root, w_root, 0)
    node = backend.start(w, np.where((w > 0) & root_open[:, None], 0, -1).astype(np.int32))
    st = np.flatnonzero(root_open)  # batch-local tree of every open slot
    sn = np.zeros(len(st), dtype=np.int64)  # its node id in that tree

    for depth in range(max_depth):
        if not len(st):
            break
        per_tree = np.bincount(st, minlength=tb)
        slot_off = np.concatenate([[0], np.cumsum(per_tree)]).astype(np.int32)
        slot_meta = np.stack([tree_ids[st], sn], axis=1).astype(np.int32)
        hist = backend.hist(node, slot_off, int(per_tree.max()))
        rec = backend.split(hist, slot_meta, max_features, min_leaf, seed)
        feat, bin_ = rec[:, 1], rec[:, 2]
        p_l, w_l, p_t, w_t = rec[:, 3], rec[:, 4], rec[:, 5], rec[:, 6]
        split = feat >= 0
        table = np.zeros((len(st), 4), dtype=np.int32)
        closed = -(sn[~split] + 1)
        table[~split, 0] = -1
        table[~split, 2] = closed
        table[~split, 3] = closed
        if not split.any():
            break
        pt, parent = st[split], sn[split]
        n_split = np.bincount(pt, minlength=tb)
        left = n_used[pt] + 2 * (np.arange(len(pt)) - _excl_cumsum(n_split)[pt])
        n_used += 2 * n_split
        cl[pt, parent], cr[pt, parent] = left, left + 1
        feature[pt, parent] = feat[split]
        threshold[pt, parent] = bin_threshold[bin_off[feat[split]] + bin_[split]]
        ct = np.repeat(pt, 2)
        child = np.stack([left, left + 1], axis=1).ravel()
        c_p = np.stack([p_l[split], (p_t - p_l)[split]], axis=1).ravel()
        c_w = np.stack([w_l[split], (w_t - w_l)[split]], axis=1).ravel()
        cover[ct, child] = c_w
        value[ct, child] = (c_p / c_w).astype(np.float32)
        opened = is_open(c_p, c_w, depth + 1)
        st, sn = ct[opened], child[opened]
        if not len(st):
            break  # every row's next stop is a leaf: nothing reads `node` again
        local = np.arange(len(st)) - _excl_cumsum(np.bincount(st, minlength=tb))[st]
        code = -(child + 1)
        code[opened] = local
        table[split, 0] = feat[split]
        table[split, 1] = bin_[split]
        table[split, 2] = code[0::2]
        table[split, 3] = code[1::2]
        node = backend.route(node, table, slot_off)

    arrays = dict(zip(_TREE_KEYS, (cl, cr, feature, threshold, value, cover)))
    return [
        {key: arrays[key][i, : n_used[i]].copy() for key in _TREE_KEYS} for i in range(tb)
    ]


class HistForestClassifier(ClassifierMixin, BaseEstimator):
    """Histogram random forest, binary Gini trees (module docstring).

    ``device``: "cuda" trains with the HIP kernels, "cpu" with the numpy
    references, "auto" takes the GPU when one is visible; with a visible GPU
    and no extension it raises ``ExtensionMissing`` and never falls back."""

    _tree_batch = None  # trees per batch; None: from HIST_BUDGET_BYTES

    def __init__(
        self,
        n_estimators=100,
        max_depth=8,
        max_features="sqrt",
        min_samples_leaf=1,
        bootstrap=True,
        max_bins=MAX_BINS,
        random_state=None,
        device="auto",
    ):
        self.n_estimators = n_estimators
        self.max_depth = max_depth
        self.max_features = max_features
        self.min_samples_leaf = min_samples_leaf
        self.bootstrap = bootstrap
        self.max_bins = max_bins
        self.random_state = random_state
        self.device = device

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
        if self.random_state is not None and not 0 <= int(self.random_state) < 2**63:
            raise ValueError("random_state must be None or in [0, 2^63)")
        if self.device not in ("auto", "cpu", "cuda"):
            raise ValueError("device must be 'auto', 'cpu' or 'cuda'")

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
        n_rows, n_feat = x.shape
        if n_feat > MAX_FEATURES:
            raise ValueError(f"HistForestClassifier takes at most {MAX_FEATURES} features")
        m = resolve_max_features(self.max_features, n_feat)
        if not np.isfinite(x).all():
            raise ValueError("HistForestClassifier needs finite features (impute first)")
        y = np.asarray(y).ravel()
        if len(y) != n_rows:
            raise ValueError("X and y have different lengths")
        self.classes_ = np.unique(y)
        if len(self.classes_) != 2:
            raise ValueError("HistForestClassifier supports binary targets only")
        y01 = (y == self.classes_[1]).astype(np.uint8)
        self.n_features_in_ = n_feat

        bins, bin_off, bin_thr = bin_features(x, int(self.max_bins))
        self.bin_offsets_ = bin_off
        self.bin_thresholds_ = bin_thr
        device = self._resolve_device()
        self.fit_device_ = device
        if device == "cuda":
            import torch

            from ..ops import gpu

            dev = torch.device("cuda", torch.cuda.current_device())
            backend = _GpuBackend(bins, bin_off, y01, gpu.ext(), dev)
        else:
            backend = _CpuBackend(bins, bin_off, y01)

        n_trees = int(self.n_estimators)
        depth, min_leaf = int(self.max_depth), int(self.min_samples_leaf)
        seed = 0 if self.random_state is None else int(self.random_state)
        tb = self._tree_batch or tree_batch_size(
            n_trees, n_rows, int(bin_off[-1]), depth, min_leaf
        )
        trees = []
        for t0 in range(0, n_trees, int(tb)):
            ids = np.arange(t0, min(t0 + int(tb), n_trees), dtype=np.int64)
            w = np.stack(
                [bootstrap_weights(seed, t, n_rows, bool(self.bootstrap)) for t in ids]
            )
            trees += grow_forest_batch(
                backend, ids, w, y01, bin_off, bin_thr, depth, m, min_leaf, seed
            )

        sizes = [len(t["feature"]) for t in trees]
        self.tree_offsets_ = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        for key in _TREE_KEYS:
            setattr(self, key + "_", np.concatenate([t[key] for t in trees]))
        return self

    # -- fitted model ------------------------------------------------------
    @property
    def n_trees_(self) -> int:
        return len(self.tree_offsets_) - 1

    def tree_arrays(self, i: int) -> dict:
        """Flat arrays of tree i (views): children_left/right, feature,
        threshold, value, cover."""
        a, b = int(self.tree_offsets_[i]), int(self.tree_offsets_[i + 1])
        return {key: getattr(self, key + "_")[a:b] for key in _TREE_KEYS}

    def _p1(self, X) -> np.ndarray:
        """P(class 1): the f32 leaf values summed in f64 in tree order, times
        1/n_trees, with the f32 compare ``x <= threshold``: the operation
        order of the packed scorer's finalize for a leaf-mean forest."""
        x = _to_dense_f32(X)
        n = len(x)
        out = np.zeros(n, dtype=np.float64)
        roots = self.tree_offsets_[:-1]
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
            for t in range(self.n_trees_):
                out[a : a + m] += leaf[t]
        return out * (1.0 / float(self.n_trees_))

    def predict_proba(self, X) -> np.ndarray:
        p1 = self._p1(X)
        return np.stack([1.0 - p1, p1], axis=1)

    def predict(self, X) -> np.ndarray:
        return self.classes_[(self._p1(X) > 0.5).astype(np.int64)]

"""Hand-built forests, rows and a naive walker for test_forest_kernels_gpu.py
(no test in here).

Every leaf payload is a multiple of 2^-16 with |v| <= 64 and no forest has
more than 5000 trees, so every partial sum of leaves is exact in f64 whatever
the order of the additions: the raw accumulators of the traversal kernels can
be compared bit for bit. Four families:

  visit-once   tree t answers 1 for x == t and 0 otherwise (tree partition)
  ragged       root-is-leaf trees next to the 26-split caterpillar
  edges        one split per tree, thresholds and rows on the f32 edges
  gbt          logits 0, +-1, +-40, +-800 and isolation-depth classes
"""

from __future__ import annotations

import dataclasses
import functools

import numpy as np

from _shap_models import (
    CATERPILLAR_SPLITS,
    N_ONEHOT,
    caterpillar_model,
    caterpillar_rows,
    f32bits,
    hand_model,
)
from creditcore.ops import cpu_ref
from creditcore.pack import N_CAT, N_NUM

Q = 2.0**-16  # leaf quantum
N_VIRTUAL = N_ONEHOT + N_NUM
FLT_MAX = float(np.finfo(np.float32).max)
NAIVE_MAX_PAIRS = 50_000  # rows x trees up to which the naive walker is used


def leaf(v: float) -> list[int]:
    assert abs(v) <= 64.0 and v / Q == round(v / Q), v
    return [-1, f32bits(v), 0, 0]


def _concat(trees):
    trees = [np.asarray(t, dtype=np.int32).reshape(-1, 4) for t in trees]
    off = np.zeros(len(trees) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(t) for t in trees])
    return trees, np.concatenate(trees), off


def check_forest(nodes: np.ndarray, off: np.ndarray, n_feat: int) -> None:
    """The kernels trust their tables: every split feature is in range, both
    children lie after their parent inside the same tree (walks terminate) and
    every tree has at least one node."""
    sizes = np.diff(off)
    assert off[0] == 0 and off[-1] == len(nodes) and (sizes > 0).all()
    assert len(off) - 1 <= 5000
    local = np.arange(len(nodes)) - np.repeat(off[:-1], sizes)
    size = np.repeat(sizes, sizes)
    split = nodes[:, 0] >= 0
    assert (nodes[:, 0] >= -1).all() and (nodes[:, 0] < n_feat).all()
    assert (nodes[split, 2:] > local[split, None]).all()
    assert (nodes[split, 2:] < size[split, None]).all()
    assert np.isfinite(nodes[~split, 1].view(np.float32)).all()


def build_model(
    cls_trees,
    if_trees,
    if_denom: float,
    if_offset: float = -0.5,
    if_threshold: float = 0.95,
    cls_kind: int = 0,
    cls_bias: float = 0.0,
):
    """hand_model around the classifier trees (virtual features) with an
    isolation forest over the numeric columns (direct features)."""
    cls_trees, cls_nodes, cls_off = _concat(cls_trees)
    if_trees, if_nodes, if_off = _concat(if_trees)
    check_forest(cls_nodes, cls_off, N_VIRTUAL)
    check_forest(if_nodes, if_off, N_NUM)
    p = hand_model(
        cls_trees, [np.ones(len(t)) for t in cls_trees], cls_kind=cls_kind, cls_bias=cls_bias
    )
    return dataclasses.replace(
        p,
        if_nodes=if_nodes,
        if_tree_offsets=if_off,
        if_denom=float(if_denom),
        if_offset=float(if_offset),
        if_threshold=float(if_threshold),
    )


# ------------------------------------------------------------ naive walker


def naive_sums(p, codes, nums, forest: str = "cls") -> np.ndarray:
    """Sum of leaf payloads per row, one Python loop per (row, tree). The f32
    values are widened to Python floats, which is exact and keeps the order of
    any two of them, so every compare is the f32 compare; the sum is f64."""
    direct = forest == "if"
    tab = p.if_nodes if direct else p.cls_nodes
    off = (p.if_tree_offsets if direct else p.cls_tree_offsets).tolist()
    nodes, thr = tab.tolist(), tab[:, 1].view(np.float32).tolist()
    col, code = p.feat_col.tolist(), p.feat_code.tolist()
    x = np.where(np.isnan(nums), p.medians[None, :], nums).astype(np.float32).tolist()
    c = np.asarray(codes).tolist()
    out = np.zeros(len(x), dtype=np.float64)
    for r in range(len(x)):
        for t in range(len(off) - 1):
            k = off[t]
            while nodes[k][0] >= 0:
                f = nodes[k][0]
                if direct or code[f] < 0:
                    v = x[r][f if direct else col[f]]
                else:
                    v = 1.0 if c[r][col[f]] == code[f] else 0.0
                k = off[t] + (nodes[k][2] if v <= thr[k] else nodes[k][3])
            out[r] += thr[k]
    return out


MUTATIONS = (
    "lt",  # v < thr in place of v <= thr
    "bits",  # signed compare of the bit patterns in place of the float compare
    "no_impute",  # NaN is not replaced by the median (and compares false)
    "drop_last",  # tree T-1 is never visited
    "double_last",  # tree T-1 is visited twice
    "stump_zero",  # a root-is-leaf tree contributes 0
    "ignore_unknown",  # the unknown category -1 is taken for category 0
)


def mutant_sums(p, codes, nums, mutation: str, forest: str = "cls") -> np.ndarray:
    """naive_sums with one deliberate error: what a subtly wrong kernel would
    compute. Only ever run on the CPU, to show that the committed cases see
    the error."""
    assert mutation in MUTATIONS
    direct = forest == "if"
    tab = p.if_nodes if direct else p.cls_nodes
    off = (p.if_tree_offsets if direct else p.cls_tree_offsets).tolist()
    nodes, thr = tab.tolist(), tab[:, 1].view(np.float32).tolist()
    col, code = p.feat_col.tolist(), p.feat_code.tolist()
    xa = np.asarray(nums, dtype=np.float32)
    if mutation != "no_impute":
        xa = np.where(np.isnan(xa), p.medians[None, :], xa).astype(np.float32)
    x = xa.tolist()
    c = np.asarray(codes).tolist()
    n_trees = len(off) - 1
    order = list(range(n_trees))
    if mutation == "drop_last":
        order = order[:-1]
    elif mutation == "double_last":
        order.append(n_trees - 1)
    out = np.zeros(len(x), dtype=np.float64)
    for r in range(len(x)):
        for t in order:
            k = off[t]
            if mutation == "stump_zero" and nodes[k][0] < 0:
                continue
            while nodes[k][0] >= 0:
                f = nodes[k][0]
                if direct or code[f] < 0:
                    v = x[r][f if direct else col[f]]
                else:
                    have = c[r][col[f]]
                    if mutation == "ignore_unknown":
                        have = max(have, 0)
                    v = 1.0 if have == code[f] else 0.0
                if mutation == "lt":
                    left = v < thr[k]
                elif mutation == "bits":
                    left = f32bits(v) <= nodes[k][1]
                else:
                    left = v <= thr[k]
                k = off[t] + (nodes[k][2] if left else nodes[k][3])
            out[r] += thr[k]
    return out


# -------------------------------------------------------------- references


def iscore_of(p, depth_sums: np.ndarray) -> np.ndarray:
    return 2.0 ** (-depth_sums / p.if_denom) + p.if_offset


def reference(p, codes, nums):
    """(exact classifier leaf sums, isolation score, outlier flag) per row:
    the naive walker up to NAIVE_MAX_PAIRS (row, tree) pairs, cpu_ref above.
    cpu_ref returns the quotient fl(s / T); s is a multiple of 2^-16 and the
    quotient's error times T is far below half of that, so rounding to the
    grid recovers s exactly."""
    b = len(codes)
    if b * max(p.cls_n_trees, p.if_n_trees) <= NAIVE_MAX_PAIRS:
        s = naive_sums(p, codes, nums, "cls")
        iscore = iscore_of(p, naive_sums(p, codes, nums, "if"))
    else:
        assert p.cls_kind == 0
        imp = cpu_ref.impute_nums(p, nums)
        s = np.round(cpu_ref.score_forest_cpu(p, codes, imp) * p.cls_n_trees / Q) * Q
        iscore, _ = cpu_ref.score_iforest_cpu(p, imp)
    return s, iscore, (iscore > p.if_threshold).astype(np.float64)


def proba_of(p, s: np.ndarray) -> np.ndarray:
    """The classifier output of exact leaf sums s: the correctly rounded
    quotient for the averaging forests, the sigmoid for gradient boosting."""
    if p.cls_kind == 1:
        with np.errstate(over="ignore"):
            return 1.0 / (1.0 + np.exp(-(s + p.cls_bias)))
    return s / p.cls_n_trees


# ------------------------------------------------- family 1: visit-once forests


def visit_once_trees(n_trees: int, feat: int) -> list[np.ndarray]:
    """Tree t: x <= t - 0.5 -> 0, else x <= t + 0.5 -> 1, else 0."""
    return [
        np.array(
            [
                [feat, f32bits(t - 0.5), 1, 2],
                leaf(0.0),
                [feat, f32bits(t + 0.5), 3, 4],
                leaf(1.0),
                leaf(0.0),
            ],
            dtype=np.int32,
        )
        for t in range(n_trees)
    ]


@functools.lru_cache(maxsize=None)
def visit_once_model(t_cls: int, t_if: int):
    """Classifier on numeric column 0 (virtual feature N_ONEHOT), isolation
    forest on the same column (direct feature 0) with its own tree count and
    if_denom = 1: a row with x = k has the raw sum [k < t_cls] and the score
    2^-[k < t_if] + if_offset."""
    return build_model(visit_once_trees(t_cls, N_ONEHOT), visit_once_trees(t_if, 0), 1.0)


def visit_once_rows(b: int, period: int, start: int = 0):
    """Row r has x = (start + r) % period in numeric column 0. The other
    columns hold a value that no tree answers 1 for."""
    codes = np.zeros((b, N_CAT), dtype=np.int16)
    nums = np.full((b, N_NUM), -7.0, dtype=np.float32)
    nums[:, 0] = (start + np.arange(b)) % period
    return codes, nums


def visit_once_expected(p, nums):
    """Analytic answer: (raw classifier sum, isolation score) per row."""
    x = nums[:, 0].astype(np.int64)
    s = (x < p.cls_n_trees).astype(np.float64)
    return s, np.where(x < p.if_n_trees, 0.5, 1.0) + p.if_offset


# ------------------------------------------------------ family 2: ragged depth

# Tree kinds in tree order: S = root-is-leaf, C = caterpillar, D = complete
# depth-3 tree. With 2-tree ILP and n = ceil(T / 2) chunks, chunk c walks trees
# c and c + n: RAGGED_ODD pairs (S,C) (C,S) (S,S) (D,C) (C,D) (D,S) (S,D) (D,D)
# (D,S) (D,C) and leaves the caterpillar at tree 10 alone; RAGGED_EVEN has the
# same pairs without it.
RAGGED_ODD = "SCSDCDSDDDC" + "CSSCDSDDSC"
RAGGED_EVEN = "SCSDCDSDDD" + "CSSCDSDDSC"


def ilp_lanes(n_trees: int, n_chunks: int, ilp: int) -> list[tuple[int, ...]]:
    """Trees walked together by one thread: t, t + n_chunks, ... (absent: -1)."""
    out = []
    for chunk in range(n_chunks):
        for t in range(chunk, n_trees, ilp * n_chunks):
            out.append(
                tuple(t + k * n_chunks if t + k * n_chunks < n_trees else -1 for k in range(ilp))
            )
    return out


def _dyadic(rng, lo: float, hi: float) -> float:
    return float(rng.integers(int(lo / Q), int(hi / Q) + 1)) * Q


def _caterpillar_tree(rng) -> np.ndarray:
    nodes = caterpillar_model().cls_nodes.copy()
    for k in np.flatnonzero(nodes[:, 0] < 0):
        nodes[k, 1] = f32bits(_dyadic(rng, -1.0, 1.0))
    return nodes


def _depth3_tree(rng, feats) -> np.ndarray:
    nodes = np.zeros((15, 4), dtype=np.int32)
    for i, f in enumerate(feats):
        thr = 0.5 if f < N_ONEHOT else float(np.float32(rng.normal(0.0, 2.0)))
        nodes[i] = [f, f32bits(thr), 2 * i + 1, 2 * i + 2]
    for i in range(7, 15):
        nodes[i] = leaf(_dyadic(rng, -1.0, 1.0))
    return nodes


def _chain_tree(splits, leaves) -> np.ndarray:
    """Caterpillar over (direct feature, threshold) splits: split i at node
    2i, its off-chain leaf at 2i+1, the chain goes on at 2i+2."""
    n = 2 * len(splits) + 1
    nodes = np.zeros((n, 4), dtype=np.int32)
    for i, (feat, thr) in enumerate(splits):
        k = 2 * i
        on_left = i % 3 != 1
        nodes[k] = [feat, f32bits(thr), k + 2 if on_left else k + 1, k + 1 if on_left else k + 2]
        nodes[k + 1] = leaf(leaves[i])
    nodes[n - 1] = leaf(leaves[len(splits)])
    return nodes


@functools.lru_cache(maxsize=None)
def ragged_model(kinds: str):
    rng = np.random.default_rng(len(kinds))
    n_d = kinds.count("D")
    assert 7 * n_d >= N_VIRTUAL  # the depth-3 trees split on every feature
    feats = np.concatenate(
        [rng.permutation(N_VIRTUAL), rng.integers(0, N_VIRTUAL, 7 * n_d - N_VIRTUAL)]
    ).reshape(n_d, 7)
    d = iter(feats)
    trees = []
    for kind in kinds:
        if kind == "S":
            trees.append(np.array([leaf(_dyadic(rng, -64.0, 64.0))], dtype=np.int32))
        elif kind == "C":
            trees.append(_caterpillar_tree(rng))
        else:
            trees.append(_depth3_tree(rng, next(d)))
    pairs = {
        (kinds[a], kinds[b] if b >= 0 else "-")
        for a, b in ilp_lanes(len(kinds), -(-len(kinds) // 2), 2)
    }
    assert {("S", "C"), ("C", "S"), ("S", "S")} <= pairs
    assert (("C", "-") in pairs) == (len(kinds) % 2 == 1)
    # isolation forest: (stump, chain) (chain, stump) and a lone stump
    num_splits = [(f - N_ONEHOT, thr) for f, thr in CATERPILLAR_SPLITS if f >= N_ONEHOT]
    if_trees = []
    for kind in "SCSCS":
        if kind == "S":
            if_trees.append(np.array([leaf(_dyadic(rng, 1.0, 8.0))], dtype=np.int32))
        else:
            depth = [i + 1 + _dyadic(rng, 0.0, 1.0) for i in range(len(num_splits) + 1)]
            if_trees.append(_chain_tree(num_splits, depth))
    return build_model(trees, if_trees, 7.0)


@functools.lru_cache(maxsize=None)
def ragged_rows(b: int = 513):
    """caterpillar_rows() (row 0 walks the whole chain) and random rows."""
    rng = np.random.default_rng(513)
    codes, nums = caterpillar_rows()
    n = b - len(codes)
    rc = rng.integers(-1, 2, size=(n, N_CAT)).astype(np.int16)
    rn = rng.normal(0.0, 2.0, size=(n, N_NUM)).astype(np.float32)
    rn[rng.uniform(size=rn.shape) < 0.02] = np.nan
    return np.concatenate([codes, rc]), np.concatenate([nums, rn])


# ------------------------------------------------------ family 3: compare edges

EDGE_THRESHOLDS = (0.0, -0.0, 1e-40, -1e-40, 1.0, FLT_MAX, -FLT_MAX)
EDGE_ONEHOT_THRESHOLDS = (0.0, 0.5, 1.0)
EDGE_CODES = (-1, 0, 1, 2, 32767)


@functools.lru_cache(maxsize=None)
def edge_model():
    """One split per tree. Numeric column j: the seven EDGE_THRESHOLDS and
    the column's own median; every one-hot feature at 0.0, 0.5 and 1.0. The
    two leaves of a tree differ, so one flipped branch changes the sum."""
    rng = np.random.default_rng(3)
    medians = np.linspace(-1.0, 1.0, N_NUM).astype(np.float32)  # hand_model's

    def two_leaves(lo, hi):
        a = b = _dyadic(rng, lo, hi)
        while b == a:
            b = _dyadic(rng, lo, hi)
        return leaf(a), leaf(b)

    def stumps(feat_of, lo, hi):
        trees = []
        for j in range(N_NUM):
            for thr in EDGE_THRESHOLDS + (float(medians[j]),):
                trees.append([[feat_of(j), f32bits(thr), 1, 2], *two_leaves(lo, hi)])
        return trees

    cls_trees = stumps(lambda j: N_ONEHOT + j, -64.0, 64.0)
    for f in range(N_ONEHOT):
        for thr in EDGE_ONEHOT_THRESHOLDS:
            cls_trees.append([[f, f32bits(thr), 1, 2], *two_leaves(-64.0, 64.0)])
    if_trees = stumps(lambda j: j, 1.0, 8.0)
    p = build_model(cls_trees, if_trees, 4.0 * len(if_trees))
    assert (p.medians == medians).all()
    assert f32bits(0.0) != f32bits(-0.0) and f32bits(1e-40) != 0
    return p


@functools.lru_cache(maxsize=None)
def edge_rows():
    """Every numeric column meets every edge value: each threshold, its two
    f32 neighbours, +-0.0, +-inf, +-FLT_MAX, denormals of both signs and NaN
    (imputed to the column's median, which is a threshold of that column).
    Row i holds value (i + 5 j) % n in column j and code (i + c) % 5 of
    EDGE_CODES in categorical column c."""
    p = edge_model()
    thr = np.array(EDGE_THRESHOLDS + tuple(p.medians.tolist()), dtype=np.float32)
    tiny = float(np.finfo(np.float32).smallest_subnormal)
    with np.errstate(over="ignore"):  # the neighbours of +-FLT_MAX are +-inf
        up = np.nextafter(thr, np.float32(np.inf))
        down = np.nextafter(thr, np.float32(-np.inf))
    vals = np.concatenate(
        [
            thr,
            up,
            down,
            np.array(
                [0.0, -0.0, np.inf, -np.inf, FLT_MAX, -FLT_MAX, 1e-40, -1e-40, tiny, -tiny, np.nan],
                dtype=np.float32,
            ),
        ]
    ).astype(np.float32)
    n = len(vals)
    i = np.arange(n)
    nums = np.stack([vals[(i + 5 * j) % n] for j in range(N_NUM)], axis=1)
    codes = np.stack(
        [np.array(EDGE_CODES, dtype=np.int16)[(i + c) % len(EDGE_CODES)] for c in range(N_CAT)],
        axis=1,
    )
    return codes.astype(np.int16), np.ascontiguousarray(nums, dtype=np.float32)


# ---------------------------------------------------- family 4: finalize_kernel

GBT_LOGITS = (0.0, 1.0, -1.0, 40.0, -40.0, 800.0, -800.0)
GBT_BIAS = 3.0
GBT_TREES = 16
GBT_IF_TREES = 4
GBT_DEPTH_CLASSES = 5
GBT_THRESHOLD_CLASS = 2
GBT_ROWS = 300


def gbt_depth_sums() -> np.ndarray:
    """Isolation depth sum of depth class k: sum_j (1 + k + j / 4)."""
    k = np.arange(GBT_DEPTH_CLASSES, dtype=np.float64)
    return GBT_IF_TREES * (1.0 + k) + 0.25 * sum(range(GBT_IF_TREES))


@functools.lru_cache(maxsize=None)
def gbt_model(threshold_step: int = 0, cls_kind: int = 1):
    """Gradient-boosting finalize: numeric column 0 selects the logit class.
    Tree j of 16 answers (logit - bias) / 16 + (2j - 15) 2^-12 (the offsets
    sum to 0), so leaf sum + cls_bias is the logit exactly. Numeric column 1
    selects the isolation depth class; if_threshold is the reference score of
    class GBT_THRESHOLD_CLASS moved by ``threshold_step`` ulps (-1, 0, +1)."""

    def chain(feat, values):
        # class i leaves the chain at split i (x <= i + 0.5 goes to the leaf)
        n = len(values)
        nodes = np.zeros((2 * n - 1, 4), dtype=np.int32)
        for i in range(n - 1):
            nodes[2 * i] = [feat, f32bits(i + 0.5), 2 * i + 1, 2 * i + 2]
            nodes[2 * i + 1] = leaf(values[i])
        nodes[2 * n - 2] = leaf(values[n - 1])
        return nodes

    cls_trees = [
        chain(N_ONEHOT, [(g - GBT_BIAS) / GBT_TREES + (2 * j - 15) * 2.0**-12 for g in GBT_LOGITS])
        for j in range(GBT_TREES)
    ]
    if_trees = [
        chain(1, [1.0 + k + 0.25 * j for k in range(GBT_DEPTH_CLASSES)])
        for j in range(GBT_IF_TREES)
    ]
    denom, offset = 3.0 * GBT_IF_TREES, -0.5
    thr = float(2.0 ** (-gbt_depth_sums()[GBT_THRESHOLD_CLASS] / denom) + offset)
    if threshold_step:
        thr = float(np.nextafter(thr, np.inf if threshold_step > 0 else -np.inf))
    return build_model(
        cls_trees, if_trees, denom, offset, thr, cls_kind=cls_kind, cls_bias=GBT_BIAS * cls_kind
    )


def gbt_rows(b: int = GBT_ROWS):
    """Row r: logit class r % 7, depth class (r // 7) % 5."""
    codes = np.zeros((b, N_CAT), dtype=np.int16)
    nums = np.zeros((b, N_NUM), dtype=np.float32)
    r = np.arange(b)
    nums[:, 0] = r % len(GBT_LOGITS)
    nums[:, 1] = (r // len(GBT_LOGITS)) % GBT_DEPTH_CLASSES
    return codes, nums


# --------------------------------------------------- small cases of every family


def small_cases():
    """(name, model, codes, nums) at shapes the naive walker handles: what the
    CPU tests cross-check against cpu_ref and run the mutants on."""
    cases = []
    for t_cls, t_if, b in ((1, 2, 1), (3, 5, 65), (5, 3, 65), (129, 127, 257)):
        p = visit_once_model(t_cls, t_if)
        cases.append((f"visit_once_{t_cls}_{t_if}", p, *visit_once_rows(b, max(t_cls, t_if))))
    codes, nums = ragged_rows()
    for name, kinds in (("ragged_odd", RAGGED_ODD), ("ragged_even", RAGGED_EVEN)):
        cases.append((name, ragged_model(kinds), codes[:65], nums[:65]))
    cases.append(("edges", edge_model(), *edge_rows()))
    cases.append(("gbt", gbt_model(), *gbt_rows()))
    return cases

"""Hand-built forests, rows, independent references and deliberately wrong
references for the four attribution kernels (forest_contrib_kernel,
forest_shap_kernel, forest_shap_inter_kernel, forest_ishap_kernel): what
test_attr_cases.py (CPU) and test_attr_kernels_gpu.py share (no test in here).

Four forests on hand_model's layout (9 two-category columns, 14 numerics):

  transitions  long and short paths back to back in leaf order: the 23-group
               caterpillar, a stump, 17- and 16-player chains, root leaves, a
               chain that splits one numeric column three times and one
               categorical column on both codes, a 2-player tree
  stripes      (root-leaf tree, 2-leaf tree) repeated: leaves 0, 3, 6, ... are
               root leaves, so with three path chunks one chunk skips them all
  cover        zero-cover children, a fraction of exactly 1, a fraction of
               2^-20, two players that never share a path, unsplit columns
  threshold    small trees whose splits and rows sit on the f32 compare edges

The references walk the BFS trees themselves (cls_nodes, cls_node_cover,
cls_node_value, feat_col, feat_code, medians); none reads the path table or
cpu_ref. f32 values are widened to Python floats (exact, order-preserving), so
every compare is the f32 compare. Everything after the compares is exact:
Fractions and integers, converted to float once at the end. The cover
fraction of a child is f32(cover[child] / cover[parent]) (0 under a
zero-cover parent), the definition the path table and the brute-force oracles
of test_shap.py share.

  Saabas          sum of v[child] - v[node] per source column
  SHAP            v (o_i - z_i) int_0^1 prod_{p != i} (z_p (1-t) + o_p t) dt
  interactions    v/2 (o_i - z_i)(o_j - z_j) int_0^1 prod_{p != i,j} (...) dt
  interventional  +v (nx-1)! nr! / (nx+nr)! for x's players, -v (nr-1)! nx! /
                  (nx+nr)! for the background row's, over pairs with a | b full

The integrals are taken term by term in the Bernstein form: with e_s the
coefficients of prod (z_p + o_p y), prod (z_p (1-t) + o_p t) is
sum_s e_s t^s (1-t)^(n-s) and int t^s (1-t)^(n-s) dt = s! (n-s)! / (n+1)!.
"""

from __future__ import annotations

import dataclasses
import functools
import math
from fractions import Fraction

import numpy as np

from _shap_models import CATERPILLAR_SPLITS, N_ONEHOT, N_SRC, f32bits, hand_model
from creditcore.pack import N_CAT, N_NUM

METHODS = ("contrib", "shap", "inter", "ishap")
FORESTS = ("transitions", "stripes", "cover", "threshold")
ROWS = {"contrib": (1, 17, 129), "shap": (1, 17, 129), "ishap": (1, 17, 129),
        "inter": (1, 15, 17, 33)}  # fmt: skip
BG_ROWS = (1, 2, 129)
GBT_BIAS = 0.375
TINY = float(np.finfo(np.float32).smallest_subnormal)


def kinds_of(forest: str) -> tuple[int, ...]:
    """cls_kind values a forest is built with: 0 = mean over trees (scale
    1/T), 1 = sum plus bias."""
    return (0,) if forest == "threshold" else (0, 1)


# ---------------------------------------------------------------- tree builders


def leaf(v: float) -> list[int]:
    return [-1, f32bits(v), 0, 0]


def num(j: int) -> int:
    """Virtual feature of numeric column j."""
    return N_ONEHOT + j


def cat(c: int, code: int) -> int:
    """Virtual feature of (categorical column c == code)."""
    return 2 * c + code


def player_of(feat: int) -> int:
    return feat // 2 if feat < N_ONEHOT else N_CAT + feat - N_ONEHOT


def with_dirs(splits):
    """(feat, thr) -> (feat, thr, chain goes left): the caterpillar's mix."""
    return [(f, thr, i % 3 != 1) for i, (f, thr) in enumerate(splits)]


def chain_tree(splits, values, keeps, reverse: bool = False, cover0: float = 2.0**20):
    """One chain of (feat, thr, left) splits, every off-chain child a leaf.
    values: the off-chain leaf of each split, then the chain's end leaf.
    keeps: share of the cover that stays on the chain at each split.
    Forward layout (the caterpillar's): split i at node 2i, its leaf at 2i+1,
    so the leaves come shallow to deep in node order. Reverse layout: splits
    at nodes 0..n-1, then the end leaf and the off-chain leaves deep to
    shallow (children still follow their parent)."""
    n = len(splits)
    assert len(values) == n + 1 and len(keeps) == n
    nodes = np.zeros((2 * n + 1, 4), dtype=np.int32)
    cover = np.zeros(2 * n + 1, dtype=np.float64)
    at = (lambda i: i) if reverse else (lambda i: 2 * i)  # chain node i (n = end leaf)
    off = (lambda i: 2 * n - i) if reverse else (lambda i: 2 * i + 1)  # leaf of split i
    cover[at(0)] = cover0
    for i, (feat, thr, left) in enumerate(splits):
        k, on, out = at(i), at(i + 1), off(i)
        nodes[k] = [feat, f32bits(thr), on if left else out, out if left else on]
        nodes[out] = leaf(values[i])
        cover[on] = float(np.float32(cover[k] * keeps[i]))
        cover[out] = cover[k] - cover[on]
    nodes[at(n)] = leaf(values[n])
    return nodes, cover


def follower(splits):
    """A row (codes, nums) that follows every (feat, thr, left) split."""
    codes = np.zeros(N_CAT, dtype=np.int16)
    nums = np.zeros(N_NUM, dtype=np.float32)
    lo, hi = np.full(N_NUM, -np.inf), np.full(N_NUM, np.inf)
    must, never = {}, {}
    for feat, thr, left in splits:
        if feat < N_ONEHOT:  # one-hot <= 0.5 goes left: "is not this code"
            (never if left else must).setdefault(feat // 2, set()).add(feat % 2)
        elif left:
            hi[feat - N_ONEHOT] = min(hi[feat - N_ONEHOT], thr)
        else:
            lo[feat - N_ONEHOT] = max(lo[feat - N_ONEHOT], thr)
    for c in range(N_CAT):
        ok = [v for v in (0, 1, -1) if v not in never.get(c, ()) and must.get(c, {v}) == {v}]
        codes[c] = ok[0]
    for j in range(N_NUM):
        nums[j] = hi[j] - 0.125 if np.isfinite(hi[j]) else (lo[j] + 0.125 if np.isfinite(lo[j]) else 0.0)
        assert lo[j] < nums[j] <= hi[j]
    return codes, nums


def breaker(splits, row, i: int):
    """``row`` with split i of the chain failed."""
    codes, nums = row[0].copy(), row[1].copy()
    feat, thr, left = splits[i]
    if feat < N_ONEHOT:
        codes[feat // 2] = feat % 2 if left else (1 - feat % 2)
    else:
        nums[feat - N_ONEHOT] = thr + 1.0 if left else thr - 1.0
    return codes, nums


def _values(rng, n: int) -> list[float]:
    """n distinct multiples of 1/64 in [-1, 1], mixed in sign, 0.0 among them
    when n >= 3."""
    v = rng.choice(np.arange(-64, 65), size=n, replace=False) / 64.0
    if n >= 3 and not (v == 0.0).any():
        v[n // 2] = 0.0
    return v.tolist()


def _keeps(rng, n: int) -> list[float]:
    return (rng.choice(np.arange(33, 63, 2), size=n) / 64.0).tolist()


def _random_rows(rng, n: int, nan_share: float = 0.05):
    codes = rng.integers(-1, 2, size=(n, N_CAT)).astype(np.int16)
    nums = rng.normal(0.0, 2.0, size=(n, N_NUM)).astype(np.float32)
    nums[rng.uniform(size=nums.shape) < nan_share] = np.nan
    return codes, nums


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    trees: tuple
    covers: tuple
    codes: np.ndarray  # 129 explained rows; the smaller sets are prefixes
    nums: np.ndarray
    bg_codes: np.ndarray  # 129 background rows; R = 1, 2 are prefixes
    bg_nums: np.ndarray
    notes: dict = dataclasses.field(default_factory=dict)


def _finish(name, trees, covers, rows, bg, **notes) -> Case:
    codes = np.ascontiguousarray(rows[0][:129], dtype=np.int16)
    nums = np.ascontiguousarray(rows[1][:129], dtype=np.float32)
    bg_codes = np.ascontiguousarray(bg[0][:129], dtype=np.int16)
    bg_nums = np.ascontiguousarray(bg[1][:129], dtype=np.float32)
    assert len(codes) == len(bg_codes) == 129 and len(trees) <= 40
    # row 0 carries a NaN and an unknown category and is background row 0
    assert np.isnan(nums[0]).any() and (codes[0] == -1).any()
    bg_codes[0], bg_nums[0] = codes[0], nums[0]
    for r in BG_ROWS:
        assert np.isnan(bg_nums[:r]).any() and (bg_codes[:r] == -1).any()
    for a in (codes, nums, bg_codes, bg_nums):
        a.setflags(write=False)
    return Case(name, tuple(np.asarray(t, dtype=np.int32) for t in trees),
                tuple(np.asarray(c, dtype=np.float64) for c in covers),
                codes, nums, bg_codes, bg_nums, notes)  # fmt: skip


# -------------------------------------------------------- forest: transitions

CATERPILLAR = with_dirs(CATERPILLAR_SPLITS)  # 26 splits, 23 players
CHAIN17 = with_dirs(
    [(cat(c, 0), 0.5) for c in range(N_CAT)] + [(num(j), 0.5 * (j - 3)) for j in range(8)]
)
CHAIN16 = with_dirs(
    [(cat(c, 1), 0.5) for c in range(1, N_CAT)] + [(num(j), 0.25 * (9 - j)) for j in range(6, 14)]
)
# numeric 5 three times, categorical 2 on both of its codes, numeric 7 once
REPEAT = [
    (num(5), 1.0, True), (cat(2, 0), 0.5, True), (num(5), -1.0, False),
    (num(7), 0.25, True), (cat(2, 1), 0.5, False), (num(5), 0.0, True),
]  # fmt: skip
# Tree kinds in tree order: C / c the caterpillar in forward / reverse layout
# (leaves shallow to deep / deep to shallow), 1 a stump, s the 17-player chain
# in reverse layout, S the 16-player chain, 0 a root leaf, R the chain with
# repeated columns, 2 a 2-player tree. Group counts of consecutive leaves:
# 23 -> 1 (C1), 1 -> 17 (1s), 16 -> root (S0), root -> 23 (0c), 23 -> root
# (C0), root -> 1 (0C), 23 -> 17 (Cs), 1 -> root (s0).
TRANSITIONS = "C1sS0cR2C0Cs0"


def _and_tree(f0: int, f1: int, values, cover=(64.0, 16.0, 48.0, 12.0, 36.0)):
    nodes = [[f0, f32bits(0.0), 1, 2], leaf(values[0]), [f1, f32bits(0.0), 3, 4],
             leaf(values[1]), leaf(values[2])]  # fmt: skip
    return np.array(nodes, dtype=np.int32), np.array(cover)


@functools.lru_cache(maxsize=None)
def transitions_case() -> Case:
    rng = np.random.default_rng(41)
    cat_keeps = _keeps(rng, len(CATERPILLAR))  # every caterpillar shares its cover
    k17, k16 = _keeps(rng, 17), _keeps(rng, 16)
    trees, covers = [], []
    for kind in TRANSITIONS:
        if kind in "Cc":
            t = chain_tree(CATERPILLAR, _values(rng, 27), cat_keeps, reverse=kind == "c")
        elif kind == "1":
            t = chain_tree([(num(9), 0.5, True)], _values(rng, 2), [0.75])
        elif kind == "s":
            t = chain_tree(CHAIN17, _values(rng, 18), k17, reverse=True)
        elif kind == "S":
            t = chain_tree(CHAIN16, _values(rng, 17), k16)
        elif kind == "0":
            t = (np.array([leaf(_values(rng, 1)[0])], dtype=np.int32), np.array([8.0]))
        elif kind == "R":
            t = chain_tree(REPEAT, _values(rng, 7), _keeps(rng, 6))
        else:
            t = _and_tree(num(0), num(1), _values(rng, 3))
        trees.append(t[0])
        covers.append(t[1])

    rows = []
    top = follower(CATERPILLAR)
    j = next(j for j in range(N_NUM) if _median_follows(CATERPILLAR, j))
    first = (top[0].copy(), top[1].copy())
    first[1][j] = np.nan  # the median of column j satisfies the chain as well
    rows.append(first)
    rows.append(top)
    for chain, cuts in ((CATERPILLAR, (0, 4, 9, 15, 22, 23, 25)), (CHAIN17, (16, 8)),
                        (CHAIN16, (15, 3)), (REPEAT, (5, 2))):  # fmt: skip
        if chain is not CATERPILLAR:
            rows.append(follower(chain))
        rows += [breaker(chain, follower(chain), i) for i in cuts]
    rc, rn = _random_rows(rng, 129 - len(rows))
    codes = np.concatenate([np.stack([r[0] for r in rows]), rc])
    nums = np.concatenate([np.stack([r[1] for r in rows]), rn])
    return _finish("transitions", trees, covers, (codes, nums), _random_rows(rng, 129),
                   nan_col=j)  # fmt: skip


def hand_medians() -> np.ndarray:
    return np.linspace(-1.0, 1.0, N_NUM).astype(np.float32)  # hand_model's


def _median_follows(chain, j: int) -> bool:
    """Does the median of numeric column j satisfy every split of the chain
    on that column?"""
    m = float(hand_medians()[j])
    own = [(thr, left) for f, thr, left in chain if f == num(j)]
    return bool(own) and all((m <= thr) == left for thr, left in own)


# ------------------------------------------------------------ forest: stripes


@functools.lru_cache(maxsize=None)
def stripes_case() -> Case:
    rng = np.random.default_rng(43)
    feats = [num(0), cat(0, 0), num(3), cat(4, 1), num(13), cat(8, 0), num(6), cat(0, 1),
             num(3), cat(7, 1), num(10), num(0)]  # fmt: skip
    trees, covers = [], []
    for i, f in enumerate(feats):
        trees.append(np.array([leaf(0.0 if i == 1 else _values(rng, 1)[0])], dtype=np.int32))
        covers.append(np.array([16.0]))
        thr = 0.5 if f < N_ONEHOT else float(np.float32(rng.normal(0.0, 1.0)))
        v = _values(rng, 2)
        if i == 2:
            v[0] = 0.0
        trees.append(np.array([[f, f32bits(thr), 1, 2], leaf(v[0]), leaf(v[1])], dtype=np.int32))
        covers.append(np.array([64.0, 64.0 * (k := float(_keeps(rng, 1)[0])), 64.0 * (1.0 - k)]))
    rows = _random_rows(rng, 129)
    rows[0][0, 0], rows[1][0, 3] = -1, np.nan
    return _finish("stripes", trees, covers, rows, _random_rows(rng, 129))


# -------------------------------------------------------------- forest: cover

# Every tree of the cover forest owns its columns, so an exact zero of a
# column can be traced to one tree. Unsplit: numerics 9..13, categoricals 4..8.
COVER_UNSPLIT = tuple(range(4, N_CAT)) + tuple(N_CAT + j for j in range(9, N_NUM))


@functools.lru_cache(maxsize=None)
def cover_case() -> Case:
    rng = np.random.default_rng(47)
    v = lambda n: _values(rng, n)  # noqa: E731
    trees, covers = [], []
    # a: numeric 0 at the root, nothing ever went right; numeric 1 below it.
    #    A row that goes left follows z = 1 and is off the z = 0 group of the
    #    other two paths: the whole tree credits it exactly 0.
    trees.append(_and_tree(num(0), num(1), v(3))[0])
    covers.append([100.0, 100.0, 0.0, 0.0, 0.0])
    # b: numeric 5 at the root, nothing ever went left (the right child has
    #    the root's whole cover: fraction exactly 1); numeric 6 below it.
    trees.append(_and_tree(num(5), num(6), v(3))[0])
    covers.append([64.0, 0.0, 64.0, 32.0, 32.0])
    # c: a fraction of 2^-20 next to 1 - 2^-20; categorical 3 below
    trees.append(_and_tree(num(7), cat(3, 1), v(3))[0])
    trees[-1][2, 1] = f32bits(0.5)
    covers.append([2.0**20, 1.0, 2.0**20 - 1.0, 2.0**18, 2.0**20 - 1.0 - 2.0**18])
    # d: numerics 3 and 4 never share a path
    val = v(4)
    trees.append(np.array(
        [[num(2), f32bits(0.0), 1, 2], [num(3), f32bits(0.0), 3, 4], [num(4), f32bits(0.0), 5, 6],
         leaf(val[0]), leaf(val[1]), leaf(val[2]), leaf(val[3])], dtype=np.int32))  # fmt: skip
    covers.append([64.0, 16.0, 48.0, 4.0, 12.0, 24.0, 24.0])
    # e: three levels, categorical 0 on both codes, a zero-cover subtree deeper
    val = v(5)
    trees.append(np.array(
        [[cat(0, 0), f32bits(0.5), 1, 2], [cat(0, 1), f32bits(0.5), 3, 4], leaf(val[0]),
         [num(8), f32bits(0.25), 5, 6], [cat(1, 0), f32bits(0.5), 7, 8],
         leaf(val[1]), leaf(val[2]), leaf(val[3]), leaf(val[4])], dtype=np.int32))  # fmt: skip
    covers.append([32.0, 24.0, 8.0, 24.0, 0.0, 6.0, 18.0, 0.0, 0.0])
    # f: numeric 8 and categorical 2 with ordinary covers
    trees.append(_and_tree(num(8), cat(2, 0), v(3))[0])
    trees[-1][2, 1] = f32bits(0.5)
    covers.append([64.0, 16.0, 48.0, 12.0, 36.0])
    rows = _random_rows(rng, 129)
    rows[0][0, 0], rows[1][0, 5] = -1, np.nan
    # rows 1..4: both sides of the zero-cover splits of trees a and b
    rows[1][1:5, 0] = [-1.0, 1.0, -1.0, 1.0]
    rows[1][1:5, 1] = [1.0, 1.0, -1.0, -1.0]
    rows[1][1:5, 5] = [1.0, -1.0, -1.0, 1.0]
    rows[1][1:5, 6] = [1.0, 1.0, -1.0, -1.0]
    return _finish("cover", trees, covers, rows, _random_rows(rng, 129))


# ---------------------------------------------------------- forest: threshold

THRESHOLD_EDGES = (
    "eq", "up", "down", "zero_neg", "zero_pos", "zero_tiny", "zero_neg_tiny", "pos_inf",
    "neg_inf", "nan_median_eq", "nan_median_up",
    "cat_0_-1", "cat_0_0", "cat_0_1", "cat_1_-1", "cat_1_0", "cat_1_1",
)  # fmt: skip


def _up(x) -> float:
    return float(np.nextafter(np.float32(x), np.float32(np.inf)))


def _down(x) -> float:
    return float(np.nextafter(np.float32(x), np.float32(-np.inf)))


@functools.lru_cache(maxsize=None)
def threshold_case() -> Case:
    """Every tree has an edge split and two companion splits (numeric 12,
    categorical 8), so that interactions exist and no tree has more than four
    players. ``notes['neighbours']`` are pairs of rows that differ in one
    column and lie on the two sides of a compare edge."""
    rng = np.random.default_rng(53)
    med = hand_medians()
    thr = {0: 1.5, 1: 0.0, 2: float(med[2]), 3: _down(med[3]), 4: -2.5}

    def edge_tree(feat, t):
        v = _values(rng, 4)
        return np.array(
            [[feat, f32bits(t), 1, 2], [num(12), f32bits(0.25), 3, 4],
             [cat(8, 1), f32bits(0.5), 5, 6], leaf(v[0]), leaf(v[1]), leaf(v[2]), leaf(v[3])],
            dtype=np.int32)  # fmt: skip

    trees = [edge_tree(num(j), t) for j, t in thr.items()]
    trees += [edge_tree(cat(0, 0), 0.5), edge_tree(cat(0, 1), 0.5)]
    # the same two thresholds one level down, on a right- and a left-going path
    v = _values(rng, 4)
    trees.append(np.array(
        [[num(11), f32bits(0.0), 1, 2], [num(1), f32bits(0.0), 3, 4], [num(0), f32bits(1.5), 5, 6],
         leaf(v[0]), leaf(v[1]), leaf(v[2]), leaf(v[3])], dtype=np.int32))  # fmt: skip
    covers = [[64.0, 16.0, 48.0, 4.0, 12.0, 24.0, 24.0]] * len(trees)

    # row 0: NaNs and unknown categories; then two base rows and their edges
    rows_c, rows_n, neighbours = [], [], []

    def add(base, col=None, value=None):
        c, x = base[0].copy(), base[1].copy()
        if col is not None and col < N_CAT:
            c[col] = value
        elif col is not None:
            x[col - N_CAT] = value
        rows_c.append(c)
        rows_n.append(x)
        return len(rows_c) - 1

    base1 = (np.zeros(N_CAT, dtype=np.int16), np.full(N_NUM, 0.5, dtype=np.float32))
    base2 = (np.ones(N_CAT, dtype=np.int16), np.full(N_NUM, -0.5, dtype=np.float32))
    first = add(base1)
    rows_c[first][[0, 5]] = -1
    rows_n[first][[2, 3]] = np.nan
    for base in (base1, base2):
        n = lambda j: N_CAT + j  # noqa: E731
        eq, up, down = add(base, n(0), 1.5), add(base, n(0), _up(1.5)), add(base, n(0), _down(1.5))
        zp, zn = add(base, n(1), 0.0), add(base, n(1), -0.0)
        tp, tn = add(base, n(1), TINY), add(base, n(1), -TINY)
        nan2, up2, eq2 = add(base, n(2), np.nan), add(base, n(2), _up(med[2])), add(base, n(2), med[2])
        nan3, eq3 = add(base, n(3), np.nan), add(base, n(3), thr[3])
        pinf, ninf = add(base, n(4), np.inf), add(base, n(4), -np.inf)
        c_unk, c0, c1 = add(base, 0, -1), add(base, 0, 0), add(base, 0, 1)
        neighbours += [(eq, up), (down, up), (zp, tp), (zn, tp), (tn, tp), (nan2, up2),
                       (eq2, up2), (eq3, nan3), (ninf, pinf), (c0, c_unk), (c1, c_unk),
                       (c0, c1)]  # fmt: skip
    n_edge = len(rows_c)
    # the rest: every column draws from its own edge values
    pools = {0: [1.5, _up(1.5), _down(1.5), np.inf], 1: [0.0, -0.0, TINY, -TINY],
             2: [np.nan, float(med[2]), _up(med[2])], 3: [np.nan, thr[3], float(med[3])],
             4: [np.inf, -np.inf, -2.5], 11: [-1.0, 1.0, 0.0], 12: [0.25, _up(0.25), -1.0]}  # fmt: skip

    def draw(n):
        c = rng.integers(-1, 2, size=(n, N_CAT)).astype(np.int16)
        x = rng.normal(0.0, 1.0, size=(n, N_NUM)).astype(np.float32)
        for j, pool in pools.items():
            x[:, j] = rng.choice(np.array(pool, dtype=np.float32), size=n)
        return c, x

    rc, rn = draw(129 - n_edge)
    codes = np.concatenate([np.stack(rows_c), rc])
    nums = np.concatenate([np.stack(rows_n), rn])
    bg = draw(129)
    bg[0][1], bg[1][1] = base2[0], base2[1]
    return _finish("threshold", trees, covers, (codes, nums), bg,
                   neighbours=tuple(neighbours), n_edge=n_edge)  # fmt: skip


def case(forest: str) -> Case:
    return {"transitions": transitions_case, "stripes": stripes_case, "cover": cover_case,
            "threshold": threshold_case}[forest]()  # fmt: skip


@functools.lru_cache(maxsize=None)
def model(forest: str, cls_kind: int = 0):
    c = case(forest)
    return hand_model(list(c.trees), list(c.covers), cls_kind=cls_kind,
                      cls_bias=GBT_BIAS * cls_kind)  # fmt: skip


@functools.lru_cache(maxsize=None)
def small_tree_model(forest: str):
    """The trees of a forest with at most 9 players (the brute-force cap) as
    a forest of their own, averaging."""
    c = case(forest)
    keep = [
        i for i, t in enumerate(c.trees)
        if len({player_of(int(f)) for f in t[:, 0] if f >= 0}) <= 9
    ]  # fmt: skip
    return hand_model([c.trees[i] for i in keep], [c.covers[i] for i in keep])


def launch_chunks(block_target: int, row_blocks: int, n_paths: int) -> int:
    """gridDim.y of the four launchers (csrc forest_contrib() ... forest_ishap())."""
    return max(1, min(-(-block_target // row_blocks), n_paths))


# ----------------------------------------------------------------- tree walk

ATTR_MUTATIONS = (
    "lt",  # v < thr in place of v <= thr
    "no_impute",  # NaN in explained rows is not replaced by the median
    "bg_no_impute",  # NaN in background rows is not replaced by the median
    "ignore_unknown",  # the unknown category -1 is taken for category 0
    "split_players",  # every split is a player of its own (no group fold)
    "last_split_only",  # a group's o and z come from its last split alone
    "drop_last_leaf",  # the last leaf is never visited
    "root_leaf_breaks",  # a root-leaf path ends its chunk instead of being skipped
    "no_scale",  # the 1/T of the averaging forest is left out
    "zero_cover_credit",  # off a z = 0 group: -v * s0 (z "cancelled") instead of 0
    "asym",  # the interaction lands in one triangle only
)

# which mutation changes which method (a mutation outside its methods is the
# reference itself)
MUTATION_METHODS = {
    "lt": METHODS,
    "no_impute": METHODS,
    "bg_no_impute": ("ishap",),
    "ignore_unknown": METHODS,
    "split_players": ("shap", "inter", "ishap"),
    "last_split_only": ("shap", "inter", "ishap"),
    "drop_last_leaf": ("shap", "inter", "ishap"),
    "root_leaf_breaks": ("shap", "inter", "ishap"),
    "no_scale": METHODS,
    "zero_cover_credit": ("shap",),
    "asym": ("inter",),
}


@dataclasses.dataclass(frozen=True)
class Leaf:
    tree: int
    value: Fraction
    path: tuple  # (feat, thr, went right, Fraction frac) from the root down


class Walk:
    """A packed model as plain Python lists (f32 widened to float)."""

    def __init__(self, p):
        self.p = p
        self.nodes = p.cls_nodes.tolist()
        self.thr = p.cls_nodes[:, 1].view(np.float32).tolist()
        self.off = p.cls_tree_offsets.tolist()
        self.cover = np.asarray(p.cls_node_cover, dtype=np.float32).tolist()
        self.value = np.asarray(p.cls_node_value, dtype=np.float32).tolist()
        self.col, self.code = p.feat_col.tolist(), p.feat_code.tolist()
        self.n_trees = len(self.off) - 1

    def rows(self, codes, nums, impute: bool = True):
        x = np.asarray(nums, dtype=np.float32)
        if impute:
            x = np.where(np.isnan(x), self.p.medians[None, :], x).astype(np.float32)
        return list(zip(np.asarray(codes).tolist(), x.tolist()))

    def right(self, feat: int, thr: float, row, mutation=None) -> bool:
        """Does the row take the right child? NaN compares false: right."""
        c, x = row
        if self.code[feat] >= 0:
            have = c[self.col[feat]]
            if mutation == "ignore_unknown":
                have = max(have, 0)
            v = 1.0 if have == self.code[feat] else 0.0
        else:
            v = x[self.col[feat]]
        return not (v < thr if mutation == "lt" else v <= thr)

    def frac(self, child: int, parent: int) -> Fraction:
        if self.cover[parent] <= 0.0:
            return Fraction(0)
        return Fraction(float(np.float32(self.cover[child] / self.cover[parent])))

    @functools.cached_property
    def leaves(self) -> list[Leaf]:
        """Every leaf in node order, the order of the path table."""
        out = []
        for t in range(self.n_trees):
            lo, hi = self.off[t], self.off[t + 1]
            parent = {}
            for k in range(lo, hi):
                if self.nodes[k][0] >= 0:
                    parent[lo + self.nodes[k][2]] = (k, False)
                    parent[lo + self.nodes[k][3]] = (k, True)
            for k in range(lo, hi):
                if self.nodes[k][0] >= 0:
                    continue
                path, c = [], k
                while c in parent:
                    q, right = parent[c]
                    path.append((self.nodes[q][0], self.thr[q], right, self.frac(c, q)))
                    c = q
                assert c == lo
                out.append(Leaf(t, Fraction(self.thr[k]), tuple(reversed(path))))
        return out

    def visited(self, mutation=None, chunks: int = 1) -> list[Leaf]:
        leaves = self.leaves
        if mutation == "drop_last_leaf":
            return leaves[:-1]
        if mutation == "root_leaf_breaks":
            out = []
            for c in range(chunks):
                for k in range(c, len(leaves), chunks):
                    if not leaves[k].path:
                        break
                    out.append(leaves[k])
            return out
        return leaves

    def scale(self, mutation=None) -> Fraction:
        if self.p.cls_kind == 1 or mutation == "no_scale":
            return Fraction(1)
        return Fraction(1, self.n_trees)


def groups_of(lf: Leaf, mutation=None):
    """Player groups of a path: [player, z, [(feat, thr, right), ...]]."""
    g = {}
    for i, (feat, thr, right, fr) in enumerate(lf.path):
        pl = player_of(feat)
        cur = g.setdefault((pl, i) if mutation == "split_players" else pl, [pl, Fraction(1), []])
        if mutation == "last_split_only":
            cur[1], cur[2] = fr, [(feat, thr, right)]
        else:
            cur[1] *= fr
            cur[2].append((feat, thr, right))
    return list(g.values())


def _follows(w: Walk, group, row, mutation) -> bool:
    return all(w.right(f, thr, row, mutation) == right for f, thr, right in group[2])


def _to_float(a, scale: Fraction) -> np.ndarray:
    flat = [float(v * scale) for v in np.asarray(a, dtype=object).ravel()]
    return np.array(flat, dtype=np.float64).reshape(np.shape(a))


# ------------------------------------------------------------------- Saabas


def naive_output(p, codes, nums) -> np.ndarray:
    """Raw model output per row (probability, or the logit for cls_kind 1):
    the walk to the leaf, summed exactly."""
    w = Walk(p)
    out = []
    for row in w.rows(codes, nums):
        s = Fraction(0)
        for t in range(w.n_trees):
            k = w.off[t]
            while w.nodes[k][0] >= 0:
                go = w.right(w.nodes[k][0], w.thr[k], row)
                k = w.off[t] + w.nodes[k][3 if go else 2]
            s += Fraction(w.thr[k])
        out.append(float(s * w.scale() + Fraction(float(p.cls_bias)) * (p.cls_kind == 1)))
    return np.array(out)


def _raw_contrib(w: Walk, codes, nums, mutation=None, chunks: int = 1):
    out = []
    for row in w.rows(codes, nums, impute=mutation != "no_impute"):
        acc = [Fraction(0)] * N_SRC
        for t in range(w.n_trees):
            k = w.off[t]
            while w.nodes[k][0] >= 0:
                feat = w.nodes[k][0]
                nxt = w.off[t] + w.nodes[k][3 if w.right(feat, w.thr[k], row, mutation) else 2]
                acc[player_of(feat)] += Fraction(w.value[nxt]) - Fraction(w.value[k])
                k = nxt
        out.append(acc)
    return out, 1


def ref_contrib(p, codes, nums, mutation=None, chunks: int = 1) -> np.ndarray:
    """Prediction-path attributions f64[B, 23]."""
    w = Walk(p)
    raw, den = _raw_contrib(w, codes, nums, mutation, chunks)
    return _to_float(raw, w.scale(mutation) / den)


# ---------------------------------------------------- SHAP and interactions


def _mul(poly, a: int, b: int):
    """poly(y) * (a + b y), integer coefficients."""
    out = [0] * (len(poly) + 1)
    for k, c in enumerate(poly):
        out[k] += c * a
        out[k + 1] += c * b
    return out


def _div(poly, a: int, b: int):
    """poly(y) / (a + b y), exact (the factor is one of the product's)."""
    n = len(poly) - 1
    q = [0] * n
    if b == 0:
        assert a != 0 and poly[n] == 0
        for k in range(n):
            q[k], r = divmod(poly[k], a)
            assert r == 0
        return q
    carry = 0
    for k in range(n, 0, -1):
        q[k - 1], r = divmod(poly[k] - carry, b)
        assert r == 0
        carry = a * q[k - 1]
    assert poly[0] == carry
    return q


_FACT = [math.factorial(k) for k in range(34)]
_FBASE = _FACT[32]  # every m! of a path divides it (a path has at most 26 splits)


def _lam(e, n: int) -> int:
    """(n+1)! int_0^1 sum_s e_s t^s (1-t)^(n-s) dt = sum_s e_s s! (n-s)!.
    A coefficient above n is left out: it occurs only in differences in
    which it cancels (_inter_unit)."""
    return sum(c * _FACT[s] * _FACT[n - s] for s, c in enumerate(e[: n + 1]))


def _prod(xs) -> int:
    return math.prod(xs)


class _PathTerms:
    """The factors of one (path, row). z_p = N_p / D_p with D_p a power of
    two (a product of f32 values). A followed group has the factor
    z_p + y = (N_p + D_p y) / D_p, the others the constant z_p. p1 is the
    integer product of the followed groups' numerators, q[i] = p1 without
    group i, n0 the product of the N_p of the other groups; K = log2 of the
    product of every D_p, the one power of two all results are written over."""

    def __init__(self, zs, os):
        self.N = [z.numerator for z in zs]
        self.D = [z.denominator for z in zs]
        assert all(d & (d - 1) == 0 for d in self.D)
        self.m = len(zs)
        self.one = [i for i, o in enumerate(os) if o]
        self.zero = [i for i, o in enumerate(os) if not o]
        self.p1 = [1]
        for i in self.one:
            self.p1 = _mul(self.p1, self.N[i], self.D[i])
        self.q = {i: _div(self.p1, self.N[i], self.D[i]) for i in self.one}
        self.n0 = _prod(self.N[i] for i in self.zero)
        self.K = sum(d.bit_length() - 1 for d in self.D)


@functools.lru_cache(maxsize=None)
def _shap_unit(zs: tuple, os: tuple, zero_cover_credit: bool = False):
    """Per group i of a path with unit leaf value,
    (o_i - z_i) int prod_{p != i} (z_p (1-t) + o_p t) dt,
    as (integers u_i, m, K): the values are u_i / (m! 2^K).
    With Z0 the product of the z_p of the groups not followed:
      o_i = 0: -z_i * (Z0 / z_i) int p1 = -Z0 int p1, the same for each;
      o_i = 1: (1 - z_i) Z0 int q_i."""
    t = _PathTerms(zs, os)
    n = t.m - 1
    u = [0] * t.m
    off = -t.n0 * _lam(t.p1, n) if t.zero else 0
    for i in t.zero:
        u[i] = off
        if zero_cover_credit and t.N[i] == 0:  # Z0 / z_i "cancelled" at z_i = 0
            u[i] = -_prod(t.N[k] for k in t.zero if k != i) * t.D[i] * _lam(t.p1, n)
    for i in t.one:
        u[i] = (t.D[i] - t.N[i]) * t.n0 * _lam(t.q[i], n)
    return tuple(u), t.m, t.K


@functools.lru_cache(maxsize=None)
def _inter_unit(zs: tuple, os: tuple):
    """Per group pair i < j of a path with unit leaf value,
    1/2 (o_i - z_i)(o_j - z_j) int prod_{p != i,j} (z_p (1-t) + o_p t) dt,
    as (((i, j, integer u), ...) without the zeros, m, K): the values are
    u / (2 (m-1)! 2^K). Neither followed: Z0 int p1, the same for each pair;
    j followed: -Z0 (1 - z_j) int q_j, the same for each i; both followed:
    (1 - z_i)(1 - z_j) Z0 int q_ij with q_ij = p1 without i and j, which is
    (D_j q_j - D_i q_i) / (D_j N_i - D_i N_j) where z_i != z_j."""
    t = _PathTerms(zs, os)
    n = t.m - 2
    if t.n0 == 0:
        return (), t.m, t.K
    out = []
    if len(t.zero) >= 2:
        u00 = t.n0 * _lam(t.p1, n)
        out += [(i, j, u00) for a, i in enumerate(t.zero) for j in t.zero[a + 1 :]]
    lam = {i: _lam(t.q[i], n) for i in t.one}
    for j in t.one:
        if t.D[j] == t.N[j]:
            continue
        u01 = -t.n0 * (t.D[j] - t.N[j]) * lam[j]
        out += [(min(i, j), max(i, j), u01) for i in t.zero]
        for i in t.one:
            if i >= j or t.D[i] == t.N[i]:
                continue
            c = t.D[j] * t.N[i] - t.D[i] * t.N[j]
            if c:
                lam_ij, r = divmod(t.D[j] * lam[j] - t.D[i] * lam[i], c)
                assert r == 0
            else:
                lam_ij = _lam(_div(t.q[j], t.N[i], t.D[i]), n)
            out.append((i, j, (t.D[i] - t.N[i]) * (t.D[j] - t.N[j]) * t.n0 * lam_ij))
    return tuple(x for x in out if x[2]), t.m, t.K


def _max_k(leaves) -> int:
    """An upper bound of K over the paths of a walk, whatever the grouping."""
    return max(
        (sum(fr.denominator.bit_length() - 1 for *_, fr in lf.path) for lf in leaves), default=0
    )


def _raw_shap(w: Walk, codes, nums, mutation=None, chunks: int = 1):
    rows = w.rows(codes, nums, impute=mutation != "no_impute")
    leaves = w.visited(mutation, chunks)
    vden = math.lcm(*(lf.value.denominator for lf in leaves))
    kmax = _max_k(leaves)
    acc = [[0] * N_SRC for _ in rows]  # over 32! 2^kmax vden
    for lf in leaves:
        groups = groups_of(lf, mutation)
        if not groups:
            continue
        zs = tuple(g[1] for g in groups)
        v = int(lf.value * vden)
        for r, row in enumerate(rows):
            os = tuple(int(_follows(w, g, row, mutation)) for g in groups)
            unit, m, k = _shap_unit(zs, os, mutation == "zero_cover_credit")
            lift = v * (_FBASE // _FACT[m]) << (kmax - k)
            for g, u in zip(groups, unit):
                if u:
                    acc[r][g[0]] += lift * u
    return acc, (_FBASE << kmax) * vden


def ref_shap(p, codes, nums, mutation=None, chunks: int = 1) -> np.ndarray:
    """Exact path-dependent TreeSHAP f64[B, 23]."""
    w = Walk(p)
    raw, den = _raw_shap(w, codes, nums, mutation, chunks)
    return _to_float(raw, w.scale(mutation) / den)


def _raw_inter(w: Walk, codes, nums, mutation=None, chunks: int = 1):
    rows = w.rows(codes, nums, impute=mutation != "no_impute")
    leaves = w.visited(mutation, chunks)
    vden = math.lcm(*(lf.value.denominator for lf in leaves))
    kmax = _max_k(leaves)
    acc = [[[0] * N_SRC for _ in range(N_SRC)] for _ in rows]  # over 2 32! 2^kmax vden
    for lf in leaves:
        groups = groups_of(lf, mutation)
        if len(groups) < 2:
            continue
        zs = tuple(g[1] for g in groups)
        v = int(lf.value * vden)
        pl = [g[0] for g in groups]
        for r, row in enumerate(rows):
            os = tuple(int(_follows(w, g, row, mutation)) for g in groups)
            unit, m, k = _inter_unit(zs, os)
            lift = v * (_FBASE // _FACT[m - 1]) << (kmax - k)
            upper = acc[r]
            for i, j, u in unit:
                a, b = pl[i], pl[j]
                if a < b:
                    upper[a][b] += lift * u
                elif b < a:  # a == b, split_players only: a column paired with itself
                    upper[b][a] += lift * u
    if mutation != "asym":
        for upper in acc:
            for a in range(N_SRC):
                for b in range(a):
                    upper[a][b] = upper[b][a]
    return acc, 2 * (_FBASE << kmax) * vden


def ref_inter(p, codes, nums, mutation=None, chunks: int = 1) -> np.ndarray:
    """Off-diagonal SHAP interaction values f64[B, 23, 23], symmetric, each
    entry half of the pair's interaction index; the diagonal is zero."""
    w = Walk(p)
    raw, den = _raw_inter(w, codes, nums, mutation, chunks)
    return _to_float(raw, w.scale(mutation) / den)


def ref_shap_base(p) -> float:
    """Cover-weighted expectation of the raw model output."""
    w = Walk(p)
    total = Fraction(0)
    for lf in w.leaves:
        reach = Fraction(1)
        for *_, fr in lf.path:
            reach *= fr
        total += lf.value * reach
    return float(total * w.scale() + Fraction(float(p.cls_bias)) * (p.cls_kind == 1))


# ----------------------------------------------------------- interventional


@functools.lru_cache(maxsize=None)
def _pair_weights():
    """W[a][b] = (a-1)! b! / (a+b)! as integers over one denominator."""
    f = math.factorial
    w = [[Fraction(f(a - 1) * f(b), f(a + b)) if a else Fraction(0) for b in range(N_SRC + 1)]
         for a in range(N_SRC + 1)]  # fmt: skip
    den = math.lcm(*(x.denominator for row in w for x in row))
    return [[int(x * den) for x in row] for row in w], den


def _bits(m: int):
    k = 0
    while m:
        if m & 1:
            yield k
        m >>= 1
        k += 1


def _raw_ishap(w: Walk, codes, nums, bg_codes, bg_nums, mutation=None, chunks: int = 1):
    rows = w.rows(codes, nums, impute=mutation != "no_impute")
    bg = w.rows(bg_codes, bg_nums, impute=mutation != "bg_no_impute")
    wi, wden = _pair_weights()
    leaves = w.visited(mutation, chunks)
    vden = math.lcm(*(lf.value.denominator for lf in leaves))
    acc = [[0] * N_SRC for _ in rows]
    for lf in leaves:
        groups = groups_of(lf, mutation)
        if not groups:
            continue
        v = int(lf.value * vden)
        full = (1 << len(groups)) - 1
        mask = lambda row: sum(  # noqa: E731
            int(_follows(w, g, row, mutation)) << k for k, g in enumerate(groups)
        )
        by_a, n_b = {}, {}
        for r, row in enumerate(rows):
            by_a.setdefault(mask(row), []).append(r)
        for row in bg:
            b = mask(row)
            n_b[b] = n_b.get(b, 0) + 1
        for a, own in by_a.items():
            for b, count in n_b.items():
                if (a | b) != full or a == b:
                    continue
                mx, mr = a & ~b, b & ~a
                nx, nr = bin(mx).count("1"), bin(mr).count("1")
                wp, wn = v * wi[nx][nr] * count, v * wi[nr][nx] * count
                for k in _bits(mx):
                    for r in own:
                        acc[r][groups[k][0]] += wp
                for k in _bits(mr):
                    for r in own:
                        acc[r][groups[k][0]] -= wn
    return acc, vden * wden * len(bg)


def ref_ishap(p, codes, nums, bg_codes, bg_nums, mutation=None, chunks: int = 1) -> np.ndarray:
    """Interventional Shapley values f64[B, 23] against the background rows."""
    w = Walk(p)
    raw, den = _raw_ishap(w, codes, nums, bg_codes, bg_nums, mutation, chunks)
    return _to_float(raw, w.scale(mutation) / den)


def ref_ishap_base(p, bg_codes, bg_nums) -> float:
    """Mean raw model output over the background rows."""
    return float(np.mean(naive_output(p, bg_codes, bg_nums)))


# ------------------------------------------------- shared, computed only once


@functools.lru_cache(maxsize=None)
def _raw_reference(forest: str, method: str, n_bg: int):
    """Exact unscaled values at the method's largest row set (the smaller
    sets are prefixes: a row's values do not depend on the other rows). The
    two builds of a forest share their trees, so they share these."""
    c, w = case(forest), Walk(model(forest, 0))
    b = max(ROWS[method])
    if method == "ishap":
        return _raw_ishap(w, c.codes[:b], c.nums[:b], c.bg_codes[:n_bg], c.bg_nums[:n_bg])
    fn = {"contrib": _raw_contrib, "shap": _raw_shap, "inter": _raw_inter}[method]
    return fn(w, c.codes[:b], c.nums[:b])


@functools.lru_cache(maxsize=None)
def reference(forest: str, cls_kind: int, method: str, n_bg: int = 0) -> np.ndarray:
    """Reference values of one build, read-only: the exact values times the
    build's scale (1/T, or 1 for cls_kind 1), rounded once."""
    assert (n_bg > 0) == (method == "ishap")
    raw, den = _raw_reference(forest, method, n_bg)
    out = _to_float(raw, Walk(model(forest, cls_kind)).scale() / den)
    out.setflags(write=False)
    return out

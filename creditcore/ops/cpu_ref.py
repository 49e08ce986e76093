"""CPU reference scorer over the packed flat-buffer model.

This is (a) the golden reference the HIP kernels are tested against and
(b) the no-GPU serving fallback. It deliberately uses float32 comparisons and
arithmetic with the same semantics as csrc/creditcore_kernels.hip, so GPU-vs-CPU
tests can use tight tolerances; CPU-ref-vs-sklearn tests use loose tolerances
(f32 vs f64 threshold rounding can flip a measure-zero set of branches).
"""

from __future__ import annotations

import numpy as np

from ..models.drift import chi2_from_counts, ks_2samp_d, ks_asymp_pvalue
from ..pack import N_CAT, N_NUM, PackedModel


def impute_nums(packed: PackedModel, nums: np.ndarray) -> np.ndarray:
    nums = np.asarray(nums, dtype=np.float32)
    out = np.where(np.isnan(nums), packed.medians[None, :], nums)
    return np.ascontiguousarray(out, dtype=np.float32)


def _traverse_forest(
    nodes: np.ndarray,
    offsets: np.ndarray,
    value_of: "callable",
    n_rows: int,
    tree_order: bool = False,
) -> np.ndarray:
    """Sum of leaf values over all trees, per row. ``tree_order`` adds the
    leaves of a row strictly in tree order (tree 0 first) and not in the
    order the walks end, which is the sum a thread that owns all trees of a
    row computes (forest_whatif_kernel): bit-identical, and monotone in a
    feature wherever every tree is.

    Level-synchronous and vectorised over ALL (tree, row) pairs at once:
    every pair advances one node per iteration, so the loop count is the
    max tree depth (~20) instead of trees x depth — the per-tree version
    cost ~8500 numpy dispatches for a single-row request."""
    bits = nodes[:, 1].view(np.float32)
    T = len(offsets) - 1
    starts = offsets[:-1].astype(np.int64)
    # absolute node index per (tree, row) pair, flattened
    cur = np.repeat(starts, n_rows)
    base = cur.copy()
    rows = np.tile(np.arange(n_rows, dtype=np.int64), T)
    acc = np.zeros(n_rows, dtype=np.float64)
    leaf_of = np.zeros(T * n_rows, dtype=np.float64) if tree_order else None
    alive = np.arange(T * n_rows, dtype=np.int64)
    while len(alive):
        nidx = cur[alive]
        feat = nodes[nidx, 0]
        leaf = feat < 0
        if leaf.any():
            done = alive[leaf]
            if tree_order:
                leaf_of[done] = bits[cur[done]].astype(np.float64)
            else:
                np.add.at(acc, rows[done], bits[cur[done]].astype(np.float64))
            alive = alive[~leaf]
            if not len(alive):
                break
            nidx = cur[alive]
            feat = nodes[nidx, 0]
        v = value_of(rows[alive], feat)
        go_left = v <= bits[nidx]
        nxt = np.where(go_left, nodes[nidx, 2], nodes[nidx, 3])
        cur[alive] = base[alive] + nxt  # children are tree-relative
    if tree_order:
        for per_tree in leaf_of.reshape(T, n_rows):
            acc += per_tree
    return acc


def score_forest_cpu(
    packed: PackedModel, codes: np.ndarray, nums_imp: np.ndarray
) -> np.ndarray:
    """Classifier P(default) per row = mean of leaf class-1 fractions."""
    s = forest_raw_cpu(packed, codes, nums_imp)
    if getattr(packed, "cls_kind", 0) == 1:  # gradient-boosted: logit sum
        return 1.0 / (1.0 + np.exp(-(s + packed.cls_bias)))
    return (s / packed.cls_n_trees).astype(np.float64)


def forest_raw_cpu(
    packed: PackedModel, codes: np.ndarray, nums_imp: np.ndarray, tree_order: bool = False
) -> np.ndarray:
    """Raw classifier sum per row, f64[B]: the leaf payloads over all trees,
    before score_forest_cpu's 1/T or bias + sigmoid (``tree_order``:
    _traverse_forest)."""
    fc, fk = packed.feat_col, packed.feat_code

    def value_of(rows: np.ndarray, feats: np.ndarray) -> np.ndarray:
        col = fc[feats]
        code = fk[feats]
        cat = code >= 0
        v = np.empty(len(rows), dtype=np.float32)
        if cat.any():
            v[cat] = (codes[rows[cat], col[cat]] == code[cat]).astype(np.float32)
        if (~cat).any():
            v[~cat] = nums_imp[rows[~cat], col[~cat]]
        return v

    return _traverse_forest(
        packed.cls_nodes, packed.cls_tree_offsets, value_of, len(codes), tree_order
    )


def forest_whatif_cpu(
    packed: PackedModel,
    codes: np.ndarray,
    nums_imp: np.ndarray,
    jobs: np.ndarray,
    max_pairs: int = 1 << 21,
) -> np.ndarray:
    """What-if raw classifier sums, f64[J, R]: row r of the (imputed) sample
    with job j's overrides applied, summed over all trees in tree order
    (forest_raw_cpu with ``tree_order``), as forest_whatif_kernel sums them.

    ``jobs`` is i32[J, 4] {player0, bits0, player1, bits1}: player is the
    schema feature index (0..N_CAT-1 categorical columns, N_CAT.. numerics;
    -1 in slot 1 = no second override), bits the category code or the f32 bit
    pattern of the value. Deliberately the dumb version: per job, copy the
    sample, write the override into the column and run the scorer's own
    traversal on the copy. Jobs are only stacked into one traversal call so
    long as it stays under ``max_pairs`` (row, tree) pairs."""
    jobs = np.ascontiguousarray(jobs, dtype=np.int32).reshape(-1, 4)
    codes = np.ascontiguousarray(codes, dtype=np.int16)
    nums_imp = np.ascontiguousarray(nums_imp, dtype=np.float32)
    n_jobs, r = len(jobs), len(codes)
    n_src = N_CAT + N_NUM
    p0, p1 = jobs[:, 0], jobs[:, 2]
    if n_jobs < 1 or r < 1:
        raise ValueError("forest_whatif needs at least one job and one row")
    if ((p0 < 0) | (p0 >= n_src) | (p1 < -1) | (p1 >= n_src) | (p0 == p1)).any():
        raise ValueError("job players must be in range and distinct")
    out = np.empty((n_jobs, r), dtype=np.float64)
    step = max(1, max_pairs // max(1, r * packed.cls_n_trees))
    for a in range(0, n_jobs, step):
        chunk = jobs[a : a + step]
        c = np.tile(codes, (len(chunk), 1))
        x = np.tile(nums_imp, (len(chunk), 1))
        for k, job in enumerate(chunk):
            rows = slice(k * r, (k + 1) * r)
            for player, bits in ((job[0], job[1]), (job[2], job[3])):
                if player < 0:
                    continue
                if player < N_CAT:
                    c[rows, player] = np.int16(bits)
                else:
                    x[rows, player - N_CAT] = np.int32(bits).view(np.float32)
        out[a : a + len(chunk)] = forest_raw_cpu(packed, c, x, tree_order=True).reshape(
            len(chunk), r
        )
    return out


def forest_sweep_cpu(
    packed: PackedModel,
    codes: np.ndarray,
    nums_imp: np.ndarray,
    jobs: np.ndarray,
    cut: float | None = None,
    tables=None,
):
    """Exact single-feature curves and their nearest decision flips, the
    reference of forest_sweep_kernel. ``jobs`` is i32[J, 2] {row, numeric
    column}; ``cut`` the decision threshold in raw space (class 1 is
    ``raw > cut``; default: counterfactual.raw_cut at 0.5).

    Returns ``(rec, raw, curves)``: rec i32[J, 3] = {k0, k_below, k_above}
    (-1 = none), raw f64[J, 3] the raw sums there (0.0 where none) and curves,
    a list of J arrays f64[K + 1]. Deliberately the dumb version: the row is
    scored by forest_whatif_cpu at one representative value per interval (the
    threshold T[k] for k < K, the next f32 above T[K-1] for the last) and the
    curve is searched with plain numpy. It shares no code with the kernel's
    interval walk; only the threshold lists come from the same tables."""
    from .. import counterfactual as cf

    jobs = np.ascontiguousarray(jobs, dtype=np.int32).reshape(-1, 2)
    codes = np.ascontiguousarray(codes, dtype=np.int16)
    nums_imp = np.ascontiguousarray(nums_imp, dtype=np.float32)
    n_jobs, r = len(jobs), len(codes)
    if n_jobs < 1 or r < 1:
        raise ValueError("forest_sweep needs at least one job and one row")
    if ((jobs[:, 0] < 0) | (jobs[:, 0] >= r) | (jobs[:, 1] < 0) | (jobs[:, 1] >= N_NUM)).any():
        raise ValueError("job rows and numeric columns must be in range")
    if tables is None:
        tables = cf.build_tables(packed)
    if cut is None:
        cut = cf.raw_cut(packed, 0.5)
    rec = np.full((n_jobs, 3), -1, dtype=np.int32)
    raw = np.zeros((n_jobs, 3), dtype=np.float64)
    curves: list = [None] * n_jobs
    for c in np.unique(jobs[:, 1]):
        mine = np.flatnonzero(jobs[:, 1] == c)
        rows, slot = np.unique(jobs[mine, 0], return_inverse=True)
        thr = tables.thresholds[c]
        values = cf.representatives(thr)
        wj = np.zeros((len(values), 4), dtype=np.int32)
        wj[:, 0], wj[:, 1], wj[:, 2] = N_CAT + c, values.view(np.int32), -1
        sums = forest_whatif_cpu(packed, codes[rows], nums_imp[rows], wj)  # [K+1, rows]
        for j, s in zip(mine, slot):
            curve = np.ascontiguousarray(sums[:, s])
            k0 = int(np.sum(thr < nums_imp[jobs[j, 0], c]))
            flips = np.flatnonzero((curve > cut) != (curve[k0] > cut))
            below, above = flips[flips < k0], flips[flips > k0]
            kb = int(below[-1]) if len(below) else -1
            ka = int(above[0]) if len(above) else -1
            rec[j] = (k0, kb, ka)
            raw[j] = (curve[k0], curve[kb] if kb >= 0 else 0.0, curve[ka] if ka >= 0 else 0.0)
            curves[j] = curve
    return rec, raw, curves


def forest_contrib_cpu(
    packed: PackedModel, codes: np.ndarray, nums_imp: np.ndarray
) -> np.ndarray:
    """Per-row prediction-path (Saabas) attributions, f64[B, N_CAT + N_NUM]
    in schema feature order.

    Every split on a row's path credits v[child taken] - v[node] to the
    source column of the split feature (one-hot features fold back onto
    their categorical column). Same traversal semantics as score_forest_cpu
    (f32 compares); differences and sums are f64. Scaled by 1/T for the
    averaging forests, 1 for gradient boosting, so that
    cls_base_value + contrib.sum(1) is the model output (probability, or
    log-odds for GBT)."""
    if packed.cls_node_value is None:
        raise ValueError(
            "model was packed without per-node expected values "
            "(cls_node_value is None); re-pack it to compute attributions"
        )
    nodes, offsets = packed.cls_nodes, packed.cls_tree_offsets
    fc, fk = packed.feat_col, packed.feat_code
    bits = nodes[:, 1].view(np.float32)
    val = packed.cls_node_value.astype(np.float64)
    n_rows = len(codes)
    n_src = N_CAT + N_NUM
    T = len(offsets) - 1
    cur = np.repeat(offsets[:-1].astype(np.int64), n_rows)
    base = cur.copy()
    rows = np.tile(np.arange(n_rows, dtype=np.int64), T)
    acc = np.zeros(n_rows * n_src, dtype=np.float64)
    alive = np.arange(T * n_rows, dtype=np.int64)
    while len(alive):
        nidx = cur[alive]
        feat = nodes[nidx, 0]
        split = feat >= 0
        alive, nidx, feat = alive[split], nidx[split], feat[split]
        if not len(alive):
            break
        r = rows[alive]
        col = fc[feat].astype(np.int64)
        code = fk[feat]
        cat = code >= 0
        v = np.empty(len(alive), dtype=np.float32)
        if cat.any():
            v[cat] = (codes[r[cat], col[cat]] == code[cat]).astype(np.float32)
        if (~cat).any():
            v[~cat] = nums_imp[r[~cat], col[~cat]]
        go_left = v <= bits[nidx]
        nxt = base[alive] + np.where(go_left, nodes[nidx, 2], nodes[nidx, 3])
        src = np.where(cat, col, N_CAT + col)
        np.add.at(acc, r * n_src + src, val[nxt] - val[nidx])
        cur[alive] = nxt
    scale = 1.0 if getattr(packed, "cls_kind", 0) == 1 else 1.0 / T
    return acc.reshape(n_rows, n_src) * scale


# 12-point Gauss-Legendre rule on [0, 1]: exact for polynomials of degree
# <= 23, and the SHAP integrand has degree (players on a path) - 1 <= 22.
# The kernel carries the same nodes and weights as literals.
SHAP_NQ = 12
_gl_x, _gl_w = np.polynomial.legendre.leggauss(SHAP_NQ)
SHAP_T = 0.5 * (_gl_x + 1.0)
SHAP_W = 0.5 * _gl_w


def forest_shap_cpu(
    packed: PackedModel,
    codes: np.ndarray,
    nums_imp: np.ndarray,
    paths=None,
    max_bytes: int = 64 << 20,
) -> np.ndarray:
    """Exact path-dependent TreeSHAP values, f64[B, N_CAT + N_NUM] in schema
    feature order (one-hot features fold onto their categorical column).

    Per leaf with value v and distinct players p on its path (z_p = product
    of cover fractions over p's splits, o_p = 1 iff the row follows them all):

        phi_i = v * (o_i - z_i) * int_0^1 prod_{p != i} (z_p (1-t) + o_p t) dt

    evaluated with the 12-point Gauss-Legendre rule (exact at this degree).
    Same f32 compares as score_forest_cpu; everything else is f64. Scaled by
    1/T for the averaging forests, 1 for gradient boosting, so that the SHAP
    base value of pack.build_shap_paths plus the row sum is the model output.
    ``paths`` takes a prebuilt table (the engine caches it). Leaves are
    processed in chunks so that temporaries stay under ``max_bytes``."""
    from ..pack import (
        SHAP_CODE_SHIFT,
        SHAP_DIR_RIGHT,
        SHAP_FIRST,
        SHAP_PLAYER_SHIFT,
        build_shap_paths,
    )

    if paths is None:
        paths, _ = build_shap_paths(packed)
    n_rows = len(codes)
    n_src = N_CAT + N_NUM
    acc = np.zeros((n_rows, n_src), dtype=np.float64)
    T = len(packed.cls_tree_offsets) - 1
    scale = 1.0 if getattr(packed, "cls_kind", 0) == 1 else 1.0 / T
    off = paths.leaf_off.astype(np.int64)
    n_rec = int(off[-1])
    if n_rows == 0 or n_rec == 0:
        return acc

    sp = paths.splits
    thr = sp[:, 1].view(np.float32)
    frac = sp[:, 2].view(np.float32).astype(np.float64)
    flags = sp[:, 3].view(np.uint32).astype(np.int64)
    right = (flags & SHAP_DIR_RIGHT) != 0
    first = (flags & SHAP_FIRST) != 0
    player = (flags >> SHAP_PLAYER_SHIFT) & 0xFF
    code = (flags >> SHAP_CODE_SHIFT) - 1

    # group = one player's run of records within one leaf
    gstart = np.flatnonzero(first)
    rec_leaf = np.repeat(np.arange(paths.n_leaves), np.diff(off))
    leaf_goff = np.zeros(len(off), dtype=np.int64)  # first group of each leaf
    np.cumsum(np.bincount(rec_leaf[gstart], minlength=paths.n_leaves), out=leaf_goff[1:])
    z_all = np.multiply.reduceat(frac, gstart)
    g_player = player[gstart]

    codes = np.asarray(codes)
    t = SHAP_T[None, None, :]
    # per group: o, f, the leaf products and the quotient — ~4 x [B, G, NQ] f64
    g_max = max(1, max_bytes // (4 * 8 * SHAP_NQ * n_rows))
    n_leaves = paths.n_leaves
    a = 0
    while a < n_leaves:
        b = int(np.searchsorted(leaf_goff, leaf_goff[a] + g_max, side="right")) - 1
        b = min(max(b, a + 1), n_leaves)
        g0, g1 = int(leaf_goff[a]), int(leaf_goff[b])
        r0, r1 = int(off[a]), int(off[b])
        if g1 == g0:
            a = b
            continue
        # does the row follow each record? (f32 compare, as the scorer)
        cat = code[r0:r1] >= 0
        pl = player[r0:r1]
        x = np.empty((n_rows, r1 - r0), dtype=np.float32)
        x[:, cat] = codes[:, pl[cat]] == code[r0:r1][cat][None, :]
        x[:, ~cat] = nums_imp[:, pl[~cat] - N_CAT]
        follows = ~(x <= thr[None, r0:r1]) == right[None, r0:r1]
        o = np.logical_and.reduceat(follows, gstart[g0:g1] - r0, axis=1)
        o = o.astype(np.float64)
        z = z_all[g0:g1][None, :]
        f = z[:, :, None] * (1.0 - t) + o[:, :, None] * t  # [B, G, NQ]
        # product over the groups of each leaf (non-empty leaves only)
        lg = leaf_goff[a:b] - g0
        ne = leaf_goff[a + 1 : b + 1] > leaf_goff[a:b]
        prod = np.multiply.reduceat(f, lg[ne], axis=1)  # [B, leaves_ne, NQ]
        n_g = (leaf_goff[a + 1 : b + 1] - leaf_goff[a:b])[ne]
        prod_g = np.repeat(prod, n_g, axis=1)
        v_g = np.repeat(paths.leaf_value[a:b][ne].astype(np.float64), n_g)
        live = o != z  # o == z contributes exactly 0 (and may have f == 0)
        np.copyto(f, 1.0, where=~live[:, :, None])
        s = ((prod_g / f) * SHAP_W[None, None, :]).sum(axis=2)
        phi = np.where(live, v_g[None, :] * (o - z) * s, 0.0)
        gp = g_player[g0:g1]
        for c in np.unique(gp):
            acc[:, c] += phi[:, gp == c].sum(axis=1)
        a = b
    return acc * scale


def forest_shap_interactions_cpu(
    packed: PackedModel,
    codes: np.ndarray,
    nums_imp: np.ndarray,
    paths=None,
    max_bytes: int = 64 << 20,
) -> np.ndarray:
    """Exact path-dependent SHAP interaction values, f64[B, 23, 23] in schema
    feature order on both axes (one-hot features fold onto their categorical
    column), in the convention of the ``shap`` package: the matrix is
    symmetric, each off-diagonal entry holds half of the pair's Shapley
    interaction index, and the diagonal is phi_i - sum_{j != i} Phi_ij with
    phi = forest_shap_cpu, so that every row sums to the SHAP value of its
    feature and the whole matrix plus the SHAP base value is the model output.

    Per leaf with value v and distinct players p on its path (z_p, o_p as in
    forest_shap_cpu), for i != j:

        Phi_ij = v/2 (o_i - z_i)(o_j - z_j)
                 * int_0^1 prod_{p != i,j} (z_p (1-t) + o_p t) dt

    evaluated with the same 12-point Gauss-Legendre rule as
    sum_q w_q L_q g_iq g_jq, L_q = prod_p f_pq, g_pq = (o_p - z_p) / f_pq.
    f_pq = 0 only for an off player with z_p = 0; the leaf then contributes
    nothing to the row (L_q = 0) and g is taken as 0, so exact zeros stay
    exact. Same f32 compares as score_forest_cpu; everything else is f64.
    Leaves are processed in chunks so that temporaries stay under
    ``max_bytes``."""
    from ..pack import (
        SHAP_CODE_SHIFT,
        SHAP_DIR_RIGHT,
        SHAP_FIRST,
        SHAP_PLAYER_SHIFT,
        build_shap_paths,
    )

    if paths is None:
        paths, _ = build_shap_paths(packed)
    codes = np.asarray(codes)
    n_rows = len(codes)
    n_src = N_CAT + N_NUM
    out = np.zeros((n_rows, n_src, n_src), dtype=np.float64)
    off = paths.leaf_off.astype(np.int64)
    if n_rows == 0 or int(off[-1]) == 0:
        return out
    phi = forest_shap_cpu(packed, codes, nums_imp, paths=paths, max_bytes=max_bytes)

    sp = paths.splits
    thr = sp[:, 1].view(np.float32)
    frac = sp[:, 2].view(np.float32).astype(np.float64)
    flags = sp[:, 3].view(np.uint32).astype(np.int64)
    right = (flags & SHAP_DIR_RIGHT) != 0
    first = (flags & SHAP_FIRST) != 0
    player = (flags >> SHAP_PLAYER_SHIFT) & 0xFF
    code = (flags >> SHAP_CODE_SHIFT) - 1

    gstart = np.flatnonzero(first)
    n_leaves = paths.n_leaves
    rec_leaf = np.repeat(np.arange(n_leaves), np.diff(off))
    leaf_goff = np.zeros(len(off), dtype=np.int64)  # first group of each leaf
    np.cumsum(np.bincount(rec_leaf[gstart], minlength=n_leaves), out=leaf_goff[1:])
    z_all = np.multiply.reduceat(frac, gstart)
    g_player = player[gstart]
    leaf_v = paths.leaf_value.astype(np.float64)

    t = SHAP_T[None, None, :]
    # upper triangle, keyed lo * n_src + hi, transposed so that np.add.at
    # adds whole [B] rows
    acc = np.zeros((n_src * n_src, n_rows), dtype=np.float64)
    # per group: f, g and the gathers of a pair step — ~6 x [B, G, NQ] f64
    g_max = max(1, max_bytes // (6 * 8 * SHAP_NQ * n_rows))
    a = 0
    while a < n_leaves:
        b = int(np.searchsorted(leaf_goff, leaf_goff[a] + g_max, side="right")) - 1
        b = min(max(b, a + 1), n_leaves)
        g0, g1 = int(leaf_goff[a]), int(leaf_goff[b])
        r0, r1 = int(off[a]), int(off[b])
        n_g = leaf_goff[a + 1 : b + 1] - leaf_goff[a:b]
        if g1 == g0 or int(n_g.max()) < 2:
            a = b
            continue
        cat = code[r0:r1] >= 0
        pl = player[r0:r1]
        x = np.empty((n_rows, r1 - r0), dtype=np.float32)
        x[:, cat] = codes[:, pl[cat]] == code[r0:r1][cat][None, :]
        x[:, ~cat] = nums_imp[:, pl[~cat] - N_CAT]
        follows = ~(x <= thr[None, r0:r1]) == right[None, r0:r1]
        o = np.logical_and.reduceat(follows, gstart[g0:g1] - r0, axis=1)
        o = o.astype(np.float64)[:, :, None]
        z = z_all[g0:g1][None, :, None]
        f = z * (1.0 - t) + o * t  # [B, G, NQ]
        ne = n_g > 0
        lg = (leaf_goff[a:b] - g0)[ne]
        # w_q v/2 L_q per non-empty leaf
        lw = np.multiply.reduceat(f, lg, axis=1) * SHAP_W[None, None, :]
        lw *= (0.5 * leaf_v[a:b][ne])[None, :, None]
        dead = f == 0.0
        np.copyto(f, 1.0, where=dead)
        g = (o - z) / f
        np.copyto(g, 0.0, where=dead)
        n_ne = n_g[ne]
        for j in range(1, int(n_ne.max())):
            sel = np.flatnonzero(n_ne > j)
            gj = lg[sel] + j
            lwg = lw[:, sel] * g[:, gj]
            for i in range(j):
                gi = lg[sel] + i
                val = (lwg * g[:, gi]).sum(axis=2)  # [B, leaves with > j groups]
                pi, pj = g_player[g0 + gi], g_player[g0 + gj]
                key = np.minimum(pi, pj) * n_src + np.maximum(pi, pj)
                np.add.at(acc, key, val.T)
        a = b

    T = len(packed.cls_tree_offsets) - 1
    scale = 1.0 if getattr(packed, "cls_kind", 0) == 1 else 1.0 / T
    upper = (acc.T * scale).reshape(n_rows, n_src, n_src)
    out = upper + upper.transpose(0, 2, 1)  # the diagonal of upper is zero
    d = np.arange(n_src)
    out[:, d, d] = phi - out.sum(axis=2)
    return out


def ishap_weight_table(n: int = N_CAT + N_NUM) -> np.ndarray:
    """W[a, b] = (a-1)! b! / (a+b)! for a >= 1 (row 0 is zero), f64[n+1, n+1]:
    the Shapley weight of a player that is one of ``a`` players on its own
    side of an (explained row, background row) pair with ``b`` players on the
    other side. Built from W[a, 0] = 1/a by W[a, b] = W[a, b-1] * b / (a+b),
    so no factorial is ever formed (23! is not exact in f64); the kernel
    builds the same table with the same operations."""
    w = np.zeros((n + 1, n + 1), dtype=np.float64)
    for a in range(1, n + 1):
        w[a, 0] = 1.0 / a
        for b in range(1, n + 1):
            w[a, b] = w[a, b - 1] * b / (a + b)
    return w


_POP16 = np.array([bin(i).count("1") for i in range(1 << 16)], dtype=np.int64)


def _popcount32(x: np.ndarray) -> np.ndarray:
    return _POP16[x & 0xFFFF] + _POP16[x >> 16]


class _IshapIndex:
    """The path table decoded once for the interventional reference: per
    record the compare, per player group its records and its leaf."""

    def __init__(self, paths):
        from ..pack import SHAP_CODE_SHIFT, SHAP_DIR_RIGHT, SHAP_FIRST, SHAP_PLAYER_SHIFT

        sp = paths.splits
        flags = sp[:, 3].view(np.uint32).astype(np.int64)
        self.thr = sp[:, 1].view(np.float32)
        self.right = (flags & SHAP_DIR_RIGHT) != 0
        self.player = (flags >> SHAP_PLAYER_SHIFT) & 0xFF
        self.code = (flags >> SHAP_CODE_SHIFT) - 1
        self.off = paths.leaf_off.astype(np.int64)
        self.n_leaves = paths.n_leaves
        self.leaf_value = paths.leaf_value.astype(np.float64)
        self.gstart = np.flatnonzero((flags & SHAP_FIRST) != 0)
        rec_leaf = np.repeat(np.arange(self.n_leaves), np.diff(self.off))
        self.n_groups = np.bincount(rec_leaf[self.gstart], minlength=self.n_leaves)
        self.leaf_goff = np.zeros(self.n_leaves + 1, dtype=np.int64)
        np.cumsum(self.n_groups, out=self.leaf_goff[1:])
        self.g_player = self.player[self.gstart]
        # bit of each record's group within its leaf's mask
        first = (flags & SHAP_FIRST) != 0
        self.rec_bit = (
            np.int64(1) << np.minimum(np.cumsum(first) - 1 - self.leaf_goff[rec_leaf], 31)
        ).astype(np.uint32)
        if self.n_leaves and int(self.n_groups.max()) > N_CAT + N_NUM:
            raise ValueError("a leaf has more player groups than source columns")
        self.full = ((np.int64(1) << self.n_groups) - 1).astype(np.uint32)

    def masks(self, a: int, b: int, codes: np.ndarray, nums_imp: np.ndarray) -> np.ndarray:
        """u32[b - a, N]: bit j of [l, n] is set iff row n satisfies every
        split of player group j of leaf a + l (f32 compares, as the scorer).
        Leaf-major, so that the per-leaf reduction runs over contiguous rows."""
        r0, r1 = int(self.off[a]), int(self.off[b])
        out = np.repeat(self.full[a:b, None], len(codes), axis=1)
        if r1 == r0 or not len(codes):
            return out
        code, pl = self.code[r0:r1], self.player[r0:r1]
        cat = code >= 0
        x = np.empty((r1 - r0, len(codes)), dtype=np.float32)
        x[cat] = codes.T[pl[cat]] == code[cat][:, None]
        x[~cat] = nums_imp.T[pl[~cat] - N_CAT]
        fails = (x <= self.thr[r0:r1, None]) == self.right[r0:r1, None]
        # OR the group bit of every failed record over each leaf's records
        ne = self.n_groups[a:b] > 0
        failed = np.bitwise_or.reduceat(
            fails * self.rec_bit[r0:r1, None], (self.off[a:b] - r0)[ne], axis=0
        )
        out[ne] &= ~failed
        return out

    def chunks(self, n_a: int, n_b: int, max_bytes: int):
        """Leaf ranges whose temporaries (the [n_a, n_b, leaves] u32 pair
        arrays and the per-record compares) stay under ``max_bytes``."""
        depth = max(1.0, float(self.off[-1]) / max(1, self.n_leaves))
        per_leaf = 12 * max(1, n_a) * n_b + 16 * (n_a + n_b) * depth
        step = max(1, int(max_bytes // per_leaf))
        for a in range(0, self.n_leaves, step):
            yield a, min(a + step, self.n_leaves)


def _ishap_scale(packed: PackedModel) -> float:
    T = len(packed.cls_tree_offsets) - 1
    return 1.0 if getattr(packed, "cls_kind", 0) == 1 else 1.0 / T


def _ishap_paths(packed: PackedModel, paths):
    if paths is None:
        from ..pack import build_shap_paths

        paths, _ = build_shap_paths(packed, require_cover=False)
    return paths


def forest_ishap_cpu(
    packed: PackedModel,
    codes: np.ndarray,
    nums_imp: np.ndarray,
    bg_codes: np.ndarray,
    bg_nums_imp: np.ndarray,
    paths=None,
    max_bytes: int = 64 << 20,
) -> np.ndarray:
    """Interventional Shapley values against a background sample,
    f64[B, N_CAT + N_NUM] in schema feature order (one-hot features fold onto
    their categorical column). The game: val(S) = mean over background rows r
    of f(hybrid row: x on the columns of S, r elsewhere).

    Closed form per (x, r, leaf) with value v: a_p / b_p = 1 iff x / r
    satisfies every split of player p on the leaf's path. The pair reaches
    the leaf for some coalition iff a_p | b_p for every p; then with
    X = {a & !b}, R = {!a & b}, nx = |X|, nr = |R|, each i in X gets
    +v (nx-1)! nr! / (nx+nr)! and each i in R gets -v (nr-1)! nx! / (nx+nr)!
    (players with a & b are dummies of the pair). Summed over leaves,
    averaged over r, scaled by 1/T for the averaging forests and 1 for
    gradient boosting, so that forest_ishap_base_cpu plus the row sum is the
    model output. Same f32 compares as score_forest_cpu; the rest is f64.
    ``paths`` takes a prebuilt table; ``frac`` is never read, so a table
    built without cover serves. Leaves go in chunks under ``max_bytes``."""
    ix = _IshapIndex(_ishap_paths(packed, paths))
    codes, bg_codes = np.asarray(codes), np.asarray(bg_codes)
    n_rows, n_bg = len(codes), len(bg_codes)
    if n_bg < 1:
        raise ValueError("the background sample is empty")
    n_src = N_CAT + N_NUM
    acc = np.zeros(n_rows * n_src, dtype=np.float64)
    if n_rows == 0 or ix.off[-1] == 0:
        return acc.reshape(n_rows, n_src)
    w_tab = ishap_weight_table()
    for a, b in ix.chunks(n_rows, n_bg, max_bytes):
        am = ix.masks(a, b, codes, nums_imp)
        bm = ix.masks(a, b, bg_codes, bg_nums_imp)
        live = (am[:, :, None] | bm[:, None, :]) == ix.full[a:b, None, None]
        li, xi, ri = np.nonzero(live)
        ma, mb = am[li, xi], bm[li, ri]
        mx, mr = ma & ~mb, mb & ~ma  # players only x / only r satisfies
        keep = (mx | mr) != 0
        xi, li, mx, mr = xi[keep], li[keep], mx[keep], mr[keep]
        if not len(xi):
            continue
        nx, nr = _popcount32(mx), _popcount32(mr)
        v = ix.leaf_value[a + li]
        wp, wn = v * w_tab[nx, nr], v * w_tab[nr, nx]
        gbase = ix.leaf_goff[a + li]
        for j in range(int(ix.n_groups[a:b].max())):
            sx, sr = (mx >> j) & 1 != 0, (mr >> j) & 1 != 0
            sel = sx | sr
            if not sel.any():
                continue
            player = ix.g_player[gbase[sel] + j]
            acc += np.bincount(
                xi[sel] * n_src + player,
                weights=np.where(sx[sel], wp[sel], -wn[sel]),
                minlength=len(acc),
            )
    return acc.reshape(n_rows, n_src) * _ishap_scale(packed) / n_bg


def forest_ishap_base_cpu(
    packed: PackedModel,
    bg_codes: np.ndarray,
    bg_nums_imp: np.ndarray,
    paths=None,
    max_bytes: int = 64 << 20,
) -> float:
    """Base value of the interventional game: the f64 mean over the
    background rows of the raw model output (probability, or log-odds for
    gradient boosting), from the same path table as forest_ishap_cpu — a row
    lands in the leaf whose every player group it satisfies."""
    ix = _IshapIndex(_ishap_paths(packed, paths))
    bg_codes = np.asarray(bg_codes)
    if len(bg_codes) < 1:
        raise ValueError("the background sample is empty")
    total = np.zeros(len(bg_codes), dtype=np.float64)
    for a, b in ix.chunks(0, len(bg_codes), max_bytes):
        hit = ix.masks(a, b, bg_codes, bg_nums_imp) == ix.full[a:b, None]
        total += ix.leaf_value[a:b] @ hit
    raw = total * _ishap_scale(packed)
    if getattr(packed, "cls_kind", 0) == 1:
        raw = raw + float(packed.cls_bias)
    return float(raw.mean())


def score_iforest_cpu(
    packed: PackedModel, nums_imp: np.ndarray
) -> tuple[np.ndarray, np.ndarray]:
    """alibi instance_score (= -decision_function) and is_outlier flags."""

    def value_of(rows: np.ndarray, feats: np.ndarray) -> np.ndarray:
        return nums_imp[rows, feats]

    depths = _traverse_forest(packed.if_nodes, packed.if_tree_offsets, value_of, len(nums_imp))
    anomaly = 2.0 ** (-depths / packed.if_denom)  # Liu et al. anomaly score
    score_samples = -anomaly  # sklearn score_samples
    decision = score_samples - packed.if_offset  # sklearn decision_function
    instance_score = -decision  # alibi-detect convention
    return instance_score, (instance_score > packed.if_threshold).astype(np.float64)


def drift_pvals_cpu(
    packed: PackedModel, codes: np.ndarray, nums_imp: np.ndarray
) -> np.ndarray:
    """Per-feature p-values [N_CAT + N_NUM] in schema feature order."""
    pvals = np.ones(N_CAT + N_NUM, dtype=np.float64)
    for j in range(N_CAT):
        lo, hi = packed.ref_cat_offsets[j], packed.ref_cat_offsets[j + 1]
        nbins = hi - lo
        bc = np.bincount(
            np.where(codes[:, j] < 0, nbins - 1, codes[:, j]).astype(np.int64),
            minlength=nbins,
        )
        pvals[j] = chi2_from_counts(packed.ref_cat_counts[lo:hi], bc)
    for j in range(N_NUM):
        lo, hi = packed.ref_sorted_offsets[j], packed.ref_sorted_offsets[j + 1]
        d = ks_2samp_d(packed.ref_sorted[lo:hi].astype(np.float64), nums_imp[:, j])
        pvals[N_CAT + j] = ks_asymp_pvalue(d, hi - lo, len(nums_imp))
    return pvals


def drift_stats_cpu(
    packed: PackedModel, codes: np.ndarray, nums_imp: np.ndarray
) -> tuple[np.ndarray, np.ndarray]:
    """The raw statistics the GPU drift kernel produces: per-categorical batch
    histograms (concatenated, ref_cat_offsets layout) and per-numeric K-S D."""
    hists = np.zeros_like(packed.ref_cat_counts)
    for j in range(N_CAT):
        lo, hi = packed.ref_cat_offsets[j], packed.ref_cat_offsets[j + 1]
        nbins = hi - lo
        bc = np.bincount(
            np.where(codes[:, j] < 0, nbins - 1, codes[:, j]).astype(np.int64),
            minlength=nbins,
        )
        hists[lo:hi] = bc
    ds = np.zeros(N_NUM, dtype=np.float32)
    for j in range(N_NUM):
        lo, hi = packed.ref_sorted_offsets[j], packed.ref_sorted_offsets[j + 1]
        # float32 ref + float32 batch — same comparison dtype as the kernel
        ds[j] = np.float32(
            ks_2samp_d(packed.ref_sorted[lo:hi].astype(np.float64), nums_imp[:, j].astype(np.float64))
        )
    return hists, ds


def pvals_from_stats(
    packed: PackedModel, cat_hists: np.ndarray, ks_d: np.ndarray, n_batch: int
) -> np.ndarray:
    """Convert GPU drift statistics to p-values (shared by GPU + CPU paths).
    Vectorized: exactly two scipy sf calls per request."""
    from ..models.drift import chi2_from_counts_many, ks_asymp_pvalue_many

    # ref columns all have n_ref rows (fitted on one matrix)
    n_ref = int(packed.ref_sorted_offsets[1] - packed.ref_sorted_offsets[0])
    if True:  # native epilogue: scipy kstwo.sf's own region selection, in C
        from . import gpu

        if gpu.available():
            return gpu._ext.drift_pvals_host(
                np.ascontiguousarray(cat_hists, dtype=np.int32),
                np.ascontiguousarray(ks_d, dtype=np.float32),
                packed.ref_cat_counts,
                packed.ref_cat_offsets,
                n_ref,
                n_batch,
            )
    pvals = np.ones(N_CAT + N_NUM, dtype=np.float64)
    pvals[:N_CAT] = chi2_from_counts_many(
        packed.ref_cat_counts, cat_hists, packed.ref_cat_offsets
    )
    pvals[N_CAT:] = ks_asymp_pvalue_many(ks_d, n_ref, n_batch)
    return pvals


def score_batch_cpu(packed: PackedModel, codes: np.ndarray, nums: np.ndarray) -> dict:
    """Full pipeline on CPU: proba + outliers + drift p-vals."""
    nums_imp = impute_nums(packed, nums)
    proba = score_forest_cpu(packed, codes, nums_imp)
    iscore, outliers = score_iforest_cpu(packed, nums_imp)
    pvals = drift_pvals_cpu(packed, codes, nums_imp)
    return {
        "predictions": proba,
        "outliers": outliers,
        "instance_score": iscore,
        "p_vals": pvals,
    }


# ---------------------------------------------------------------------------
# Histogram gradient-boosted-tree trainer: the three level primitives
# (golden reference of hgbt_hist / hgbt_split / hgbt_route in
# csrc/creditcore_kernels.hip; all results are integers or the same f64
# formula, so the kernels are tested against these with exact equality)
# ---------------------------------------------------------------------------

HGBT_SHIFT = 20  # fractional bits of the int32 fixed-point gradients
HGBT_REC = 9  # split record: gain bits, feat, bin, GL, HL, CL, G, H, C


def hgbt_hist_cpu(
    bins: np.ndarray,
    bin_off: np.ndarray,
    node: np.ndarray,
    gq: np.ndarray,
    hq: np.ndarray,
    n_nodes: int,
) -> np.ndarray:
    """Level histogram i64[n_nodes, 3, total_bins]: per (open node, bin) the
    sums of gq and hq and the row count. ``bins`` is u8[F, N] (feature-major),
    ``node`` the per-row slot among the level's open nodes; rows with a
    negative node id already sit in a leaf and are skipped.

    bincount sums in f64, which is exact here: every partial sum is an
    integer below 2^53 (N * 2^HGBT_SHIFT with N < 2^33)."""
    n_feat = bins.shape[0]
    total = int(bin_off[-1])
    hist = np.zeros((n_nodes, 3, total), dtype=np.int64)
    live = np.flatnonzero((node >= 0) & (node < n_nodes))
    if not len(live):
        return hist
    nd = node[live].astype(np.int64)
    g = gq[live].astype(np.float64)
    h = hq[live].astype(np.float64)
    for f in range(n_feat):
        a, b = int(bin_off[f]), int(bin_off[f + 1])
        nb = b - a
        idx = nd * nb + bins[f, live].astype(np.int64)
        size = n_nodes * nb
        hist[:, 0, a:b] = np.bincount(idx, weights=g, minlength=size).astype(
            np.int64
        ).reshape(n_nodes, nb)
        hist[:, 1, a:b] = np.bincount(idx, weights=h, minlength=size).astype(
            np.int64
        ).reshape(n_nodes, nb)
        hist[:, 2, a:b] = np.bincount(idx, minlength=size).reshape(n_nodes, nb)
    return hist


def hgbt_split_cpu(
    hist: np.ndarray, bin_off: np.ndarray, lam: float, min_leaf: int
) -> np.ndarray:
    """Best split per open node, i64[n_nodes, HGBT_REC].

    For every (feature, bin b) the candidate "bin <= b goes left" has
    gain = GL^2/(HL+lam) + GR^2/(HR+lam) - G^2/(H+lam), in f64 from the
    integer prefix sums scaled by 2^-HGBT_SHIFT (exact). It is valid when both
    sides keep ``min_leaf`` rows and gain > 0. Ties: highest gain, then lowest
    feature, then lowest bin. No valid split: feat = -1 and zeros. The kernel
    evaluates the same expression in the same order with contraction off."""
    n_nodes, _, total = hist.shape
    bin_off = np.asarray(bin_off, dtype=np.int64)
    out = np.zeros((n_nodes, HGBT_REC), dtype=np.int64)
    if n_nodes == 0:
        return out
    feat_of_bin = np.repeat(np.arange(len(bin_off) - 1), np.diff(bin_off))
    start = bin_off[:-1][feat_of_bin]  # first bin of the own feature
    cs = np.cumsum(hist, axis=2)
    # prefix within the feature = running sum minus the sum before its start
    before = np.where(start > 0, cs[:, :, np.maximum(start - 1, 0)], 0)
    pre = cs - before  # [n_nodes, 3, total]
    f0_last = int(bin_off[1]) - 1
    tot = pre[:, :, f0_last]  # node totals (feature 0 sees every open row)
    GL, HL, CL = pre[:, 0], pre[:, 1], pre[:, 2]
    G, H, C = tot[:, 0:1], tot[:, 1:2], tot[:, 2:3]
    sc = 1.0 / float(1 << HGBT_SHIFT)
    with np.errstate(divide="ignore", invalid="ignore"):
        gl, hl = GL.astype(np.float64) * sc, HL.astype(np.float64) * sc
        gr, hr = (G - GL).astype(np.float64) * sc, (H - HL).astype(np.float64) * sc
        g, h = G.astype(np.float64) * sc, H.astype(np.float64) * sc
        a = (gl * gl) / (hl + lam)
        b = (gr * gr) / (hr + lam)
        c = (g * g) / (h + lam)
        gain = (a + b) - c
        valid = (CL >= min_leaf) & (C - CL >= min_leaf) & (gain > 0.0)
    gain = np.where(valid, gain, -np.inf)
    # argmax returns the first maximum: lowest (feature, bin) among ties
    best = np.argmax(gain, axis=1)
    k = np.arange(n_nodes)
    ok = valid[k, best]
    out[:, 0] = np.where(ok, gain[k, best], 0.0).view(np.int64)
    out[:, 1] = np.where(ok, feat_of_bin[best], -1)
    out[:, 2] = np.where(ok, best - start[best], 0)
    out[:, 3] = np.where(ok, GL[k, best], 0)
    out[:, 4] = np.where(ok, HL[k, best], 0)
    out[:, 5] = np.where(ok, CL[k, best], 0)
    out[:, 6:9] = tot
    return out


def hgbt_mono_weight(g: np.ndarray, d: np.ndarray, lo, hi) -> np.ndarray:
    """Newton weight -g/d clamped to [lo, hi]. The clamp is two selects, not
    np.clip, so that it picks the operand the kernel's compares pick."""
    w = -g / d
    w = np.where(w < lo, lo, w)
    return np.where(w > hi, hi, w)


def hgbt_split_mono_cpu(
    hist: np.ndarray,
    bin_off: np.ndarray,
    lam: float,
    min_leaf: int,
    mono: np.ndarray,
    bounds: np.ndarray,
) -> np.ndarray:
    """Best split per open node under monotone constraints, i64[n_nodes,
    HGBT_REC] (golden reference of hgbt_split_mono).

    ``mono`` i32[F] is the sign of every feature (-1, 0, +1; only the sign is
    read), ``bounds`` f64[n_nodes, 2] the leaf-weight interval {lo, hi} of
    every open node. With g = G 2^-SHIFT and d = H 2^-SHIFT + lam, a side
    takes w = min(max(-g/d, lo), hi) and scores s = -((2g)w + (dw)w); left,
    right and parent are all clamped to the node's interval and
    gain = (s_L + s_R) - s_P. A candidate is valid when both sides keep
    ``min_leaf`` rows, d_L > 0 and d_R > 0, gain > 0, and w_L <= w_R on a
    +1 feature (w_L >= w_R on a -1 feature). Ties and the no-split record are
    hgbt_split_cpu's."""
    n_nodes, _, total = hist.shape
    bin_off = np.asarray(bin_off, dtype=np.int64)
    out = np.zeros((n_nodes, HGBT_REC), dtype=np.int64)
    if n_nodes == 0:
        return out
    feat_of_bin = np.repeat(np.arange(len(bin_off) - 1), np.diff(bin_off))
    start = bin_off[:-1][feat_of_bin]
    cs = np.cumsum(hist, axis=2)
    before = np.where(start > 0, cs[:, :, np.maximum(start - 1, 0)], 0)
    pre = cs - before
    f0_last = int(bin_off[1]) - 1
    tot = pre[:, :, f0_last]
    GL, HL, CL = pre[:, 0], pre[:, 1], pre[:, 2]
    G, H, C = tot[:, 0:1], tot[:, 1:2], tot[:, 2:3]
    sign = np.sign(np.asarray(mono, dtype=np.int64))[feat_of_bin][None, :]
    bounds = np.asarray(bounds, dtype=np.float64).reshape(n_nodes, 2)
    lo, hi = bounds[:, 0:1], bounds[:, 1:2]
    sc = 1.0 / float(1 << HGBT_SHIFT)

    def side(g_int, h_int):
        g = g_int.astype(np.float64) * sc
        d = h_int.astype(np.float64) * sc + lam
        w = hgbt_mono_weight(g, d, lo, hi)
        return d, w, -(((2.0 * g) * w) + ((d * w) * w))

    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        d_l, w_l, s_l = side(GL, HL)
        d_r, w_r, s_r = side(G - GL, H - HL)
        _, _, s_p = side(G, H)
        gain = (s_l + s_r) - s_p
        order = (sign == 0) | ((sign > 0) & (w_l <= w_r)) | ((sign < 0) & (w_l >= w_r))
        valid = (
            (CL >= min_leaf) & (C - CL >= min_leaf)
            & (d_l > 0.0) & (d_r > 0.0) & (gain > 0.0) & order
        )
    gain = np.where(valid, gain, -np.inf)
    best = np.argmax(gain, axis=1)
    k = np.arange(n_nodes)
    ok = valid[k, best]
    out[:, 0] = np.where(ok, gain[k, best], 0.0).view(np.int64)
    out[:, 1] = np.where(ok, feat_of_bin[best], -1)
    out[:, 2] = np.where(ok, best - start[best], 0)
    out[:, 3] = np.where(ok, GL[k, best], 0)
    out[:, 4] = np.where(ok, HL[k, best], 0)
    out[:, 5] = np.where(ok, CL[k, best], 0)
    out[:, 6:9] = tot
    return out


def hgbt_route_cpu(bins: np.ndarray, table: np.ndarray, node: np.ndarray) -> np.ndarray:
    """New per-row node ids. ``table[k] = {feat, bin, left, right}`` for open
    node k: rows with bins[feat] <= bin take ``left``, the others ``right``;
    feat < 0 closes the node and every row takes ``left``. Targets >= 0 are
    slots of the next level, negative ones encode leaf node t as -(t + 1).
    Rows already in a leaf keep their id."""
    out = node.copy()
    live = np.flatnonzero((node >= 0) & (node < len(table)))
    if not len(live):
        return out
    t = table[node[live]]
    feat = t[:, 0]
    b = bins[np.maximum(feat, 0), live].astype(np.int64)
    go_left = (feat < 0) | (b <= t[:, 1])
    out[live] = np.where(go_left, t[:, 2], t[:, 3]).astype(node.dtype)
    return out


# ---------------------------------------------------------------------------
# Histogram random-forest trainer: the three level primitives over a batch of
# trees (golden reference of hrf_hist / hrf_split / hrf_route in
# csrc/creditcore_kernels.hip). A level is a flat list of open slots;
# ``slot_off i32[TB+1]`` gives each tree's range in it and
# ``slot_meta i32[K, 2]`` = (global tree index, node id) per slot. Everything
# is an integer or the same f64 formula: the kernels match with exact equality.
# ---------------------------------------------------------------------------

HRF_REC = 7  # split record: proxy bits, feat, bin, PL, WL, P, W
# odd 64-bit multipliers of the per-node feature key (also in the .hip file)
HRF_C1 = 0x9E3779B97F4A7C15  # tree
HRF_C2 = 0xC2B2AE3D27D4EB4F  # node id
HRF_C3 = 0x165667B19E3779F9  # feature
_U64 = (1 << 64) - 1


def hrf_feature_keys(seed: int, tree, node_id, n_feat: int) -> np.ndarray:
    """u64[..., n_feat] feature keys of one or many nodes:
    splitmix64_finalizer(seed ^ tree*C1 ^ node_id*C2 ^ f*C3), all mod 2^64.
    A node's features are ranked by (key, f) ascending; the first
    ``max_features`` ranks are its candidates (hrf_split_cpu)."""
    u = np.uint64
    tree = np.asarray(tree, dtype=np.int64).astype(u)[..., None]
    node_id = np.asarray(node_id, dtype=np.int64).astype(u)[..., None]
    f = np.arange(n_feat, dtype=u)
    with np.errstate(over="ignore"):
        z = u(int(seed) & _U64) ^ (tree * u(HRF_C1)) ^ (node_id * u(HRF_C2)) ^ (f * u(HRF_C3))
        z = (z ^ (z >> u(30))) * u(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> u(27))) * u(0x94D049BB133111EB)
        return z ^ (z >> u(31))


def hrf_hist_cpu(
    bins: np.ndarray,
    bin_off: np.ndarray,
    y: np.ndarray,
    w: np.ndarray,
    node: np.ndarray,
    slot_off: np.ndarray,
) -> np.ndarray:
    """Level histogram i64[K, 2, total_bins] with planes {sum w*y, sum w}.

    ``bins`` u8[F, N] and ``y`` u8[N] (0/1) are shared by the batch;
    ``w`` u8[TB, N] are the trees' bootstrap counts and ``node`` i32[TB, N]
    the row's local slot within its tree (negative: in a leaf, or weight 0).
    Tree t's local slot s is row ``slot_off[t] + s`` of the result."""
    n_feat = bins.shape[0]
    total = int(bin_off[-1])
    hist = np.zeros((int(slot_off[-1]), 2, total), dtype=np.int64)
    for t in range(len(slot_off) - 1):
        s0, k = int(slot_off[t]), int(slot_off[t + 1] - slot_off[t])
        live = np.flatnonzero((node[t] >= 0) & (node[t] < k))
        if k == 0 or not len(live):
            continue
        nd = node[t, live].astype(np.int64)
        wt = w[t, live].astype(np.int64)
        wy = wt * y[live]
        for f in range(n_feat):
            a, b = int(bin_off[f]), int(bin_off[f + 1])
            nb = b - a
            idx = nd * nb + bins[f, live]
            # bincount sums in f64: exact, every sum is an integer < 2^53
            for plane, val in ((0, wy), (1, wt)):
                hist[s0 : s0 + k, plane, a:b] = np.bincount(
                    idx, weights=val, minlength=k * nb
                ).astype(np.int64).reshape(k, nb)
    return hist


def hrf_split_cpu(
    hist: np.ndarray,
    bin_off: np.ndarray,
    slot_meta: np.ndarray,
    max_features: int,
    min_leaf: int,
    seed: int,
) -> np.ndarray:
    """Chosen split per open slot, i64[K, HRF_REC].

    "bin <= b goes left" of feature f has the Gini proxy
    PL^2/WL + PR^2/WR - P^2/W (P positives, W weight) in f64 from the integer
    sums; it is valid when WL >= min_leaf, WR >= min_leaf and proxy > 0. A
    feature's best split is its highest valid proxy, ties to the lowest bin.
    Features are ranked by (hrf_feature_keys, f); the candidates are the
    first max(max_features, r* + 1) ranks, r* the lowest rank that has a valid
    split, and the slot takes the candidate with the highest proxy, ties to
    the lower rank. No valid split anywhere: feat = -1 and zeros. P and W are
    always reported. The kernel evaluates the same expression in the same
    order with contraction off."""
    n_slots, _, total = hist.shape
    bin_off = np.asarray(bin_off, dtype=np.int64)
    n_feat = len(bin_off) - 1
    out = np.zeros((n_slots, HRF_REC), dtype=np.int64)
    if n_slots == 0:
        return out
    feat_of_bin = np.repeat(np.arange(n_feat), np.diff(bin_off))
    start = bin_off[:-1][feat_of_bin]
    cs = np.cumsum(hist, axis=2)
    before = np.where(start > 0, cs[:, :, np.maximum(start - 1, 0)], 0)
    pre = cs - before  # prefix sums within each feature
    PL, WL = pre[:, 0], pre[:, 1]
    tot = pre[:, :, int(bin_off[1]) - 1]  # feature 0 sees every open row
    P, W = tot[:, 0:1], tot[:, 1:2]
    with np.errstate(divide="ignore", invalid="ignore"):
        pl, wl = PL.astype(np.float64), WL.astype(np.float64)
        pr, wr = (P - PL).astype(np.float64), (W - WL).astype(np.float64)
        p, w = P.astype(np.float64), W.astype(np.float64)
        a = (pl * pl) / wl
        b = (pr * pr) / wr
        c = (p * p) / w
        proxy = (a + b) - c
        valid = (WL >= min_leaf) & (W - WL >= min_leaf) & (proxy > 0.0)
    proxy = np.where(valid, proxy, -np.inf)
    # per feature: highest proxy, then the first bin that reaches it
    f_best = np.maximum.reduceat(proxy, bin_off[:-1], axis=1)  # [K, F]
    at_best = valid & (proxy == f_best[:, feat_of_bin])
    pos = np.where(at_best, np.arange(total), total)
    f_pos = np.minimum.reduceat(pos, bin_off[:-1], axis=1)  # flat bin index
    f_valid = f_pos < total

    keys = hrf_feature_keys(seed, slot_meta[:, 0], slot_meta[:, 1], n_feat)
    order = np.argsort(keys, axis=1, kind="stable")  # rank -> feature, ties by f
    v_ranked = np.take_along_axis(f_valid, order, axis=1)
    any_valid = v_ranked.any(axis=1)
    r_star = np.argmax(v_ranked, axis=1)  # first valid rank
    limit = np.maximum(int(max_features), r_star + 1)
    cand = v_ranked & (np.arange(n_feat) < limit[:, None])
    p_ranked = np.where(cand, np.take_along_axis(f_best, order, axis=1), -np.inf)
    k = np.arange(n_slots)
    feat = order[k, np.argmax(p_ranked, axis=1)]  # first maximum: lower rank
    at = np.where(any_valid, f_pos[k, feat], 0)
    out[:, 0] = np.where(any_valid, f_best[k, feat], 0.0).view(np.int64)
    out[:, 1] = np.where(any_valid, feat, -1)
    out[:, 2] = np.where(any_valid, at - start[at], 0)
    out[:, 3] = np.where(any_valid, PL[k, at], 0)
    out[:, 4] = np.where(any_valid, WL[k, at], 0)
    out[:, 5:7] = tot
    return out


def hrf_route_cpu(
    bins: np.ndarray, table: np.ndarray, node: np.ndarray, slot_off: np.ndarray
) -> np.ndarray:
    """New node ids i32[TB, N]. ``table[slot_off[t] + s] = {feat, bin, left,
    right}`` for local slot s of tree t, with hgbt_route_cpu's protocol:
    bins[feat] <= bin takes ``left``, the rest ``right``; feat < 0 closes the
    slot and every row takes ``left``. Targets >= 0 are local slots of the
    tree's next level, negative ones encode leaf node i as -(i + 1)."""
    out = node.copy()
    for t in range(len(slot_off) - 1):
        a, b = int(slot_off[t]), int(slot_off[t + 1])
        out[t] = hgbt_route_cpu(bins, table[a:b], node[t])
    return out

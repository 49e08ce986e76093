"""Loader for the in-tree HIP extension (csrc/ -> creditcore/_ccore.so).

The extension is built for gfx950 by ``python setup.py build_ext --inplace``
or ``__graft_entry__.build()``; the resulting .so lives inside the package so
it travels with the repo snapshot. On a machine with a visible GPU the
extension is REQUIRED: scoring ops raise ExtensionMissing rather than
silently falling back to an eager/CPU path (the CPU path must be requested
explicitly via device="cpu").
"""

from __future__ import annotations

import importlib

_ext = None
_err: Exception | None = None


class ExtensionMissing(RuntimeError):
    pass


def _try_load():
    global _ext, _err
    if _ext is not None or _err is not None:
        return
    try:
        import torch  # noqa: F401  (the extension links against libtorch)

        _ext = importlib.import_module("creditcore._ccore")
    except Exception as e:  # pragma: no cover
        _err = e


def available() -> bool:
    _try_load()
    return _ext is not None


def ext():
    """Return the extension module; raise loudly if missing."""
    _try_load()
    if _ext is None:
        raise ExtensionMissing(
            "creditcore._ccore HIP extension not built/loadable "
            f"(build with `python setup.py build_ext --inplace`): {_err}"
        )
    return _ext


def forest_sweep(codes, nums, forest: dict, sweep: dict, jobs, cut: float, want_curves=False):
    """forest_sweep of the extension on device tensors: ``forest`` holds the
    classifier tables (cls_nodes, cls_off, feat_col, feat_code, medians),
    ``sweep`` the breakpoint tables (node_rank, thr on the device; thr_off on
    the host; max_depth), ``jobs`` a host i32[J, 2] numpy table. Returns numpy
    ``(rec i32[J, 3], raw f64[J, 3], curves)``, curves a list of J arrays
    f64[K + 1] (views of one buffer) or None."""
    import numpy as np
    import torch

    jobs = np.ascontiguousarray(jobs, dtype=np.int32).reshape(-1, 2)
    rec, raw, flat = ext().forest_sweep(
        codes,
        nums,
        forest["cls_nodes"],
        forest["cls_off"],
        forest["feat_col"],
        forest["feat_code"],
        forest["medians"],
        sweep["node_rank"],
        sweep["thr"],
        sweep["thr_off"],
        torch.from_numpy(jobs),
        float(cut),
        int(sweep["max_depth"]),
        bool(want_curves),
    )
    rec, raw = rec.cpu().numpy(), raw.cpu().numpy()  # D2H copies synchronize
    if not want_curves:
        return rec, raw, None
    off = np.asarray(sweep["thr_off"])
    ends = np.cumsum(np.diff(off)[jobs[:, 1]] + 1)
    return rec, raw, np.split(flat.cpu().numpy(), ends[:-1])


def mmd_perm_w(z, norms, gamma: float, ind, cols_per_block: int, launch_rows: int = 0):
    """mmd_perm_w of the extension on device tensors (z f32[N, Dp], norms
    f32[N], ind u8[N, Q]): W = K . ind as numpy f64[N, Q]. ``launch_rows``
    > 0 runs it as several launches over slices of that many rows i (a
    multiple of the 64-row tile)."""
    import numpy as np

    n = int(z.shape[0])
    step = int(launch_rows) if launch_rows and launch_rows < n else n
    parts = [
        ext().mmd_perm_w(z, norms, float(gamma), ind, int(cols_per_block), a, min(step, n - a))
        for a in range(0, n, step)
    ]
    return np.concatenate([p.cpu().numpy() for p in parts])  # D2H copies synchronize


def knn_topk(
    z_batch,
    z_ref,
    norms_batch,
    norms_ref,
    k: int,
    exclude_self: bool = False,
    cols_per_block: int = 0,
    launch_rows: int = 0,
):
    """knn_topk of the extension on device tensors (z_batch f32[B, Dp], z_ref
    f32[M, Dp], their squared norms f32[B] and f32[M]): the k nearest
    reference rows per batch row as numpy ``(d2 f32[B, k], idx i32[B, k])``,
    ascending in (d2, j). ``cols_per_block`` (a multiple of the 64-row tile;
    0 picks knn.default_cols_per_block) is the reference slice of one block
    and does not change the result; ``launch_rows`` > 0 runs it as several
    launches over slices of that many batch rows (a multiple of the tile)."""
    import numpy as np

    from ..knn import default_cols_per_block

    b, m = int(z_batch.shape[0]), int(z_ref.shape[0])
    cols = int(cols_per_block) or default_cols_per_block(b, m)
    step = int(launch_rows) if launch_rows and launch_rows < b else b
    parts = [
        ext().knn_topk(z_batch, z_ref, norms_batch, norms_ref, int(k),
                       bool(exclude_self), cols, a, min(step, b - a))
        for a in range(0, b, step)
    ]
    # D2H copies synchronize
    return (np.concatenate([p[0].cpu().numpy() for p in parts]),
            np.concatenate([p[1].cpu().numpy() for p in parts]))


def forest_leaves(codes, nums, forest: dict):
    """forest_leaves of the extension on device tensors: leaf i32[R, T] on the
    device, the absolute node index of the leaf every row reaches in every
    classifier tree. ``forest`` holds the classifier tables as forest_sweep
    takes them."""
    return ext().forest_leaves(
        codes,
        nums,
        forest["cls_nodes"],
        forest["cls_off"],
        forest["feat_col"],
        forest["feat_code"],
        forest["medians"],
    )


def prox_index(leaf_ref, n_nodes: int) -> dict:
    """The inverted index of a reference's leaf table leaf_ref i32[M, T] (on
    the device): ``leaf_start`` i32[n_nodes + 1], a CSR keyed by absolute node
    index, and ``leaf_rows`` i16[<= M T], the reference rows of each leaf
    (below 16384; the kernel reads them unsigned). Entries of -1 (trees the
    leaf kernel skipped) are left out. Plain torch on the device: the order
    inside a list does not reach the result. ``lanes_per_tree`` is the
    kernel's default group width for these lists."""
    import torch

    from ..proximity import lanes_per_tree

    m, t = int(leaf_ref.shape[0]), int(leaf_ref.shape[1])
    flat = leaf_ref.reshape(-1).to(torch.int64)
    order = torch.argsort(flat)
    n_skipped = int((flat < 0).sum())
    rows = torch.div(order[n_skipped:], t, rounding_mode="floor").to(torch.int16)
    sizes = torch.bincount(flat[order[n_skipped:]], minlength=int(n_nodes))[: int(n_nodes)]
    start = torch.zeros(int(n_nodes) + 1, dtype=torch.int32, device=leaf_ref.device)
    start[1:] = torch.cumsum(sizes, 0).to(torch.int32)
    sq = float((sizes.to(torch.float64) ** 2).sum())
    return {
        "leaf_start": start,
        "leaf_rows": rows.contiguous(),
        "n_ref": m,
        "lanes_per_tree": lanes_per_tree(sq, int(rows.numel())),
    }


def forest_prox_topk(
    leaf_batch, index: dict, k: int, exclude_self: bool = False,
    lanes_per_tree: int = 0, launch_rows: int = 0,
):
    """forest_prox_topk of the extension: the k reference rows sharing most
    leaves with every row of leaf_batch i32[B, T] (on the device) as numpy
    ``(count i32[B, k], idx i32[B, k])`` in the order (count descending, j
    ascending). ``index`` is prox_index of the reference's leaf table;
    ``lanes_per_tree`` (a power of two up to 64; 0 takes the index's) does
    not change the result; ``launch_rows`` > 0 runs it as several launches
    over slices of that many batch rows."""
    import numpy as np

    b = int(leaf_batch.shape[0])
    lanes = int(lanes_per_tree) or int(index["lanes_per_tree"])
    step = int(launch_rows) if launch_rows and launch_rows < b else b
    parts = [
        ext().forest_prox_topk(leaf_batch, index["leaf_start"], index["leaf_rows"],
                               int(index["n_ref"]), int(k), bool(exclude_self), lanes,
                               a, min(step, b - a))
        for a in range(0, b, step)
    ]
    # D2H copies synchronize
    return (np.concatenate([p[0].cpu().numpy() for p in parts]),
            np.concatenate([p[1].cpu().numpy() for p in parts]))


def bin_select(x, f0: int, f1: int, max_bins: int, launch_rows: int):
    """bin_select of the extension on the device matrix ``x`` f32[N, F]: the
    radix-select summary of the columns [f0, f1). Returns ``(keys, state)``:
    the group's u32 keys i32[G, N], which stay on the device for
    ``ext().bin_assign``, and the per-column state as numpy i64[G, 2 + 2 *
    BIN_SLOTS] = {slot count, mode, keys, first ranks} (models/hgbt.py
    ``_state_edges`` reads it); the summary's only device-to-host copy."""
    keys, state = ext().bin_select(x, int(f0), int(f1), int(max_bins), int(launch_rows))
    return keys, state.cpu().numpy()  # the D2H copy synchronizes

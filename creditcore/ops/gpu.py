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

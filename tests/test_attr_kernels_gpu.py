"""forest_contrib_kernel, forest_shap_kernel, forest_shap_inter_kernel and
forest_ishap_kernel (csrc/creditcore_kernels.hip) on the hand-built forests
of _attr_cases.py, called through the bindings with device tensors uploaded
here, so that block_target (and with it the number of path chunks per row
block) can be chosen. Run on a real MI355X (`pytest -m gpu`);
test_attr_cases.py holds the CPU side of the same cases.

The reference is the exact tree-walk reference of _attr_cases.py, which reads
neither the path table nor cpu_ref. The bound is the project's GPU-vs-CPU
forest bound of 1e-9 (ATOL of test_shap_gpu.py). Exact properties (zeros,
symmetry) are asserted bit for bit."""

from __future__ import annotations

import itertools

import numpy as np
import pytest

import _attr_cases as ac
from _shap_models import N_SRC
from creditcore import engine as engine_mod
from creditcore.ops import cpu_ref
from creditcore.pack import N_CAT, build_shap_paths
from test_ishap import brute_force_ishap
from test_shap import brute_force_shap
from test_shap_interactions import brute_force_interactions

pytestmark = pytest.mark.gpu

ATOL = 1e-9
EDGE = 1e-6  # what neighbours across a compare edge differ by at least
ROWS_PER_BLOCK = {"contrib": 128, "shap": 128, "ishap": 128, "inter": 16}
BUILDS = [(f, k) for f in ac.FORESTS for k in ac.kinds_of(f)]


@pytest.fixture(scope="module")
def ext():
    from creditcore.ops import gpu as gpu_ops

    assert gpu_ops.available(), (
        "HIP extension must be present on a GPU box (no silent CPU fallback)"
    )
    return gpu_ops.ext()


def _dev(a, dtype=None):
    import torch

    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).cuda()  # a writable copy


@pytest.fixture(scope="module")
def build_of(ext):
    """(forest, cls_kind) -> the model, its checked tables and rows on the
    device, uploaded on first use."""
    cache = {}

    def get(forest: str, kind: int = 0) -> dict:
        if (forest, kind) not in cache:
            c, p = ac.case(forest), ac.model(forest, kind)
            paths, base = build_shap_paths(p)
            engine_mod._check_forest_tables(p)
            engine_mod._check_shap_paths(paths)
            cache[forest, kind] = {
                "p": p, "case": c, "paths": paths, "shap_base": base, "kind": kind,
                "n": {"contrib": p.cls_n_trees, "shap": paths.n_leaves,
                      "inter": paths.n_leaves, "ishap": paths.n_leaves},
                "codes": _dev(c.codes), "nums": _dev(c.nums),
                "bg_codes": _dev(c.bg_codes), "bg_nums": _dev(c.bg_nums),
                "cls_nodes": _dev(p.cls_nodes, np.int32),
                "cls_node_value": _dev(p.cls_node_value, np.float32),
                "cls_off": _dev(p.cls_tree_offsets, np.int32),
                "feat_col": _dev(p.feat_col, np.int32), "feat_code": _dev(p.feat_code, np.int32),
                "medians": _dev(p.medians, np.float32),
                "leaf_value": _dev(paths.leaf_value), "leaf_off": _dev(paths.leaf_off),
                "splits": _dev(paths.splits),
            }  # fmt: skip
        return cache[forest, kind]

    return get


def _args(d: dict, method: str, b: int, n_bg: int = 0) -> list:
    """Positional arguments of a binding, without block_target."""
    rows = [d["codes"][:b], d["nums"][:b]]
    if method == "contrib":
        return rows + [d["cls_nodes"], d["cls_node_value"], d["cls_off"], d["feat_col"],
                       d["feat_code"], d["medians"], d["kind"]]  # fmt: skip
    table = [d["leaf_value"], d["leaf_off"], d["splits"], d["medians"], d["kind"],
             int(d["p"].cls_n_trees)]  # fmt: skip
    if method == "ishap":
        return rows + [d["bg_codes"][:n_bg], d["bg_nums"][:n_bg]] + table
    return rows + table


def _binding(ext, method: str):
    return {"contrib": ext.forest_contrib, "shap": ext.forest_shap,
            "inter": ext.forest_shap_interactions, "ishap": ext.forest_ishap}[method]  # fmt: skip


def run(ext, d: dict, method: str, b: int, chunks: int, n_bg: int = 0) -> np.ndarray:
    """One launch with the block_target that gives ``chunks`` path (tree)
    chunks per row block, by the launchers' own formula."""
    rb = -(-b // ROWS_PER_BLOCK[method])
    block_target = chunks * rb
    assert ac.launch_chunks(block_target, rb, d["n"][method]) == chunks
    out = _binding(ext, method)(*_args(d, method, b, n_bg), block_target)
    return out.cpu().numpy()  # the D2H copy synchronizes the stream


def _chunk_counts(n: int) -> list[int]:
    return sorted({c for c in (1, 2, 3, n - 1, n) if 1 <= c <= n})


def check_exact(d: dict, forest: str, method: str, got: np.ndarray, n_bg: int) -> None:
    """What must hold bit for bit, whatever the chunking."""
    b = len(got)
    assert got.dtype == np.float64 and np.isfinite(got).all()
    if method == "inter":
        assert got.shape == (b, N_SRC, N_SRC)
        np.testing.assert_array_equal(got, got.transpose(0, 2, 1))
        idx = np.arange(N_SRC)
        assert (got[:, idx, idx] == 0.0).all()  # the diagonal is the engine's
    else:
        assert got.shape == (b, N_SRC)
    if method == "ishap" and n_bg == 1:
        assert (got[0] == 0.0).all()  # row 0 is its own background: all dummies
    if forest != "cover":
        return
    unsplit = list(ac.COVER_UNSPLIT)
    assert (got[:, unsplit] == 0.0).all()
    if method == "inter":
        assert (got[:, :, unsplit] == 0.0).all()
    if method in ("shap", "inter"):
        imp = cpu_ref.impute_nums(d["p"], d["case"].nums[:b])
        # tree a: a row that goes left at numeric 0 follows its z = 1 group and
        # is off the z = 0 group of the paths through numeric 1: exactly
        # nothing for either column, alone or in a pair
        left0 = imp[:, 0] <= 0.0
        # tree b: a row that goes right at numeric 5 follows z = 1
        right5 = ~(imp[:, 5] <= 0.0)
        assert (got[left0][:, [N_CAT, N_CAT + 1]] == 0.0).all()
        assert (got[right5][:, N_CAT + 5] == 0.0).all()
    if method == "inter":  # numerics 3 and 4 never share a path
        assert (got[:, N_CAT + 3, N_CAT + 4] == 0.0).all()


@pytest.mark.parametrize("method", ac.METHODS)
@pytest.mark.parametrize("forest,kind", BUILDS)
def test_chunk_sweep(ext, build_of, forest, kind, method):
    """1, 2, 3, n - 1 and n chunks per row block (n = leaves, or trees for
    the Saabas kernel): one block walks every path, or one path per block,
    or a chunk of root leaves alone (stripes, three chunks). Every result is
    held to the reference and to the results at the other chunk counts."""
    d = build_of(forest, kind)
    worst, spread = 0.0, 0.0
    for b, n_bg in itertools.product(ac.ROWS[method], ac.BG_ROWS if method == "ishap" else (0,)):
        ref = ac.reference(forest, kind, method, n_bg)[:b]
        outs = []
        for chunks in _chunk_counts(d["n"][method]):
            got = run(ext, d, method, b, chunks, n_bg)
            check_exact(d, forest, method, got, n_bg)
            worst = max(worst, float(np.abs(got - ref).max()))
            np.testing.assert_allclose(
                got, ref, rtol=0, atol=ATOL, err_msg=f"b={b} R={n_bg} chunks={chunks}"
            )
            outs.append(got)
        for x, y in itertools.combinations(outs, 2):
            spread = max(spread, float(np.abs(x - y).max()))
            np.testing.assert_allclose(x, y, rtol=0, atol=ATOL, err_msg=f"b={b} R={n_bg}")
        if b == max(ac.ROWS[method]):  # the reference is not trivially zero
            assert np.abs(ref).max() > 1e-3 or (forest, method) == ("stripes", "inter")
    print(f"{forest}/{kind} {method}: max |err| = {worst:.3e}, "
          f"max spread over chunk counts = {spread:.3e}")  # fmt: skip


@pytest.mark.parametrize("forest,kind", BUILDS)
def test_additivity_on_the_gpu(ext, build_of, forest, kind):
    """base + row sum is the raw model output of the naive walk (the logit
    for cls_kind 1), from the GPU values alone; the interaction rows close
    onto SHAP through the engine's diagonal."""
    from creditcore.engine import ScoringEngine

    d = build_of(forest, kind)
    c, p = d["case"], d["p"]
    out = ac.naive_output(p, c.codes, c.nums)
    errs = {}
    for chunks in (1, 3):
        got = run(ext, d, "contrib", 129, chunks)
        errs["contrib"] = np.abs(p.cls_base_value + got.sum(1) - out).max()
        got = run(ext, d, "shap", 129, chunks)
        errs["shap"] = np.abs(d["shap_base"] + got.sum(1) - out).max()
        for r in ac.BG_ROWS:
            base = float(np.mean(ac.naive_output(p, c.bg_codes[:r], c.bg_nums[:r])))
            got = run(ext, d, "ishap", 129, chunks, r)
            errs[f"ishap R={r}"] = np.abs(base + got.sum(1) - out).max()
        assert max(errs.values()) <= ATOL, (chunks, errs)
    b = max(ac.ROWS["inter"])
    res = ScoringEngine(p, device="cuda", device_index=0).explain_arrays(
        c.codes[:b], c.nums[:b], method="shap", interactions=True
    )
    m = res["interactions"]
    np.testing.assert_array_equal(m, m.transpose(0, 2, 1))
    errs["inter rows"] = np.abs(m.sum(2) - res["contributions"]).max()
    errs["inter total"] = np.abs(res["base_value"] + m.sum((1, 2)) - out[:b]).max()
    idx = np.arange(N_SRC)
    off = m.copy()
    off[:, idx, idx] = 0.0
    errs["inter engine"] = np.abs(off - ac.reference(forest, kind, "inter")).max()
    print(f"{forest}/{kind} additivity: " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) <= ATOL, errs


def test_threshold_forest_equals_brute_force(ext, build_of):
    """Rows on x == thr, one ulp to either side, +-0.0 and denormals against
    0.0, +-inf, NaN imputed onto a threshold and one ulp above it, codes -1,
    0 and 1 against either one-hot split: the kernels agree with the subset
    enumeration (Saabas has no coalition form: with the tree-walk sum), and
    two rows on the two sides of an edge get different values, so a wrong
    compare cannot pass by symmetry."""
    d = build_of("threshold", 0)
    c, p = d["case"], d["p"]
    b = max(ac.ROWS["inter"])
    want = {
        "contrib": ac.ref_contrib(p, c.codes, c.nums),
        "shap": brute_force_shap(p, c.codes, c.nums)[0],
        "inter": brute_force_interactions(p, c.codes[:b], c.nums[:b]),
        "ishap": brute_force_ishap(p, c.codes, c.nums, c.bg_codes, c.bg_nums)[0],
    }
    idx = np.arange(N_SRC)
    want["inter"][:, idx, idx] = 0.0
    for method in ac.METHODS:
        n_bg = 129 if method == "ishap" else 0
        for chunks in (1, d["n"][method]):
            got = run(ext, d, method, len(want[method]), chunks, n_bg)
            print(f"threshold {method} chunks={chunks}: brute force max |err| = "
                  f"{np.abs(got - want[method]).max():.3e}")  # fmt: skip
            np.testing.assert_allclose(got, want[method], rtol=0, atol=ATOL)
            pairs = [(x, y) for x, y in c.notes["neighbours"] if max(x, y) < len(got)]
            assert len(pairs) >= 12
            for x, y in pairs:
                assert np.abs(got[x] - got[y]).max() > EDGE, (method, x, y)


# ------------------------------------------------------------- the launchers

PATH_METHODS = ("shap", "inter", "ishap")


def _refused(ext, method, args, block_target=64):
    with pytest.raises(RuntimeError):
        _binding(ext, method)(*args, block_target)


def test_launcher_refusals(ext, build_of):
    """Host-side checks that raise before any launch."""
    import torch

    d = build_of("cover", 0)
    for method in ac.METHODS:
        good = _args(d, method, 17, 2)
        assert _binding(ext, method)(*good, 64).shape[0] == 17
        for bad_target in (0, 65536, -1):
            _refused(ext, method, good, bad_target)

        def swapped(i, t):
            return good[:i] + [t] + good[i + 1 :]

        def at(t):
            return next(k for k, x in enumerate(good) if x is t)

        # every tensor argument: on the host, of the wrong dtype, not contiguous
        for i, t in enumerate(good):
            if not isinstance(t, torch.Tensor):
                continue
            _refused(ext, method, swapped(i, t.cpu()))
            wrong = torch.float64 if t.dtype == torch.float32 else torch.int64
            _refused(ext, method, swapped(i, t.to(wrong)))
            if t.dim() == 2:
                strided = t.t().contiguous().t()
                assert strided.shape == t.shape and not strided.is_contiguous()
                _refused(ext, method, swapped(i, strided))
        _refused(ext, method, swapped(0, good[0][:16]))  # codes and nums: rows differ
        _refused(ext, method, swapped(at(d["medians"]), d["medians"][:13].contiguous()))
        if method == "contrib":
            _refused(ext, method, swapped(3, d["cls_node_value"][:-1].contiguous()))
            _refused(ext, method, swapped(4, d["cls_off"][:1].contiguous()))  # no trees
            continue
        off = at(d["leaf_off"])
        _refused(ext, method, swapped(off, d["leaf_off"][:-1].contiguous()))
        _refused(ext, method, swapped(off + 1, d["splits"][:, :3].contiguous()))
        _refused(ext, method, good[:-1] + [0])  # n_trees = 0
        if method == "ishap":
            _refused(ext, method, swapped(2, d["bg_codes"][:3]))  # 3 rows against 2
            _refused(ext, method, swapped(3, d["bg_nums"][:1]))
            _refused(ext, method, good[:2] + [d["bg_codes"][:0], d["bg_nums"][:0]] + good[4:])


def test_empty_inputs(ext, build_of):
    """B == 0 and L == 0 return zero tensors of the documented shapes."""
    import torch

    d = build_of("cover", 1)
    shape = {"contrib": (N_SRC,), "shap": (N_SRC,), "ishap": (N_SRC,), "inter": (N_SRC, N_SRC)}
    for method in ac.METHODS:
        out = _binding(ext, method)(*_args(d, method, 0, 2), 64)
        assert tuple(out.shape) == (0,) + shape[method] and out.dtype == torch.float64
        assert out.is_cuda
    empty = dict(d, leaf_value=d["leaf_value"][:0].contiguous(),
                 leaf_off=d["leaf_off"][:1].contiguous(), splits=d["splits"][:0].contiguous())  # fmt: skip
    for method in PATH_METHODS:
        out = _binding(ext, method)(*_args(empty, method, 17, 2), 64)
        assert tuple(out.shape) == (17,) + shape[method] and out.dtype == torch.float64
        assert (out.cpu().numpy() == 0.0).all()

"""Anchor rules for the classifier (Ribeiro et al. 2018; alibi's
``AnchorTabular``): request parsing, the caps, the predicates, the ``sat``
table, the beam search and the assembly of the answer.

The forest work (per candidate anchor: how many composite rows score above
the cut) is forest_anchor_kernel on the GPU and cpu_ref.forest_anchor_cpu on
the host; ScoringEngine.anchors ties them together. Everything in here is
host-side numpy and knows nothing about devices, so both engines return the
same answer. Nothing is random: precision and coverage are exact on the
sample, there is no bandit and no perturbation sampler.

Players are the 23 schema features in the attribution kernels' numbering
(0..N_CAT-1 categorical, N_CAT.. numeric); an anchor is a u32 set of players.
The predicate of a categorical player is ``feature == the row's category``.
The predicate of a numeric player is ``lo < value <= hi``, the interval of the
row's imputed value among ``z = unique(f32(quantile(sample column as f64,
disc_perc / 100)))``: interval ``k = #{z < x}`` (ale.py's rule, f32 compares),
(z[k-1], z[k]] with z[-1] = -inf and z[K] = +inf.

``sat[i, b]`` is the set of players whose predicate, taken from row i, sample
row b satisfies. The composite z(i, A, b) is sample row b with every player of
``A & ~sat[i, b]`` replaced by row i's value. ``precision(i, A)`` is the share
of sample rows whose composite has row i's decision (raw sum > cut,
counterfactual.raw_cut), ``coverage(i, A)`` the share with ``sat[i, b]``
containing A. A composite keeps the sample's value inside the row's interval,
so the full anchor has precision 1 only where no threshold of the forest lies
strictly inside a row's interval; the search does not rely on it.
"""

from __future__ import annotations

import numpy as np

from .counterfactual import check_threshold  # noqa: F401  (the same rule)
from .pack import N_CAT, N_NUM
from .schema import FEATURES

N_SRC = N_CAT + N_NUM

# caps of one anchors call (conditions, not measurements)
ANCHOR_MAX_ROWS = 1024  # rows per call, as ScoringEngine.SHAP_MAX_ROWS
ANCHOR_MAX_SAMPLE = 1024  # rows of a sample= override
ANCHOR_MAX_BEAM = 4
ANCHOR_MAX_PERC = 16  # entries of disc_perc


class AnchorTooLarge(ValueError):
    """An anchors request exceeded one of the caps above (the engine re-raises
    it as ExplainTooLarge)."""


def check_args(precision_threshold, beam_size, max_anchor_size, disc_perc):
    """(precision_threshold, beam_size, max_anchor_size, percentiles f64)."""
    def number(v):
        return not isinstance(v, (bool, str)) and isinstance(v, (int, float, np.number))

    def integer(v):
        return not isinstance(v, bool) and isinstance(v, (int, np.integer))

    if not number(precision_threshold) or not (0.0 < float(precision_threshold) <= 1.0):
        raise ValueError("precision_threshold must be a number in (0, 1]")
    if not integer(beam_size) or beam_size < 1:
        raise ValueError("beam_size must be a positive integer")
    if beam_size > ANCHOR_MAX_BEAM:
        raise AnchorTooLarge(f"beam_size is capped at {ANCHOR_MAX_BEAM}")
    if not integer(max_anchor_size) or not (1 <= max_anchor_size <= N_SRC):
        raise ValueError(f"max_anchor_size must be an integer in [1, {N_SRC}]")
    if isinstance(disc_perc, (str, bytes)) or not isinstance(disc_perc, (list, tuple)):
        raise ValueError("disc_perc must be a list of percentiles")
    if not disc_perc or not all(number(q) for q in disc_perc):
        raise ValueError("disc_perc must hold at least one number")
    if len(disc_perc) > ANCHOR_MAX_PERC:
        raise AnchorTooLarge(f"disc_perc is capped at {ANCHOR_MAX_PERC} percentiles")
    perc = np.asarray(disc_perc, dtype=np.float64)
    if not ((perc > 0.0) & (perc < 100.0)).all() or not (np.diff(perc) > 0).all():
        raise ValueError("disc_perc must ascend strictly inside (0, 100)")
    return float(precision_threshold), int(beam_size), int(max_anchor_size), perc


def disc_edges(bg_nums_imp: np.ndarray, perc: np.ndarray) -> list:
    """Per numeric column the distinct f32 quantile edges of the imputed
    sample column (module docstring)."""
    cols = np.asarray(bg_nums_imp, dtype=np.float32).astype(np.float64)
    q = np.quantile(cols, perc / 100.0, axis=0)  # [n_perc, N_NUM]
    return [np.unique(q[:, c].astype(np.float32)) for c in range(N_NUM)]


def intervals(edges: list, nums_imp: np.ndarray) -> np.ndarray:
    """i32[R, N_NUM]: per value the number of its column's edges below it."""
    x = np.asarray(nums_imp, dtype=np.float32)
    return np.stack(
        [np.searchsorted(edges[c], x[:, c], side="left") for c in range(N_NUM)], axis=1
    ).astype(np.int32)


def sat_table(codes, nums_imp, bg_codes, bg_nums_imp, edges) -> np.ndarray:
    """u32[R, S]: bit p of ``sat[i, b]`` says that sample row b has row i's
    category (p < N_CAT) or lies in row i's interval (numeric p)."""
    own = np.concatenate([np.asarray(codes, dtype=np.int32), intervals(edges, nums_imp)], axis=1)
    bg = np.concatenate(
        [np.asarray(bg_codes, dtype=np.int32), intervals(edges, bg_nums_imp)], axis=1
    )
    sat = np.zeros((len(own), len(bg)), dtype=np.uint32)
    for p in range(N_SRC):
        sat |= (own[:, p, None] == bg[None, :, p]).astype(np.uint32) << np.uint32(p)
    return sat


def coverage_counts(sat_row: np.ndarray, masks: np.ndarray) -> np.ndarray:
    """i64[n]: per mask the number of sample rows whose sat word holds it."""
    m = np.asarray(masks, dtype=np.uint32)[:, None]
    return ((sat_row[None, :] & m) == m).sum(axis=1)


def extensions(beam: list) -> np.ndarray:
    """The distinct one-player extensions of the beam's anchors, ascending."""
    out = {a | (1 << p) for a in beam for p in range(N_SRC) if not (a >> p) & 1}
    return np.array(sorted(out), dtype=np.uint32)


def search(run, sat: np.ndarray, decision: np.ndarray, thr: float, beam_size: int, max_size: int):
    """The beam search of every row, level by level: one ``run(masks u32[M],
    mask_off i32[R + 1]) -> counts[M]`` call per level carries the candidate
    lists of all rows still searching (an empty list for the others).
    ``counts[m]`` is the number of sample rows whose composite scores above the
    cut; ``decision`` the rows' own 0/1 decisions. Returns per row ``(mask,
    hits, covered, met)`` with hits and covered counted in sample rows."""
    r, s = sat.shape
    result = [None] * r
    beams = [[0] for _ in range(r)]
    for level in range(max_size + 1):
        lists = [
            np.empty(0, dtype=np.uint32) if result[i] is not None
            else (np.zeros(1, dtype=np.uint32) if level == 0 else extensions(beams[i]))
            for i in range(r)
        ]
        mask_off = np.zeros(r + 1, dtype=np.int32)
        mask_off[1:] = np.cumsum([len(c) for c in lists])
        if mask_off[-1] == 0:
            break
        counts = np.asarray(run(np.concatenate(lists), mask_off), dtype=np.int64)
        for i in range(r):
            cand = lists[i]
            if not len(cand):
                continue
            cnt = counts[mask_off[i] : mask_off[i + 1]]
            hits = cnt if decision[i] else s - cnt
            cov = coverage_counts(sat[i], cand)
            met = hits / s >= thr
            if met.any():
                # largest coverage, then higher precision, then the lower mask
                k = np.lexsort((cand, -hits, -cov, ~met))[0]
                result[i] = (int(cand[k]), int(hits[k]), int(cov[k]), True)
                continue
            # best precision, then larger coverage, then the lower mask
            order = np.lexsort((cand, -cov, -hits))
            k = order[0]
            if level == max_size or level == N_SRC:
                result[i] = (int(cand[k]), int(hits[k]), int(cov[k]), False)
            elif level > 0:
                beams[i] = [int(a) for a in cand[order[:beam_size]]]
    return result


def describe(mask: int, codes_row, nums_row, edges: list, vocabs) -> tuple[list, list]:
    """(anchor entries, readable names) of one row's anchor, in player order."""
    entries, names = [], []
    for p in range(N_SRC):
        if not (mask >> p) & 1:
            continue
        name = FEATURES[p]
        if p < N_CAT:
            code = int(codes_row[p])
            cat = vocabs[p][code] if 0 <= code < len(vocabs[p]) else None
            entries.append({"feature": name, "category": cat})
            names.append(f"{name} = {cat}")
            continue
        z = edges[p - N_CAT]
        k = int(np.searchsorted(z, np.float32(nums_row[p - N_CAT]), side="left"))
        lo = float(z[k - 1]) if k > 0 else None
        hi = float(z[k]) if k < len(z) else None
        entries.append({"feature": name, "low": lo, "high": hi})
        if lo is None and hi is None:  # a constant sample column: always true
            names.append(f"{name} = any")
        elif lo is None:
            names.append(f"{name} <= {hi}")
        elif hi is None:
            names.append(f"{name} > {lo}")
        else:
            names.append(f"{lo} < {name} <= {hi}")
    return entries, names


def launch_slices(mask_off: np.ndarray, n_sample: int, max_pairs: int):
    """Row ranges [a, b) whose (mask, sample row) pairs stay within
    ``max_pairs`` (a row's list is never cut, so one row may exceed it)."""
    r = len(mask_off) - 1
    budget = max(1, max_pairs // max(1, n_sample))
    a = 0
    while a < r:
        b = a + 1
        while b < r and mask_off[b + 1] - mask_off[a] <= budget:
            b += 1
        yield a, b
        a = b

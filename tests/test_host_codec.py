"""The host side of /score (csrc/host_codec.h: JSON request parser, response
writer, drift p-value epilogue) compiled on its own into
tests/host/codec_harness.cpp with AddressSanitizer and UBSan and run as a
child process: nothing is loaded into Python and nothing here needs a GPU.

Every body of tests/_json_cases.py goes through the harness and through the
oracle, ``TypeAdapter(list[LoanApplicant]).validate_json`` followed by
``encode_batch`` (what serve.py falls back to). The contract:

(a) a body the oracle rejects, the parser rejects;
(b) a body the parser accepts encodes exactly as the oracle's;
(c) the parser may reject what the oracle takes (the request then goes the
    slow way), but never the bodies the fast path exists for, and at most
    10 % of the other bodies the oracle takes;
(d) the extension's JsonEncoder.encode, where built, behaves as the harness.
"""

from __future__ import annotations

import json
import os
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from _json_cases import VOCABS, _hash_twins, corpus, must_accept
from creditcore.schema import (
    CATEGORICAL_FEATURES,
    FEATURES,
    MISSING_CATEGORY,
    NUMERIC_FEATURES,
    LoanApplicant,
)

REPO = Path(__file__).resolve().parent.parent
N_CAT, N_NUM = len(CATEGORICAL_FEATURES), len(NUMERIC_FEATURES)
SANITIZE = ["-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def find_clangxx() -> str | None:
    """ROCm's clang++ (the compiler the extension's host code is built by)."""
    roots = [os.environ.get(v) for v in ("ROCM_PATH", "ROCM_HOME")] + ["/opt/rocm"]
    for root in roots:
        for sub in ("llvm/bin", "lib/llvm/bin"):
            cand = Path(root, sub, "clang++") if root else None
            if cand and cand.is_file():
                return str(cand)
    return None


def build_harness(out: Path, flags: list[str], header_dir: Path = REPO / "csrc") -> Path:
    cxx = find_clangxx()
    if cxx is None:
        pytest.skip("no clang++ under $ROCM_PATH/llvm/bin or /opt/rocm/llvm/bin: "
                    "ROCm's clang++ is needed to build tests/host/codec_harness.cpp")
    cmd = [cxx, *flags, "-I", str(header_dir), str(REPO / "tests/host/codec_harness.cpp"),
           "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"harness build failed: {' '.join(cmd)}\n{r.stderr[-4000:]}"
    return out


@pytest.fixture(scope="session")
def harness(tmp_path_factory) -> Path:
    return build_harness(tmp_path_factory.mktemp("codec_harness") / "codec_harness", SANITIZE)


def run_harness(exe: Path, mode: str, blobs: list[bytes], tmp: Path) -> list[str]:
    """Write the case file, run the harness as a child and return its lines.
    Any sanitizer report or non-zero exit fails the test."""
    path = tmp / f"{mode}.cases"
    with open(path, "wb") as f:
        for b in blobs:
            f.write(struct.pack("<I", len(b)))
            f.write(b)
    r = subprocess.run([str(exe), mode, str(path)], capture_output=True)
    err = r.stderr.decode("utf-8", "replace")
    assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, (
        f"harness {mode}: exit {r.returncode}\n{err[-6000:]}")
    return r.stdout.decode("ascii").splitlines()


def _str(s: str) -> bytes:
    b = s.encode()
    return struct.pack("<I", len(b)) + b


def default_row() -> tuple[np.ndarray, np.ndarray]:
    from creditcore.pack import encode_batch

    dc, dn = encode_batch([LoanApplicant().__dict__], VOCABS)
    return np.ascontiguousarray(dc[0], np.int16), np.ascontiguousarray(dn[0], np.float32)


def config_blob() -> bytes:
    dc, dn = default_row()
    out = struct.pack("<II", N_CAT, N_NUM)
    for name, vocab in zip(CATEGORICAL_FEATURES, VOCABS):
        out += _str(name) + struct.pack("<I", len(vocab)) + b"".join(_str(w) for w in vocab)
    out += b"".join(_str(n) for n in NUMERIC_FEATURES) + _str(MISSING_CATEGORY)
    return out + dc.tobytes() + dn.tobytes()


def parse_line(line: str):
    """None for ERR, else (codes int16 [B, 9], nums float32 [B, 14])."""
    if line.startswith("ERR "):
        return None
    tag, rows, hc, hn = line.split(" ")
    assert tag == "OK"
    b = int(rows)
    codes = np.frombuffer(bytes.fromhex(hc.strip("-")), np.int16).reshape(b, N_CAT)
    nums = np.frombuffer(bytes.fromhex(hn.strip("-")), np.float32).reshape(b, N_NUM)
    return codes, nums


@pytest.fixture(scope="session")
def oracle():
    return compute_oracle()


def compute_oracle() -> dict:
    """Per case: None where the pydantic path rejects, else its arrays."""
    from pydantic import TypeAdapter, ValidationError

    from creditcore.pack import encode_batch

    adapter = TypeAdapter(list[LoanApplicant])
    out = {}
    with np.errstate(over="ignore"):
        for name, body in corpus():
            try:
                data = adapter.validate_json(body)
            except ValidationError:
                out[name] = None
                continue
            if not data:
                out[name] = (np.zeros((0, N_CAT), np.int16), np.zeros((0, N_NUM), np.float32))
                continue
            c, n = encode_batch([r.__dict__ for r in data], VOCABS)
            out[name] = (np.asarray(c, np.int16), np.asarray(n, np.float32))
    return out


@pytest.fixture(scope="session")
def parsed(harness, tmp_path_factory):
    cases = corpus()
    lines = run_harness(harness, "parse", [config_blob()] + [b for _, b in cases],
                        tmp_path_factory.mktemp("parse"))
    assert len(lines) == len(cases)
    return {name: parse_line(line) for (name, _), line in zip(cases, lines)}


def same_arrays(got, want) -> bool:
    """Codes equal; nums equal as float32 values: NaN matches NaN, and -0.0
    may stand for 0.0."""
    return (got[0].shape == want[0].shape and got[1].shape == want[1].shape
            and np.array_equal(got[0], want[0])
            and np.array_equal(got[1], want[1], equal_nan=True))


def _show(names, per_group=12) -> str:
    """The first few offenders of every group, so that one flood (the
    mutations) does not hide the rest."""
    bodies = dict(corpus())
    seen: dict[str, int] = {}
    rows = []
    for n in names:
        g = n.split("/")[0]
        seen[g] = seen.get(g, 0) + 1
        if seen[g] <= per_group:
            rows.append(f"  {n}: {bodies[n][:90]!r}")
    return "\n".join(rows) + f"\n  in all: {seen}"


def test_corpus_is_deterministic_and_covers_both_sides(oracle):
    cases = corpus()
    assert len(cases) > 10000
    accepted = sum(v is not None for v in oracle.values())
    print(f"{len(cases)} cases, {accepted} accepted by the pydantic path")
    assert 500 < accepted < len(cases) - 5000
    groups = {n.split("/")[0] for n, _ in cases}
    assert groups == {"base", "trunc", "mut", "num", "str", "struct", "rand"}
    # the parser's dispatch hash is (length, last character) of the key: when
    # the schema gains two keys that collide, their cases must be there
    twins = _hash_twins()
    print(f"schema keys colliding in the dispatch hash: {twins or 'none (near misses stand in)'}")
    names = {n for n, _ in cases}
    assert all(f"str/hash_twin/{k}" in names for k in range(len(twins)))
    assert sum(n.startswith("str/hash_near/") for n in names) >= 10


def test_a_rejected_by_oracle_is_rejected(parsed, oracle):
    wrong = [n for n, v in oracle.items() if v is None and parsed[n] is not None]
    assert not wrong, (f"{len(wrong)} bodies answered 200 on the fast path that the pydantic "
                       f"path answers 422:\n{_show(wrong)}")


def test_b_accepted_encodes_as_oracle(parsed, oracle):
    wrong = [n for n, v in oracle.items()
             if v is not None and parsed[n] is not None and not same_arrays(parsed[n], v)]
    assert not wrong, f"{len(wrong)} bodies encode differently:\n{_show(wrong)}"


def test_c_fast_path_takes_what_it_exists_for(parsed, oracle):
    names = [n for n, _ in corpus() if must_accept(n)]
    assert len(names) == 203
    assert all(oracle[n] is not None for n in names), "corpus error: a valid body the oracle rejects"
    wrong = [n for n in names if parsed[n] is None]
    assert not wrong, f"valid bodies sent to the fallback:\n{_show(wrong)}"
    rest = [n for n, v in oracle.items() if v is not None and not must_accept(n)]
    lost = [n for n in rest if parsed[n] is None]
    print(f"(c) {len(lost)} of {len(rest)} other oracle-accepted bodies go to the fallback")
    assert len(lost) <= 0.10 * len(rest), _show(lost)


def test_d_extension_matches_harness(parsed):
    import torch  # noqa: F401  (loads libc10 for the extension)

    from creditcore.ops import gpu

    if not gpu.available():
        # absent is a skip; built but not importable (say an undefined symbol
        # after the header split) is a failure
        built = list((REPO / "creditcore").glob("_ccore*.so"))
        assert not built, f"extension built but not importable: {gpu._err!r}"
        pytest.skip("extension not built: no creditcore/_ccore*.so")
    dc, dn = default_row()
    enc = gpu.ext().JsonEncoder(VOCABS, CATEGORICAL_FEATURES, NUMERIC_FEATURES,
                                MISSING_CATEGORY, dc, dn)
    wrong = []
    for name, body in corpus():
        try:
            c, n = enc.encode(body)
            got = (np.asarray(c), np.asarray(n))
        except ValueError:
            got = None
        want = parsed[name]
        if (got is None) != (want is None):
            wrong.append(name)
        elif got is not None and not (
            got[0].dtype == np.int16 and got[1].dtype == np.float32
            and got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
            and got[0].shape == want[0].shape and got[1].shape == want[1].shape
        ):
            wrong.append(name)
    assert not wrong, f"extension and harness disagree:\n{_show(wrong)}"


# ------------------------------------------------------------------ timing


def parse_time_ns(tmp: Path, header_dir: Path = REPO / "csrc", runs: int = 1) -> list[int]:
    """The harness's ``time`` mode, built with -O2 and no sanitizer against
    the host_codec.h in ``header_dir``: per run, the median over 200 parses of
    the 1024-row ``make_request_batch`` body, in ns. To compare two versions
    of the parser, call it with two directories, alternating the runs: the
    spread between runs of one version is several per cent."""
    from creditcore.data import make_request_batch

    tmp.mkdir(parents=True, exist_ok=True)
    exe = build_harness(tmp / "codec_harness_o2", ["-std=c++17", "-O2"], header_dir)
    body = json.dumps(make_request_batch(1024)).encode()
    out = []
    for _ in range(runs):
        (line,) = run_harness(exe, "time", [config_blob(), body], tmp)
        tag, median, fastest, rows = line.split()
        assert tag == "TIME" and int(rows) == 1024
        out.append(int(median))
    return out


def test_time_mode_parses_the_benchmark_body(tmp_path):
    """Prints the figure; a time is not asserted (it belongs to the machine)."""
    (median,) = parse_time_ns(tmp_path)
    print(f"1024-row body: median parse {median / 1e3:.1f} us (-O2, 200 parses)")


# ------------------------------------------------------------------ writer

AWKWARD = [0.0, 1.0, 0.1, 2 / 3, 1e-300, 1.7976931348623157e308, 5e-324,
           123456789.123456789, 0.49999999999999994, 1e16, 1e-5]


def _bits(v: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def test_e_writer_round_trips_and_spells_as_json_dumps(harness, tmp_path):
    rng = np.random.default_rng(2024)
    pats = rng.integers(0, 2**64, size=12000, dtype=np.uint64)
    rand = pats.view(np.float64)
    rand = rand[np.isfinite(rand)][:10000]
    assert len(rand) == 10000
    special = [-0.0, float("nan"), float("inf"), float("-inf")]
    vals = np.concatenate([rand, np.array(AWKWARD + [-v for v in AWKWARD] + special)])
    b = len(vals)
    outl = np.array([(0.0, 1.0, -0.0, 2.5, float("nan"))[i % 5] for i in range(b)])
    pvals = np.concatenate([np.linspace(0.0, 1.0, len(FEATURES) - 4),
                            [float("nan"), float("inf"), float("-inf"), 1e-300]])
    blob = (struct.pack("<I", b) + vals.astype("<f8").tobytes() + outl.astype("<f8").tobytes()
            + struct.pack("<I", len(FEATURES)) + b"".join(_str(f) for f in FEATURES)
            + pvals.astype("<f8").tobytes())
    (raw,) = run_harness(harness, "write", [blob], tmp_path)

    doc = json.loads(raw)
    assert list(doc) == ["predictions", "outliers", "feature_drift_batch"]
    assert len(doc["predictions"]) == b
    bad = [(i, float(vals[i]), g) for i, g in enumerate(doc["predictions"])
           if not isinstance(g, float) or _bits(g) != _bits(float(vals[i]))]
    assert not bad, bad[:10]
    assert doc["outliers"] == [0.0 if o == 0.0 else 1.0 for o in outl]
    # 1 - p formed in float32
    with np.errstate(invalid="ignore"):
        want = (np.float32(1.0) - pvals.astype(np.float32)).astype(np.float64)
    assert list(doc["feature_drift_batch"]) == FEATURES
    for f, w in zip(FEATURES, want):
        assert _bits(doc["feature_drift_batch"][f]) == _bits(float(w)), f
    # the text itself: every token is a float literal to Python's json, and
    # the non-finite ones are spelled as json.dumps spells them
    head = '{"predictions": ['
    assert raw.startswith(head)
    tokens = raw[len(head):raw.index("]")].split(", ")
    assert len(tokens) == b
    for tok, v in zip(tokens, vals):
        if not np.isfinite(v):
            assert tok == json.dumps(float(v)), (tok, v)
        else:
            assert "." in tok or "e" in tok, tok  # a float to json.loads, not an int
    for f, w in zip(FEATURES[-4:], want[-4:]):
        assert f'"{f}": {json.dumps(float(w))}' in raw


# ---------------------------------------------------------------- p-values

PV_N = (1, 2, 139, 140, 141, 299, 300, 499, 500, 16384)
_REF_COUNTS = [[50, 40, 31, 22, 12], [17], [300, 120], [9, 0, 4]]  # [17]: a one-bin category


def _pv_d(n: int) -> np.ndarray:
    return np.array([0.0, 1.0 / n, 0.5, 1.0 - 1.0 / n, 1.0], dtype=np.float32)


def _pv_hists() -> dict[str, list[list[int]]]:
    return {
        "all_zero": [[0] * len(r) for r in _REF_COUNTS],
        "as_reference": [list(r) for r in _REF_COUNTS],
        # p strictly inside (0, 1), statistic below 94: the range in which
        # test_drift_pvals_host.py states its 2.2e-14. (exp(-x/2) carries the
        # rounding of x, x/2 * 1.1e-16 relative, in this code and in scipy
        # alike, so a far larger statistic has no reference that good.)
        "shifted": [[5, 9, 14, 20, 16], [64], [20, 31], [2, 0, 7]],
    }


def test_f_pvalues_on_the_edge_grid(harness, tmp_path):
    """drift_pvals_raw on the grid where its algorithm changes (en = 140/141,
    299/300, 499/500), at both ends of D and with degenerate histograms.
    Tolerances are those of tests/test_drift_pvals_host.py: K-S 4.5e-14
    absolute against scipy.stats.kstwo.sf for en <= 140 and 3e-7 above;
    chi-square 2.2e-14 relative against chi2_contingency, exact where p is 0
    or 1."""
    from scipy import stats

    from creditcore.models.drift import chi2_from_counts

    off = np.concatenate([[0], np.cumsum([len(r) for r in _REF_COUNTS])]).astype("<i4")
    rc = np.concatenate(_REF_COUNTS).astype("<i4")
    blobs, keys = [], []
    for n in PV_N:
        for kind, hist in _pv_hists().items():
            d = _pv_d(n)
            blobs.append(struct.pack("<qqI", 2 * n, 2 * n, len(_REF_COUNTS)) + off.tobytes()
                         + rc.tobytes() + np.concatenate(hist).astype("<i4").tobytes()
                         + struct.pack("<I", len(d)) + d.astype("<f4").tobytes())
            keys.append((n, kind, hist))
    lines = run_harness(harness, "pvals", blobs, tmp_path)
    assert len(lines) == len(blobs)
    for (n, kind, hist), line in zip(keys, lines):
        pv = np.array([int(h, 16) for h in line.split(" ")], dtype=np.uint64).view(np.float64)
        assert pv.shape == (len(_REF_COUNTS) + 5,)
        assert np.isfinite(pv).all() and ((pv >= 0.0) & (pv <= 1.0)).all(), (n, kind, pv)
        for j, (r, h) in enumerate(zip(_REF_COUNTS, hist)):
            ref = chi2_from_counts(np.asarray(r, np.int32), np.asarray(h, np.int32))
            if kind != "shifted" or len(r) == 1:
                assert pv[j] == ref == 1.0, (n, kind, j, pv[j], ref)
            else:
                assert 0.0 < ref < 1.0
                assert abs(pv[j] - ref) <= 2.2e-14 * ref, (n, kind, j, pv[j], ref)
        d = _pv_d(n)
        ref = stats.kstwo.sf(d.astype(np.float64), n)
        err = np.abs(pv[len(_REF_COUNTS):] - ref)
        assert err.max() <= (4.5e-14 if n <= 140 else 3e-7), (n, kind, d, err)
        assert pv[len(_REF_COUNTS)] == 1.0 and pv[-1] == 0.0  # D = 0, D = 1

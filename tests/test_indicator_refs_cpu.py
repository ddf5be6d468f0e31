"""The indicator ESS of include/mcmcref_iess.h without a GPU: a Python-integer restatement of the definition held to the
reference's own `_ess` (tests/golden/indicator_ess_cases.json, written by make_indicator_ess_golden.py), the host routine
mci_indicator_ess_host held to the restatement, the edges and refusals, and the mirror `_iabi` against the header and the
exports of libmcmcref_iess.so.  libmcmcref_hip.so keeps exactly the symbols its two headers declare.

Tolerances: the truncation lag and the counts are integers and must be equal; ESS is held to 1e-9 relative, the project's
gate for a floating output against the reference's algorithm (the restatement itself is exact rational arithmetic, rounded
once).  A fixture case is flagged when A(lag) == 0 at a lag up to the truncation: there the reference decides on the sign
of a rounding error, so its lag is compared only where it agrees.
"""
from __future__ import annotations

import ctypes as C
import functools
import json
import math
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from test_abi_mirror_cpu import DECLARATION, ROOT, c_class, py_class
from test_host_cpu import built_lib  # noqa: F401  (the fixture: an up-to-date build of both libraries)

RTOL = 1e-9
INF = float("inf")


def restate(bits) -> tuple[float, int, int]:
    """(ESS, trunc, ones) of 0/1 chains [C][N] by the definition: Python integers for every count and A(lag), exact
    rationals for var_hat and the sum of rho, one rounding at the end."""
    b = np.asarray(bits, dtype=np.int64)
    m, n = b.shape
    ks = [int(v) for v in b.sum(axis=1)]
    ones = sum(ks)
    if n < 2:
        return math.nan, -1, ones
    W = Fraction(sum(k * (n - k) for k in ks), m * n * (n - 1))
    B = Fraction(m * sum(k * k for k in ks) - ones * ones, m * n * (m - 1)) if m > 1 else Fraction(0)
    var_hat = Fraction(n - 1, n) * W + B / n
    if var_hat == 0:
        return float(m * n), 0, ones
    R, trunc = Fraction(0), n
    for lag in range(1, n):
        A = 0
        for c in range(m):
            S = int((b[c, :n - lag] & b[c, lag:]).sum())
            H, T = int(b[c, :n - lag].sum()), int(b[c, lag:].sum())
            A += n * n * S - n * ks[c] * (H + T) + (n - lag) * ks[c] * ks[c]
        if A < 0:
            trunc = lag
            break
        R += Fraction(A, n * n * (n - lag)) / (m * var_hat)
    return float(Fraction(m * n) / (1 + 2 * R)), trunc, ones


@functools.lru_cache(maxsize=None)
def fixture_cases() -> tuple:
    cases = json.loads((ROOT / "tests" / "golden" / "indicator_ess_cases.json").read_text())["cases"]
    return tuple(cases)


def case_bits(case) -> np.ndarray:
    return np.array([[int(ch) for ch in row] for row in case["chains"]], dtype=np.int64)


def host(bits) -> tuple[float, int, int]:
    """mci_indicator_ess_host of 0/1 chains, the indicator being 0.5 < x."""
    from mcmc_ref_hip import indicator
    r = indicator.indicator_ess_host(np.asarray(bits, dtype=np.float64)[None], 0.5, INF)
    return float(r["ess"][0, 0]), int(r["trunc"][0, 0]), int(r["ones"][0, 0])


def close(a: float, b: float) -> bool:
    return (math.isnan(a) and math.isnan(b)) or abs(a - b) <= RTOL * abs(b)


def ar1_bits(rng, C_: int, N: int, phi: float, prob: float = 0.5, ties: bool = False) -> np.ndarray:
    e = rng.normal(size=(C_, N))
    y = e.copy()
    for t in range(1, N):
        y[:, t] = phi * y[:, t - 1] + e[:, t]
    if ties:
        y = np.round(y * 2) / 2
    return (y <= np.quantile(y, prob)).astype(np.int64)


# ---- the restatement against the reference ---------------------------------------------------------------------------------

def test_fixture_has_the_cases():
    cases = fixture_cases()
    assert len(cases) >= 100 and len({c["name"] for c in cases}) == len(cases)
    assert {c["N"] for c in cases} >= {2, 3, 5, 63, 64, 65, 127, 128, 129, 500} and {c["C"] for c in cases} >= {1, 2, 3, 4, 5}
    assert {c["phi"] for c in cases} == {0.0, 0.5, 0.9} and {c["prob"] for c in cases} == {0.05, 0.5, 0.95}
    assert all(c["C"] * c["N"] <= 2000 and len(c["chains"]) == c["C"] and all(len(r) == c["N"] for r in c["chains"]) for c in cases)
    assert sum(c["flagged"] for c in cases) <= len(cases) // 10


def test_restatement_matches_the_reference():
    for c in fixture_cases():
        ess, trunc, ones = restate(case_bits(c))
        assert ones == sum(r.count("1") for r in c["chains"]), c["name"]
        if not c["flagged"]:
            assert trunc == c["trunc"], c["name"]
        if trunc == c["trunc"]:
            assert close(ess, c["ess"]), (c["name"], ess, c["ess"])


# ---- the host routine against the restatement ------------------------------------------------------------------------------

def test_host_matches_the_restatement_on_the_fixture(built_lib):  # noqa: F811
    for c in fixture_cases():
        bits = case_bits(c)
        ess, trunc, ones = host(bits)
        exp = restate(bits)
        assert (trunc, ones) == exp[1:] and close(ess, exp[0]), (c["name"], (ess, trunc, ones), exp)


LB = 256                                                           # MCI_LAG_BLOCK (test_mirror_constants holds it to the header)


@functools.lru_cache(maxsize=None)
def long_walk_cases() -> dict:
    """0/1 chains of AR(1) draws at phi = 0.995 around the lag block: N = LB - 1, LB, LB + 1 and two blocks + 1.  The
    first negative lag of such a chain lies near N / 3 (a chain's autocovariances about its own mean sum to a negative
    number, so none was found past N / 2.5), hence no chain of two blocks + 1 draws walks past the first block; the two
    chains of three blocks + 7 draws do (seeds picked for it: truncation at 260 and 311)."""
    rng = np.random.default_rng(7)
    cases = {f"n{N}_c{C_}": ar1_bits(rng, C_, N, 0.995) for N in (LB - 1, LB, LB + 1, 2 * LB + 1) for C_ in (1, 3)}
    cases["n775_c1"] = ar1_bits(np.random.default_rng(3), 1, 3 * LB + 7, 0.995)
    rng = np.random.default_rng(38)
    ar1_bits(rng, 2, 3 * LB + 7, 0.995)
    cases["n775_c2"] = ar1_bits(rng, 2, 3 * LB + 7, 0.995, 0.2)
    return cases


def test_host_matches_the_restatement_past_one_lag_block(built_lib):  # noqa: F811
    """Chains whose truncation lies beyond the first block of MCI_LAG_BLOCK lags, and an indicator with no negative lag."""
    truncs = {}
    for name, bits in long_walk_cases().items():
        exp = restate(bits)
        got = host(bits)
        assert got[1:] == exp[1:] and close(got[0], exp[0]), (name, got, exp)
        truncs[name] = exp[1]
    assert truncs["n775_c1"] > LB and truncs["n775_c2"] > LB, truncs
    # (a single chain always has a negative lag; chains that are constant at different levels have A == 0 at every lag)
    level = np.stack([np.ones(2 * LB + 1, dtype=np.int64), np.zeros(2 * LB + 1, dtype=np.int64)])
    exp = restate(level)
    assert exp == (float(level.size), level.shape[1], 2 * LB + 1)  # no negative lag: trunc = n, every rho is 0
    got = host(level)
    assert got == exp


def test_hand_case_and_the_zero_rule(built_lib):  # noqa: F811
    bits = np.array([[1, 1, 1, 0, 0, 0]])
    assert restate(bits) == (30 / 11, 3, 3)
    ess, trunc, ones = host(bits)
    assert (trunc, ones) == (3, 3) and close(ess, 30 / 11)


def test_edges(built_lib):  # noqa: F811
    from mcmc_ref_hip import indicator
    ess, trunc, ones = host(np.array([[1], [0], [1]]))            # n < 2
    assert math.isnan(ess) and (trunc, ones) == (-1, 2)
    x = np.arange(24, dtype=np.float64).reshape(1, 3, 8)
    r = indicator.indicator_ess_host(x, [-INF, 100.0, 5.0, 5.0, -INF], [INF, INF, 5.0, 4.0, -INF])
    assert r["ess"].tolist() == [[24.0] * 5] and r["trunc"].tolist() == [[0] * 5]       # var_hat == 0: m n, trunc 0
    assert r["ones"].tolist() == [[24, 0, 0, 0, 0]]            # all ones, all zeros, lower == upper, lower > upper, empty
    y = x.copy()
    y[0, 1, 3] = math.nan                                          # a NaN draw counts as 0
    assert indicator.indicator_ess_host(y, -INF, INF)["ones"].tolist() == [[23]]
    one = np.array([[1, 0, 0, 1, 1, 0, 1, 0, 0, 0, 1]])           # one chain
    assert host(one)[1:] == restate(one)[1:] and close(host(one)[0], restate(one)[0])
    # per-parameter thresholds [P][K], and the same tensor in another layout
    rng = np.random.default_rng(3)
    t = rng.normal(size=(3, 4, 50))
    lo, hi = np.array([[-INF, 0.0]] * 3), np.array([[0.0, 1.0], [0.5, 2.0], [-0.5, INF]])
    a = indicator.indicator_ess_host(t, lo, hi, "pcn")
    b = indicator.indicator_ess_host(np.ascontiguousarray(t.transpose(1, 2, 0)), lo, hi, "cnp")
    assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)
    for p in range(3):
        for k in range(2):
            bits = ((t[p] > lo[p, k]) & (t[p] <= hi[p, k])).astype(np.int64)
            exp = restate(bits)
            assert (int(a["trunc"][p, k]), int(a["ones"][p, k])) == exp[1:] and close(float(a["ess"][p, k]), exp[0])


def test_refusals(built_lib):  # noqa: F811
    from mcmc_ref_hip import _abi, _iabi
    lib = _iabi.load_iess_library()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))        # noqa: E731
    x, lo, hi, out = np.zeros(8), np.zeros(40), np.ones(40), np.zeros(40)

    def refused(*args, cause):
        assert lib.mci_indicator_ess_host(*args) == _abi.MCR_EINVAL
        assert cause in lib.mci_last_error(None).decode(), lib.mci_last_error(None)

    refused(None, 2, 4, dp(lo), dp(hi), 1, dp(out), None, None, cause="NULL")
    refused(dp(x), 2, 4, None, dp(hi), 1, dp(out), None, None, cause="NULL")
    refused(dp(x), 0, 4, dp(lo), dp(hi), 1, dp(out), None, None, cause=">= 1")
    refused(dp(x), 2, 0, dp(lo), dp(hi), 1, dp(out), None, None, cause=">= 1")
    refused(dp(x), 1, _iabi.MCI_MAX_DRAWS + 1, dp(lo), dp(hi), 1, dp(out), None, None, cause="MCI_MAX_DRAWS")
    refused(dp(x), 2 ** 31 // 1024, 1024, dp(lo), dp(hi), 1, dp(out), None, None, cause="2^31")
    refused(dp(x), 2, 4, dp(lo), dp(hi), 0, dp(out), None, None, cause="MCI_MAX_REQUESTS")
    refused(dp(x), 2, 4, dp(lo), dp(hi), _iabi.MCI_MAX_REQUESTS + 1, dp(out), None, None, cause="MCI_MAX_REQUESTS")
    bad = lo.copy()
    bad[2] = math.nan
    refused(dp(x), 2, 4, dp(bad), dp(hi), 3, dp(out), None, None, cause="NaN")
    refused(dp(x), 2, 4, dp(lo), dp(bad), 3, dp(out), None, None, cause="NaN")
    assert lib.mci_indicator_ess_host(dp(x), 2, 4, dp(lo), dp(hi), _iabi.MCI_MAX_REQUESTS, None, None, None) == _abi.MCR_OK
    # the entries that take a handle refuse a NULL one without touching a device
    assert lib.mci_set_workspace_limit(None, 1) == _abi.MCR_EINVAL and lib.mci_kernel_ms(None, dp(out), 2) == _abi.MCR_EINVAL
    assert lib.mci_indicator_ess_dev(None, dp(x), 0, 2, 4, 1, 4, 1, 8, dp(lo), dp(hi), 1, None, None, None) == _abi.MCR_EINVAL
    assert lib.mci_version() == _iabi.MCI_VERSION


# ---- the mirror of the header, and the two libraries' exports --------------------------------------------------------------------

IDEFINE = re.compile(r"^[ \t]*#define[ \t]+(MCI_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", re.M)
IDECLARATION = re.compile(DECLARATION.pattern.replace("mcr_", "mci_"), re.M)


@pytest.fixture(scope="module")
def iheader() -> str:
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mcmcref_iess.h").read_text(), flags=re.S)


def exported(path) -> set:
    nm = shutil.which("nm")
    if nm is None:
        pytest.skip("nm is not on the path")
    out = subprocess.run([nm, "-D", "--defined-only", str(path)], check=True, capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.split()}


def test_mirror_constants(iheader):
    from mcmc_ref_hip import _iabi
    defines = {k: int(v) for k, v in IDEFINE.findall(iheader)}
    mirrored = {k: v for k, v in vars(_iabi).items() if k.startswith("MCI_") and isinstance(v, int)}
    assert mirrored == defines and len(defines) == 8
    assert defines["MCI_LAG_BLOCK"] == LB and defines["MCI_MAX_REQUESTS"] == 32 and defines["MCI_MAX_DRAWS"] == 1 << 20
    assert defines["MCI_KERNELS"] == len(_iabi.KERNEL_NAMES) and defines["MCI_LAG_BLOCK"] & (defines["MCI_LAG_BLOCK"] - 1) == 0
    assert "typedef" not in iheader and "struct" not in iheader
    text = (ROOT / "include" / "mcmcref_iess.h").read_text()
    assert "NOT Geyer" in text and "30/11" in text                 # the rule is named, the definition worked through


def test_mirror_functions_and_exports(iheader, built_lib):  # noqa: F811
    from mcmc_ref_hip import _iabi
    named = set(re.findall(r"\b(mci_[a-z0-9_]+)\s*\(", iheader))
    parsed = {m.group(2): (m.group(1), m.group(3)) for m in IDECLARATION.finditer(iheader)}
    assert named == set(parsed) == set(_iabi.ISYMBOLS) and len(named) == 11
    lib = _iabi.load_iess_library()
    for name, (ret, params) in sorted(parsed.items()):
        restype, argtypes = _iabi.ISYMBOLS[name]
        params = [p for p in params.split(",") if p.strip() != "void"]
        assert [py_class(t) for t in argtypes] == [c_class(p) for p in params], name
        assert py_class(restype) == c_class(ret), name
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype is restype, name
    second = built_lib.with_name("libmcmcref_iess.so")
    assert second.exists()
    assert exported(second) == named                               # mci_* and nothing else


def test_main_library_is_untouched(built_lib):  # noqa: F811
    """libmcmcref_hip.so exports what its two headers declared before the companion library existed, and nothing of it."""
    from mcmc_ref_hip import _abi, _xabi
    defined = exported(built_lib)
    assert defined == set(_abi.SYMBOLS) | set(_xabi.XSYMBOLS)
    assert len(_abi.SYMBOLS) == 143 and len(_xabi.XSYMBOLS) == 10
    for header in ("mcmcref_hip.h", "mcmcref_hip_ext.h"):
        assert "mci_" not in (ROOT / "include" / header).read_text().lower()


def test_ffi_knows_nothing_of_the_companion():
    from mcmc_ref_hip import _ffi, _iabi, indicator
    assert not [k for k, v in vars(_ffi).items() if v is _iabi or v is indicator]
    assert not [k for k in vars(_ffi) if k.lower().startswith(("mci", "indicator", "ess_quantile", "ess_local"))]
    assert not set(_ffi.SYMBOLS) & set(_iabi.ISYMBOLS)

"""The references of the dense linear algebra and the joint Gaussian check (include/mcmcref_hip_ext.h), and everything about
them that needs no GPU: the `*_host` routines, the `info` convention, and the Python mirror of the extension header.
tests/test_gaussian_gpu.py imports the references, the bounds and the cases from here, so what is pinned here with numpy,
scipy and long double is what the device is held to there.

The bounds are derived, not fitted.  With u = 2^-53 and gamma_k = k u / (1 - k u), for ANY order of summation
(Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Theorems 10.3 and 8.5):

    |A - L L^T| <= gamma_{P+1} |L| |L|^T        |L X - B| <= gamma_P |L| |X|        entry by entry.

The residuals are evaluated in numpy.longdouble (u = 2^-64 here: its own rounding is 2^-11 of the bound).  The tests first
hold numpy's and scipy's own factors and solves to the bounds, then the library's.

* logdet against 2 fsum(log diag L) of the RETURNED factor, within 1e-13 (sum |2 log l_ii| + 1): the level the project
  accepts between two logarithms (mcr_pareto_fit_host).
* The eight statistics against `gaussian_reference` (unblocked Cholesky and forward solves in long double), within
  1e-9 max(|want|, P_live) -- 1e-9 is the project's gate for floating-point outputs, P_live the size of the cancelling terms
  of the KL -- on inputs whose two scaled covariance matrices have a condition number of at most 2e3 (asserted).
* info against scipy.linalg.lapack.dpotrf(lower=1) on matrices whose failure is exact (a NaN pivot against the
  definition: see defect_matrix).
"""
from __future__ import annotations

import ctypes as C
import functools
import math
import re
import shutil
import subprocess

import numpy as np
import pytest

from test_abi_mirror_cpu import DECLARATION, ROOT, c_class, py_class
from test_host_cpu import built_lib  # noqa: F401  (the fixture: an up-to-date build)

LD = np.longdouble
U = 2.0 ** -53
NB = 64                                                      # MCRX_CHOL_NB (checked against the header below)
KEYS = ("d2_ref", "d2_act", "trace_ref", "trace_act", "logdet_ref", "logdet_act", "kl_act_ref", "kl_ref_act")
CHOL_SIZES = (1, 2, 17, 64, 65, 129, 257)
CONDS = (1e3, 1e12)
GAUSS_CASES = ((2, 33, 47), (17, 400, 300), (65, 1000, 700), (129, 2000, 1500))       # (P, Mr, Ma)


def gamma(k: int) -> float:
    return k * U / (1.0 - k * U)


# ---- inputs ---------------------------------------------------------------------------------------------------------------

def _basis(P: int, rng) -> np.ndarray:
    return np.linalg.qr(rng.standard_normal((P, P)))[0]


def spd(P: int, cond: float, seed: int) -> np.ndarray:
    """A symmetric positive definite matrix with a unit diagonal: a random eigenbasis, eigenvalues spaced evenly in the
    logarithm from 1 down to 1 / cond, then scaled from both sides to a unit diagonal (which moves the condition number
    by a modest factor)."""
    rng = np.random.default_rng(seed)
    lam = np.logspace(0.0, -math.log10(cond), P) if P > 1 else np.ones(1)
    Q = _basis(P, rng)
    A = (Q * lam) @ Q.T
    d = 1.0 / np.sqrt(np.diag(A))
    A = A * d[:, None] * d[None, :]
    A = (A + A.T) / 2
    np.fill_diagonal(A, 1.0)
    return A


def pair(P: int, Mr: int, Ma: int, cond: float = 50.0, seed: int = 0, shift: float = 0.3, twist: float = 1.5):
    """Two samples sharing an eigenbasis: ref [P][Mr] with the spectrum of `spd`'s recipe, act [P][Ma] with every
    eigenvalue multiplied by a factor in [1 / twist, twist] and the mean moved by `shift` standard deviations along a
    random direction."""
    rng = np.random.default_rng(1000 + seed)
    lam = np.logspace(0.0, -math.log10(cond), P) if P > 1 else np.ones(1)
    Q = _basis(P, rng)
    f = twist ** rng.uniform(-1.0, 1.0, P)
    ref = (Q * np.sqrt(lam)) @ rng.standard_normal((P, Mr)) + rng.standard_normal((P, 1))
    act = (Q * np.sqrt(lam * f)) @ rng.standard_normal((P, Ma)) + (ref.mean(axis=1, keepdims=True) +
                                                                  shift * (Q * np.sqrt(lam)) @ rng.standard_normal((P, 1)) / math.sqrt(P))
    return np.ascontiguousarray(ref), np.ascontiguousarray(act)


# ---- references in long double --------------------------------------------------------------------------------------------

def chol_ld(A) -> np.ndarray:
    """The unblocked Cholesky factor in long double (column by column)."""
    A = np.asarray(A, dtype=LD)
    P = A.shape[0]
    L = np.zeros((P, P), dtype=LD)
    for j in range(P):
        L[j, j] = np.sqrt(A[j, j] - L[j, :j] @ L[j, :j])
        if j + 1 < P:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def solve_ld(L, B) -> np.ndarray:
    L, B = np.asarray(L, dtype=LD), np.asarray(B, dtype=LD)
    X = np.zeros_like(B)
    for i in range(L.shape[0]):
        X[i] = (B[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


def gaussian_reference(ref, act, scale=None, jitter: float = 0.0) -> dict:
    """The definition of mcrx_gaussian_check in long double; also "C_ref" / "C_act" (the scaled matrices, as double)."""
    ref, act = np.asarray(ref, dtype=LD), np.asarray(act, dtype=LD)
    s = np.ones(ref.shape[0]) if scale is None else np.asarray(scale, dtype=np.float64)
    live = s > 0
    s, ref, act = s[live].astype(LD), ref[live], act[live]
    PL = int(live.sum())
    mr, ma = ref.mean(axis=1), act.mean(axis=1)
    xr, xa = ref - mr[:, None], act - ma[:, None]
    Cr = (xr @ xr.T) / LD(ref.shape[1]) * s[:, None] * s[None, :] + LD(jitter) * np.eye(PL, dtype=LD)
    Ca = (xa @ xa.T) / LD(act.shape[1]) * s[:, None] * s[None, :] + LD(jitter) * np.eye(PL, dtype=LD)
    d = s * (ma - mr)
    Lr, La = chol_ld(Cr), chol_ld(Ca)
    yr, ya = solve_ld(Lr, d[:, None])[:, 0], solve_ld(La, d[:, None])[:, 0]
    out = {"d2_ref": yr @ yr, "d2_act": ya @ ya, "trace_ref": (solve_ld(Lr, La) ** 2).sum(),
           "trace_act": (solve_ld(La, Lr) ** 2).sum(), "logdet_ref": 2 * np.log(np.diag(Lr)).sum(),
           "logdet_act": 2 * np.log(np.diag(La)).sum()}
    out["kl_act_ref"] = (out["trace_ref"] + out["d2_ref"] - PL + out["logdet_ref"] - out["logdet_act"]) / 2
    out["kl_ref_act"] = (out["trace_act"] + out["d2_act"] - PL + out["logdet_act"] - out["logdet_ref"]) / 2
    out = {k: float(v) for k, v in out.items()}
    out.update(p_live=PL, shift=yr.astype(np.float64), C_ref=Cr.astype(np.float64), C_act=Ca.astype(np.float64))
    return out


@functools.lru_cache(maxsize=None)
def gauss_case(P: int, Mr: int, Ma: int):
    """(ref, act, scale, want) of a case, computed once: scale = 1 / reference std, the statistics in long double.  The
    arrays are shared between the tests and read only."""
    ref, act = pair(P, Mr, Ma, seed=P)
    scale = 1.0 / ref.std(axis=1)
    want = gaussian_reference(ref, act, scale)
    for a in (ref, act, scale):
        a.setflags(write=False)
    return ref, act, scale, want


# ---- the checks the GPU file shares ---------------------------------------------------------------------------------------

def chol_residual_ratio(A, L) -> float:
    """max over the lower triangle of |A - L L^T| / (gamma_{P+1} |L| |L|^T): at most 1 for a factor within the bound."""
    P = A.shape[0]
    Ll = np.asarray(L, dtype=LD)
    res = np.abs(np.asarray(A, dtype=LD) - Ll @ Ll.T)
    bound = gamma(P + 1) * (np.abs(Ll) @ np.abs(Ll).T)
    low = np.tril_indices(P)
    return float((res[low] / bound[low]).max())


def solve_residual_ratio(L, X, B) -> float:
    """max of |L X - B| / (gamma_P |L| |X|) over the entries with a non-zero bound (a zero bound asks for a zero residual)."""
    Ll, Xl = np.tril(np.asarray(L, dtype=LD)), np.asarray(X, dtype=LD)
    res = np.abs(Ll @ Xl - np.asarray(B, dtype=LD))
    bound = gamma(L.shape[0]) * (np.abs(Ll) @ np.abs(Xl))
    assert (res[bound == 0] == 0).all()
    return float((res[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def check_factor(A, L, info, logdet, what=""):
    """A factor as the header states it: info 0, lower triangular with a positive diagonal and +0.0 above it (in bits),
    within the residual bound, and the logdet rule."""
    P = A.shape[0]
    assert info == 0, (what, info)
    assert L.shape == (P, P) and (np.diag(L) > 0).all(), what
    up = np.triu_indices(P, 1)
    assert not L[up].view(np.int64).any(), (what, "the strict upper triangle is not +0.0")
    ratio = chol_residual_ratio(A, L)
    assert ratio <= 1.0, (what, ratio)
    logs = 2.0 * np.log(np.diag(L))
    assert abs(logdet - math.fsum(logs)) <= 1e-13 * (np.abs(logs).sum() + 1.0), (what, logdet, math.fsum(logs))
    return ratio


def check_statistics(got: dict, want: dict, what=""):
    PL = want["p_live"]
    assert got["p_live"] == PL and got["info_ref"] == 0 and got["info_act"] == 0, (what, got)
    for k in KEYS:
        assert abs(got[k] - want[k]) <= 1e-9 * max(abs(want[k]), PL), (what, k, got[k], want[k])
    assert got["mahalanobis"] == math.sqrt(got["d2_ref"]) and got["kl_sym"] == got["kl_act_ref"] + got["kl_ref_act"]


def defect_matrix(P: int, kind: str, k: int) -> tuple[np.ndarray, int]:
    """The identity with an exact defect, and the info the definition gives for it (c + 1 for the first column whose pivot
    fails p > 0): -1, 0 or NaN at diagonal position k, or the block [[1, 2], [2, 1]] at (k, k + 1), whose second pivot is
    1 - 4.  scipy's dpotrf must give the same for the three defects that are numbers.  For the NaN it is not asked: the
    reference LAPACK tests `ajj <= 0 || disnan(ajj)`, but an optimised dpotrf may not look for NaN at all (OpenBLAS's
    returns 0 and a factor full of NaN), so there the definition alone is the reference."""
    A = np.eye(P)
    if kind == "block":
        A[k + 1, k] = A[k, k + 1] = 2.0
    else:
        A[k, k] = {"neg": -1.0, "zero": 0.0, "nan": np.nan}[kind]
    want = k + 2 if kind == "block" else k + 1
    if kind != "nan":
        from scipy.linalg import lapack
        assert int(lapack.dpotrf(A, lower=1)[1]) == want
    return A, want


def bits(a) -> list:
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64).tolist()


def stat_bits(r: dict) -> dict:
    return {k: bits(r[k]) for k in KEYS + ("mahalanobis", "kl_sym")} | {k: r[k] for k in ("p_live", "info_ref", "info_act")}


# ---- the references themselves --------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def g(built_lib):  # noqa: F811
    from mcmc_ref_hip import gaussian
    return gaussian


@pytest.mark.parametrize("cond", CONDS)
def test_numpy_and_scipy_meet_the_bounds(cond):
    from scipy.linalg import solve_triangular
    for P in CHOL_SIZES:
        A = spd(P, cond, seed=P)
        L = np.linalg.cholesky(A)
        assert chol_residual_ratio(A, L) <= 1.0, P
        B = np.random.default_rng(P).standard_normal((P, 3))
        assert solve_residual_ratio(L, solve_triangular(L, B, lower=True), B) <= 1.0, P


def test_the_cases_are_well_conditioned_and_double_is_enough():
    """cond(C_ref), cond(C_act) <= 2e3, and the same definition in plain double agrees with long double five orders inside
    the gate: the reference is not what limits the tests."""
    for P, Mr, Ma in GAUSS_CASES + ((1, 50, 40),):
        ref, act, scale, want = gauss_case(P, Mr, Ma)
        assert np.linalg.cond(want["C_ref"]) <= 2e3 and np.linalg.cond(want["C_act"]) <= 2e3, (P, Mr, Ma)
        Cr, Ca = want["C_ref"], want["C_act"]
        Lr, La = np.linalg.cholesky(Cr), np.linalg.cholesky(Ca)
        from scipy.linalg import solve_triangular
        tr = (solve_triangular(Lr, La, lower=True) ** 2).sum()
        assert abs(tr - want["trace_ref"]) <= 1e-12 * want["trace_ref"]


# ---- the host routines ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cond", CONDS)
def test_cholesky_host(g, cond):
    for P in CHOL_SIZES:
        A = spd(P, cond, seed=P)
        L, info, logdet = g.cholesky_host(A)
        check_factor(A, L, info, logdet, (P, cond))
        # the upper triangle is not read; a padded row stride changes nothing
        poisoned = A.copy()
        poisoned[np.triu_indices(P, 1)] = np.nan
        padded = np.full((P, P + 3), np.nan)
        padded[:, :P] = poisoned
        for other in (poisoned, padded[:, :P]):
            L2, info2, logdet2 = g.cholesky_host(other)
            assert info2 == 0 and bits(L2) == bits(L) and bits(logdet2) == bits(logdet), P


def test_cholesky_host_leading_minors(g):
    A = spd(3 * NB + 1, 1e3, seed=7)
    L = g.cholesky_host(A)[0]
    for n in (1, 2, 17, NB - 1, NB, NB + 1, 2 * NB + 1):
        assert bits(g.cholesky_host(A[:n, :n])[0]) == bits(L[:n, :n]), n


@pytest.mark.parametrize("kind", ["neg", "zero", "nan", "block"])
def test_cholesky_host_info(g, kind):
    P = 2 * NB + 5
    for k in (0, 1, NB - 1, NB, NB + 1, 2 * NB, P - 1):
        if kind == "block" and k == P - 1:
            continue
        A, want = defect_matrix(P, kind, k)
        L, info, logdet = g.cholesky_host(A)
        c = want - 1
        assert info == want and math.isnan(logdet), (kind, k, info)
        assert bits(L[:c, :c]) == bits(g.cholesky_host(A[:c, :c])[0]), (kind, k)
    A = spd(40, 1e3, seed=3)
    A[20, 7] = np.nan                                        # a NaN at (i, j) of the lower triangle: found by row i at the latest
    assert 1 <= g.cholesky_host(A)[1] <= 21


@pytest.mark.parametrize("cond", CONDS)
def test_solve_lower_host(g, cond):
    rng = np.random.default_rng(5)
    for P in CHOL_SIZES:
        L = np.linalg.cholesky(spd(P, cond, seed=P))
        for K in (1, 2, 65):
            B = rng.standard_normal((P, K))
            X = g.solve_lower_host(L, B)
            assert solve_residual_ratio(L, X, B) <= 1.0, (P, K)
            assert bits(g.solve_lower_host(L, B[:, K - 1])) == bits(X[:, K - 1])          # a column alone
            padded = np.full((P, K + 5), np.nan)
            padded[:, :K] = B
            noisy = L + np.triu(np.full((P, P), np.nan), 1)
            assert bits(g.solve_lower_host(noisy, padded[:, :K])) == bits(X)


def test_gaussian_check_host_against_long_double(g):
    for P, Mr, Ma in GAUSS_CASES + ((1, 50, 40),):
        ref, act, scale, want = gauss_case(P, Mr, Ma)
        got = g.gaussian_check_host(ref, act, scale=scale, shift=True)
        check_statistics(got, want, (P, Mr, Ma))
        assert np.abs(got["shift"] - want["shift"]).max() <= 1e-9 * max(1.0, np.abs(want["shift"]).max())


def test_gaussian_check_host_symmetries(g):
    ref, act, scale, _ = gauss_case(17, 400, 300)
    P = ref.shape[0]
    same = g.gaussian_check_host(ref, ref)
    assert same["d2_ref"] == 0.0 and same["d2_act"] == 0.0 and abs(same["kl_act_ref"]) <= 1e-9 * P and abs(same["kl_ref_act"]) <= 1e-9 * P
    one, two = g.gaussian_check_host(ref, act), g.gaussian_check_host(act, ref)
    for a, b in (("d2_ref", "d2_act"), ("trace_ref", "trace_act"), ("logdet_ref", "logdet_act"), ("kl_act_ref", "kl_ref_act")):
        assert bits(one[a]) == bits(two[b]) and bits(one[b]) == bits(two[a]), (a, b)
    r4, a4, s4 = ref.copy(), act.copy(), scale.copy()
    r4[3] *= 4.0
    a4[3] *= 4.0
    s4[3] *= 0.25
    assert stat_bits(g.gaussian_check_host(r4, a4, scale=s4)) == stat_bits(g.gaussian_check_host(ref, act, scale=scale))


def test_gaussian_check_host_findings_and_errors(g):
    from mcmc_ref_hip import _ffi
    ref, act, scale, _ = gauss_case(17, 400, 300)
    flat = ref.copy()
    flat[5] = 1.0                                            # a constant parameter: its pivot is exactly zero
    s = np.ones(17)
    s[2] = 0.0                                               # ... at live index 4
    r = g.gaussian_check_host(flat, act, scale=s, shift=True)
    assert (r["p_live"], r["info_ref"], r["info_act"]) == (16, 5, 0)
    assert all(math.isnan(r[k]) for k in ("d2_ref", "trace_ref", "trace_act", "logdet_ref", "kl_act_ref", "kl_ref_act", "mahalanobis"))
    assert math.isfinite(r["d2_act"]) and math.isfinite(r["logdet_act"]) and np.isnan(r["shift"]).all()
    r = g.gaussian_check_host(flat, act, scale=s, jitter=1e-8)
    assert r["info_ref"] == 0 and all(math.isfinite(r[k]) for k in KEYS)
    flat[5] = 3.7                                            # any constant: the mean is taken around the first draw
    assert g.gaussian_check_host(act, flat)["info_act"] == 6
    r = g.gaussian_check_host(ref, act, scale=np.zeros(17))
    assert (r["p_live"], r["info_ref"], r["info_act"]) == (0, 0, 0) and all(math.isnan(r[k]) for k in KEYS)
    lib, dp = _ffi.load_library(), lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    out, info = np.zeros(8), np.zeros(3, dtype=np.int64)
    ip = info.ctypes.data_as(C.POINTER(C.c_int64))
    bad = np.ones(17)
    for sc, jit, Mr in ((-bad, 0.0, 400), (bad * np.inf, 0.0, 400), (bad, -1.0, 400), (bad, math.nan, 400), (bad, 0.0, 0)):
        assert lib.mcrx_gaussian_check_host(dp(ref), Mr, dp(act), 300, 17, dp(sc), jit, dp(out), ip, None) == _ffi.MCR_EINVAL
    assert lib.mcrx_gaussian_check_host(None, 400, dp(act), 300, 17, None, 0.0, dp(out), ip, None) == _ffi.MCR_EINVAL
    assert lib.mcrx_cholesky_host(dp(ref), 5, 4, dp(out), None, None) == _ffi.MCR_EINVAL          # lda < P
    assert lib.mcrx_cholesky_host(None, 0, 0, None, None, None) == _ffi.MCR_OK
    assert lib.mcrx_solve_lower_host(dp(ref), 5, 5, dp(act), 3, 2, dp(out)) == _ffi.MCR_EINVAL     # ldb < K
    assert lib.mcrx_solve_lower_host(None, 0, 0, None, 0, 0, None) == _ffi.MCR_OK


# ---- the mirror of the extension header -----------------------------------------------------------------------------------

XDEFINE = re.compile(r"^[ \t]*#define[ \t]+(MCRX_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", re.M)
XDECLARATION = re.compile(DECLARATION.pattern.replace("mcr_", "mcrx_"), re.M)


@pytest.fixture(scope="module")
def xheader() -> str:
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mcmcref_hip_ext.h").read_text(), flags=re.S)


def test_extension_constants(xheader):
    from mcmc_ref_hip import _xabi
    defines = {k: int(v) for k, v in XDEFINE.findall(xheader)}
    mirrored = {k: v for k, v in vars(_xabi).items() if k.startswith("MCRX_") and isinstance(v, int)}
    assert mirrored == defines and len(defines) >= 15
    assert defines["MCRX_CHOL_NB"] == NB and defines["MCRX_G_OUT"] == len(KEYS) == len(_xabi.GAUSSIAN_KEYS)
    assert tuple(_xabi.GAUSSIAN_KEYS) == KEYS
    assert [defines[f"MCRX_G_{k.upper()}"] for k in KEYS] == list(range(8))
    assert [defines[f"MCRX_G_{k.upper()}"] for k in _xabi.GAUSSIAN_INFO_KEYS] == list(range(defines["MCRX_G_INFO"]))
    assert "typedef" not in xheader and "struct" not in xheader           # plain pointers and sizes


def test_extension_functions(xheader, built_lib):  # noqa: F811
    from mcmc_ref_hip import _abi, _xabi
    named = set(re.findall(r"\b(mcrx_[a-z0-9_]+)\s*\(", xheader))
    parsed = {m.group(2): (m.group(1), m.group(3)) for m in XDECLARATION.finditer(xheader)}
    assert named == set(parsed) == set(_xabi.XSYMBOLS) and len(named) == 10
    lib = _xabi.bind(_abi.load_library())
    for name, (ret, params) in sorted(parsed.items()):
        restype, argtypes = _xabi.XSYMBOLS[name]
        assert [py_class(t) for t in argtypes] == [c_class(p) for p in params.split(",")], name
        assert py_class(restype) == c_class(ret), name
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype is restype, name
    nm = shutil.which("nm")
    if nm is not None:
        out = subprocess.run([nm, "-D", "--defined-only", str(built_lib)], check=True, capture_output=True, text=True).stdout
        defined = {line.split()[-1] for line in out.splitlines() if line.split()}
        assert {s for s in defined if s.startswith("mcrx_")} == named
        assert not {s for s in defined if not s.startswith(("mcr_", "mcrx_"))}


def test_ffi_knows_nothing_of_the_extension():
    import sys
    from mcmc_ref_hip import _ffi, _xabi, gaussian
    new = {id(v) for mod in (_xabi, gaussian) for k, v in vars(mod).items()
           if getattr(v, "__module__", None) in (_xabi.__name__, gaussian.__name__)}
    assert not [k for k, v in vars(_ffi).items() if id(v) in new or v is _xabi or v is gaussian]
    assert not [k for k in vars(_ffi) if k.startswith(("mcrx", "MCRX", "gaussian", "cholesky", "solve_lower"))]
    assert not set(_ffi.SYMBOLS) & set(_xabi.XSYMBOLS)
    assert sys.modules["mcmc_ref_hip._ffi"] is _ffi


def test_validate_result_defaults():
    """ValidateResult keeps its fields (other tests pin the list) and answers None for the two a GaussianValidateResult adds."""
    import dataclasses
    from mcmc_ref_hip.validate import GaussianValidateResult, ValidateResult
    base = dict(passed=True, compare=None, ks={}, wasserstein={}, wasserstein_scaled={})
    plain = ValidateResult(**base)
    assert plain.gaussian is None and plain.gaussian_shift is None
    names = [f.name for f in dataclasses.fields(ValidateResult)]
    assert "gaussian" not in names and "gaussian_shift" not in names
    more = [f.name for f in dataclasses.fields(GaussianValidateResult)]
    assert more == names + ["gaussian", "gaussian_shift"] and issubclass(GaussianValidateResult, ValidateResult)
    full = GaussianValidateResult(**base, gaussian={"kl_sym": 0.0}, gaussian_shift=0.5)
    assert full.gaussian_shift == 0.5 and GaussianValidateResult(**base).gaussian is None
    assert all(getattr(full, n) == getattr(plain, n) for n in names)
    with pytest.raises(dataclasses.FrozenInstanceError):
        full.gaussian = None

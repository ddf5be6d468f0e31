"""Pareto k-hat: the reference in numpy, pinned on the CPU, and the inputs of tests/test_pareto_gpu.py.

`pareto_reference(x, ndraws_tail, dtype)` is the specification of mcr_pareto_khat (include/mcmcref_hip.h) for one parameter,
in float64 or longdouble: posterior::pareto_khat(tail = "both") with Zhang and Stephens' profile fit, and this project's
edge rules.  The exceedances are float64 subtractions in either case (the definition says so); `dtype` is the arithmetic
of the fit.  The tests hold the reference against itself in the two precisions, against every edge rule, and hold the
library's two host routines (mcr_pareto_tail_length, mcr_pareto_fit_host: no device) against it.
"""
from __future__ import annotations

import math

import numpy as np
import pytest

GATE = 1e-9          # |got - ref| <= GATE * max(1, |ref|): the project's float gate on the scale 1 (khat is read against 0.5 and 0.7)

# ---------------------------------------------------------------------------------------------------------------------
# The reference
# ---------------------------------------------------------------------------------------------------------------------


def tail_length_rule(M: int, r_eff: float = 1.0) -> int:
    """The default t_req: the smallest t with t^2 r_eff >= 9 M for M > 225, else M // 5.  Integers for r_eff = 1 and 0.5
    (the product with 0.5 is exact); otherwise the one rounding of float(t^2) * r_eff, searched from a float guess."""
    if M < 1:
        return 0
    if M <= 225:
        return M // 5
    if r_eff == 1.0:
        return math.isqrt(9 * M - 1) + 1
    if r_eff == 0.5:
        return math.isqrt(18 * M - 1) + 1
    ok = lambda t: float(t * t) * r_eff >= float(9 * M)
    t = max(int(3.0 * math.sqrt(M / r_eff)), 1)
    while ok(t - 1):
        t -= 1
    while not ok(t):
        t += 1
    return t


def effective_tail(M: int, ndraws_tail: int | None = None) -> int:
    t_req = tail_length_rule(M) if ndraws_tail is None else int(ndraws_tail)
    return min(max(t_req, 5), M // 2)


def fit_tail(e, dtype=np.float64) -> float:
    """khat of one tail of ascending float64 exceedances e (steps 1 to 6 of the definition), arithmetic in `dtype`."""
    e = np.asarray(e, dtype=np.float64).astype(dtype)
    n = e.size
    if e[-1] == e[0]:
        return float("nan")
    G = 30 + math.isqrt(n)
    xstar = e[(n + 2) // 4 - 1]                                # floor(n / 4 + 0.5) - 1
    if xstar == 0:
        return float("inf")
    dn = dtype(n)
    with np.errstate(all="ignore"):
        j = np.arange(1, G + 1).astype(dtype)
        theta = dtype(1) / e[-1] + (dtype(1) - np.sqrt(dtype(G) / (j - dtype(0.5)))) / dtype(3) / xstar
        k = np.empty(G, dtype=dtype)
        rows = max(1, (1 << 22) // n)                          # a block of grid points at a time
        for j0 in range(0, G, rows):
            k[j0:j0 + rows] = np.log1p(-theta[j0:j0 + rows, None] * e[None, :]).sum(axis=1) / dn
        l = dn * (np.log(-theta / k) - k - dtype(1))
        m = l.max()
        L = m + np.log(np.exp(l - m).sum())
        th = (theta * np.exp(l - L)).sum()
        kk = np.log1p(-th * e).sum() / dn
        khat = float((kk * dn + dtype(5)) / (dn + dtype(10)))
    return float("inf") if khat != khat else khat


def pymax(a: float, b: float) -> float:
    return b if b > a else a


def pareto_reference(x, ndraws_tail: int | None = None, dtype=np.float64) -> dict:
    """Every output of mcr_pareto_khat for one parameter's pooled draws x (any order, any shape)."""
    s = np.sort(np.asarray(x, dtype=np.float64).reshape(-1))
    M = s.size
    t = effective_tail(M, ndraws_tail)
    nan = float("nan")
    if t < 5:
        return {"khat": nan, "khat_left": nan, "khat_right": nan, "ndraws_tail": t}
    left = fit_tail(s[t] - s[:t][::-1], dtype)                 # e_i = x_(t) - x_(t-1-i)
    right = fit_tail(s[M - t:] - s[M - t - 1], dtype)          # e_i = x_(M-t+i) - x_(M-t-1)
    return {"khat": pymax(left, right), "khat_left": left, "khat_right": right, "ndraws_tail": t}


def same(got: float, ref: float) -> bool:
    """NaN and +-inf exactly, everything else within the gate."""
    if ref != ref or got != got:
        return ref != ref and got != got
    if math.isinf(ref) or math.isinf(got):
        return got == ref
    return abs(got - ref) <= GATE * max(1.0, abs(ref))


def err_of(got: float, ref: float) -> float:
    return abs(got - ref) / max(1.0, abs(ref)) if math.isfinite(ref) and math.isfinite(got) else 0.0


# ---------------------------------------------------------------------------------------------------------------------
# Inputs
# ---------------------------------------------------------------------------------------------------------------------

DISTS = ("normal", "t2", "cauchy", "exponential", "rounded")


def draws(dist: str, M: int, seed: int = 1) -> np.ndarray:
    """M float64 draws.  exponential is one-sided (the left tail crowds at the bound); rounded is a normal rounded to one
    decimal (ties everywhere: constant tails and xstar == 0 at small sizes)."""
    rng = np.random.default_rng([seed, DISTS.index(dist), M])
    if dist == "normal":
        return rng.normal(size=M)
    if dist == "t2":
        return rng.standard_t(2, size=M)
    if dist == "cauchy":
        return rng.standard_cauchy(size=M)
    if dist == "exponential":
        return rng.exponential(size=M)
    return np.round(rng.normal(size=M), 1)


def ties_at_cutoff(M: int, seed: int = 3) -> np.ndarray:
    """M draws rounded to one decimal whose right tail starts with a run of ties that covers the cutoff and the tail's first
    quarter (xstar == 0: khat_right = +inf) and then rises; the left tail is ordinary."""
    t = effective_tail(M)
    run = 1 + (t + 2) // 4 + 2                                 # the cutoff, the first quarter, two more
    body = np.round(np.linspace(-3.0, 1.0, M - t - 1), 1)
    rest = np.round(2.1 + 0.1 * np.arange(t - run + 1), 1)
    x = np.concatenate([body, np.full(run, 2.0), rest])
    assert x.size == M
    return np.random.default_rng(seed).permutation(x)


def constant_right_tail(M: int, seed: int = 4) -> np.ndarray:
    """M draws whose largest t + 1 values are one value (khat_right = NaN); the left tail is ordinary."""
    t = effective_tail(M)
    x = np.concatenate([np.random.default_rng(seed).normal(size=M - t - 1) - 10.0, np.full(t + 1, 1.5)])
    return np.random.default_rng(seed + 1).permutation(x)


# ---------------------------------------------------------------------------------------------------------------------
# The reference against itself
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("M", [25, 226, 1000, 4096, 65536, 1 << 20])
def test_float64_and_longdouble_agree(M):
    x = np.random.default_rng(M).standard_t(3, size=M)
    a, b = pareto_reference(x), pareto_reference(x, dtype=np.longdouble)
    assert a["ndraws_tail"] == b["ndraws_tail"]
    for key in ("khat_left", "khat_right"):
        assert abs(a[key] - b[key]) < 1e-12, (key, a[key], b[key])


def test_sanity_normal_and_cauchy():
    rng = np.random.default_rng(1)
    r = pareto_reference(rng.normal(size=40_000))
    assert r["ndraws_tail"] == 600 and r["khat_left"] < 0.3 and r["khat_right"] < 0.3, r
    r = pareto_reference(np.random.default_rng(1).standard_cauchy(size=40_000))
    assert r["khat_left"] > 0.8 and r["khat_right"] > 0.8, r


# ---------------------------------------------------------------------------------------------------------------------
# Edge rules
# ---------------------------------------------------------------------------------------------------------------------


def test_tail_lengths():
    x = np.random.default_rng(0).normal(size=226)
    r = pareto_reference(x[:9])
    assert r["ndraws_tail"] == 4 and all(r[k] != r[k] for k in ("khat", "khat_left", "khat_right"))
    assert pareto_reference(x[:10])["ndraws_tail"] == 5 and math.isfinite(pareto_reference(x[:10])["khat"])
    assert pareto_reference(x[:225])["ndraws_tail"] == 45
    assert pareto_reference(x)["ndraws_tail"] == 46
    assert pareto_reference(x, ndraws_tail=1)["ndraws_tail"] == 5                 # at least 5
    assert pareto_reference(x, ndraws_tail=113)["ndraws_tail"] == 113
    a, b = pareto_reference(x, ndraws_tail=114), pareto_reference(x, ndraws_tail=10 ** 9)    # the cap at floor(M / 2)
    assert a["ndraws_tail"] == b["ndraws_tail"] == 113 and a == pareto_reference(x, ndraws_tail=113) == b


def test_constant_tail_is_nan():
    r = pareto_reference(constant_right_tail(1000))
    assert r["khat_right"] != r["khat_right"] and math.isfinite(r["khat_left"])
    assert r["khat"] == r["khat_left"]                                              # Python's max(left, NaN) is left
    r = pareto_reference(np.full(100, 2.5))
    assert all(r[k] != r[k] for k in ("khat", "khat_left", "khat_right"))


def test_xstar_zero_is_inf():
    r = pareto_reference(ties_at_cutoff(1000))
    assert r["khat_right"] == float("inf") and math.isfinite(r["khat_left"]) and r["khat"] == float("inf")


def test_left_is_right_of_negated():
    for dist in DISTS:
        x = draws(dist, 3000)
        for dtype in (np.float64, np.longdouble):
            a, b = pareto_reference(x, dtype=dtype), pareto_reference(-x, dtype=dtype)
            for u, v in ((a["khat_left"], b["khat_right"]), (a["khat_right"], b["khat_left"])):
                assert u == v or (u != u and v != v)


# ---------------------------------------------------------------------------------------------------------------------
# The library's host routines (no GPU)
# ---------------------------------------------------------------------------------------------------------------------


def test_library_exports_and_declarations():
    from mcmc_ref_hip import _ffi
    lib = _ffi.load_library()
    for name in ("mcr_pareto_khat", "mcr_pareto_khat_dev", "mcr_pareto_plan", "mcr_pareto_tail_length", "mcr_pareto_fit_host"):
        assert name in _ffi.SYMBOLS, name
        assert getattr(lib, name) is not None
    assert _ffi.MCR_PARETO_LDS_TAIL == 8192


def test_tail_length_rule_of_the_library():
    from mcmc_ref_hip import _ffi
    fn = _ffi.load_library().mcr_pareto_tail_length
    sizes = list(range(1, 5001))
    roots = [2, 3, 15, 16, 100, 1000, 4096, 12345, 32768, 46340, 46341]
    sizes += [k * k + d for k in roots for d in (-1, 0, 1)] + [2 ** 31 - 3, 2 ** 31 - 2, 2 ** 31 - 1, 2 ** 31]
    for r_eff in (1.0, 0.5, 0.1):
        for M in sizes:
            assert fn(M, r_eff) == tail_length_rule(M, r_eff), (M, r_eff)
    # 9 M a perfect square: ceil(3 sqrt(M)) is 3 k itself, one more just above
    for k in (16, 1000, 46340):
        assert fn(k * k, 1.0) == 3 * k and fn(k * k + 1, 1.0) == 3 * k + 1
    assert fn(0, 1.0) == 0 and fn(-5, 1.0) == 0
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert fn(1000, bad) == _ffi.MCR_EINVAL
        with pytest.raises(ValueError):
            _ffi.pareto_tail_length(1000, bad)


HOST_SIZES = (9, 10, 11, 225, 226, 4096, 4097, 65535, 65536, 600_000)


@pytest.mark.parametrize("dist", DISTS)
def test_host_fit_against_longdouble(dist):
    from mcmc_ref_hip import _ffi
    worst = 0.0
    for M in HOST_SIZES:
        s = np.sort(draws(dist, M))
        kl, kr, t = _ffi.pareto_fit_host(s)
        ref = pareto_reference(s, dtype=np.longdouble)
        assert t == ref["ndraws_tail"], (M, t, ref)
        assert same(kl, ref["khat_left"]) and same(kr, ref["khat_right"]), (dist, M, kl, kr, ref)
        worst = max(worst, err_of(kl, ref["khat_left"]), err_of(kr, ref["khat_right"]))
    print(f"host fit, {dist}: worst error against longdouble {worst:.3g}")


@pytest.mark.parametrize("tail", [1, 5, 63, 64, 65, 255, 256, 257, 8192, 8193, 10_000, 10_001])
def test_host_fit_explicit_tail(tail):
    from mcmc_ref_hip import _ffi
    s = np.sort(draws("t2", 20_000))
    kl, kr, t = _ffi.pareto_fit_host(s, tail)
    ref = pareto_reference(s, tail, dtype=np.longdouble)
    assert t == ref["ndraws_tail"] == min(max(tail, 5), 10_000)
    assert same(kl, ref["khat_left"]) and same(kr, ref["khat_right"]), (kl, kr, ref)


def test_host_fit_branches():
    from mcmc_ref_hip import _ffi
    nan, inf = float("nan"), float("inf")
    for x in (constant_right_tail(1000), ties_at_cutoff(1000), np.full(100, 2.5), np.zeros(0), np.arange(9.0)):
        s = np.sort(x)
        kl, kr, t = _ffi.pareto_fit_host(s)
        ref = pareto_reference(s, dtype=np.longdouble)
        assert t == ref["ndraws_tail"] and same(kl, ref["khat_left"]) and same(kr, ref["khat_right"]), (kl, kr, t, ref)
    assert _ffi.pareto_fit_host(np.sort(ties_at_cutoff(1000)))[1] == inf
    kr = _ffi.pareto_fit_host(np.sort(constant_right_tail(1000)))[1]
    assert kr != kr and nan != nan
    with pytest.raises(ValueError):
        _ffi.pareto_fit_host(np.arange(100.0), -1)


def test_host_fit_symmetries_in_bits():
    """The left tail is the right tail of -x, and a power of two scales nothing: the same bits."""
    from mcmc_ref_hip import _ffi
    for dist in DISTS:
        s = np.sort(draws(dist, 5000))
        kl, kr, t = _ffi.pareto_fit_host(s)
        nl, nr, nt = _ffi.pareto_fit_host(np.sort(-s))
        sl, sr, _ = _ffi.pareto_fit_host(4.0 * s)
        eq = lambda a, b: a == b or (a != a and b != b)
        assert nt == t and eq(nr, kl) and eq(nl, kr) and eq(sl, kl) and eq(sr, kr), dist


def test_python_surface_value_errors():
    from mcmc_ref_hip import _ffi, diagnostics
    with pytest.raises(ValueError, match="not both"):
        diagnostics.pareto_khat([[1.0, 2.0, 3.0]] * 4, r_eff=1.0, ndraws_tail=5)
    k = np.array([-0.2, 0.0, 0.5, 0.7, 1.0, 1.5, float("nan"), float("inf")])
    min_ss, thr = _ffi.pareto_companions(k, 1000)
    assert min_ss[:4].tolist() == [10.0, 10.0, 100.0, 10.0 ** (1.0 / (1.0 - 0.7))]
    assert all(math.isinf(v) for v in min_ss[[4, 5, 7]]) and math.isnan(min_ss[6])
    assert thr == 1.0 - 1.0 / 3.0


def test_null_context_answers_einval():
    import ctypes

    from mcmc_ref_hip import _ffi
    lib = _ffi.load_library()
    x = np.zeros((1, 4, 4))
    out = _ffi.Pareto()
    for fn in (lib.mcr_pareto_khat, lib.mcr_pareto_khat_dev):
        rc = fn(None, x.ctypes.data_as(ctypes.c_void_p), *_ffi.tensor_args(x, "pcn"), None, ctypes.byref(out))
        assert rc == _ffi.MCR_EINVAL
        assert lib.mcr_last_error(None) == b"ctx is NULL"


def test_commands_take_the_options():
    from click.testing import CliRunner
    from mcmc_ref_hip.cli import main
    out = CliRunner().invoke(main, ["pareto-khat", "--help"])
    assert out.exit_code == 0 and all(opt in out.output for opt in ("--params", "--tail-draws", "--format"))
    out = CliRunner().invoke(main, ["validate", "--help"])
    assert out.exit_code == 0 and "--khat-max" in out.output
    out = CliRunner().invoke(main, ["pareto-khat", "no_such_file.csv"])
    assert out.exit_code != 0

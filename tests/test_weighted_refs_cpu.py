"""Importance-weighted summaries without a GPU: the host routine mcr_weighted_host against numpy and exact references.

* Quantiles are numpy.quantile(x, q, weights=w, method="inverted_cdf").  With integer weights every sum of weights is
  exact, so the values must be EQUAL, ties included.  With real weights a cumulative weight within rounding of a
  threshold could fall on either side; the tests first show from exact prefix sums (rationals, rounded once: what
  math.fsum gives) that no cum_j lies within 1e-9 S1 of any t, and then ask for equality as well.
* mean, sd, mean_se and ess against exact rational / long-double references within 1e-9, the project's gate for its
  extensions: relative for sd, mean_se and ess; for the mean in units of max(sd, |mean|).
* Zero-weight edges, the refusals of the Python layer and of the host routine, the command's options, the result types.
tests/test_weighted_gpu.py holds the device to this host routine bit for bit.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
from fractions import Fraction

import numpy as np
import pytest

GATE = 1e-9
QS = [0.0, 1e-9, 0.05, 0.5, 0.95, 1.0]
BLOCK_EDGES = [1, 2, 3, 1023, 1024, 1025, 2048, 2049, 5000]


@pytest.fixture(scope="module")
def ffi():
    from mcmc_ref_hip import _ffi
    return _ffi


def numpy_quantiles(x, w, qs):
    return np.quantile(np.asarray(x, dtype=np.float64), qs, weights=np.asarray(w, dtype=np.float64), method="inverted_cdf")


def tied_sample(M: int, seed: int):
    """Draws from a grid of 50 values (heavily tied) and integer weights 0 .. 7, at least one of them positive."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 50, M) / 7.0 - 3.0
    w = rng.integers(0, 8, M).astype(np.float64)
    if not w.any():
        w[0] = 1.0
    return x, w


def real_sample(M: int, seed: int, offset: float = 0.0):
    rng = np.random.default_rng(seed)
    return offset + rng.standard_normal(M), np.exp(2.0 * rng.standard_normal(M))


def exact_moments(x, w) -> dict:
    """mean, sd, mean_se, ess and S1 in exact rational arithmetic, rounded at the end."""
    fx, fw = [Fraction(float(v)) for v in x], [Fraction(float(v)) for v in w]
    s1, s2 = sum(fw), sum(v * v for v in fw)
    mean = sum(a * b for a, b in zip(fw, fx)) / s1
    q1 = sum(a * (b - mean) ** 2 for a, b in zip(fw, fx))
    q2 = sum(a * a * (b - mean) ** 2 for a, b in zip(fw, fx))
    root = lambda f: float(np.sqrt(np.longdouble(f.numerator) / np.longdouble(f.denominator)))
    return {"mean": float(mean), "sd": root(q1 / s1), "mean_se": root(q2 / (s1 * s1)), "ess": float(s1 * s1 / s2),
            "weight_sum": float(s1)}


def threshold_margin(x, w, qs) -> float:
    """The least |cum_j - q S1| / S1 over every sorted index j and probability q, from exact prefix sums of the weights
    in the draws' ascending order (ties change the order within a run, not the prefix at its end; within a run every
    prefix is a sum of the same weights in some order, so the margin is taken over both orders of each run)."""
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    margin = math.inf
    for order in (np.lexsort((np.arange(x.size), x)), np.lexsort((-np.arange(x.size), x))):
        cum, acc = [], Fraction(0)
        for v in w[order]:
            acc += Fraction(float(v))
            cum.append(acc)
        total = cum[-1]
        c = np.array([float(v / total) for v in cum])
        for q in qs:
            margin = min(margin, float(np.min(np.abs(c - q))))
    return margin


def check_floats(got: dict, x, w):
    want = exact_moments(x, w)
    scale = max(want["sd"], abs(want["mean"]))
    assert abs(got["mean"] - want["mean"]) <= GATE * scale, (got["mean"], want["mean"])
    for k in ("sd", "mean_se", "ess", "weight_sum"):
        assert abs(got[k] - want[k]) <= GATE * abs(want[k]), (k, got[k], want[k])


# ---- symbols ----------------------------------------------------------------------------------------------------------------
def test_symbols_and_version(ffi):
    lib = ffi.load_library()
    for name in ("mcr_weighted_summary", "mcr_weighted_summary_dev", "mcr_weighted_plan", "mcr_weighted_host"):
        assert name in ffi.SYMBOLS and hasattr(lib, name), name
    assert lib.mcr_version() == 100
    assert [f for f, _ in ffi.Weighted._fields_] == ["mean", "sd", "mean_se", "quantiles", "ess", "weight_sum", "weights"]
    for name in ("weighted_summary", "weighted_params_per_chunk"):
        assert callable(getattr(ffi.Context, name))


def test_constants_match_the_header(ffi):
    import re
    from pathlib import Path
    header = (Path(__file__).resolve().parents[1] / "include" / "mcmcref_hip.h").read_text()
    for name in ("MCR_WEIGHTED_BLOCK", "MCR_WEIGHTED_MAX_Q", "MCR_W_LOG"):
        assert int(re.search(rf"#define {name}\s+(\d+)", header).group(1)) == getattr(ffi, name), name
    assert ffi.MCR_WEIGHTED_BLOCK == 1024


# ---- quantiles ----------------------------------------------------------------------------------------------------------------
def test_the_example_of_the_definition(ffi):
    q = [0.0, 1e-9, 2 / 3, 0.67, 1.0]
    got = ffi.weighted_host(np.arange(1.0, 6.0), weights=[0, 2, 0, 1, 0], quantiles=q)
    assert got["quantiles"].tolist() == [2, 2, 2, 4, 4] == numpy_quantiles(np.arange(1.0, 6.0), [0, 2, 0, 1, 0], q).tolist()


@pytest.mark.parametrize("M", BLOCK_EDGES)
def test_integer_weights_and_tied_draws_equal_numpy(ffi, M):
    for seed in (1, 2, 3):
        x, w = tied_sample(M, seed)
        got = ffi.weighted_host(x, weights=w, quantiles=QS)
        assert np.array_equal(got["quantiles"], numpy_quantiles(x, w, QS)), (M, seed)
        assert got["weight_sum"] == w.sum() and got["ess"] == w.sum() ** 2 / (w * w).sum()
        check_floats(got, x, w)


@pytest.mark.parametrize("M,seed", [(1025, 11), (5000, 12), (40_000, 13)])
def test_real_weights(ffi, M, seed):
    x, w = real_sample(M, seed)
    assert threshold_margin(x, w, QS[2:5]) >= 1e-9            # (q = 0 and 1 meet cum exactly: no rounding decides them)
    got = ffi.weighted_host(x, weights=w, quantiles=QS)
    assert np.array_equal(got["quantiles"], numpy_quantiles(x, w, QS))
    check_floats(got, x, w)
    again = ffi.weighted_host(x, log_weights=np.log(w), quantiles=QS, return_weights=True)      # libm's exp: to rounding
    assert np.array_equal(again["quantiles"], got["quantiles"])
    assert again["weights"].max() == 1.0 and np.allclose(again["weights"], w / w.max(), rtol=1e-12, atol=0)
    assert again["mean"] == pytest.approx(got["mean"], abs=GATE * got["sd"]) and again["ess"] == pytest.approx(got["ess"], rel=GATE)


def test_an_offset_keeps_the_digits_of_sd(ffi):
    x, w = real_sample(20_000, 21, offset=1e8)
    got = ffi.weighted_host(x, weights=w)
    want = exact_moments(x, w)
    assert abs(got["sd"] - want["sd"]) <= GATE * want["sd"], (got["sd"], want["sd"])
    assert abs(got["mean"] - want["mean"]) <= GATE * abs(want["mean"])


# ---- zero weights -------------------------------------------------------------------------------------------------------------
def test_leading_zero_weights(ffi):
    x, w = real_sample(3000, 31)
    w[np.argsort(x)[:1500]] = 0.0                             # more than a block of zeros in front of the sorted order
    got = ffi.weighted_host(x, weights=w, quantiles=QS)
    assert np.array_equal(got["quantiles"], numpy_quantiles(x, w, QS))
    assert got["quantiles"][0] == np.sort(x)[1500]            # q = 0: the first draw with a weight
    check_floats(got, x, w)


def test_trailing_zero_weights(ffi):
    x, w = real_sample(3000, 32)
    w[np.argsort(x)[-1500:]] = 0.0
    got = ffi.weighted_host(x, weights=w, quantiles=QS)
    assert np.array_equal(got["quantiles"], numpy_quantiles(x, w, QS))
    assert got["quantiles"][-1] == np.sort(x)[1499]           # q = 1: the last draw with a weight
    check_floats(got, x, w)


@pytest.mark.parametrize("M,at", [(1, 0), (1500, 0), (1500, 1024), (1500, 1499)])
def test_a_single_positive_weight(ffi, M, at):
    x, _ = real_sample(M, 33)
    w = np.zeros(M)
    w[at] = 0.37
    got = ffi.weighted_host(x, weights=w, quantiles=QS)
    assert got["quantiles"].tolist() == [x[at]] * len(QS)
    assert got["mean"] == pytest.approx(x[at], rel=1e-15) and got["sd"] == pytest.approx(0.0, abs=1e-15 * max(1.0, abs(x[at])))
    assert got["ess"] == pytest.approx(1.0, rel=GATE)


@pytest.mark.parametrize("M", [7, 1024, 4097])
def test_equal_weights(ffi, M):
    x, _ = real_sample(M, 34)
    got = ffi.weighted_host(x, weights=np.full(M, 0.25), quantiles=QS)
    assert np.array_equal(got["quantiles"], np.quantile(x, QS, method="inverted_cdf"))
    assert got["ess"] == pytest.approx(M, rel=GATE)
    assert got["mean"] == pytest.approx(x.mean(), abs=GATE * x.std()) and got["sd"] == pytest.approx(x.std(), rel=GATE)


def test_minus_infinity_is_a_zero_weight(ffi):
    x, w = real_sample(2000, 35)
    lw = np.log(w)
    lw[::3] = -np.inf
    w[::3] = 0.0
    got = ffi.weighted_host(x, log_weights=lw, quantiles=QS, return_weights=True)
    assert np.array_equal(got["quantiles"], numpy_quantiles(x, w, QS))
    assert (got["weights"][::3] == 0.0).all()


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_the_python_layer_refuses_before_any_call(ffi):
    from mcmc_ref_hip import convert
    x = np.arange(4.0)
    one = np.ones(4)
    for kw in ({}, {"weights": one, "log_weights": one}):     # neither, both
        with pytest.raises(ValueError, match="exactly one"):
            ffi.weight_arguments(4, kw.get("log_weights"), kw.get("weights"), (0.5,))
        with pytest.raises(ValueError, match="exactly one"):
            ffi.weighted_host(x, **kw)
    with pytest.raises(ValueError, match="3 entries for 4"):
        ffi.weighted_host(x, weights=np.ones(3))
    with pytest.raises(ValueError, match="at most 16"):
        ffi.weighted_host(x, weights=one, quantiles=[0.5] * 17)
    for q in (-0.1, 1.0000001, float("nan")):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            ffi.weighted_host(x, weights=one, quantiles=[0.5, q])
    assert ffi.weighted_host(x, weights=one, quantiles=())["quantiles"].shape == (0,)          # no quantile is allowed
    assert ffi.weighted_host(x, weights=one, quantiles=[0.5] * 16)["quantiles"].tolist() == [1.0] * 16
    with pytest.raises(ValueError, match="exactly one"):
        convert.weighted_summary_file("nowhere.csv")
    with pytest.raises(ValueError, match="psis=True"):
        convert.weighted_summary_file("nowhere.csv", weights="w")


def test_the_host_routine_refuses_bad_weights(ffi):
    lib = ffi.load_library()
    x = np.arange(1.0, 5.0)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    q = np.array([0.5])
    out = np.full(8, 7.0)                                      # mean, sd, mean_se, quantile, ess, weight_sum
    po = [dp(out[i:i + 1]) for i in range(6)]

    def call(v, flags=0, nq=1, probs=q):
        v = np.ascontiguousarray(v, dtype=np.float64)
        return lib.mcr_weighted_host(dp(x), dp(v), 4, flags, dp(probs), nq, *po, None)

    for bad in ([1, -1, 1, 1], [1, np.nan, 1, 1], [0, 0, 0, 0], [1, np.inf, 1, 1], [-np.inf, 1, 1, 1]):
        assert call(bad) == ffi.MCR_EINVAL, bad
    for bad in ([0, np.nan, 0, 0], [0, np.inf, 0, 0], [-np.inf] * 4):
        assert call(bad, ffi.MCR_W_LOG) == ffi.MCR_EINVAL, bad
    assert call([1, 1, 1, 1], flags=2) == ffi.MCR_EINVAL and call([1, 1, 1, 1], nq=17) == ffi.MCR_EINVAL
    assert call([1, 1, 1, 1], probs=np.array([1.5])) == ffi.MCR_EINVAL
    assert (out == 7.0).all()                                  # nothing was written
    assert call([-np.inf, 0, -np.inf, -5], ffi.MCR_W_LOG) == ffi.MCR_OK and out[3] == 2.0
    x[2] = np.nan
    assert call([1, 1, 1, 1]) == ffi.MCR_ENONFINITE
    f = [C.c_double(1.0) for _ in range(5)]
    assert lib.mcr_weighted_host(None, None, 0, 0, dp(q), 1, C.byref(f[0]), C.byref(f[1]), C.byref(f[2]), dp(out), C.byref(f[3]),
                                 C.byref(f[4]), None) == ffi.MCR_OK                               # M == 0: NaN
    assert all(math.isnan(c.value) for c in f) and math.isnan(out[0])
    v = C.c_int64(-1)
    assert lib.mcr_weighted_plan(None, ffi.MCR_F64, 4, 4, 1, 4, 1, 16, 3, C.byref(v)) == ffi.MCR_EINVAL


# ---- the command and the result types -------------------------------------------------------------------------------------------
def test_commands_take_the_options():
    from click.testing import CliRunner
    from mcmc_ref_hip.cli import main
    out = CliRunner().invoke(main, ["weighted-summary", "--help"])
    assert out.exit_code == 0
    assert all(opt in out.output for opt in ("--log-weights", "--weights", "--params", "--quantile", "--no-psis", "--format"))
    out = CliRunner().invoke(main, ["weighted-summary", "no_such_file.csv", "--log-weights", "lw"])
    assert out.exit_code != 0


def test_result_types():
    from mcmc_ref_hip.validate import ValidateResult, WeightedValidateResult, validate_weighted
    assert [f.name for f in dataclasses.fields(WeightedValidateResult)] == ["passed", "compare", "stats", "ess", "khat", "failures"]
    assert WeightedValidateResult.__dataclass_params__.frozen and callable(validate_weighted)
    assert [f.name for f in dataclasses.fields(ValidateResult)] == [
        "passed", "compare", "ks", "wasserstein", "wasserstein_scaled", "failures", "sliced_ks", "sliced_w1", "sliced",
        "khat_ref", "khat_actual", "hdi_ref", "hdi_actual", "energy", "energy_detail"]

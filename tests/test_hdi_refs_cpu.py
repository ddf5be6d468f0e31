"""Highest-density intervals on the host: the numpy reference of the definition in include/mcmcref_hip.h, the input
generators that tests/test_hdi_gpu.py shares, and mcr_hdi_sorted_host against the reference.

The reference is the definition itself (ArviZ's unimodal hdi): numpy.argmin(s[inc:] - s[:M - inc]) on the sorted draws,
inc = floor(prob * M).  No rounding choice is left open -- a width is one IEEE subtraction, the minimum is exact, the first
of several minima is taken -- so every comparison here is exact: `index` as an integer, `lo` and `hi` with ==.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import pytest

GENERATORS = ("normal", "exponential", "bimodal", "tied", "constant")


def hdi_reference(x, prob: float) -> tuple[float, float, int]:
    """(lo, hi, index) of one parameter's draws, straight from the definition."""
    s = np.sort(np.asarray(x, dtype=np.float64).reshape(-1))
    M = s.size
    inc = int(math.floor(prob * float(M)))                   # one rounded product
    W = M - inc
    if W < 1:
        return float("nan"), float("nan"), -1
    with np.errstate(over="ignore"):
        i = int(np.argmin(s[inc:] - s[:W]))                  # the first minimum
    return float(s[i]), float(s[i + inc]), i


def windows(M: int, prob: float) -> int:
    return M - int(math.floor(prob * float(M)))


def draws(kind: str, M: int, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(1000 * GENERATORS.index(kind) + seed)
    if kind == "normal":
        return rng.normal(size=M)
    if kind == "exponential":
        return rng.exponential(size=M)
    if kind == "bimodal":                                    # 70 % around -2 (the heavier mode), 30 % around +3
        return np.where(rng.random(M) < 0.7, rng.normal(-2.0, 0.5, size=M), rng.normal(3.0, 0.5, size=M))
    if kind == "tied":                                       # integer-valued: many equal draws, many equal widths
        return rng.integers(0, max(2, M // 8 + 2), size=M).astype(np.float64)
    if kind == "constant":
        return np.full(M, 2.5)
    raise ValueError(kind)


@pytest.fixture(scope="module")
def ffi():
    from mcmc_ref_hip import _ffi
    return _ffi


SIZES = (1, 2, 3, 10, 1000)
PROBS = (0.01, 0.5, 0.94, 0.999)


@pytest.mark.parametrize("M", SIZES)
def test_sorted_host_against_the_reference(ffi, M):
    for kind in GENERATORS:
        x = draws(kind, M, seed=M)
        s = np.sort(x)
        for prob in PROBS:
            want = hdi_reference(x, prob)
            lo, hi, idx = ffi.hdi_sorted_host(s, prob)
            assert idx == want[2], (kind, M, prob, idx, want)
            assert lo == want[0] and hi == want[1], (kind, M, prob, (lo, hi), want)
            assert lo == s[idx] and hi == s[idx + int(math.floor(prob * M))]
        los, his, idxs = ffi.hdi_sorted_host(s, list(PROBS))            # four probabilities in one call
        assert [(a, b, int(i)) for a, b, i in zip(los, his, idxs)] == [ffi.hdi_sorted_host(s, q) for q in PROBS]


def test_the_cases_hold_the_edges():
    """inc == 0 (every draw its own window, the first of M zero widths), W == 1 (one window: the whole range)."""
    cases = [(M, q, int(math.floor(q * M)), windows(M, q)) for M in SIZES for q in PROBS]
    assert any(inc == 0 and M > 1 for M, _, inc, _ in cases)
    assert any(W == 1 and M > 1 for M, _, _, W in cases)
    assert (1, 0.5, 0, 1) in cases and (1000, 0.999, 999, 1) in cases and (10, 0.01, 0, 10) in cases


def test_edges_by_hand(ffi):
    s = np.array([0.0, 5.0, 6.0, 20.0, 21.0, 40.0])
    assert ffi.hdi_sorted_host(s, 0.2) == (5.0, 6.0, 1)                 # inc = 1: widths 5 1 14 1 19, the first of two minima
    assert ffi.hdi_sorted_host(s, 0.1) == (0.0, 0.0, 0)                 # inc = 0: six zero widths
    assert ffi.hdi_sorted_host(s, 0.9) == (0.0, 40.0, 0)                # inc = 5: one window
    assert ffi.hdi_sorted_host(s, 0.5) == (5.0, 21.0, 1)                # inc = 3: widths 20 16 34
    assert ffi.hdi_sorted_host(np.array([7.0]), 0.94) == (7.0, 7.0, 0)
    lo, hi, idx = ffi.hdi_sorted_host(np.zeros(0), 0.94)                # M == 0
    assert math.isnan(lo) and math.isnan(hi) and idx == -1
    big = np.array([-1.7e308, -1.0, 1.7e308, 1.75e308])                 # a width that overflows is an ordinary value
    assert ffi.hdi_sorted_host(big, 0.5) == hdi_reference(big, 0.5) == (-1.0, 1.75e308, 1)        # +inf loses to a finite width
    inf2 = np.array([-1.7e308, -1.6e308, 1.6e308, 1.7e308])
    assert ffi.hdi_sorted_host(inf2, 0.5) == hdi_reference(inf2, 0.5) == (-1.7e308, 1.6e308, 0)   # two +inf widths: the first


def test_the_first_of_equal_minima(ffi):
    x = draws("tied", 1000, seed=3)
    s = np.sort(x)
    for prob in (0.1, 0.5, 0.94):
        inc = int(math.floor(prob * 1000))
        w = s[inc:] - s[:1000 - inc]
        assert np.count_nonzero(w == w.min()) > 1                       # several windows are the narrowest
        lo, hi, idx = ffi.hdi_sorted_host(s, prob)
        assert idx == int(np.flatnonzero(w == w.min())[0]) and (lo, hi, idx) == hdi_reference(x, prob)
    const = draws("constant", 1000)
    for prob in PROBS:
        assert ffi.hdi_sorted_host(const, prob) == (2.5, 2.5, 0)


def test_behaviour(ffi):
    x = np.sort(draws("exponential", 1000, seed=1))
    lo, hi, _ = ffi.hdi_sorted_host(x, 0.94)
    q3, q97 = np.quantile(x, [0.03, 0.97])
    assert lo < q3 and hi < q97                                         # a right-skewed density: the interval hugs zero
    b = np.sort(draws("bimodal", 1000, seed=1))
    lo, hi, _ = ffi.hdi_sorted_host(b, 0.5)
    assert -4.0 < lo < hi < 0.0                                         # on the heavier mode around -2


def test_argument_checks(ffi):
    s = np.sort(draws("normal", 100))
    for bad in (0.0, 1.0, float("nan"), -0.5, 1.5, float("inf")):
        with pytest.raises(ValueError):
            ffi.hdi_sorted_host(s, bad)
    with pytest.raises(ValueError):
        ffi.hdi_sorted_host(s, [0.5, 0.0])                              # one bad probability among good ones
    with pytest.raises(ValueError):
        ffi.hdi_sorted_host(s, [])                                      # nprob == 0
    assert ffi.MCR_HDI_MAX_PROBS == 16
    assert len(ffi.hdi_sorted_host(s, [0.5] * 16)[0]) == 16
    with pytest.raises(ValueError):
        ffi.hdi_sorted_host(s, [0.5] * 17)
    lib = ffi.load_library()
    pr = (C.c_double * 1)(0.5)
    out = (C.c_double * 1)()
    idx = (C.c_int64 * 1)()
    args = (C.cast(pr, C.POINTER(C.c_double)), 1, C.cast(out, C.POINTER(C.c_double)), C.cast(out, C.POINTER(C.c_double)),
            C.cast(idx, C.POINTER(C.c_int64)))
    sp = s.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.mcr_hdi_sorted_host(sp, -1, *args) == ffi.MCR_EINVAL      # negative M
    assert lib.mcr_hdi_sorted_host(None, 5, *args) == ffi.MCR_EINVAL     # no array
    assert lib.mcr_hdi_sorted_host(sp, 100, *args) == ffi.MCR_OK
    assert lib.mcr_hdi_sorted_host(sp, 100, args[0], 1, None, None, None) == ffi.MCR_OK      # NULL outputs are skipped
    assert ffi.MCR_HDI_SLICE & (ffi.MCR_HDI_SLICE - 1) == 0

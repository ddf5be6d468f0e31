"""The numpy reference of the autocorrelation functions and times (mcr_autocorr), its own properties, and the library's host
routine mcr_autocorr_host against it.  No device is needed.

`acf_reference` is the definition of include/mcmcref_hip.h in plain numpy, in long double: direct sums for every lag, the
running tau left to right.  tests/test_acf_gpu.py gates the kernels against it.

The float gate is the project's standing one, |got - ref| <= 1e-9 * max(1, |ref|); NaN must match exactly.  `window` is an
integer and is compared as one: every gated input must satisfy, in the reference, |W - window_c * tau_W| > 1e-6 for every W
up to the window (up to L when none is found), so that the integer cannot hinge on rounding.  `gate` asserts that margin
before it compares.
"""
from __future__ import annotations

import numpy as np
import pytest

GATE = 1e-9
MARGIN = 1e-6


def ar1(phi: float, C: int, N: int, seed: int, offset: float = 0.0, scale: float = 1.0) -> np.ndarray:
    """C stationary AR(1) chains of N draws, x_t = phi x_{t-1} + e_t, started from the stationary law."""
    rng = np.random.default_rng(seed)
    e = rng.standard_normal((C, N))
    x = np.empty((C, N))
    if N:
        x[:, 0] = e[:, 0] / np.sqrt(1.0 - phi * phi) if abs(phi) < 1 else e[:, 0]
    for t in range(1, N):
        x[:, t] = phi * x[:, t - 1] + e[:, t]
    return offset + scale * x


def _tau(rho: np.ndarray, window_c: float):
    """(tau, window, margin) of one row rho[0 .. L]: the running sum left to right (cumsum is sequential)."""
    L = rho.size - 1
    if np.isnan(rho).any():
        return np.nan, -1, np.inf
    tau_w = 2 * np.cumsum(rho) - 1
    w = np.arange(L + 1, dtype=rho.dtype)
    ok = w >= window_c * tau_w
    window = int(np.argmax(ok)) if ok.any() else -1
    upto = window if window >= 0 else L
    margin = float(np.min(np.abs(w[:upto + 1] - window_c * tau_w[:upto + 1])))
    return float(tau_w[upto]), window, margin


def acf_reference(x, L: int, unbiased: bool = False, window_c: float = 5.0, dtype=np.longdouble) -> dict:
    """The definition on x[C][N]: float64 arrays acf [C][L+1], var, tau [C], window [C] (int64), acf_pooled [L+1], floats
    tau_pooled, the int window_pooled -- and `margin`, the least |W - window_c tau_W| any window decision looked at."""
    x = np.asarray(x, dtype=dtype)
    C, N = x.shape
    d = x - (x.sum(axis=1) / N)[:, None]
    gam = np.empty((C, L + 1), dtype=dtype)
    for l in range(L + 1):
        gam[:, l] = (d[:, :N - l] * d[:, l:]).sum(axis=1) / (N - l if unbiased else N)
    with np.errstate(all="ignore"):
        rho = np.where(gam[:, :1] == 0, np.nan, gam / gam[:, :1])
        gbar = gam.sum(axis=0) / C
        rbar = np.where(gbar[0] == 0, np.nan, gbar / gbar[0])
    rows = [_tau(rho[c], window_c) for c in range(C)]
    tp, wp, mp = _tau(rbar, window_c)
    return {"acf": rho.astype(np.float64), "var": gam[:, 0].astype(np.float64),
            "tau": np.array([r[0] for r in rows], dtype=np.float64), "window": np.array([r[1] for r in rows], dtype=np.int64),
            "acf_pooled": rbar.astype(np.float64), "tau_pooled": float(tp), "window_pooled": wp,
            "margin": min([mp] + [r[2] for r in rows])}


def worst(got, ref) -> float:
    """The largest |got - ref| / max(1, |ref|) over the entries; NaN must stand where NaN stands (inf otherwise)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not np.array_equal(np.isnan(got), np.isnan(ref)):
        return float("inf")
    live = ~np.isnan(ref)
    if not live.any():
        return 0.0
    return float(np.max(np.abs(got[live] - ref[live]) / np.maximum(1.0, np.abs(ref[live]))))


FLOAT_KEYS = ("acf", "var", "tau", "acf_pooled", "tau_pooled")


def gate(got: dict, x: np.ndarray, L: int, unbiased: bool, window_c: float, what) -> float:
    """One parameter's outputs `got` (the keys of acf_reference) on its chains x[C][N] against the reference: the margin, the
    float gate, the windows as integers.  Returns the worst float error."""
    ref = acf_reference(x, L, unbiased, window_c)
    assert ref["margin"] > MARGIN, (what, ref["margin"])
    err = max(worst(got[k], ref[k]) for k in FLOAT_KEYS)
    assert err <= GATE, (what, {k: worst(got[k], ref[k]) for k in FLOAT_KEYS})
    assert np.asarray(got["window"]).tolist() == ref["window"].tolist(), (what, got["window"], ref["window"])
    assert int(got["window_pooled"]) == ref["window_pooled"], (what, got["window_pooled"], ref["window_pooled"])
    return err


def one(res: dict, p: int = 0) -> dict:
    """Parameter p of a Context.autocorr / autocorr_host result, in the keys of acf_reference."""
    return {"acf": res["acf"][p], "var": res["var"][p], "tau": res["tau"][p], "window": res["window"][p],
            "acf_pooled": res["acf_pooled"][p], "tau_pooled": float(res["tau_pooled"][p]),
            "window_pooled": int(res["window_pooled"][p])}


# ---- the reference itself ---------------------------------------------------------------------------------------------------

def fft_acf(x: np.ndarray, L: int) -> np.ndarray:
    """arviz.autocorr: the zero-padded FFT autocovariance of one chain, normalised by lag 0."""
    n = x.size
    size = 1 << int(np.ceil(np.log2(2 * n)))
    f = np.fft.rfft(x - x.mean(), size)
    cov = np.fft.irfft(f * np.conj(f), size)[:n] / n
    return (cov / cov[0])[:L + 1]


@pytest.mark.parametrize("N", [1000, 10_000])
def test_biased_form_is_the_fft_formula(N):
    x = ar1(0.7, 2, N, seed=1)
    ref = acf_reference(x, 100)
    for c in range(2):
        assert np.max(np.abs(ref["acf"][c] - fft_acf(x[c], 100))) <= 1e-12
    assert np.all(ref["acf"][:, 0] == 1.0) and ref["acf_pooled"][0] == 1.0
    full = acf_reference(x, N - 1)
    assert np.all(np.abs(full["acf"]) <= 1.0) and np.all(np.abs(full["acf_pooled"]) <= 1.0)


def test_unbiased_form_divides_by_the_number_of_products():
    x = ar1(0.5, 3, 50, seed=2)
    b, u = acf_reference(x, 49), acf_reference(x, 49, unbiased=True)
    n = 50.0
    scale = n / (n - np.arange(50))
    assert np.allclose(u["acf"], b["acf"] * scale, rtol=1e-13, atol=0)
    d = x - x.mean(axis=1, keepdims=True)
    assert np.allclose(u["acf"][:, 49] * u["var"], d[:, 0] * d[:, 49], rtol=1e-12)     # lag N - 1: one product, divisor 1


def test_sokal_window_on_ar1():
    """phi = 0.5: the window is found and tau is near (1 + phi) / (1 - phi) = 3 (its standard error at N = 10 000 and a
    window of ~16 is about 3 sqrt(2 * 33 / 10 000) = 0.24: three of them).  phi = 0.9, tau = 19: at L = 100 the window
    needs tau_100 <= 20 -- this seeded chain does not give it: no window, and tau is tau_L."""
    a = acf_reference(ar1(0.5, 1, 10_000, seed=7), 100)
    assert 10 <= a["window"][0] <= 20 and a["window_pooled"] == a["window"][0]
    assert abs(a["tau"][0] - 3.0) < 0.75
    assert a["margin"] > MARGIN
    b = acf_reference(ar1(0.9, 1, 10_000, seed=7), 100)
    assert b["window"][0] == -1 and b["window_pooled"] == -1 and b["margin"] > MARGIN
    assert abs(b["tau"][0] - (2 * b["acf"][0].sum() - 1)) < 1e-12 and b["tau"][0] > 20.0


def test_constant_chains_are_nan():
    x = ar1(0.3, 3, 40, seed=3)
    x[1] = 2.5
    r = acf_reference(x, 10)
    assert np.isnan(r["acf"][1]).all() and np.isnan(r["tau"][1]) and r["window"][1] == -1 and r["var"][1] == 0.0
    assert np.isfinite(r["acf"][[0, 2]]).all() and np.isfinite(r["acf_pooled"]).all() and r["window_pooled"] >= 0
    r = acf_reference(np.full((2, 5), 1.0), 4)
    assert np.isnan(r["acf_pooled"]).all() and np.isnan(r["tau_pooled"]) and r["window_pooled"] == -1
    r = acf_reference(np.array([[3.0]]), 0)                                       # N == 1
    assert np.isnan(r["acf"]).all() and r["window"][0] == -1


# ---- the host routine (fails before mcr_autocorr_host exists) ---------------------------------------------------------------------

@pytest.fixture(scope="module")
def ffi():
    from mcmc_ref_hip import _ffi
    return _ffi


HOST_CASES = [  # (phi, C, N, L, unbiased, window_c, offset)
    (0.5, 2, 1000, 100, False, 5.0, 0.0),
    (0.9, 3, 777, 100, False, 5.0, 1e6),          # odd N, a large offset (the two-pass mean), no window
    (0.0, 1, 513, 512, False, 5.0, 0.0),          # L = N - 1, one draw past a block
    (0.5, 2, 1025, 600, True, 1.0, 0.0),          # the unbiased form, three blocks
    (0.99, 4, 300, 50, False, 10.0, -3.0),
    (0.3, 5, 2, 1, True, 5.0, 0.0),               # N == 2, lag N - 1 with divisor 1
    (0.3, 2, 3, 0, False, 5.0, 0.0),              # L == 0
]


@pytest.mark.parametrize("case", HOST_CASES, ids=[f"phi{c[0]}-C{c[1]}-N{c[2]}-L{c[3]}" for c in HOST_CASES])
def test_host_routine_against_the_reference(ffi, case):
    phi, C, N, L, unbiased, wc, offset = case
    x = ar1(phi, C, N, seed=11, offset=offset)
    got = ffi.autocorr_host(x, max_lag=L, unbiased=unbiased, window_c=wc)
    assert got["max_lag"] == L and got["acf"].shape == (1, C, L + 1) and got["acf_pooled"].shape == (1, L + 1)
    gate(one(got), x, L, unbiased, wc, case)
    assert np.array_equal(got["ess_chain"], N / got["tau"]) and np.array_equal(got["ess_pooled"], C * N / got["tau_pooled"])


def test_host_routine_edges(ffi):
    x = ar1(0.4, 3, 64, seed=5)
    x[1] = -7.0                                                                   # a constant chain among varying ones
    got = ffi.autocorr_host(x, max_lag=20)
    gate(one(got), x, 20, False, 5.0, "constant chain")
    assert np.isnan(got["acf"][0, 1]).all() and got["window"][0, 1] == -1 and np.isfinite(got["acf_pooled"]).all()
    got = ffi.autocorr_host(np.full((2, 9), 4.0), max_lag=8)
    assert np.isnan(got["acf_pooled"]).all() and np.isnan(got["tau_pooled"][0]) and got["window_pooled"][0] == -1
    got = ffi.autocorr_host(np.array([[1.5]]))                                    # N == 1: the default max_lag is 0
    assert got["max_lag"] == 0 and np.isnan(got["acf"]).all() and got["window"].tolist() == [[-1]]
    assert ffi.autocorr_host(ar1(0.4, 1, 500, seed=1))["max_lag"] == 100          # the default: min(100, N - 1)
    assert ffi.autocorr_host(ar1(0.4, 1, 50, seed=1))["max_lag"] == 49
    empty = ffi.autocorr_host(np.empty((2, 0)), max_lag=3)                        # no draws: NaN and -1
    assert np.isnan(empty["acf"]).all() and empty["window"].tolist() == [[-1, -1]] and empty["window_pooled"].tolist() == [-1]
    for kw in ({"max_lag": -1}, {"max_lag": 64}, {"max_lag": ffi.MCR_ACF_MAX_LAG + 1}, {"window_c": 0.0}, {"window_c": -1.0},
               {"window_c": float("nan")}, {"window_c": float("inf")}):
        with pytest.raises(ValueError):
            ffi.autocorr_host(x, **kw)
    bad = x.copy()
    bad[2, 3] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        ffi.autocorr_host(bad, max_lag=5)
    out = ffi.Acf()
    rc = ffi.load_library().mcr_autocorr_host(x.ctypes.data_as(ffi._dp), 3, 64, 5, 2, 5.0, out)      # an unknown flag bit
    assert rc == ffi.MCR_EINVAL


def test_host_routine_does_not_depend_on_the_other_chains(ffi):
    """A chain's outputs have the same bits alone and among others; the pooled ones of a single chain are its own."""
    x = ar1(0.6, 4, 1100, seed=9, offset=10.0)
    all_ = ffi.autocorr_host(x, max_lag=130)
    for c in range(4):
        alone = ffi.autocorr_host(x[c:c + 1], max_lag=130)
        for k in ("acf", "var", "tau", "window"):
            assert np.array_equal(alone[k][0, 0], all_[k][0, c], equal_nan=True), (c, k)
        assert np.array_equal(alone["acf_pooled"][0], alone["acf"][0, 0]) and alone["tau_pooled"][0] == alone["tau"][0, 0]

"""The energy distance on the host: mcr_energy_distance_host against the definition in include/mcmcref_hip.h, restated
here in numpy long double (sums) and in exact Python arithmetic (one pair), plus the inputs tests/test_energy_gpu.py shares.

Gates: A, B, C within 1e-9 relative (the project's gate for floating-point outputs), E within 1e-9 * 2A absolute (E is a
difference of the three; 2A is its scale).  Wherever the inputs make every distance an integer the comparison is in bits.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import importlib.util
import math
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

from test_sliced_cpu import separation_case

ROOT = Path(__file__).resolve().parents[1]
REL = 1e-9
PAIR_P = (1, 2, 3, 63, 64, 65, 257)
LATTICE_P = (1, 4, 9, 64, 100)
MCR_OK, MCR_EINVAL, MCR_ENONFINITE, MCR_ENOMEM = 0, -1, -4, -6


@pytest.fixture(scope="module")
def ffi():
    spec = importlib.util.spec_from_file_location("mcr_build", ROOT / "mcmc-db_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()
    from mcmc_ref_hip import _ffi
    _ffi.load_library()
    return _ffi


# ---- the definition, restated -------------------------------------------------------------------------------------------
def energy_reference(ref, act, scale=None) -> dict:
    """The six outputs with the pair sums in numpy long double.  u = x * scale is the definition's one rounding; the
    squared differences are summed over p in long double (the routine's fma chain is within P ulp of that)."""
    ref, act = np.asarray(ref, dtype=np.float64), np.asarray(act, dtype=np.float64)
    s = np.ones(ref.shape[0]) if scale is None else np.asarray(scale, dtype=np.float64)
    ur, ua = (ref * s[:, None]).astype(np.longdouble), (act * s[:, None]).astype(np.longdouble)

    def pair_sum(x, y):
        sq = np.zeros((x.shape[1], y.shape[1]), dtype=np.longdouble)
        for p in range(x.shape[0]):
            sq += (x[p][:, None] - y[p][None, :]) ** 2
        return np.sqrt(sq).sum(dtype=np.longdouble)

    mr, ma = ref.shape[1], act.shape[1]
    a = pair_sum(ur, ua) / (mr * ma)
    b = pair_sum(ur, ur) / (mr * mr)
    c = pair_sum(ua, ua) / (ma * ma)
    e = (a - b) + (a - c)
    return {"a": float(a), "b": float(b), "c": float(c), "e": float(e), "h": float(e / (2 * a)) if a else 0.0,
            "t": float(mr * ma / (mr + ma) * e)}


def assert_close(got: dict, exp: dict, what=""):
    for k in "abc":
        assert abs(got[k] - exp[k]) <= REL * abs(exp[k]), (what, k, got[k], exp[k])
    assert abs(got["e"] - exp["e"]) <= REL * 2 * exp["a"], (what, "e", got["e"], exp["e"])


def _fma(a: float, b: float, c: float) -> float:
    if hasattr(math, "fma"):
        return math.fma(a, b, c)
    return float(Fraction(a) * Fraction(b) + Fraction(c))        # exact, then the one rounding (int / int is correctly rounded)


def pair_distance(x, y, scale=None) -> float:
    """d(x, y) of the definition, step by step: every operation below rounds once."""
    acc = 0.0
    for p in range(len(x)):
        s = 1.0 if scale is None else float(scale[p])
        t = float(x[p]) * s - float(y[p]) * s                     # two rounded products, one rounded difference
        acc = _fma(t, t, acc)
    return math.sqrt(acc)


def pair_case(P: int):
    rng = np.random.default_rng(900 + P)
    return rng.normal(size=P) * 3.0 + 1e3, rng.normal(size=P) * 3.0 + 1e3, rng.uniform(0.1, 2.0, size=P)


def lattice_case(P: int, Mr: int, Ma: int, pad: int = 2, seed: int = 0):
    """(ref [P + pad][Mr], act [P + pad][Ma], exact integer S_xy, S_xx, S_yy): draws a_i (1, .., 1) with integer a_i and
    P a perfect square, padded with parameters constant across both samples.  Every distance is the integer sqrt(P) |a_i -
    a_j|, every partial sum an integer far below 2^53: exact in any order."""
    root = math.isqrt(P)
    assert root * root == P
    rng = np.random.default_rng(7000 + 31 * P + seed)
    a, b = rng.integers(-50, 51, size=Mr), rng.integers(-50, 51, size=Ma)
    rows = lambda v: np.vstack([np.tile(v.astype(np.float64), (P, 1))] + [np.full((1, v.size), 3.25 - k) for k in range(pad)])
    sums = tuple(root * int(np.abs(x[:, None] - y[None, :]).sum()) for x, y in ((a, b), (a, a), (b, b)))
    return rows(a), rows(b), sums


def lattice_expected(sums, Mr: int, Ma: int):
    return tuple(float(s) / float(n) for s, n in zip(sums, (Mr * Ma, Mr * Mr, Ma * Ma)))


def abs_diff_sum(x, y) -> int:
    """sum_{i, j} |x_i - y_j| of integer-valued draws from a sort and a cumulative sum, exactly (Python integers)."""
    x, y = np.asarray(x).astype(np.int64), np.sort(np.asarray(y).astype(np.int64))
    cum = np.concatenate([[0], np.cumsum(y)])
    k = np.searchsorted(y, x, side="right")                       # y[:k] <= x
    below = x * k - cum[k]
    above = (cum[-1] - cum[k]) - x * (y.size - k)
    return int(below.sum()) + int(above.sum())


def line_case(M: int = 40000):
    rng = np.random.default_rng(40)
    return rng.integers(-1000, 1001, size=M).astype(np.float64)[None, :], rng.integers(-900, 1101, size=M).astype(np.float64)[None, :]


def line_expected(ref, act):
    mr, ma = ref.shape[1], act.shape[1]
    return (float(abs_diff_sum(ref[0], act[0])) / float(mr * ma), float(abs_diff_sum(ref[0], ref[0])) / float(mr * mr),
            float(abs_diff_sum(act[0], act[0])) / float(ma * ma))


def general_case(Mr: int, Ma: int, P: int, variant: str):
    rng = np.random.default_rng(10007 * Mr + 101 * Ma + P)
    ref, act = rng.normal(size=(P, Mr)), rng.normal(size=(P, Ma)) * 1.3 + 0.2
    scale = None
    if variant in ("scale", "zero"):
        scale = rng.uniform(0.2, 3.0, size=P)
    if variant == "zero":
        scale[P // 2] = 0.0
    if variant == "offset":
        ref, act = ref + 1e6, act + 1e6
    return ref, act, scale


def separation_scaled():
    ref, wrong, control = separation_case()
    return ref, wrong, control, 1.0 / ref.std(axis=1)


# ---- symbols and argument errors ------------------------------------------------------------------------------------------
def test_symbols_and_version(ffi):
    L = ffi.load_library()
    for name in ("mcr_energy_distance", "mcr_energy_distance_dev", "mcr_energy_distance_host", "mcr_energy_workspace"):
        assert name in ffi.SYMBOLS and hasattr(L, name)
    assert L.mcr_version() == 100
    for name in ("energy_distance", "energy_distance_dev", "energy_workspace"):
        assert callable(getattr(ffi.Context, name))


def test_constants_match_the_header(ffi):
    import re
    header = (ROOT / "include" / "mcmcref_hip.h").read_text()
    defs = {k: int(v) for k, v in re.findall(r"#define (MCR_ENERGY_[A-Z_]+) (\d+)", header)}
    assert defs == {"MCR_ENERGY_TILE_I": ffi.MCR_ENERGY_TILE_I, "MCR_ENERGY_TILE_J": ffi.MCR_ENERGY_TILE_J,
                    "MCR_ENERGY_CHUNK_P": ffi.MCR_ENERGY_CHUNK_P, "MCR_ENERGY_MAX_WORK": ffi.MCR_ENERGY_MAX_WORK,
                    "MCR_ENERGY_LAUNCH_WORK": ffi.MCR_ENERGY_LAUNCH_WORK}
    assert ffi.MCR_ENERGY_MAX_WORK == 1 << 44 and ffi.MCR_ENERGY_LAUNCH_WORK == 1 << 38
    assert ffi.energy_launches(40000, 40000, 100) == 2               # the flagship shape is two launches


def test_host_argument_errors(ffi):
    L = ffi.load_library()
    x = np.arange(6, dtype=np.float64).reshape(2, 3)
    y = np.arange(8, dtype=np.float64).reshape(2, 4) + 0.5
    out = np.full(6, np.nan)
    dp = ffi._as_dp
    call = lambda r, mr, a, ma, p, s, o: L.mcr_energy_distance_host(dp(r), mr, dp(a), ma, p, dp(s), dp(o))
    assert call(x, 3, y, 4, 2, None, out) == MCR_OK and np.isfinite(out).all()
    assert call(None, 3, y, 4, 2, None, out) == MCR_EINVAL
    assert call(x, 3, None, 4, 2, None, out) == MCR_EINVAL
    assert call(x, 3, y, 4, 2, None, None) == MCR_EINVAL
    assert call(x, 0, y, 4, 2, None, out) == MCR_EINVAL
    assert call(x, 3, y, 0, 2, None, out) == MCR_EINVAL
    assert call(x, 3, y, 4, 0, None, out) == MCR_EINVAL
    for bad in (-1.0, np.nan, np.inf):
        assert call(x, 3, y, 4, 2, np.array([1.0, bad]), out) == MCR_EINVAL
    assert call(x, 1 << 22, y, 1 << 22, 1, None, out) == MCR_EINVAL            # over MCR_ENERGY_MAX_WORK: refused unread
    assert call(x, 1 << 40, y, 1 << 40, 1 << 40, None, out) == MCR_EINVAL
    for bad in (np.nan, np.inf, -np.inf):
        z = x.copy(); z[1, 1] = bad
        assert call(z, 3, y, 4, 2, None, out) == MCR_ENONFINITE
        assert call(x, 3, z, 3, 2, None, out) == MCR_ENONFINITE
    big = np.array([[1e200, -1e200]])                                           # t = 2e200: the squared distance overflows
    assert call(big, 2, big, 2, 1, None, out) == MCR_ENONFINITE
    assert call(x, 3, y, 4, 2, np.array([0.0, 0.0]), out) == MCR_OK and out[0] == 0.0 and out[4] == 0.0   # A == 0: H = 0


def test_null_context_calls(ffi):
    L = ffi.load_library()
    x = np.zeros((1, 2))
    out = np.zeros(6)
    dp = ffi._as_dp
    assert L.mcr_energy_distance(None, dp(x), 2, dp(x), 2, 1, None, dp(out)) == MCR_EINVAL
    assert L.mcr_energy_distance_dev(None, None, 2, None, 2, 1, None, dp(out)) == MCR_EINVAL
    assert L.mcr_energy_workspace(None, 2, 2, 1, C.byref(C.c_size_t(0))) == MCR_EINVAL
    assert b"NULL" in L.mcr_last_error(None)


# ---- against the long-double brute force ----------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ("plain", "scale", "zero", "offset"))
@pytest.mark.parametrize("P", (1, 2, 3, 7, 100))
def test_host_against_brute_force(ffi, P, variant):
    for Mr in (1, 2, 3, 37, 300):
        for Ma in (1, 2, 3, 37, 300):
            ref, act, scale = general_case(Mr, Ma, P, variant)
            got = ffi.energy_distance_host(ref, act, scale)
            exp = energy_reference(ref, act, scale)
            assert_close(got, exp, (Mr, Ma, P, variant))
            assert got["h"] == (got["e"] / (2 * got["a"]) if got["a"] else 0.0)
            assert got["t"] == Mr * Ma / (Mr + Ma) * got["e"]
            if variant == "zero" and P > 1:                       # a parameter with scale 0 drops out, in bits
                keep = np.arange(P) != P // 2
                assert got == ffi.energy_distance_host(ref[keep], act[keep], scale[keep])


@pytest.mark.parametrize("P", PAIR_P)
def test_host_pair_bits(ffi, P):
    x, y, s = pair_case(P)
    for scale in (None, s):
        got = ffi.energy_distance_host(x[:, None], y[:, None], scale)
        assert got["a"] == pair_distance(x, y, scale)
        assert got["b"] == 0.0 and got["c"] == 0.0 and got["e"] == 2 * got["a"] and got["h"] == 1.0
        assert ffi.energy_distance_host(y[:, None], x[:, None], scale)["a"] == got["a"]       # d(x, y) = d(y, x)


@pytest.mark.parametrize("P", LATTICE_P)
def test_host_lattice_bits(ffi, P):
    for Mr, Ma in ((1, 1), (5, 3), (130, 257)):
        ref, act, sums = lattice_case(P, Mr, Ma)
        got = ffi.energy_distance_host(ref, act)
        assert (got["a"], got["b"], got["c"]) == lattice_expected(sums, Mr, Ma)


def test_host_line_identity_bits(ffi):
    ref, act = line_case()
    got = ffi.energy_distance_host(ref, act)
    assert (got["a"], got["b"], got["c"]) == line_expected(ref, act)


def test_identical_samples(ffi):
    x = np.random.default_rng(5).normal(size=(7, 211))
    got = ffi.energy_distance_host(x, x.copy())
    assert abs(got["e"]) <= REL * 2 * got["a"] and got["a"] > 0


def test_separation(ffi):
    ref, wrong, control, scale = separation_scaled()
    bad, good = ffi.energy_distance_host(ref, wrong, scale), ffi.energy_distance_host(ref, control, scale)
    assert bad["e"] > 0.1, bad
    assert 0.0 <= good["e"] < 0.01, good


# ---- the validate logic that needs no GPU ---------------------------------------------------------------------------------
def test_thinning_stride():
    from mcmc_ref_hip.validate import energy_stride
    assert energy_stride(2000, None) == 1
    assert [energy_stride(m, n) for m, n in ((2000, 500), (2037, 500), (2037, 2037), (2037, 5000), (10, 1), (1, 1))] == [4, 5, 1, 1, 10, 1]
    for m, n in ((2037, 500), (40000, 999), (7, 3)):
        kept = np.arange(m)[::energy_stride(m, n)]
        assert kept.size <= n and kept.size == -(-m // -(-m // n))
    with pytest.raises(ValueError):
        energy_stride(10, 0)


def test_validate_result_defaults():
    from mcmc_ref_hip.validate import ValidateResult
    base = dict(passed=True, compare=None, ks={}, wasserstein={}, wasserstein_scaled={})
    assert ValidateResult(**base) == ValidateResult(**base, energy=None, energy_detail=None)
    assert ValidateResult(**base).energy is None and ValidateResult(**base).energy_detail is None
    names = [f.name for f in dataclasses.fields(ValidateResult)]
    assert names[-2:] == ["energy", "energy_detail"]

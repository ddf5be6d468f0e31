"""PSIS and PSIS-LOO: the reference in numpy, pinned on the CPU, and the inputs of tests/test_psis_gpu.py.

`psis_reference(v, negate, r_eff, ndraws_tail, dtype)` is the definition of mcr_psis (include/mcmcref_hip.h) for one column
in plain numpy, every step in `dtype` (float64 or longdouble) from the float64 values: tail length, cutoff, tail
membership by value, Zhang and Stephens' fit with the power-of-two scaling, sigma from the unregularised k, the run rule
for ties, the three log-sum-exps.  Its sums are numpy's; the library's order of summation is its own, and the two meet
under the gate.

The gate is the project's: |got - ref| <= 1e-9 * max(1, |ref|) against the longdouble run, for every log weight and every
scalar; ndraws_tail, +inf and NaN are compared exactly.  A float64 run of this reference against its longdouble run
disagrees by at most ~3e-12 on these distributions and sizes (`test_float64_and_longdouble_agree` holds every input used
here and in the GPU file to 1e-10, so that an ill-conditioned input shows as a bad input and not as a kernel failure):
the gate has more than two decimal orders of margin.
"""
from __future__ import annotations

import json
import math
import struct
from pathlib import Path

import numpy as np
import pytest

GATE = 1e-9
REF_AGREE = 1e-10
LOG_MIN = float(np.log(np.finfo(np.float64).tiny))           # log(DBL_MIN) as a double: -708.3964185322641
GOLDEN = Path(__file__).resolve().parent / "golden"



@pytest.fixture(scope="module", autouse=True)
def psis_library():
    """Everything here specifies or exercises the library's PSIS entries: without them there is nothing to hold."""
    from mcmc_ref_hip import _ffi
    lib = _ffi.load_library()
    assert "mcr_psis" in _ffi.SYMBOLS and lib.mcr_psis_host is not None
    return lib


# ---------------------------------------------------------------------------------------------------------------------
# The reference
# ---------------------------------------------------------------------------------------------------------------------


def tail_bisect_rule(M: int, r_eff: float = 1.0) -> int:
    """T: the smallest t with float(t^2) * r_eff >= float(9 M)."""
    if r_eff == 1.0:
        return math.isqrt(9 * M - 1) + 1
    ok = lambda t: float(t * t) * r_eff >= float(9 * M)
    t = max(int(3.0 * math.sqrt(M / r_eff)), 1)
    while ok(t - 1):
        t -= 1
    while not ok(t):
        t += 1
    return t


def tail_length_rule(M: int, r_eff: float = 1.0) -> int:
    """The default t_req = min((M + 4) // 5, T) = ceil(min(M / 5, 3 sqrt(M / r_eff)))."""
    return 0 if M < 1 else min((M + 4) // 5, tail_bisect_rule(M, r_eff))


def gpd_fit(e, dtype):
    """(khat, sigma) of n >= 5 ascending exceedances e in `dtype`: rules 1 to 6 of the Pareto section, khat NaN -> +inf,
    sigma = -k / theta / 2^s from the unregularised k (NaN where the grid is not run)."""
    inf, nan = float("inf"), float("nan")
    n = e.size
    if e[-1] == e[0]:
        return inf, nan                                        # a constant tail
    G = 30 + math.isqrt(n)
    if e[(n + 2) // 4 - 1] == 0:
        return inf, nan                                        # xstar == 0
    ex = int(np.frexp(np.float64(e[-1]))[1])                   # e_(n-1) 2^(1 - ex) lies in [1, 2)
    sc = dtype(2.0) ** (1 - min(max(ex, -1000), 1000))
    es = e * sc
    xstar, dn = es[(n + 2) // 4 - 1], dtype(n)
    with np.errstate(all="ignore"):
        j = np.arange(1, G + 1).astype(dtype)
        theta = dtype(1) / es[-1] + (dtype(1) - np.sqrt(dtype(G) / (j - dtype(0.5)))) / dtype(3) / xstar
        k = np.log1p(-theta[:, None] * es[None, :]).sum(axis=1) / dn
        l = dn * (np.log(-theta / k) - k - dtype(1))
        m = l.max()
        L = m + np.log(np.exp(l - m).sum())
        th = (theta * np.exp(l - L)).sum()
        kk = np.log1p(-th * es).sum() / dn
        khat = (kk * dn + dtype(5)) / (dn + dtype(10))
        sigma = -kk / th / sc
    return (inf if khat != khat else khat), sigma


def lse(a):
    m = a.max()
    return m + np.log(np.exp(a - m).sum())


def psis_reference(v, negate: bool = False, r_eff: float = 1.0, ndraws_tail: int | None = None, dtype=np.longdouble) -> dict:
    """Every output of mcr_psis for one column v (any order): khat, ndraws_tail (the n used), lppd, elpd, p_loo (NaN
    without negate), log_weights in the order of v; and lw_max, the largest smoothed log ratio before normalisation,
    clamp (the log(DBL_MIN) clamp is active), smoothed."""
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    M = v.size
    nan = float("nan")
    out = {"khat": nan, "ndraws_tail": 0, "lppd": nan, "elpd": nan, "p_loo": nan, "log_weights": np.zeros(0, dtype=dtype),
           "lw_max": nan, "clamp": False, "smoothed": False}
    if M == 0:
        return out
    x = (-v if negate else v).astype(dtype)
    order = np.argsort(x, kind="stable")
    xs = x[order]
    y = xs - xs[-1]
    t = min(tail_length_rule(M, r_eff) if ndraws_tail is None else int(ndraws_tail), M - 1)
    lw = y.copy()
    khat, n = float("inf"), 0
    if t >= 1:
        cut = y[M - t - 1]
        if not cut > dtype(LOG_MIN):
            cut, out["clamp"] = dtype(LOG_MIN), True
        n = int(np.count_nonzero(y > cut))
        if n > 4:
            with np.errstate(all="ignore"):
                ecut = np.exp(cut)
                e = np.exp(y[M - n:]) - ecut
                khat, sigma = gpd_fit(e, dtype)
                if math.isfinite(khat) and sigma > 0:
                    s, en = np.searchsorted(e, e, "left"), np.searchsorted(e, e, "right")     # the runs of equal e
                    p = (s + en).astype(dtype) / dtype(2 * n)
                    l1 = np.log1p(-p)
                    q = -sigma * l1 if abs(khat) < np.finfo(np.float64).eps else sigma * np.expm1(-khat * l1) / khat
                    lw[M - n:] = np.minimum(np.log(q + ecut), dtype(0))
                    out["smoothed"] = True
    log_norm = lse(lw)
    logw = np.empty(M, dtype=dtype)
    logw[order] = lw - log_norm
    out.update(khat=float(khat), ndraws_tail=n, log_weights=logw, lw_max=float(lw.max()))
    if negate:
        lppd = lse(-xs) - np.log(dtype(M))
        elpd = lse(lw - xs) - log_norm
        out.update(lppd=float(lppd), elpd=float(elpd), p_loo=float(lppd - elpd))
    return out


SCALARS = ("khat", "lppd", "elpd", "p_loo")


def same(got: float, ref: float, gate: float = GATE) -> bool:
    """NaN and +-inf exactly, everything else within the gate."""
    if ref != ref or got != got:
        return ref != ref and got != got
    if math.isinf(ref) or math.isinf(got):
        return got == ref
    return abs(got - ref) <= gate * max(1.0, abs(ref))


def worst_error(got: dict, ref: dict) -> float:
    """The largest |got - ref| / max(1, |ref|) over the finite scalars and every log weight."""
    w = 0.0
    for k in SCALARS:
        g, r = float(got.get(k, float("nan"))), float(ref.get(k, float("nan")))
        if math.isfinite(g) and math.isfinite(r):
            w = max(w, abs(g - r) / max(1.0, abs(r)))
    if "log_weights" in got:
        r = np.asarray(ref["log_weights"], dtype=np.longdouble)
        g = np.asarray(got["log_weights"]).astype(np.longdouble)
        if r.size:
            w = max(w, float(np.max(np.abs(g - r) / np.maximum(1.0, np.abs(r)))))
    return w


def check(got: dict, ref: dict, what, gate: float = GATE) -> float:
    """got (a column's outputs: the scalars given, ndraws_tail, log_weights if given) against ref; the worst error."""
    assert int(got["ndraws_tail"]) == ref["ndraws_tail"], (what, got["ndraws_tail"], ref["ndraws_tail"])
    for k in SCALARS:
        if k in got:
            assert same(float(got[k]), float(ref[k]), gate), (what, k, float(got[k]), float(ref[k]))
    if "log_weights" in got:
        g, r = np.asarray(got["log_weights"]).astype(np.longdouble), np.asarray(ref["log_weights"], dtype=np.longdouble)
        assert g.shape == r.shape, (what, g.shape, r.shape)
        if r.size:
            bad = np.flatnonzero(~(np.abs(g - r) <= gate * np.maximum(1.0, np.abs(r))))
            assert bad.size == 0, (what, "log_weights", bad[:5], g[bad[:5]], r[bad[:5]])
    return worst_error(got, ref)


# ---------------------------------------------------------------------------------------------------------------------
# Inputs
# ---------------------------------------------------------------------------------------------------------------------

DISTS = ("normal", "normal3", "t3", "cauchy5", "exponential", "constant", "rounded", "normal400", "chi2_loglik")
SIZES = (1, 4, 5, 9, 10, 24, 25, 26, 225, 226, 1000, 4097, 40_000)


def values(dist: str, M: int, seed: int = 1) -> np.ndarray:
    """M float64 values of a column.  As log ratios: light (normal) to hopeless (5 Cauchy, 400 normal: the clamp); rounded
    has ties everywhere; chi2_loglik are log-likelihoods -(z^2 + log 2 pi) / 2 of a normal observation, z ~ N(0.3, 0.3)."""
    rng = np.random.default_rng([seed, DISTS.index(dist), M])
    if dist == "normal":
        return rng.normal(size=M)
    if dist == "normal3":
        return 3.0 * rng.normal(size=M)
    if dist == "t3":
        return rng.standard_t(3, size=M)
    if dist == "cauchy5":
        return 5.0 * rng.standard_cauchy(size=M)
    if dist == "exponential":
        return rng.exponential(size=M)
    if dist == "constant":
        return np.full(M, 1.25)
    if dist == "rounded":
        return np.round(rng.normal(size=M), 1)
    if dist == "normal400":
        return 400.0 * rng.normal(size=M)
    return -0.5 * (rng.normal(loc=0.3, scale=0.3, size=M) ** 2 + math.log(2.0 * math.pi))


def tied_tail(M: int = 2000, seed: int = 5) -> np.ndarray:
    """Normal log ratios whose tail holds two runs of ties (three and four equal values) among distinct values."""
    x = np.sort(np.random.default_rng(seed).normal(size=M))
    x[-20:-17] = x[-19]
    x[-9:-5] = x[-7]
    return np.random.default_rng(seed + 1).permutation(x)


def xstar_zero_column() -> np.ndarray:
    """Eleven log ratios, ndraws_tail = 5: the first tail value lies one ulp above the cutoff -0.3 and has the cutoff's exp
    in float64, so e_0 = xstar = 0 (in longdouble it is not: the branch is a float64 one)."""
    c = -0.3
    return np.array([-9.0, -8.0, -7.0, -6.0, -5.0, c, np.nextafter(c, 0.0), -0.2, -0.1, -0.05, 0.0])


# ---------------------------------------------------------------------------------------------------------------------
# The reference against itself
# ---------------------------------------------------------------------------------------------------------------------


def assert_reference_agrees(v, what, **kw) -> dict:
    """The float64 and the longdouble run of the reference agree to REF_AGREE on this input; the longdouble run."""
    a, b = psis_reference(v, dtype=np.float64, **kw), psis_reference(v, dtype=np.longdouble, **kw)
    assert a["ndraws_tail"] == b["ndraws_tail"] and a["smoothed"] == b["smoothed"], (what, a["ndraws_tail"], b["ndraws_tail"])
    check(a, b, ("reference f64 vs longdouble", what), REF_AGREE)
    return b


@pytest.mark.parametrize("dist", DISTS)
def test_float64_and_longdouble_agree(dist):
    worst = 0.0
    for M in SIZES:
        for negate in (False, True):
            b = assert_reference_agrees(values(dist, M), (dist, M, negate), negate=negate)
            worst = max(worst, worst_error(psis_reference(values(dist, M), negate=negate, dtype=np.float64), b))
    print(f"reference, {dist}: float64 against longdouble {worst:.3g}")


def test_sanity():
    r = psis_reference(values("normal", 40_000))
    assert r["ndraws_tail"] == 600 and r["khat"] < 0.5 and r["smoothed"], r["khat"]
    r = psis_reference(values("cauchy5", 40_000))
    assert r["khat"] > 1.0 and r["clamp"]
    r = psis_reference(values("chi2_loglik", 4000), negate=True)
    assert r["khat"] < 0.7 and 0.0 < r["p_loo"] < 1.0 and r["elpd"] < r["lppd"]


# ---------------------------------------------------------------------------------------------------------------------
# The library's host routines (no GPU)
# ---------------------------------------------------------------------------------------------------------------------


def test_library_exports_and_declarations():
    from mcmc_ref_hip import _ffi
    lib = _ffi.load_library()
    for name in ("mcr_psis", "mcr_psis_dev", "mcr_psis_plan", "mcr_psis_tail_length", "mcr_psis_host"):
        assert name in _ffi.SYMBOLS, name
        assert getattr(lib, name) is not None
    assert [f for f, _ in _ffi.Psis._fields_] == ["khat", "ndraws_tail", "lppd", "elpd", "p_loo", "log_weights"]
    header = (Path(__file__).resolve().parents[1] / "include" / "mcmcref_hip.h").read_text()
    assert "typedef struct mcr_psis_out" in header and "int mcr_psis_host(" in header
    assert lib.mcr_version() == 100
    for name in ("psis", "loo", "psis_params_per_chunk"):
        assert callable(getattr(_ffi.Context, name))


def test_tail_length_rule_of_the_library():
    from mcmc_ref_hip import _ffi
    fn = _ffi.load_library().mcr_psis_tail_length
    sizes = list(range(1, 5001))
    roots = [2, 3, 15, 16, 100, 1000, 4096, 12345, 32768, 46340, 46341]
    sizes += [k * k + d for k in roots for d in (-1, 0, 1)] + [2 ** 31 - 3, 2 ** 31 - 2]
    for r_eff in (1.0, 0.5, 0.1):
        for M in sizes:
            assert fn(M, r_eff) == tail_length_rule(M, r_eff), (M, r_eff)
    for M in sizes:                                            # ceil(min(M / 5, 3 sqrt(M))): loo's and ArviZ's rule
        assert tail_length_rule(M) == min(-(-M // 5), math.isqrt(9 * M - 1) + 1)
    assert [fn(M, 1.0) for M in (1, 4, 5, 6, 224, 225, 226)] == [1, 1, 1, 2, 45, 45, 46]
    for k in (16, 1000, 46340):
        assert fn(k * k, 1.0) == 3 * k and fn(k * k + 1, 1.0) == 3 * k + 1
    assert fn(0, 1.0) == 0 and fn(-5, 1.0) == 0
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert fn(1000, bad) == _ffi.MCR_EINVAL
        with pytest.raises(ValueError):
            _ffi.psis_tail_length(1000, bad)


@pytest.mark.parametrize("dist", DISTS)
def test_host_routine_against_longdouble(dist):
    from mcmc_ref_hip import _ffi
    worst = 0.0
    for M in SIZES:
        v = values(dist, M)
        for negate in (False, True):
            for kw in ({}, {"r_eff": 0.1}):
                ref = assert_reference_agrees(v, (dist, M, negate, kw), negate=negate, **kw)
                got = _ffi.psis_host(v, negate=negate, **kw)
                worst = max(worst, check(got, ref, (dist, M, negate, kw)))
                assert got["log_weights"].max(initial=-1.0) <= GATE            # a normalised weight is at most 1
                if M:
                    assert abs(float(np.exp(got["log_weights"].astype(np.longdouble)).sum()) - 1.0) <= GATE
    print(f"mcr_psis_host, {dist}: worst error against longdouble {worst:.3g}")


@pytest.mark.parametrize("tail", [1, 4, 5, 6, 63, 64, 65, 255, 256, 257, 8192, 8193, 19_999, 20_000, 10 ** 9])
def test_host_routine_explicit_tail(tail):
    from mcmc_ref_hip import _ffi
    for dist, negate in (("t3", False), ("chi2_loglik", True)):
        v = values(dist, 20_000)
        ref = assert_reference_agrees(v, (dist, tail), negate=negate, ndraws_tail=tail)
        got = _ffi.psis_host(v, negate=negate, ndraws_tail=tail)
        check(got, ref, (dist, tail))
        assert got["ndraws_tail"] == min(tail, 19_999) or dist != "t3"           # (no ties: n = t)
        if tail <= 4:
            assert got["khat"] == float("inf")


def test_branches():
    from mcmc_ref_hip import _ffi
    inf = float("inf")
    # t == 0 at M = 1: one weight of 1
    got = _ffi.psis_host([3.5], negate=True)
    assert got["khat"] == inf and got["ndraws_tail"] == 0 and got["log_weights"].tolist() == [0.0]
    assert got["lppd"] == 3.5 and got["elpd"] == 3.5 and got["p_loo"] == 0.0
    # n <= 4: the normalised raw ratios
    for M in (2, 4, 5, 9, 10, 20):
        v = values("normal", M)
        got, ref = _ffi.psis_host(v), psis_reference(v)
        assert got["khat"] == inf and got["ndraws_tail"] == ref["ndraws_tail"] <= 4 and not ref["smoothed"]
        raw = v - v.max()
        check({"log_weights": got["log_weights"], "ndraws_tail": got["ndraws_tail"]},
              {"log_weights": raw - lse(raw.astype(np.longdouble)), "ndraws_tail": ref["ndraws_tail"]}, ("raw", M))
    assert psis_reference(values("normal", 21))["ndraws_tail"] == 5              # the first size that fits a tail
    # a constant column: nothing lies above the cutoff, uniform weights
    for M in (1, 7, 1000):
        got = _ffi.psis_host(np.full(M, -2.5), negate=True)
        assert got["khat"] == inf and got["ndraws_tail"] == 0
        assert np.allclose(got["log_weights"], -math.log(M), rtol=0, atol=GATE)
        assert same(got["lppd"], -2.5) and same(got["elpd"], -2.5) and abs(got["p_loo"]) <= GATE
    # ties at the cutoff: n < t
    v = values("rounded", 4097)
    ref = assert_reference_agrees(v, "rounded")
    t = tail_length_rule(4097)
    assert 4 < ref["ndraws_tail"] < t
    assert _ffi.psis_host(v)["ndraws_tail"] == ref["ndraws_tail"]
    # the log(DBL_MIN) clamp
    for M in (1000, 4097):
        v = values("cauchy5", M)
        ref = assert_reference_agrees(v, "cauchy5")
        assert ref["clamp"] and ref["ndraws_tail"] < tail_length_rule(M)
        check(_ffi.psis_host(v), ref, ("clamp", M))
    # xstar == 0 (a float64 branch: see xstar_zero_column)
    v = xstar_zero_column()
    ref = psis_reference(v, ndraws_tail=5, dtype=np.float64)
    y = np.sort(v) - v.max()
    assert np.exp(y[6]) - np.exp(y[5]) == 0.0 and ref["ndraws_tail"] == 5 and ref["khat"] == inf and not ref["smoothed"]
    got = _ffi.psis_host(v, ndraws_tail=5)
    assert got["khat"] == inf
    check(got, ref, "xstar == 0")
    # a constant tail: khat NaN becomes +inf
    v = np.concatenate([np.linspace(-9.0, -1.0, 50), np.full(12, 0.5)])
    got = _ffi.psis_host(v, ndraws_tail=12)
    ref = psis_reference(v, ndraws_tail=12)
    assert got["khat"] == inf == ref["khat"] and got["ndraws_tail"] == 12
    check(got, ref, "constant tail")


def test_tied_values_get_equal_weights():
    from mcmc_ref_hip import _ffi
    v = tied_tail()
    ref = assert_reference_agrees(v, "tied tail")
    got = _ffi.psis_host(v)
    check(got, ref, "tied tail")
    s = np.sort(v)
    runs = 0
    for val in (s[-19], s[-7]):
        w = got["log_weights"][v == val]
        assert w.size >= 3 and np.all(w == w[0])               # in bits: a weight is a function of the value alone
        runs += 1
    assert runs == 2 and ref["ndraws_tail"] > 20
    order = np.argsort(v, kind="stable")                       # and the weights never fall as the ratios rise
    assert np.all(np.diff(got["log_weights"][order]) >= 0.0)
    # any order of the values: the same weight for the same value
    perm = np.random.default_rng(9).permutation(v.size)
    again = _ffi.psis_host(v[perm])
    assert again["khat"] == got["khat"] and np.array_equal(again["log_weights"], got["log_weights"][perm])


def test_properties():
    from mcmc_ref_hip import _ffi
    for dist in ("normal", "t3", "chi2_loglik", "rounded"):
        v = values(dist, 4097)
        for negate in (False, True):
            ref = psis_reference(v, negate=negate)
            assert ref["lw_max"] <= 0.0                        # the smoothed maximum, before normalisation
            got = _ffi.psis_host(v, negate=negate)
            assert abs(float(np.exp(got["log_weights"].astype(np.longdouble)).sum()) - 1.0) <= GATE
            shifted = _ffi.psis_host(v + 3.0, negate=negate)   # a constant: nothing but lppd and elpd move, by it
            assert shifted["ndraws_tail"] == got["ndraws_tail"] and same(shifted["khat"], got["khat"])
            check({"log_weights": shifted["log_weights"], "ndraws_tail": shifted["ndraws_tail"]},
                  {"log_weights": got["log_weights"], "ndraws_tail": got["ndraws_tail"]}, ("shift", dist))
            if negate:
                assert same(shifted["lppd"], got["lppd"] + 3.0) and same(shifted["elpd"], got["elpd"] + 3.0)
                assert same(shifted["p_loo"], got["p_loo"])


def test_negation_in_bits():
    """negate = 1 on v against negate = 0 on -v: the same bits."""
    from mcmc_ref_hip import _ffi
    for dist in DISTS:
        v = values(dist, 4097)
        a, b = _ffi.psis_host(v, negate=True), _ffi.psis_host(-v, negate=False)
        assert a["ndraws_tail"] == b["ndraws_tail"] and (a["khat"] == b["khat"])
        assert np.array_equal(a["log_weights"], b["log_weights"])
        assert math.isnan(b["lppd"]) and math.isnan(b["elpd"]) and math.isnan(b["p_loo"])


def test_pareto_fit_host_keeps_its_bits():
    """pareto_fit hands out its unregularised k and theta now; khat of mcr_pareto_fit_host as recorded before that."""
    from mcmc_ref_hip import _ffi
    from test_pareto_refs_cpu import constant_right_tail, draws, ties_at_cutoff
    rec = json.loads((GOLDEN / "pareto_fit_host_bits.json").read_text())
    hexd = lambda x: struct.pack(">d", x).hex()
    assert len(rec["cases"]) == 32
    for c in rec["cases"]:
        if c["input"] == "constant_right_tail":
            x = constant_right_tail(c["M"])
        elif c["input"] == "ties_at_cutoff":
            x = ties_at_cutoff(c["M"])
        else:
            x = draws(c["input"], c["M"])
        kl, kr, t = _ffi.pareto_fit_host(np.sort(x), c["ndraws_tail"])
        assert (t, hexd(kl), hexd(kr)) == (c["t"], c["khat_left"], c["khat_right"]), c


def test_python_surface_value_errors():
    from mcmc_ref_hip import _ffi, convert, diagnostics
    for kw in ({"r_eff": 0.0}, {"r_eff": float("nan")}, {"ndraws_tail": -1}):
        with pytest.raises(ValueError):
            _ffi.psis_host(np.arange(10.0), **kw)
    for bad in (float("nan"), float("inf"), float("-inf")):
        with pytest.raises(ValueError, match="non-finite"):
            _ffi.psis_host([0.0, bad, 1.0])
    empty = _ffi.psis_host([])
    assert math.isnan(empty["khat"]) and empty["ndraws_tail"] == 0 and empty["log_weights"].size == 0
    with pytest.raises(ValueError, match="not both"):
        diagnostics.psis_log_weights([[1.0, 2.0, 3.0]] * 4, r_eff=1.0, ndraws_tail=5)
    tot = _ffi.loo_totals([-1.0, -2.0, -4.5], [0.1, 0.2, 0.3], [-0.9, -1.8, -4.2], [0.2, 0.6, float("inf")])
    assert tot["elpd_loo"] == -7.5 and tot["khat_counts"] == [1, 1, 0, 1] and tot["n_obs"] == 3
    assert tot["se"] == math.sqrt(3 * np.var([-1.0, -2.0, -4.5]))
    assert callable(convert.loo_file) and callable(convert.loo_compare_files)


def test_null_context_answers_einval():
    import ctypes

    from mcmc_ref_hip import _ffi
    lib = _ffi.load_library()
    x = np.zeros((1, 4, 4))
    out = _ffi.Psis()
    for fn in (lib.mcr_psis, lib.mcr_psis_dev):
        rc = fn(None, x.ctypes.data_as(ctypes.c_void_p), *_ffi.tensor_args(x, "pcn"), 0, None, None, ctypes.byref(out))
        assert rc == _ffi.MCR_EINVAL
        assert lib.mcr_last_error(None) == b"ctx is NULL"
    v = ctypes.c_int64(7)
    assert lib.mcr_psis_plan(None, _ffi.MCR_F64, 4, 4, 1, 4, 1, 16, 0, ctypes.byref(v)) == _ffi.MCR_EINVAL


def test_commands_take_the_options():
    from click.testing import CliRunner
    from mcmc_ref_hip.cli import main
    out = CliRunner().invoke(main, ["loo", "--help"])
    assert out.exit_code == 0 and all(opt in out.output for opt in ("--prefix", "--params", "--against", "--pointwise", "--format"))
    out = CliRunner().invoke(main, ["loo", "no_such_file.csv"])
    assert out.exit_code != 0

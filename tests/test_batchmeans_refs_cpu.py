"""Batch means, the long-run covariance, the mean test and the multivariate ESS of include/mcmcref_bm.h without a GPU: a
numpy restatement of the definition (an explicit tree) that the host routines must equal in bits, a long double reference
for Sigma, T and mESS, the edges and refusals, the mirror `_babi` against the header and the exports of libmcmcref_bm.so,
and the calibration of the test on autocorrelated chains.  tests/test_batchmeans_gpu.py imports the restatement, the
reference and the cases from here, so what is pinned here is what the device is held to there.

Tolerances.  Bits where the header promises bits.  1e-9 relative -- the project's gate for a floating output -- for Sigma,
T and mESS against the long double reference, on cases whose scaled V has a condition number of at most 1e3 (asserted):
the forward error of a Cholesky solve is of the order cond * P * 2^-53 < 1e-11 there.  The calibration bounds were set before the code ran:
at most 4 of 40 pairs with p < 0.01 under equal means (the expected count is 0.4), at least 36 of 40 for the
naive statistic, p < 1e-6 for a shift of half a standard deviation, the mean mESS within a factor 1.5 of
M (1 - phi) / (1 + phi).
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
from test_gaussian_refs_cpu import bits, chol_ld, solve_ld, spd
from test_host_cpu import built_lib  # noqa: F401  (the fixture: an up-to-date build of the libraries)

LD = np.longdouble
RTOL = 1e-9
BLOCK = 1024                                                 # MCB_BLOCK (checked against the header below)
PHI = 0.9


# ---- the restatement of the definition in numpy ---------------------------------------------------------------------------

def tree_sum(leaves) -> np.ndarray:
    """The sum over the last axis in the one association: blocks of 1024 consecutive leaves, in each the balanced binary
    tree over adjacent leaves with +0 past the end, the blocks' roots added in ascending order from +0."""
    t = np.asarray(leaves, dtype=np.float64)
    n = t.shape[-1]
    blocks = max(1, -(-n // BLOCK))
    padded = np.zeros(t.shape[:-1] + (blocks * BLOCK,))
    padded[..., :n] = t
    level = padded.reshape(t.shape[:-1] + (blocks, BLOCK))
    while level.shape[-1] > 1:
        level = level[..., 0::2] + level[..., 1::2]
    acc = np.zeros(t.shape[:-1])
    for k in range(blocks):
        acc = acc + level[..., k, 0]
    return acc


def pcn_view(x, layout: str) -> np.ndarray:
    return np.transpose(x, [layout.index(a) for a in "pcn"])


def restate_batch_means(x, layout: str, b: int):
    """(bm [P][A], mu [P]) by the definition."""
    v = pcn_view(np.asarray(x), layout)
    P, C_, N = v.shape
    a = N // b
    n0 = N - a * b
    K = v[:, 0, n0].astype(np.float64)
    t = v[:, :, n0:].astype(np.float64) - K[:, None, None]
    s = tree_sum(t.reshape(P, C_, a, b))
    bm = K[:, None, None] + s / float(b)
    S = tree_sum(s.reshape(P, C_ * a))
    return bm.reshape(P, C_ * a), K + S / float(C_ * a * b)


def restate_finish(cb, cb3, b: int, A: int, A3: int, r: int) -> np.ndarray:
    if A < 2:
        return np.full_like(cb, np.nan)
    sb = cb * ((float(b) * float(A)) / float(A - 1))
    if r == 1:
        return sb
    s3 = cb3 * ((float(b // 3) * float(A3)) / float(A3 - 1))
    return 2.0 * sb - s3


def restate_pool(sr, mur, Mr, sa, mua, Ma, scale, jitter):
    P = sr.shape[0]
    s = np.ones(P) if scale is None else np.asarray(scale, dtype=np.float64)
    live = np.flatnonzero(s > 0)
    sl = s[live]
    t = sr[np.ix_(live, live)] / float(Mr)
    if sa is not None:
        t = t + sa[np.ix_(live, live)] / float(Ma)
    v = (sl[:, None] * sl[None, :]) * t
    v[np.diag_indices(live.size)] = np.diag(v) + jitter
    d = sl * ((mua[live] - mur[live]) if sa is not None else mur[live])
    with np.errstate(invalid="ignore", divide="ignore"):
        z = d / np.sqrt(np.diag(v))
    return v, d, z


# ---- the reference in long double -----------------------------------------------------------------------------------------

def lrv_ld(x_pcn, b: int, r: int):
    """(Sigma, mu, M) in long double, straight from the formulas."""
    x = np.asarray(x_pcn, dtype=LD)
    P, C_, N = x.shape

    def sigma_b(bb):
        a = N // bb
        bm = x[:, :, N - a * bb:].reshape(P, C_, a, bb).mean(axis=3).reshape(P, C_ * a)
        c = bm - bm.mean(axis=1, keepdims=True)
        A = C_ * a
        return (c @ c.T) / LD(A) * LD(bb) * LD(A) / LD(A - 1)

    a = N // b
    sig = sigma_b(b) if r == 1 else 2 * sigma_b(b) - sigma_b(b // 3)
    return sig, x[:, :, N - a * b:].reshape(P, -1).mean(axis=1), C_ * a * b


def logdet_ld(A) -> float:
    return 2 * np.log(np.diag(chol_ld(A))).sum()


def mean_test_ld(ref, act, scale, jitter: float, r: int, b_ref: int, b_act: int) -> dict:
    """T, z, shift, V and the two mESS of `mean_shift_test` in long double (ref, act [P][C][N])."""
    s = np.asarray(scale, dtype=np.float64)
    live = s > 0
    sl = s[live].astype(LD)
    out = {}
    parts = []
    for name, x, b in (("ref", ref, b_ref), ("act", act, b_act)):
        sig, mu, M = lrv_ld(x, b, r)
        sig, mu = sig[np.ix_(live, live)] * sl[:, None] * sl[None, :], mu[live] * sl
        parts.append((sig, mu, M))
        pooled = np.asarray(x, dtype=LD)[live].reshape(int(live.sum()), -1)
        c = pooled - pooled.mean(axis=1, keepdims=True)
        lam = (c @ c.T) / LD(pooled.shape[1]) * sl[:, None] * sl[None, :]
        out[f"mess_{name}"] = float(pooled.shape[1] * np.exp((logdet_ld(lam) - logdet_ld(sig)) / LD(sl.size)))
        out[f"sigma_{name}"] = sig.astype(np.float64)
    (sr, mr, Mr), (sa, ma, Ma) = parts
    V = sr / LD(Mr) + sa / LD(Ma) + LD(jitter) * np.eye(sl.size, dtype=LD)
    d = ma - mr
    y = solve_ld(chol_ld(V), d[:, None])[:, 0]
    out.update(T=float(y @ y), shift=y.astype(np.float64), z=(d / np.sqrt(np.diag(V))).astype(np.float64),
               V=V.astype(np.float64), dof=int(sl.size))
    return out


# ---- inputs ---------------------------------------------------------------------------------------------------------------

def ar1(rng, mix, C_: int, N: int, phi: float = PHI) -> np.ndarray:
    """[P][C][N]: P AR(1) chains with unit stationary variance, mixed by `mix` [P][P] (so that their covariance is
    mix mix^T), every chain started from the stationary distribution."""
    from scipy.signal import lfilter
    P = mix.shape[0]
    e = rng.standard_normal((P, C_, N)) * math.sqrt(1.0 - phi * phi)
    e[:, :, 0] = rng.standard_normal((P, C_))
    y = lfilter([1.0], [1.0, -phi], e, axis=2)
    return np.ascontiguousarray(np.einsum("ij,jcn->icn", mix, y))


@functools.lru_cache(maxsize=None)
def e2e_case(P: int):
    """(ref, act, scale, b_ref, b_act, want) of an end-to-end case with P live parameters and one dropped one (index 1
    when P > 1): short batches and weakly autocorrelated chains, so that there are many more batches than parameters and
    the scaled V is well conditioned.  Computed once; the arrays are shared and read only."""
    rng = np.random.default_rng(100 + P)
    total = P + (1 if P > 1 else 0)
    mix = np.linalg.cholesky(spd(total, 10.0, seed=P))
    ref = ar1(rng, mix, 3, 2004, phi=0.3) + rng.standard_normal((total, 1, 1))
    act = ar1(rng, mix, 4, 3003, phi=0.3) + ref.mean(axis=(1, 2), keepdims=True) + 0.02 * rng.standard_normal((total, 1, 1))
    scale = 1.0 / ref.reshape(total, -1).std(axis=1)
    if P > 1:
        scale[1] = 0.0
    want = mean_test_ld(ref, act, scale, 0.0, 3, 6, 9)
    for a in (ref, act, scale):
        a.setflags(write=False)
    return ref, act, scale, 6, 9, want


E2E_P = (1, 16, 17, 64, 65, 129)


def close(got: float, want: float) -> bool:
    return abs(got - want) <= RTOL * abs(want)


def check_mean_test(got: dict, want: dict, what=""):
    assert got["info"] == 0 and got["dof"] == want["dof"], (what, got["info"], got["dof"])
    assert close(got["T"], want["T"]), (what, got["T"], want["T"])
    assert close(got["mess_ref"], want["mess_ref"]) and close(got["mess_act"], want["mess_act"]), (what, got["mess_ref"], want["mess_ref"])
    assert np.abs(got["shift"] - want["shift"]).max() <= RTOL * max(1.0, np.abs(want["shift"]).max()), what
    assert np.abs(got["z"] - want["z"]).max() <= RTOL * max(1.0, np.abs(want["z"]).max()), what


@pytest.fixture(scope="module")
def bm(built_lib):  # noqa: F811
    from mcmc_ref_hip import batchmeans
    return batchmeans


# ---- the host definitions against the restatement, in bits ----------------------------------------------------------------

BITS_B = (1, 2, 3, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2049)


def test_tree_sum_restatement_is_the_tree():
    """Against a scalar recursion on a few lengths, including the sign of a zero."""
    def node(v, lo, n):
        return v[lo] if n == 1 else node(v, lo, n // 2) + node(v, lo + n // 2, n // 2)
    rng = np.random.default_rng(0)
    for n in (1, 2, 3, 1023, 1024, 1025, 2049):
        v = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 8, n)
        pad = np.zeros(-(-n // BLOCK) * BLOCK)
        pad[:n] = v
        want = 0.0
        for k in range(pad.size // BLOCK):
            want = want + node(pad, k * BLOCK, BLOCK)
        assert bits(tree_sum(v)) == bits(want), n
    assert bits(tree_sum(np.array([-0.0]))) == bits(0.0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_batch_means_host_in_bits(bm, dtype):
    rng = np.random.default_rng(1)
    for i, b in enumerate(BITS_B):
        for r0 in sorted({0, 1, b - 1}):
            N = 3 * b + r0
            C_, P = (1, 3)[i % 2], (1, 2, 5)[i % 3]
            x = (rng.standard_normal((P, C_, N)) * 10.0 ** rng.integers(-3, 4, (P, 1, 1)) + 7.0).astype(dtype)
            for layout in ("pcn", "cnp", "ncp"):
                y = np.ascontiguousarray(np.transpose(x, ["pcn".index(a) for a in layout]))
                got = bm.batch_means_host(y, layout, batch=b, r=1)
                want_bm, want_mu = restate_batch_means(y, layout, b)
                assert got["a"] == N // b and bits(got["bm"]) == bits(want_bm) and bits(got["mu"]) == bits(want_mu), (b, r0, layout)


def test_batch_means_host_strides_and_head(bm):
    rng = np.random.default_rng(2)
    base = rng.standard_normal((3, 2, 2 * 211 + 5))
    thin = base[:, :, ::2]                                   # stride_n = 2
    want = bm.batch_means_host(np.ascontiguousarray(thin), batch=20, r=1)
    got = bm.batch_means_host(thin, batch=20, r=1)
    assert bits(got["bm"]) == bits(want["bm"]) and bits(got["mu"]) == bits(want["mu"])
    rep = np.broadcast_to(base[:, :1, :], (3, 4, base.shape[2]))          # stride_c = 0: one chain four times
    got = bm.batch_means_host(rep, batch=33, r=3)
    one = bm.batch_means_host(base[:, :1, :], batch=33, r=3)
    assert bits(got["bm"]) == bits(np.tile(one["bm"], (1, 4)))
    # N is no multiple of b: the head is dropped, the batches cover the last a b draws
    x = rng.standard_normal((2, 2, 107))
    got = bm.batch_means_host(x, batch=10, r=1)
    poisoned = x.copy()
    poisoned[:, :, :7] = np.nan
    again = bm.batch_means_host(poisoned, batch=10, r=1)
    assert got["a"] == 10 and bits(again["bm"]) == bits(got["bm"]) and bits(again["mu"]) == bits(got["mu"])
    assert np.allclose(got["mu"], x[:, :, 7:].mean(axis=(1, 2)), rtol=1e-12, atol=1e-15)
    # a parameter alone and in a batch
    assert bits(bm.batch_means_host(x[1:], batch=10, r=1)["bm"]) == bits(got["bm"][1:])
    # NaN propagates
    poisoned[0, 1, 50] = np.nan
    r = bm.batch_means_host(poisoned, batch=10, r=1)
    assert np.isnan(r["mu"][0]) and np.isnan(r["bm"][0]).sum() == 1 and np.isfinite(r["bm"][1]).all()


def test_batch_size_rule(bm):
    for N in (1, 2, 3, 8, 9, 10, 35, 36, 80, 81, 99, 100, 1000, 2000, 10 ** 6, 10 ** 6 - 1, 2 ** 40 + 1):
        b, a = bm.batch_size(N, 1)
        assert b == math.isqrt(N) and a == N // b, N
        if N >= 3:
            b, a = bm.batch_size(N, 3)
            assert b == 3 * max(1, math.isqrt(N) // 3) and b <= N and a == N // b, N
    assert bm.batch_size(1000, 3) == (30, 33) and bm.batch_size(2000, 3) == (42, 47) and bm.batch_size(3, 3) == (3, 1)


def test_finish_and_pool_host_in_bits(bm):
    rng = np.random.default_rng(3)
    be = bm._Host()
    P = 7
    g = rng.standard_normal((P, 3 * P))
    cb, cb3 = g @ g.T, (g * 1.1) @ g.T
    for r, b, A, A3 in ((1, 5, 40, 0), (3, 6, 40, 121), (3, 3, 2, 6), (1, 1, 2, 0)):
        got = be.finish(cb, cb3 if r == 3 else None, P, b, A, A3, r)
        assert bits(got) == bits(restate_finish(cb, cb3, b, A, A3, r)), (r, b, A)
    assert np.isnan(be.finish(cb, None, P, 4, 1, 0, 1)).all()                       # A < 2
    sr, sa = cb, cb3 + np.eye(P)
    mur, mua = rng.standard_normal(P), rng.standard_normal(P)
    for drop in ((), (0,), (3,), (P - 1,), (0, 3, P - 1)):
        scale = rng.uniform(0.5, 2.0, P)
        scale[list(drop)] = 0.0
        for jitter in (0.0, 1e-3):
            v, d, z, n = be.pool(sr, mur, 900, sa, mua, 1700, P, scale, jitter)
            wv, wd, wz = restate_pool(sr, mur, 900, sa, mua, 1700, scale, jitter)
            assert n == P - len(drop) and bits(v) == bits(wv) and bits(d) == bits(wd) and bits(z) == bits(wz), (drop, jitter)
        v, d, z, n = be.pool(sr, mur, 1, None, None, 1, P, scale, 0.0)                 # one matrix alone
        wv, wd, wz = restate_pool(sr, mur, 1, None, None, 1, scale, 0.0)
        assert bits(v) == bits(wv) and bits(d) == bits(wd) and bits(z) == bits(wz)
    v, d, z, n = be.pool(sr, mur, 9, sa, mua, 7, P, None, 0.0)                         # NULL scale: all ones
    assert n == P and bits(v) == bits(restate_pool(sr, mur, 9, sa, mua, 7, None, 0.0)[0])
    assert be.pool(sr, mur, 9, sa, mua, 7, P, np.zeros(P), 0.0)[3] == 0
    y = rng.standard_normal(2049)
    assert bits(bm.tree_sum_host(y, squares=True)) == bits(tree_sum(y * y)) and bits(bm.tree_sum_host(y)) == bits(tree_sum(y))
    assert bm.tree_sum_host(np.zeros(0)) == 0.0


# ---- against long double --------------------------------------------------------------------------------------------------

def test_the_cases_are_well_conditioned():
    for P in E2E_P:
        want = e2e_case(P)[5]
        assert want["dof"] == P and np.linalg.cond(want["V"]) <= 1e3, (P, np.linalg.cond(want["V"]))


def test_host_against_long_double(bm):
    from scipy.stats import chi2
    from mcmc_ref_hip._hostdefs import chi2_sf
    for P in E2E_P:
        ref, act, scale, b_ref, b_act, want = e2e_case(P)
        got = bm.mean_shift_test_host(ref, act, scale=scale, r=3, batch_ref=b_ref, batch_act=b_act)
        check_mean_test(got, want, P)
        assert (got["b_ref"], got["a_ref"], got["b_act"], got["a_act"]) == (6, 334, 9, 333)
        assert got["p_value"] == chi2_sf(got["T"], P) and abs(got["p_value"] - float(chi2.sf(want["T"], P))) <= 1e-7
    ref, act, scale, b_ref, _, want = e2e_case(17)
    lr = bm.long_run_covariance_host(ref, batch=b_ref, r=3)
    live = scale > 0
    s = scale[live]
    sig = lr["sigma"][np.ix_(live, live)] * s[:, None] * s[None, :]
    assert np.abs(sig - want["sigma_ref"]).max() <= RTOL * np.abs(want["sigma_ref"]).max()
    assert lr["info"] == 0 and (lr["b"], lr["a"]) == (6, 334)
    assert np.allclose(lr["mcse_mean"], np.sqrt(np.diag(lr["sigma"]) / (3 * 334 * 6)), rtol=1e-15)
    assert np.allclose(lr["ess_bm"], 3 * 2004 * np.diag(lr["lambda"]) / np.diag(lr["sigma"]), rtol=1e-15)
    m = bm.multi_ess_host(ref, batch=b_ref, r=3, scale=scale)
    assert m["p_live"] == 17 and close(m["mess"], want["mess_ref"])
    one = bm.multi_ess_host(ref, batch=b_ref, r=1, scale=scale)                       # the plain estimator: another number
    sig1 = lrv_ld(ref, b_ref, 1)[0][np.ix_(live, live)] * s[:, None] * s[None, :]
    assert close(one["logdet_sigma"], float(logdet_ld(sig1)))


# ---- edges ----------------------------------------------------------------------------------------------------------------

def test_edges(bm):
    rng = np.random.default_rng(5)
    mix = np.linalg.cholesky(spd(3, 5.0, seed=1))
    x, y = ar1(rng, mix, 4, 60, 0.3), ar1(rng, mix, 5, 48, 0.3)
    # b = 1: every draw is a batch; b = N: one batch per chain, A = C
    r = bm.batch_means_host(x, batch=1, r=1)
    assert r["a"] == 60 and r["bm"].shape == (3, 240) and np.allclose(r["bm"], x.reshape(3, -1), rtol=1e-13, atol=1e-15)
    r = bm.batch_means_host(x, batch=60, r=1)
    assert r["a"] == 1 and r["bm"].shape == (3, 4)
    t = bm.mean_shift_test_host(x, y, r=1, batch_ref=60, batch_act=48, mess=False)
    assert t["info"] == 0 and math.isfinite(t["T"]) and t["dof"] == 3              # A - 1 = 3 and 4 >= P_live
    # C = 1 with a = 1: A < 2, Sigma is NaN and the factor reports its first pivot
    lr = bm.long_run_covariance_host(x[:, :1], batch=60, r=1)
    assert np.isnan(lr["sigma"]).all() and lr["info"] == 1 and np.isnan(lr["mcse_mean"]).all()
    t = bm.mean_shift_test_host(x[:, :1], y, r=1, batch_ref=60, batch_act=4, mess=False)
    assert t["info"] == 1 and math.isnan(t["T"]) and math.isnan(t["p_value"]) and np.isnan(t["shift"]).all()
    # a constant parameter: exactly its value, exactly zero variance, the singular info names it
    flat = x.copy()
    flat[1] = 3.7
    lr = bm.long_run_covariance_host(flat, batch=6, r=3)
    assert lr["mu"][1] == 3.7 and not lr["sigma"][1].any() and not lr["sigma"][:, 1].any() and lr["info"] == 2
    assert bits(bm.batch_means_host(flat, batch=6)["bm"][1]) == bits(np.full(40, 3.7))
    t = bm.mean_shift_test_host(flat, flat, r=3, batch_ref=6, batch_act=6, mess=False)
    assert t["info"] == 2 and math.isnan(t["T"])
    t = bm.mean_shift_test_host(flat, flat, r=3, batch_ref=6, batch_act=6, mess=False, jitter=1e-6)
    assert t["info"] == 0 and t["T"] == 0.0 and t["p_value"] == 1.0
    s = np.ones(3)
    s[1] = 0.0                                               # scale 0 drops it
    t = bm.mean_shift_test_host(flat, flat + 0.0, scale=s, r=3, batch_ref=6, batch_act=6)
    assert t["info"] == 0 and t["dof"] == 2 and t["T"] == 0.0 and t["p_value"] == 1.0 and t["z"].shape == (2,)
    # A - 1 < P_live: certainly singular
    wide = ar1(rng, np.eye(6), 1, 40, 0.3)
    t = bm.mean_shift_test_host(wide, wide, r=1, batch_ref=10, batch_act=10, mess=False)
    assert t["dof"] == 6 and 1 <= t["info"] <= 5 and math.isnan(t["T"]) and math.isnan(t["p_value"])
    # r = 3 wants b divisible by 3
    with pytest.raises(ValueError, match="divisible by 3"):
        bm.mean_shift_test_host(x, y, r=3, batch_ref=10)
    with pytest.raises(ValueError, match="1 or 3"):
        bm.batch_means_host(x, r=2)
    # the reference against itself
    t = bm.mean_shift_test_host(x, x, r=3, batch_ref=6, batch_act=6, mess=False)
    assert t["T"] == 0.0 and t["p_value"] == 1.0 and not t["z"].any()


def test_refusals_name_their_cause(built_lib):  # noqa: F811
    from mcmc_ref_hip import _abi, _babi
    lib = _babi.load_bm_library()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    x, bmo, mu = np.ones(24), np.zeros(24), np.zeros(4)

    def refused(rc, cause):
        msg = (lib.mcb_last_error(None) or b"").decode()
        assert rc == _abi.MCR_EINVAL and cause in msg, (rc, cause, msg)

    means = lib.mcb_batch_means_host
    ok = (_abi.MCR_F64, 2, 6, 2, 6, 1, 12)                   # dtype, C, N, P, strides of [P][C][N]
    assert means(vp(x), *ok, 3, dp(bmo), 4, dp(mu)) == _abi.MCR_OK
    refused(means(None, *ok, 3, dp(bmo), 4, dp(mu)), "NULL")
    refused(means(vp(x), *ok, 3, None, 4, None), "NULL")
    refused(means(vp(x), 7, *ok[1:], 3, dp(bmo), 4, dp(mu)), "dtype")
    for bad in ((0, 6, 2), (2, 0, 2), (2, 6, 0)):
        refused(means(vp(x), _abi.MCR_F64, *bad, 6, 1, 12, 3, dp(bmo), 4, dp(mu)), ">= 1")
    refused(means(vp(x), *ok, 0, dp(bmo), 4, dp(mu)), "outside [1, N")
    refused(means(vp(x), *ok, 7, dp(bmo), 4, dp(mu)), "outside [1, N")
    for i in (4, 5, 6):
        neg = list(ok)
        neg[i] = -1
        refused(means(vp(x), *neg, 3, dp(bmo), 4, dp(mu)), "negative stride")
    refused(means(vp(x), *ok, 3, dp(bmo), 3, dp(mu)), "ld = 3")
    assert means(vp(x), *ok, 3, None, 0, dp(mu)) == _abi.MCR_OK                       # ld is bm's
    b, a = C.c_int64(0), C.c_int64(0)
    refused(lib.mcb_batch_size(10, 3, None, C.byref(a)), "NULL")
    refused(lib.mcb_batch_size(0, 1, C.byref(b), C.byref(a)), "N must be >= 1")
    refused(lib.mcb_batch_size(10, 2, C.byref(b), C.byref(a)), "neither 1 nor 3")
    refused(lib.mcb_batch_size(2, 3, C.byref(b), C.byref(a)), "N >= 3")
    m = np.eye(2).ravel()
    fin = lib.mcb_lrv_finish_host
    refused(fin(None, None, 2, 3, 4, 0, 1, dp(m)), "NULL")
    refused(fin(dp(m), None, 2, 3, 4, 12, 3, dp(m)), "NULL")
    refused(fin(dp(m), dp(m), 2, 4, 4, 12, 3, dp(m)), "divisible by 3")
    refused(fin(dp(m), dp(m), 2, 3, 4, 12, 2, dp(m)), "neither 1 nor 3")
    refused(fin(dp(m), dp(m), 0, 3, 4, 12, 3, dp(m)), "P must be >= 1")
    refused(fin(dp(m), dp(m), 2, 0, 4, 12, 1, dp(m)), "b and A")
    pool = lib.mcb_pool_host
    v, d, z, s, pl = np.zeros(4), np.zeros(2), np.zeros(2), np.ones(2), C.c_int64(0)
    args = lambda sc, jit: (dp(m), dp(d), 5, dp(m), dp(d), 5, 2, sc, jit, dp(v), dp(d), dp(z), C.byref(pl))  # noqa: E731
    assert pool(*args(dp(s), 0.0)) == _abi.MCR_OK and pl.value == 2
    for sc in (-s, s * np.inf, s * np.nan):
        refused(pool(*args(dp(sc), 0.0)), "scale 0 must be finite and >= 0")
    for jit in (-1.0, math.inf, math.nan):
        refused(pool(*args(dp(s), jit)), "jitter must be finite and >= 0")
    refused(pool(None, dp(d), 5, dp(m), dp(d), 5, 2, None, 0.0, dp(v), dp(d), dp(z), C.byref(pl)), "NULL")
    refused(pool(dp(m), dp(d), 5, dp(m), None, 5, 2, None, 0.0, dp(v), dp(d), dp(z), C.byref(pl)), "NULL")
    refused(pool(dp(m), dp(d), 0, dp(m), dp(d), 5, 2, None, 0.0, dp(v), dp(d), dp(z), C.byref(pl)), "M_ref and M_act")
    refused(lib.mcb_tree_sum_host(dp(s), -1, 0, dp(v)), "n must be >= 0")
    refused(lib.mcb_tree_sum_host(dp(s), 2, 0, None), "NULL")
    # the entries that take a handle refuse a NULL one without touching a device
    assert lib.mcb_set_workspace_limit(None, 1) == _abi.MCR_EINVAL and lib.mcb_kernel_ms(None, dp(v), 6) == _abi.MCR_EINVAL
    assert lib.mcb_batch_means_dev(None, vp(x), *ok, 3, None, 4, None) == _abi.MCR_EINVAL
    assert lib.mcb_version() == _babi.MCB_VERSION


# ---- the mirror of the header, and the library's exports --------------------------------------------------------------------

BDEFINE = re.compile(r"^[ \t]*#define[ \t]+(MCB_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", re.M)
BDECLARATION = re.compile(DECLARATION.pattern.replace("mcr_", "mcb_"), re.M)


@pytest.fixture(scope="module")
def bheader() -> str:
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mcmcref_bm.h").read_text(), flags=re.S)


def test_mirror_constants(bheader):
    from mcmc_ref_hip import _babi
    defines = {k: int(v) for k, v in BDEFINE.findall(bheader)}
    mirrored = {k: v for k, v in vars(_babi).items() if k.startswith("MCB_") and isinstance(v, int)}
    assert mirrored == defines and len(defines) == 9
    assert defines["MCB_BLOCK"] == BLOCK and defines["MCB_KERNELS"] == len(_babi.KERNEL_NAMES)
    assert [defines[f"MCB_KERNEL_{k.upper()}"] for k in _babi.KERNEL_NAMES] == list(range(defines["MCB_KERNELS"]))
    assert "typedef" not in bheader and "struct" not in bheader
    text = (ROOT / "include" / "mcmcref_bm.h").read_text()
    assert "ASYMPTOTIC" in text and "replicated multivariate batch-means" in text and "not compared against" in text


def test_mirror_functions_and_exports(bheader, built_lib):  # noqa: F811
    from mcmc_ref_hip import _babi
    named = set(re.findall(r"\b(mcb_[a-z0-9_]+)\s*\(", bheader))
    parsed = {m.group(2): (m.group(1), m.group(3)) for m in BDECLARATION.finditer(bheader)}
    assert named == set(parsed) == set(_babi.BSYMBOLS) and len(named) == 17
    lib = _babi.load_bm_library()
    for name, (ret, params) in sorted(parsed.items()):
        restype, argtypes = _babi.BSYMBOLS[name]
        params = [p for p in params.split(",") if p.strip() != "void"]
        assert [py_class(t) for t in argtypes] == [c_class(p) for p in params], name
        assert py_class(restype) == c_class(ret), name
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype is restype, name
    third = built_lib.with_name("libmcmcref_bm.so")
    assert third.exists()
    nm = shutil.which("nm")
    if nm is not None:
        out = subprocess.run([nm, "-D", "--defined-only", str(third)], check=True, capture_output=True, text=True).stdout
        assert {line.split()[-1] for line in out.splitlines() if line.split()} == named        # mcb_* and nothing else


def test_ffi_knows_nothing_of_batch_means():
    from mcmc_ref_hip import _babi, _ffi, _iabi, _xabi, batchmeans
    assert not [k for k, v in vars(_ffi).items() if v is _babi or v is batchmeans]
    assert not [k for k in vars(_ffi) if k.lower().startswith(("mcb", "batch_means", "mean_shift", "multi_ess", "long_run"))]
    assert not set(_ffi.SYMBOLS) & set(_babi.BSYMBOLS)
    assert not set(_babi.BSYMBOLS) & (set(_iabi.ISYMBOLS) | set(_xabi.XSYMBOLS))
    for header in ("mcmcref_hip.h", "mcmcref_hip_ext.h", "mcmcref_iess.h"):
        assert "mcb_" not in (ROOT / "include" / header).read_text().lower()


def test_build_units():
    import importlib.util
    spec = importlib.util.spec_from_file_location("mcr_build_bm", ROOT / "mcmc-db_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.BM_UNITS == ("mcb_api",) and "-ffp-contract=off" in mod.IESS_FLAGS
    assert mod.BM_OUT.name == "libmcmcref_bm.so" and (ROOT / "mcmc-db_amd" / "csrc" / "mcb_exports.map").exists()


# ---- calibration ------------------------------------------------------------------------------------------------------------

CAL_PAIRS, CAL_P, CAL_SEED = 40, 8, 4711


@functools.lru_cache(maxsize=None)
def calibration_pairs() -> tuple:
    """The 40 pairs of the calibration: AR(1) chains with phi = 0.9 from one correlated 8-parameter distribution, 10 x 1000
    draws against 4 x 2000, seed 4711.  (ref, act, scale) each; read only."""
    rng = np.random.default_rng(CAL_SEED)
    mix = np.linalg.cholesky(spd(CAL_P, 20.0, seed=CAL_SEED))
    out = []
    for _ in range(CAL_PAIRS):
        ref, act = ar1(rng, mix, 10, 1000), ar1(rng, mix, 4, 2000)
        scale = 1.0 / ref.reshape(CAL_P, -1).std(axis=1)
        for a in (ref, act, scale):
            a.setflags(write=False)
        out.append((ref, act, scale))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def calibration_host(i: int) -> dict:
    from mcmc_ref_hip import batchmeans
    ref, act, scale = calibration_pairs()[i]
    return batchmeans.mean_shift_test_host(ref, act, scale=scale, r=3)


def test_calibration(bm):
    from scipy.stats import chi2
    p, naive, mess_ref, mess_act = [], [], [], []
    for i, (ref, act, scale) in enumerate(calibration_pairs()):
        t = calibration_host(i)
        assert t["info"] == 0 and (t["b_ref"], t["b_act"]) == (30, 42)
        p.append(t["p_value"])
        mess_ref.append(t["mess_ref"])
        mess_act.append(t["mess_act"])
        # the same statistic with the sample covariance in place of the long-run covariance
        xr, xa = ref.reshape(CAL_P, -1) * scale[:, None], act.reshape(CAL_P, -1) * scale[:, None]
        V = np.cov(xr, ddof=0) / xr.shape[1] + np.cov(xa, ddof=0) / xa.shape[1]
        d = xa.mean(axis=1) - xr.mean(axis=1)
        naive.append(float(chi2.sf(d @ np.linalg.solve(V, d), CAL_P)))
    print("pairs with p < 0.01:", sum(v < 0.01 for v in p), "naive:", sum(v < 0.01 for v in naive),
          "mean mESS:", np.mean(mess_ref), np.mean(mess_act))
    assert sum(v < 0.01 for v in p) <= 4
    assert sum(v < 0.01 for v in naive) >= 36
    for got, M in ((np.mean(mess_ref), 10000), (np.mean(mess_act), 8000)):
        truth = M * (1 - PHI) / (1 + PHI)
        assert truth / 1.5 <= got <= truth * 1.5, (got, truth)
    sd = np.sqrt(np.diag(np.linalg.cholesky(spd(CAL_P, 20.0, seed=CAL_SEED)) @ np.linalg.cholesky(spd(CAL_P, 20.0, seed=CAL_SEED)).T))
    for i in range(10):                                      # one parameter moved by half a standard deviation
        ref, act, scale = calibration_pairs()[i]
        moved = act.copy()
        moved[i % CAL_P] += 0.5 * sd[i % CAL_P]
        t = bm.mean_shift_test_host(ref, moved, scale=scale, r=3, mess=False)
        assert t["info"] == 0 and t["p_value"] < 1e-6, (i, t["p_value"])


# ---- the commands -----------------------------------------------------------------------------------------------------------

def test_commands_take_the_options():
    from click.testing import CliRunner
    from mcmc_ref_hip.cli import main
    out = CliRunner().invoke(main, ["multi-ess", "--help"])
    assert out.exit_code == 0 and all(opt in out.output for opt in ("--params", "--batch", "--r", "--format"))
    out = CliRunner().invoke(main, ["mean-test", "--help"])
    assert out.exit_code == 0 and all(opt in out.output for opt in ("--params", "--jitter", "--p-min", "--format"))
    assert CliRunner().invoke(main, ["multi-ess", "no_such_file.csv"]).exit_code != 0
    assert CliRunner().invoke(main, ["mean-test", "no_such_file.csv", "neither.csv"]).exit_code != 0
    assert CliRunner().invoke(main, ["multi-ess", __file__, "--r", "2"]).exit_code != 0


def test_result_type():
    import dataclasses
    from mcmc_ref_hip.validate import MeanShiftValidateResult, validate_mean_shift
    assert [f.name for f in dataclasses.fields(MeanShiftValidateResult)] == ["passed", "test", "p_value", "failures"]
    assert MeanShiftValidateResult.__dataclass_params__.frozen and callable(validate_mean_shift)

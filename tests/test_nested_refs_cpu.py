"""Nested R-hat: the reference in numpy, pinned on the CPU, and the inputs of tests/test_nested_gpu.py.

`nested_reference(v, ids, dtype)` is the specification of mcr_nested_rhat (include/mcmcref_hip.h) for one kind of value, in
float64 or longdouble, every variance two-pass.  The rank-normalised kinds are built with the helpers pinned in
tests/test_rank_refs_cpu.py (`rank_codes`, `fold`, `z_of_codes`: CPython's own `inv_cdf`).  The tests hold the reference to a
literal transcription of posterior::rhat_nested, to hand-sized cases and to every branch, and check that the input builders
do what the GPU file relies on: sums with one right answer, a separating pair, superchains that remember their starts.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import pytest

from test_rank_refs_cpu import fold, rank_codes, z_of_codes

KINDS = ("raw", "bulk", "tail")

# ---------------------------------------------------------------------------------------------------------------------
# The reference
# ---------------------------------------------------------------------------------------------------------------------


def nested_reference(v, ids, dtype=np.float64) -> tuple[float, float, float]:
    """(nrhat, B, W) of the values v[C][N] with chain c in superchain ids[c], all arithmetic in `dtype`."""
    v = np.asarray(v, dtype=dtype)
    ids = np.asarray(ids)
    C, N = v.shape
    nan = float("nan")
    labels = np.unique(ids)
    K = labels.size
    if C * N == 0:
        return nan, nan, nan
    L = C // K
    assert all(np.count_nonzero(ids == g) == L for g in labels), "superchains of unequal size"
    m = v.sum(axis=1) / dtype(N)                               # chain means
    q = ((v - m[:, None]) ** 2).sum(axis=1)                    # squared deviations from them
    mu_k, t_k = [], []
    for g in labels:
        mk, qk = m[ids == g], q[ids == g]
        mu = mk.sum() / dtype(L)
        b = ((mk - mu) ** 2).sum()
        w = qk.sum()
        tb = b / dtype(L - 1) if L > 1 else dtype(0)
        tw = w / (dtype(L) * dtype(N - 1)) if N > 1 else dtype(0)
        mu_k.append(mu)
        t_k.append(tb + tw)
    mu_k, t_k = np.asarray(mu_k, dtype=dtype), np.asarray(t_k, dtype=dtype)
    W = t_k.sum() / dtype(K)
    if K < 2:
        return nan, nan, float(W)
    mu = mu_k.sum() / dtype(K)
    B = ((mu_k - mu) ** 2).sum() / dtype(K - 1)
    if W == 0:
        r = 1.0 if B == 0 else float("inf")
    else:
        r = float(np.sqrt(dtype(1) + B / W))
    return r, float(B), float(W)


def kinds_of(x) -> dict[str, np.ndarray]:
    """The three kinds of value of the draws x[C][N]: the draws, z of the pooled ranks, z of the ranks of |x - median|."""
    x = np.asarray(x, dtype=np.float64)
    M = x.size
    flat = x.reshape(-1)
    return {"raw": x,
            "bulk": z_of_codes(rank_codes(flat), M).reshape(x.shape),
            "tail": z_of_codes(rank_codes(fold(flat)[0]), M).reshape(x.shape)}


def pymax(a: float, b: float) -> float:
    return b if b > a else a


def nested_all(x, ids, dtype=np.float64) -> dict[str, float]:
    """Every output of mcr_nested_rhat for one parameter."""
    out = {}
    for kind, v in kinds_of(x).items():
        r, B, W = nested_reference(v, ids, dtype)
        out[f"nrhat_{kind}"], out[f"between_{kind}"], out[f"within_{kind}"] = r, B, W
    out["nrhat"] = pymax(out["nrhat_bulk"], out["nrhat_tail"])
    return out


def posterior_rhat_nested(x, ids) -> float:
    """posterior::rhat_nested, line by line: var of the superchain means over the mean over superchains of (var of the
    chain means + mean of the chain vars), every var with ddof = 1, a var of one value taken as 0."""
    x = np.asarray(x, dtype=np.float64)
    ids = np.asarray(ids)
    C, N = x.shape
    chain_mean = x.mean(axis=1)
    chain_var = x.var(axis=1, ddof=1) if N > 1 else np.zeros(C)
    labels = np.unique(ids)
    L = C // labels.size
    superchain_mean = np.array([chain_mean[ids == g].mean() for g in labels])
    var_chain_in_superchain = np.array([chain_mean[ids == g].var(ddof=1) if L > 1 else 0.0 for g in labels])
    var_within_chain = np.array([chain_var[ids == g].mean() for g in labels])
    var_superchain = superchain_mean.var(ddof=1)
    var_within_superchain = (var_chain_in_superchain + var_within_chain).mean()
    return float(np.sqrt(1.0 + var_superchain / var_within_superchain))


# ---------------------------------------------------------------------------------------------------------------------
# Inputs
# ---------------------------------------------------------------------------------------------------------------------


def block_ids(C: int, K: int) -> np.ndarray:
    return np.repeat(np.arange(K, dtype=np.int32), C // K)


def exact_sums(C: int, N: int, seed: int = 1) -> np.ndarray:
    """x = 2^27 + j / 8, j an integer in [-64, 64]: with N and L powers of two every sum, mean and squared deviation of the
    statistic is exact in float64, so m_c, q_c, b_k, w_k have one right answer whatever the order of summation."""
    rng = np.random.default_rng(seed)
    return 2.0 ** 27 + rng.integers(-64, 65, size=(C, N)).astype(np.float64) / 8.0


SEP_C, SEP_N, SEP_K = 512, 20, 16


def separating(seed: int = 7) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(good, bad, ids): 512 x 20 standard normal draws with interleaved labels c % 16; `bad` has superchain 3 shifted by +3."""
    rng = np.random.default_rng(seed)
    good = rng.normal(size=(SEP_C, SEP_N))
    ids = (np.arange(SEP_C) % SEP_K).astype(np.int32)
    bad = good.copy()
    bad[ids == 3] += 3.0
    return good, bad, ids


def starts_remembered(seed: int = 11) -> tuple[np.ndarray, np.ndarray]:
    """(x, ids): AR(1) chains with phi = 0.99 (stationary sd 7.1), 512 x 20, the 32 chains of a superchain started at one
    point drawn three times as wide as the target, N(0, 21.3^2): twenty draws later every superchain still sits at its start."""
    rng = np.random.default_rng(seed)
    phi, sd = 0.99, 1.0 / math.sqrt(1.0 - 0.99 ** 2)
    ids = block_ids(SEP_C, SEP_K)
    x = np.empty((SEP_C, SEP_N))
    cur = (rng.normal(size=SEP_K) * 3.0 * sd)[ids]
    for n in range(SEP_N):
        cur = phi * cur + rng.normal(size=SEP_C)
        x[:, n] = cur
    return x, ids


# ---------------------------------------------------------------------------------------------------------------------
# Tests of the reference
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("C,N,K,interleave", [(8, 10, 2, False), (12, 5, 3, True), (64, 16, 8, True), (30, 7, 10, False)])
def test_reference_equals_posterior_transcription(C, N, K, interleave):
    rng = np.random.default_rng(C * 1000 + N)
    x = rng.normal(size=(C, N)) + 0.3 * rng.normal(size=(C, 1))
    ids = (np.arange(C) % K) if interleave else block_ids(C, K)
    for dtype in (np.float64, np.longdouble):
        r, _, _ = nested_reference(x, ids, dtype)
        assert abs(r - posterior_rhat_nested(x, ids)) <= 1e-12 * r


def test_by_hand():
    # two superchains of two chains of two draws
    x = np.array([[0.0, 2.0], [2.0, 4.0], [10.0, 12.0], [12.0, 14.0]])
    ids = [0, 0, 1, 1]
    # chain means 1 3 11 13, q_c = 2 each; mu_k = 2, 12; b_k = 2, 2; w_k = 4, 4; T_k = 2 / 1 + 4 / (2 * 1) = 4
    # mu = 7, B = (25 + 25) / 1 = 50, W = 4
    r, B, W = nested_reference(x, ids)
    assert (B, W) == (50.0, 4.0) and r == math.sqrt(1.0 + 50.0 / 4.0)
    # labels are names only: any relabelling, any order
    assert nested_reference(x[[2, 0, 3, 1]], [7, -2, 7, -2]) == (r, B, W)


def test_branches():
    nan = float("nan")
    const = np.full((8, 4), 2.5)
    assert nested_reference(const, block_ids(8, 4)) == (1.0, 0.0, 0.0)
    levels = np.repeat(np.arange(4.0), 2)[:, None] * np.ones((8, 4))               # constant chains, a level per superchain
    r, B, W = nested_reference(levels, block_ids(8, 4))
    assert r == float("inf") and W == 0.0 and B > 0.0
    r, B, W = nested_reference(np.random.default_rng(0).normal(size=(8, 4)), np.zeros(8, dtype=int))      # K = 1
    assert r != r and B != B and W > 0.0
    x1 = np.random.default_rng(1).normal(size=(8, 1))                              # N = 1: W is the spread of the chain means
    r, B, W = nested_reference(x1, block_ids(8, 4))
    assert W == np.mean([x1[2 * k:2 * k + 2, 0].var(ddof=1) for k in range(4)]) and r == math.sqrt(1.0 + B / W)
    xl = np.random.default_rng(2).normal(size=(8, 16))                             # L = 1: W is the mean chain variance
    r, B, W = nested_reference(xl, np.arange(8))
    assert abs(W - xl.var(axis=1, ddof=1).mean()) <= 1e-15 * W
    assert abs(B - xl.mean(axis=1).var(ddof=1)) <= 1e-15 * B
    assert all(v != v for v in nested_reference(np.empty((4, 0)), block_ids(4, 2)))
    assert nan != nan


def test_exact_sums_have_one_right_answer():
    x = exact_sums(64, 16)
    ids = block_ids(64, 8)
    base = nested_reference(x, ids)
    assert base == nested_reference(x, ids, np.longdouble)                         # nothing was rounded on the way to B and W's terms
    rng = np.random.default_rng(5)
    for _ in range(4):                                                              # any order of the draws: the same bits
        shuffled = np.stack([row[rng.permutation(16)] for row in x])
        assert nested_reference(shuffled, ids) == base
    # the one-pass form Q - S m loses everything at this offset
    S, Q = x.sum(axis=1), (x * x).sum(axis=1)
    q_two = ((x - (S / 16)[:, None]) ** 2).sum(axis=1)
    q_one = Q - S * (S / 16)
    assert np.max(np.abs(q_one - q_two) / q_two) > 0.1


def test_separating_pair():
    good, bad, ids = separating()
    g, b = nested_all(good, ids), nested_all(bad, ids)
    for kind in KINDS:
        assert g[f"nrhat_{kind}"] < 1.01, (kind, g)
        assert b[f"nrhat_{kind}"] > 1.1, (kind, b)
    assert g["nrhat"] < 1.01 and b["nrhat"] > 1.1


def test_starts_remembered():
    x, ids = starts_remembered()
    assert nested_reference(x, ids)[0] > 2.0


# ---------------------------------------------------------------------------------------------------------------------
# Signatures (no GPU: every one of these answers before a device is touched)
# ---------------------------------------------------------------------------------------------------------------------


def test_diagnostics_value_errors():
    from mcmc_ref_hip import diagnostics
    chains = [[1.0, 2.0, 3.0]] * 4
    with pytest.raises(ValueError, match="chains of equal length"):
        diagnostics.nested_rhat([[1.0, 2.0, 3.0], [1.0, 2.0]] * 2, [0, 0, 1, 1])
    with pytest.raises(ValueError, match="same number of chains"):
        diagnostics.nested_rhat(chains, [0, 0, 0, 1])
    with pytest.raises(ValueError, match="one label per chain: got 3 for 4 chains"):
        diagnostics.nested_rhat(chains, [0, 0, 1])
    with pytest.raises(ValueError, match="3 superchains do not divide 4 chains"):
        diagnostics.nested_rhat(chains, 3)
    assert math.isnan(diagnostics.nested_rhat(chains, [5, 5, 5, 5]))               # fewer than two superchains
    assert math.isnan(diagnostics.nested_rhat(chains, 1))


def test_int_shorthand():
    from mcmc_ref_hip import _ffi
    assert _ffi.superchain_labels(3, 12).tolist() == [0] * 4 + [1] * 4 + [2] * 4
    assert _ffi.superchain_labels(12, 12).tolist() == list(range(12))
    got = _ffi.superchain_labels([7, -2, 100, 7, -2, 100], 6)
    assert got.dtype == np.int32 and got.tolist() == [7, -2, 100, 7, -2, 100]
    for bad in (0, 5, -1):
        with pytest.raises(ValueError):
            _ffi.superchain_labels(bad, 12)
    with pytest.raises(ValueError, match="int32"):
        _ffi.superchain_labels([0, 2 ** 31], 2)


def test_null_context_answers_einval():
    from mcmc_ref_hip import _ffi
    lib = _ffi.load_library()
    x = np.zeros((1, 4, 4))
    ids = np.zeros(4, dtype=np.int32)
    out = _ffi.Nested()
    for fn in (lib.mcr_nested_rhat, lib.mcr_nested_rhat_dev):
        rc = fn(None, x.ctypes.data_as(ctypes.c_void_p), *_ffi.tensor_args(x, "pcn"), ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                ctypes.byref(out))
        assert rc == _ffi.MCR_EINVAL
        assert lib.mcr_last_error(None) == b"ctx is NULL"

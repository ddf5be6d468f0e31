"""Batch means, the long-run covariance of the Markov-chain central limit theorem, the multivariate effective sample size
and a calibrated joint test of two samples' means.  The entries of include/mcmcref_bm.h (`mcb_*`, mirrored by `_babi`) as
free functions; they live in the companion library libmcmcref_bm.so.  The covariance, the Cholesky factor and the
triangular solve are the main library's (`mcr_covariance_dev`, `mcrx_cholesky_dev`, `mcrx_solve_lower_dev`), reached
through their public entries in the sequence the header documents.

`mean_shift_test(ref, act)` answers "have the means moved?" with a p-value: T = d^T (Sigma_ref / M_ref + Sigma_act /
M_act)^-1 d is asymptotically chi-square with P_live degrees of freedom when they have not, because Sigma is the long-run
covariance -- the sample covariance in its place rejects everything once the draws are autocorrelated.  `multi_ess` is
mESS = C N (det Lambda / det Sigma)^(1 / P) of Vats, Flegal and Jones (2019): how many independent joint draws the sample
is worth.  The estimator is the replicated multivariate batch means, by default in its lugsail form (r = 3).  The numbers
differ from R's mcmcse in which draws are dropped and in the batch-size rule; no parity is claimed.

Every device function takes `context=None` (the calling thread's `_ffi.default_context()`): draws may be a numpy array or a
DeviceTensor of that context, and the companion library gets a handle of its own on the context's device, made at the
first call and freed with the context.  The `*_host` functions are the definitions on the host and need neither.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
import time

import numpy as np

from . import _ffi
from ._abi import _as_dp, tensor_args
from ._babi import BM, KERNEL_NAMES, host_check, load_bm_library
from ._companion import device_tensor
from ._device import DeviceBuffer, DeviceTensor
from ._hostdefs import chi2_sf

_handle = BM.handle                     # Context -> its BmHandle


def batch_size(N: int, r: int = 3) -> tuple[int, int]:
    """(b, a) of mcb_batch_size: the default batch size of chains of N draws and the batches per chain.  r = 1:
    b = floor(sqrt(N)); r = 3 (lugsail): b = 3 max(1, floor(sqrt(N) / 3)), which needs N >= 3."""
    b, a = C.c_int64(0), C.c_int64(0)
    host_check(load_bm_library().mcb_batch_size(int(N), int(r), C.byref(b), C.byref(a)))
    return int(b.value), int(a.value)


def tree_sum_host(y, squares: bool = False) -> float:
    """mcb_tree_sum_host: the sum of y (or of its squares) in the library's summation tree."""
    y = np.ascontiguousarray(y, dtype=np.float64).ravel()
    out = C.c_double(0.0)
    host_check(load_bm_library().mcb_tree_sum_host(_as_dp(y), y.size, int(bool(squares)), C.byref(out)))
    return float(out.value)


def _batch(N: int, batch, r: int) -> int:
    if r not in (1, 3):
        raise ValueError(f"r must be 1 or 3; got {r}")
    b = batch_size(N, r)[0] if batch is None else int(batch)
    if r == 3 and b % 3:
        raise ValueError(f"r = 3 needs a batch size divisible by 3; got {b}")
    return b


def _scale(scale, P: int):
    if scale is None:
        return None
    s = np.ascontiguousarray(scale, dtype=np.float64)
    if s.shape != (P,):
        raise ValueError("scale must have one entry per parameter")
    return s


def _cov_around(x: np.ndarray) -> np.ndarray:
    """The population covariance of the rows of x [P][M] around the means K + mean(x - K), K the first column: a constant
    row has exactly its value as mean and an exactly zero variance (the host's stand-in for mcr_covariance_dev)."""
    k = x[:, :1]
    xc = x - (k + (x - k).mean(axis=1, keepdims=True))
    return (xc @ xc.T) / x.shape[1]


class _Host:
    """The steps on the host: numpy arrays in place of device buffers."""

    def __init__(self, stages=None):
        self.lib, self.stages = load_bm_library(), stages

    def tensor(self, draws, layout):
        x = np.asarray(draws)
        return x, tensor_args(x, layout), layout

    def batch_means(self, t, b: int, want_mu: bool = True):
        x, targs, _ = t
        P, A = targs[3], targs[1] * (targs[2] // b)
        bm, mu = np.full((P, A), np.nan), (np.full(P, np.nan) if want_mu else None)
        host_check(self.lib.mcb_batch_means_host(x.ctypes.data_as(C.c_void_p), *targs, b, _as_dp(bm), A, _as_dp(mu)))
        return bm, mu

    def pooled(self, t):
        x, targs, layout = t
        pcn = np.transpose(x, [layout.index(a) for a in "pcn"])
        return np.ascontiguousarray(pcn, dtype=np.float64).reshape(targs[3], targs[1] * targs[2])

    def cov(self, x, M: int, P: int):
        return _cov_around(x)

    def finish(self, cb, cb3, P, b, A, A3, r):
        out = np.full((P, P), np.nan)
        host_check(self.lib.mcb_lrv_finish_host(_as_dp(np.ascontiguousarray(cb)), _as_dp(None if cb3 is None else np.ascontiguousarray(cb3)),
                                                P, b, A, A3, r, _as_dp(out)))
        return out

    def pool(self, sr, mur, Mr, sa, mua, Ma, P, scale, jitter):
        v, d, z, pl = np.full((P, P), np.nan), np.full(P, np.nan), np.full(P, np.nan), C.c_int64(0)
        host_check(self.lib.mcb_pool_host(_as_dp(sr), _as_dp(mur), Mr, _as_dp(sa), _as_dp(mua), Ma, P, _as_dp(scale), float(jitter),
                                          _as_dp(v), _as_dp(d), _as_dp(z), C.byref(pl)))
        n = int(pl.value)
        return v.ravel()[:n * n].reshape(n, n).copy(), d[:n].copy(), z[:n].copy(), n

    def chol(self, v, n: int):
        from .gaussian import cholesky_host
        L, info, logdet = cholesky_host(v)
        return L, info, logdet

    def solve(self, L, n: int, d):
        from .gaussian import solve_lower_host
        return solve_lower_host(L, d)

    def get(self, a, count: int):
        return np.array(a, dtype=np.float64).ravel()[:count]


class _Dev:
    """The steps on the device: every array is a DeviceBuffer of the context, freed when the call's stack unwinds."""

    def __init__(self, ctx, stack: contextlib.ExitStack, stages=None):
        self.ctx, self.h, self.stack, self.stages = ctx, _handle(ctx), stack, stages

    def buf(self, count: int) -> DeviceBuffer:
        return self.stack.enter_context(DeviceBuffer(self.ctx, max(8 * int(count), 8)))

    def tensor(self, draws, layout):
        t = device_tensor(draws)
        if t is not None:
            return t, t.targs
        t = self.stack.enter_context(self.ctx.upload(np.ascontiguousarray(draws), layout))
        return t, t.targs

    def batch_means(self, t, b: int, want_mu: bool = True):
        dt, targs = t
        P, A = targs[3], targs[1] * (targs[2] // b)
        bm, mu = self.buf(P * A), (self.buf(P) if want_mu else None)
        self.h.check(self.h.lib.mcb_batch_means_dev(self.h.handle, dt.buf.ptr, *targs, b, bm.ptr, A, mu.ptr if mu else None))
        return bm, mu

    def pooled(self, t):
        dt, targs = t
        out = self.buf(targs[1] * targs[2] * targs[3])
        self.h.check(self.h.lib.mcb_pooled_dev(self.h.handle, dt.buf.ptr, *targs, out.ptr, targs[1] * targs[2]))
        return out

    def cov(self, x, M: int, P: int):
        out = self.buf(P * P)
        self.ctx._check(self.ctx.lib.mcr_covariance_dev(self.ctx.handle, x.ptr, M, P, out.ptr))
        return out

    def finish(self, cb, cb3, P, b, A, A3, r):
        self.h.check(self.h.lib.mcb_lrv_finish_dev(self.h.handle, cb.ptr, cb3.ptr if cb3 else None, P, b, A, A3, r, cb.ptr))
        return cb

    def pool(self, sr, mur, Mr, sa, mua, Ma, P, scale, jitter):
        v, d, z, pl = self.buf(P * P), self.buf(P), self.buf(P), C.c_int64(0)
        self.h.check(self.h.lib.mcb_pool_dev(self.h.handle, sr.ptr, mur.ptr, Mr, sa.ptr if sa else None, mua.ptr if mua else None, Ma, P,
                                             _as_dp(scale), float(jitter), v.ptr, d.ptr, z.ptr, C.byref(pl)))
        return v, d, z, int(pl.value)

    def chol(self, v, n: int):
        from .gaussian import cholesky_dev
        info, logdet = cholesky_dev(v.ptr, n, context=self.ctx)
        return v, info, logdet

    def solve(self, L, n: int, d):
        from .gaussian import solve_lower_dev
        solve_lower_dev(L.ptr, n, d.ptr, 1, context=self.ctx)
        return self.get(d, n)

    def get(self, a, count: int):
        return a.download(np.float64, count) if count else np.zeros(0)


def _timed(be, stage: str, fn, *args, **kw):
    """Run a step; with be.stages (a dict) add its wall time in seconds under `stage` (every step is synchronous)."""
    if be.stages is None:
        return fn(*args, **kw)
    t0 = time.perf_counter()
    out = fn(*args, **kw)
    be.stages[stage] = be.stages.get(stage, 0.0) + time.perf_counter() - t0
    return out


def _lrv(be, t, batch, r: int) -> dict:
    """Sigma (in the backend's memory), mu and the batch geometry of one sample."""
    _, C_, N, P = t[1][:4]
    b = _batch(N, batch, r)
    if not 1 <= b <= N:
        raise ValueError(f"batch size {b} is outside [1, N = {N}]")
    a = N // b
    A, A3, cb3 = C_ * a, 0, None
    bm, mu = _timed(be, "batch_means", be.batch_means, t, b)
    cb = _timed(be, "covariance", be.cov, bm, A, P)
    if r == 3:
        A3 = C_ * (N // (b // 3))
        bm3, _ = _timed(be, "batch_means", be.batch_means, t, b // 3, False)
        cb3 = _timed(be, "covariance", be.cov, bm3, A3, P)
    sigma = _timed(be, "finish_pool", be.finish, cb, cb3, P, b, A, A3, r)
    return {"sigma": sigma, "mu": mu, "b": b, "a": a, "A": A, "M": A * b, "C": C_, "N": N, "P": P}


def _lambda(be, t):
    _, C_, N, P = t[1][:4]
    pooled = _timed(be, "pooled", be.pooled, t)
    return _timed(be, "covariance", be.cov, pooled, C_ * N, P)


def _mess(be, lr: dict, lam, scale) -> dict:
    """mESS from Sigma and Lambda on the scaled live matrices."""
    P, M = lr["P"], lr["C"] * lr["N"]
    vs, _, _, n = _timed(be, "finish_pool", be.pool, lr["sigma"], lr["mu"], 1, None, None, 1, P, scale, 0.0)
    vl, _, _, _ = _timed(be, "finish_pool", be.pool, lam, lr["mu"], 1, None, None, 1, P, scale, 0.0)
    if n == 0:
        return {"mess": math.nan, "p_live": 0, "info_sigma": 0, "info_lambda": 0, "logdet_sigma": math.nan, "logdet_lambda": math.nan}
    _, info_s, ld_s = _timed(be, "cholesky", be.chol, vs, n)
    _, info_l, ld_l = _timed(be, "cholesky", be.chol, vl, n)
    ok = info_s == 0 and info_l == 0
    return {"mess": M * math.exp((ld_l - ld_s) / n) if ok else math.nan, "p_live": n, "info_sigma": info_s, "info_lambda": info_l,
            "logdet_sigma": ld_s, "logdet_lambda": ld_l}


def _per_parameter(be, lr: dict, lam) -> dict:
    P = lr["P"]
    sig = be.get(lr["sigma"], P * P).reshape(P, P)
    out = {"sigma": sig, "mu": be.get(lr["mu"], P), "b": lr["b"], "a": lr["a"]}
    with np.errstate(invalid="ignore", divide="ignore"):
        out["mcse_mean"] = np.sqrt(np.diag(sig) / float(lr["M"]))
        if lam is not None:
            out["lambda"] = be.get(lam, P * P).reshape(P, P)
            out["ess_bm"] = lr["C"] * lr["N"] * np.diag(out["lambda"]) / np.diag(sig)
    return out


def _long_run_covariance(be, draws, layout, batch, r) -> dict:
    t = be.tensor(draws, layout)
    lr = _lrv(be, t, batch, r)
    lam = _lambda(be, t)
    out = _per_parameter(be, lr, lam)
    m = _mess(be, lr, lam, None)
    out["info"] = m["info_sigma"]
    return out


def _multi_ess(be, draws, layout, batch, r, scale) -> dict:
    t = be.tensor(draws, layout)
    lr = _lrv(be, t, batch, r)
    lam = _lambda(be, t)
    out = _mess(be, lr, lam, _scale(scale, lr["P"]))
    per = _per_parameter(be, lr, lam)
    out.update(ess_bm=per["ess_bm"], mcse_mean=per["mcse_mean"], mu=per["mu"], b=lr["b"], a=lr["a"])
    return out


def _mean_shift_test(be, ref, act, layout, scale, jitter, r, batch_ref, batch_act, mess) -> dict:
    tr, ta = be.tensor(ref, layout), be.tensor(act, layout)
    if tr[1][3] != ta[1][3]:
        raise ValueError("ref and act must have the same parameters")
    P = tr[1][3]
    s = _scale(scale, P)
    lr, la = _lrv(be, tr, batch_ref, r), _lrv(be, ta, batch_act, r)
    out = {"b_ref": lr["b"], "a_ref": lr["a"], "b_act": la["b"], "a_act": la["a"], "mess_ref": math.nan, "mess_act": math.nan}
    if mess:
        out["mess_ref"] = _mess(be, lr, _lambda(be, tr), s)["mess"]
        out["mess_act"] = _mess(be, la, _lambda(be, ta), s)["mess"]
    v, d, z, n = _timed(be, "finish_pool", be.pool, lr["sigma"], lr["mu"], lr["M"], la["sigma"], la["mu"], la["M"], P, s, jitter)
    out.update(dof=n, z=be.get(z, n), d=be.get(d, n), T=math.nan, p_value=math.nan, info=0, shift=np.full(n, np.nan))
    if n == 0:
        return out
    L, info, _ = _timed(be, "cholesky", be.chol, v, n)
    out["info"] = info
    if info == 0:
        y = _timed(be, "solve", be.solve, L, n, d)
        out["shift"] = y
        out["T"] = tree_sum_host(y, squares=True)
        out["p_value"] = chi2_sf(out["T"], n)
    return out


# ---- the definitions on the host ------------------------------------------------------------------------------------------

def batch_means_host(draws, layout: str = "pcn", batch=None, r: int = 3) -> dict:
    """mcb_batch_means_host: the definition of `batch_means` on the host, without a GPU.  The same bits as the device."""
    be = _Host()
    t = be.tensor(draws, layout)
    b = _batch(t[1][2], batch, r)
    bm, mu = be.batch_means(t, b)
    return {"bm": bm, "mu": mu, "b": b, "a": t[1][2] // b}


def long_run_covariance_host(draws, layout: str = "pcn", batch=None, r: int = 3) -> dict:
    """`long_run_covariance` from the host definitions (numpy for the covariance of the batch means)."""
    return _long_run_covariance(_Host(), draws, layout, batch, r)


def multi_ess_host(draws, layout: str = "pcn", batch=None, r: int = 3, scale=None) -> dict:
    """`multi_ess` from the host definitions."""
    return _multi_ess(_Host(), draws, layout, batch, r, scale)


def mean_shift_test_host(ref, act, scale=None, jitter: float = 0.0, r: int = 3, layout: str = "pcn", batch_ref=None,
                         batch_act=None, mess: bool = True) -> dict:
    """`mean_shift_test` from the host definitions: mcb_*_host, numpy for the covariances, mcrx_cholesky_host and
    mcrx_solve_lower_host."""
    return _mean_shift_test(_Host(), ref, act, layout, scale, jitter, r, batch_ref, batch_act, mess)


# ---- on the device ----------------------------------------------------------------------------------------------------------

def batch_means(draws, layout: str = "pcn", batch=None, r: int = 3, context=None) -> dict:
    """Batch means of every parameter of `draws` (a 3-D numpy array whose axes are `layout`, or a DeviceTensor of the
    context): bm [P][A] (A = C a batch means, chain by chain), mu [P] (the mean of the draws the batches cover), b and a.
    `batch` is the batch size (None: `batch_size(N, r)`); the batches cover the last a b draws of each chain.  One
    streaming pass -- mcb_batch_means(_dev).  Calls `context.sync()` first.  The same bits in any layout and chunking."""
    ctx = context or _ffi.default_context()
    h = _handle(ctx)
    ctx.sync()
    if isinstance(draws, DeviceTensor):
        with contextlib.ExitStack() as stack:
            be = _Dev(ctx, stack)
            t = be.tensor(draws, layout)
            b = _batch(t[1][2], batch, r)
            bm, mu = be.batch_means(t, b)
            P, A = t[1][3], t[1][1] * (t[1][2] // b)
            return {"bm": be.get(bm, P * A).reshape(P, A), "mu": be.get(mu, P), "b": b, "a": t[1][2] // b}
    x = np.asarray(draws)
    targs = tensor_args(x, layout)
    b = _batch(targs[2], batch, r)
    P, A = targs[3], targs[1] * (targs[2] // b)
    bm, mu = np.full((P, A), np.nan), np.full(P, np.nan)
    h.check(h.lib.mcb_batch_means(h.handle, x.ctypes.data_as(C.c_void_p), *targs, b, _as_dp(bm), A, _as_dp(mu)))
    return {"bm": bm, "mu": mu, "b": b, "a": targs[2] // b}


def long_run_covariance(draws, layout: str = "pcn", batch=None, r: int = 3, context=None) -> dict:
    """The long-run covariance of the draws: sigma [P][P] (the batch-means estimate of the matrix of the Markov-chain CLT,
    lugsail for r = 3), mu [P], mcse_mean [P] = sqrt(sigma_pp / (A b)), ess_bm [P] = C N lambda_pp / sigma_pp, lambda
    [P][P] (the sample covariance of the pooled draws), b, a and info (0, or 1 + the first parameter at which sigma is not
    positive definite; with fewer than two batches sigma is NaN)."""
    ctx = context or _ffi.default_context()
    ctx.sync()
    with contextlib.ExitStack() as stack:
        return _long_run_covariance(_Dev(ctx, stack), draws, layout, batch, r)


def multi_ess(draws, layout: str = "pcn", batch=None, r: int = 3, scale=None, context=None) -> dict:
    """The multivariate effective sample size mESS = C N exp((logdet Lambda - logdet Sigma) / P_live) of the live parameters
    (scale [P] > 0; None: all), with p_live, info_sigma / info_lambda (a singular or, after lugsail, indefinite matrix
    gives mess = NaN), the two logdets, and per parameter mu, ess_bm and mcse_mean."""
    ctx = context or _ffi.default_context()
    ctx.sync()
    with contextlib.ExitStack() as stack:
        return _multi_ess(_Dev(ctx, stack), draws, layout, batch, r, scale)


def mean_shift_test(ref, act, scale=None, jitter: float = 0.0, r: int = 3, context=None, layout: str = "pcn", batch_ref=None,
                    batch_act=None, mess: bool = True, stages: dict | None = None) -> dict:
    """The joint test of equal means of two samples of the same parameters (3-D arrays or DeviceTensors, chains may
    differ in number and length): T = d^T V^-1 d with V = Sigma_ref / M_ref + Sigma_act / M_act on the scaled live
    parameters (scale [P]: 0 drops one; jitter is added to V's diagonal), dof = P_live, p_value = chi2_sf(T, dof)
    (asymptotic), z [dof] (each parameter's shift in Monte Carlo standard errors), d [dof] (the scaled shifts), shift [dof]
    (= L^-1 d: entry i is parameter i's shift given the ones before it), info (0, or 1 + the live index at which V is
    singular or indefinite: then T, p_value and shift are NaN), mess_ref / mess_act (`multi_ess` of each; NaN with
    mess=False) and the batch geometry b_ref, a_ref, b_act, a_act.  `stages` (a dict) receives the wall time of each step."""
    ctx = context or _ffi.default_context()
    ctx.sync()
    with contextlib.ExitStack() as stack:
        return _mean_shift_test(_Dev(ctx, stack, stages), ref, act, layout, scale, jitter, r, batch_ref, batch_act, mess)


def set_workspace_limit(nbytes: int, context=None) -> None:
    """The most device workspace one chunk of parameters of a batch-means call may take (mcb_set_workspace_limit)."""
    BM.set_workspace_limit(context or _ffi.default_context(), nbytes)


def profile(on: bool, context=None) -> None:
    """Time the kernels of every later mcb call with HIP events (mcb_profile_enable)."""
    BM.profile(context or _ffi.default_context(), on)


def kernel_ms(context=None) -> dict:
    """The last mcb call's kernel times in milliseconds by kernel name (mcb_kernel_ms); 0 for a kernel that did not run."""
    return BM.kernel_ms(context or _ffi.default_context(), KERNEL_NAMES)

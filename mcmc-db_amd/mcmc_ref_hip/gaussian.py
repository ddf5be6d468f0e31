"""Dense symmetric positive definite linear algebra on the GPU and the joint Gaussian check built on it: the extension
entries of include/mcmcref_hip_ext.h (`mcrx_*`, mirrored by `_xabi`) as free functions.

`gaussian_check(ref, act)` answers the cheapest joint question about two samples: do the first two moments of their joint
distributions agree?  `mahalanobis` is the number of posterior standard deviations the mean vector has moved, measured in
the reference's own metric; `kl_act_ref` / `kl_ref_act` are the Kullback-Leibler divergences of the two Gaussian fits, in
both directions.  Cost O(M P^2 + P^3), against the energy distance's O(M^2 P).

Every function takes `context=None` (the calling thread's `_ffi.default_context()`) and uses of it only `lib`, `handle`
and `_check`; the `*_host` functions are the definitions on the host and need neither a context nor a GPU.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _ffi
from ._abi import MCR_OK, McrError, _as_dp, _as_ip, load_library
from ._hostdefs import _sample_pair
from ._xabi import GAUSSIAN_INFO_KEYS, GAUSSIAN_KEYS, MCRX_G_INFO, MCRX_G_OUT, bind


def _ctx(context):
    ctx = context or _ffi.default_context()
    bind(ctx.lib)
    return ctx


def _void_p(v) -> C.c_void_p:
    """A device address given as an int or as a c_void_p (DeviceBuffer.ptr)."""
    return v if isinstance(v, C.c_void_p) else C.c_void_p(int(v))


def _host_rc(rc: int, what: str):
    if rc != MCR_OK:
        raise McrError(rc, what)


def _matrix(a, what: str) -> tuple[np.ndarray, int, int]:
    """A 2-D float64 array whose rows are contiguous (a padded row stride is passed on as it is): (array, rows, stride)."""
    a = np.asarray(a, dtype=np.float64)
    if a.ndim != 2:
        raise ValueError(f"{what} must be 2-D")
    rows, cols = a.shape
    if rows > 1 and cols > 0 and a.strides[1] == 8 and a.strides[0] % 8 == 0 and a.strides[0] >= 8 * cols:
        return a, rows, a.strides[0] // 8
    return np.ascontiguousarray(a), rows, cols


def _square(a, what: str) -> tuple[np.ndarray, int, int]:
    a, n, ld = _matrix(a, what)
    if a.shape[1] != n:
        raise ValueError(f"{what} must be square")
    return a, n, ld


def _chol(entry, handle, a):
    a, P, lda = _square(a, "a")
    out = np.zeros((P, P))
    info, logdet = C.c_int64(0), C.c_double(0.0)
    rc = entry(*handle, _as_dp(a), P, lda, _as_dp(out), C.byref(info), C.byref(logdet))
    return rc, out, int(info.value), float(logdet.value)


def cholesky(a, context=None) -> tuple[np.ndarray, int, float]:
    """(L, info, logdet) of the symmetric matrix a [P][P] (only its lower triangle is read) -- mcrx_cholesky.  L is lower
    triangular with L L^T = a and +0.0 above the diagonal; logdet = log det a = 2 sum log l_ii.  info = 0, or c + 1 for the
    first column c whose pivot is not > 0 (LAPACK dpotrf): then L[:c, :c] is the factor of a[:c, :c], the rest of L is
    unspecified and logdet is NaN.  L[:n, :n] equals cholesky(a[:n, :n]) in bits for every n."""
    ctx = _ctx(context)
    rc, out, info, logdet = _chol(ctx.lib.mcrx_cholesky, (ctx.handle,), a)
    ctx._check(rc)
    return out, info, logdet


def cholesky_host(a) -> tuple[np.ndarray, int, float]:
    """mcrx_cholesky_host: the definition of `cholesky` on the host, without a GPU (the same error bound, not the same bits)."""
    rc, out, info, logdet = _chol(bind(load_library()).mcrx_cholesky_host, (), a)
    _host_rc(rc, "mcrx_cholesky_host")
    return out, info, logdet


def cholesky_dev(a_ptr, P: int, lda: int | None = None, context=None) -> tuple[int, float]:
    """`cholesky` in place on a [P][P] f64 matrix with row stride lda (default P) in the context's device memory
    (a device address or DeviceBuffer.ptr): (info, logdet) -- mcrx_cholesky_dev."""
    ctx = _ctx(context)
    info, logdet = C.c_int64(0), C.c_double(0.0)
    ctx._check(ctx.lib.mcrx_cholesky_dev(ctx.handle, _void_p(a_ptr), int(P), int(P if lda is None else lda), C.byref(info),
                                         C.byref(logdet)))
    return int(info.value), float(logdet.value)


def _solve(entry, handle, l, b):
    l, P, ldl = _square(l, "l")
    b = np.asarray(b, dtype=np.float64)
    vector = b.ndim == 1
    b, rows, ldb = _matrix(b[:, None] if vector else b, "b")
    if rows != P:
        raise ValueError("l and b must have the same number of rows")
    K = b.shape[1]
    x = np.zeros((P, K))
    rc = entry(*handle, _as_dp(l), P, ldl, _as_dp(b), K, ldb, _as_dp(x))
    return rc, (x[:, 0] if vector else x)


def solve_lower(l, b, context=None) -> np.ndarray:
    """X with l X = b for the lower triangular l [P][P] (only its lower triangle is read) and b [P][K] or [P] --
    mcrx_solve_lower.  A column of X has the same bits alone or anywhere in a batch."""
    ctx = _ctx(context)
    rc, x = _solve(ctx.lib.mcrx_solve_lower, (ctx.handle,), l, b)
    ctx._check(rc)
    return x


def solve_lower_host(l, b) -> np.ndarray:
    """mcrx_solve_lower_host: the definition of `solve_lower` on the host, without a GPU."""
    rc, x = _solve(bind(load_library()).mcrx_solve_lower_host, (), l, b)
    _host_rc(rc, "mcrx_solve_lower_host")
    return x


def solve_lower_dev(l_ptr, P: int, b_ptr, K: int, ldl: int | None = None, ldb: int | None = None, context=None) -> None:
    """`solve_lower` on device memory: l [P][P] with row stride ldl (default P), b [P][K] with row stride ldb (default K),
    overwritten by the solution -- mcrx_solve_lower_dev."""
    ctx = _ctx(context)
    ctx._check(ctx.lib.mcrx_solve_lower_dev(ctx.handle, _void_p(l_ptr), int(P), int(P if ldl is None else ldl), _void_p(b_ptr),
                                            int(K), int(K if ldb is None else ldb)))


def _scale_jitter(scale, jitter, P: int):
    s = None if scale is None else np.ascontiguousarray(scale, dtype=np.float64)
    if s is not None and s.shape != (P,):
        raise ValueError("scale must have one entry per parameter")
    if s is not None and not (np.isfinite(s).all() and (s >= 0).all()):
        raise ValueError("scale must be finite and >= 0")
    jitter = float(jitter)
    if not (math.isfinite(jitter) and jitter >= 0):
        raise ValueError("jitter must be finite and >= 0")
    return s, jitter


def _gauss(entry, handle, ref, Mr, act, Ma, P, s, jitter, shift: bool):
    out = np.full(MCRX_G_OUT, np.nan)
    info = np.zeros(MCRX_G_INFO, dtype=np.int64)
    y = np.full(max(P, 1), np.nan) if shift else None
    rc = entry(*handle, ref, Mr, act, Ma, P, _as_dp(s), jitter, _as_dp(out), _as_ip(info), _as_dp(y))
    r = dict(zip(GAUSSIAN_KEYS, (float(v) for v in out)))
    r.update(zip(GAUSSIAN_INFO_KEYS, (int(v) for v in info)))
    r["mahalanobis"] = math.sqrt(r["d2_ref"]) if r["d2_ref"] >= 0 else float("nan")
    r["kl_sym"] = r["kl_act_ref"] + r["kl_ref_act"]
    if shift:
        r["shift"] = y[:r["p_live"]].copy()
    return rc, r


def gaussian_check(ref, act, scale=None, jitter: float = 0.0, shift: bool = False, context=None) -> dict:
    """The joint Gaussian check of the draws ref [P][Mr] against act [P][Ma] -- mcrx_gaussian_check.  Parameter p is
    multiplied by scale[p] (None: ones; 0 drops it: the others are the `p_live` live parameters, in their order), and
    `jitter` is added to the diagonal of both scaled covariance matrices.  Keys: d2_ref / d2_act (the squared Mahalanobis
    distance of the mean shift in the reference's / the actual sample's metric), trace_ref = tr(C_ref^-1 C_act) and
    trace_act, logdet_ref, logdet_act, kl_act_ref = KL(N_act || N_ref), kl_ref_act, p_live, info_ref / info_act (0, or
    1 + the live index of the first parameter at which the covariance is singular: what needs that factor is NaN),
    mahalanobis = sqrt(d2_ref), kl_sym = kl_act_ref + kl_ref_act, and with shift=True `shift` [p_live]: entry i is the
    shift of live parameter i given the ones before it, in conditional standard deviations."""
    ctx = _ctx(context)
    r, a = _sample_pair(ref, act, finite=False)
    s, jitter = _scale_jitter(scale, jitter, r.shape[0])
    rc, res = _gauss(ctx.lib.mcrx_gaussian_check, (ctx.handle,), _as_dp(r), r.shape[1], _as_dp(a), a.shape[1], r.shape[0], s,
                     jitter, shift)
    ctx._check(rc)
    return res


def gaussian_check_dev(ref_ptr, Mr: int, act_ptr, Ma: int, P: int, scale=None, jitter: float = 0.0, shift: bool = False,
                       context=None) -> dict:
    """`gaussian_check` on draws already in the context's device memory: ref_ptr -> [P][Mr] f64, act_ptr -> [P][Ma] f64."""
    ctx = _ctx(context)
    s, jitter = _scale_jitter(scale, jitter, int(P))
    rc, res = _gauss(ctx.lib.mcrx_gaussian_check_dev, (ctx.handle,), _void_p(ref_ptr), int(Mr), _void_p(act_ptr), int(Ma), int(P),
                     s, jitter, shift)
    ctx._check(rc)
    return res


def gaussian_check_host(ref, act, scale=None, jitter: float = 0.0, shift: bool = False) -> dict:
    """mcrx_gaussian_check_host: the definition of `gaussian_check` on the host, without a GPU (plain loops in double)."""
    r, a = _sample_pair(ref, act, finite=False)
    s, jitter = _scale_jitter(scale, jitter, r.shape[0])
    rc, res = _gauss(bind(load_library()).mcrx_gaussian_check_host, (), _as_dp(r), r.shape[1], _as_dp(a), a.shape[1], r.shape[0],
                     s, jitter, shift)
    _host_rc(rc, "mcrx_gaussian_check_host")
    return res


def gaussian_workspace(Mr: int, Ma: int, P: int, context=None) -> int:
    """Bytes of workspace a gaussian_check call of this shape carves (mcrx_gaussian_workspace)."""
    ctx = _ctx(context)
    v = C.c_size_t(0)
    ctx._check(ctx.lib.mcrx_gaussian_workspace(ctx.handle, int(Mr), int(Ma), int(P), C.byref(v)))
    return int(v.value)

"""Which chain disagrees, where, and by more than chance: the per-chain rank-ECDF uniformity test with simultaneous bands
of Saeilynoja, Buerkner and Vehtari (2022), the test behind bayesplot's mcmc_rank_ecdf and ArviZ's
plot_ecdf(confidence_bands="simulated").  For every chain the ECDF of its draws' pooled ranks is taken at K points, every
point is compared with its exact hypergeometric distribution, and the smallest pointwise tail probability is calibrated
against a simulated null sample so that the whole envelope has level 1 - alpha.  The entries of
include/mcmcref_recdf.h (`mce_*`, mirrored by `_eabi`) as free functions; the header holds the definition in full.

The test assumes EXCHANGEABLE draws.  Autocorrelated chains are rejected for being autocorrelated: unthinned AR(0.9)
chains of 250 draws are rejected 98 % of the time at alpha = 0.05 (iid draws: 5.75 %; the same chains thinned by 20:
7.5 %), so thinning -- `thin`, or `thin="ess"` -- is part of the interface.

The functions live in the companion library libmcmcref_recdf.so, which carries its own copy of the main library's sort
stage and summary pipeline.  Every device function takes `context=None` (the calling thread's `_ffi.default_context()`):
draws may be a numpy array or a DeviceTensor of that context, and the companion library gets a handle of its own on the
context's device, made at the first call and freed with the context.  `rank_ecdf_host` is the definition on the host and
needs neither.
"""
from __future__ import annotations

import ctypes as C
import math
import weakref
from pathlib import Path
from typing import Iterable

import numpy as np

from . import _ffi
from ._abi import _as_dp, _dtype_code, tensor_args
from ._companion import device_tensor
from ._eabi import KERNEL_NAMES, MCE_HIST_BYTES, MCE_MAX_POINTS, MCE_SLICE_DRAWS, OUTPUTS, RECDF

_handle = RECDF.handle                  # Context -> its RecdfHandle
_null_cache: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()         # Context -> {(C, n, K, S, seed): g0}
_host_null_cache: dict = {}


def chain_tile(C_: int, n: int, K: int) -> int:
    """Chains of one workgroup of the count kernel (mce_kernels.hpp: chain_tile)."""
    return int(min(max(min(MCE_HIST_BYTES // (4 * K), MCE_SLICE_DRAWS // n), 1), C_))


def _outputs(P: int, C_: int, K: int) -> dict:
    return {name: np.zeros(shape(P, C_, K), dtype=dtype) for name, dtype, shape in OUTPUTS}


_CTYPES = {"int32": C.POINTER(C.c_int32), "int64": C.POINTER(C.c_int64), "float64": C.POINTER(C.c_double)}


def _pointers(out: dict, p: int | None = None) -> list:
    """The outputs' pointers in the entries' order; `p`: those of parameter p alone."""
    return [(out[name] if p is None else out[name][p:p + 1]).ctypes.data_as(_CTYPES[dtype]) for name, dtype, _ in OUTPUTS]


def _thinned(targs, thin: int):
    """The arguments of the same tensor with the draws 0, thin, 2 thin, ... of every chain: a larger stride_n."""
    if int(thin) != thin or thin < 1:
        raise ValueError("thin must be an integer >= 1 or \"ess\"")
    code, C_, N, P, sc, sn, sp = targs
    return (code, C_, -(-N // int(thin)), P, sc, sn * int(thin), sp)


def _points(points, n: int, M: int) -> int:
    K = min(n, 100) if points is None else int(points)
    if K < 2 or K > min(M, MCE_MAX_POINTS):
        raise ValueError(f"points = {K}: must be in [2, min(C * n, {MCE_MAX_POINTS})] (C * n = {M})")
    return K


def _assemble(out: dict, g0: np.ndarray, alpha: float, thin: int, n: int, K: int) -> dict:
    """The p-values from the null sample, and the bookkeeping: p = (1 + #{ g0 <= g }) / (S + 1)."""
    g0 = np.sort(g0)
    out["pvalue"] = (1.0 + np.searchsorted(g0, out["g"], side="right")) / (len(g0) + 1.0)
    out["reject"] = out["pvalue"] <= alpha
    out.update(thin=int(thin), n=int(n), points=int(K))
    return out


def null_sample(C_: int, n: int, points: int, sims: int = 4000, seed: int = 0, context=None) -> np.ndarray:
    """mce_null_sample: g0[sims], the statistic g of `sims` simulated samples of C_ chains of n iid uniform draws, cached on
    the context per (C_, n, points, sims, seed).  The same bits as `null_sample_host`."""
    ctx = context or _ffi.default_context()
    cache = _null_cache.setdefault(ctx, {})
    key = (int(C_), int(n), int(points), int(sims), int(seed))
    if key not in cache:
        g0 = np.zeros(int(sims))
        ctx.sync()
        h = _handle(ctx)
        h.check(h.lib.mce_null_sample(h.handle, *key[:4], key[4] & (2 ** 64 - 1), _as_dp(g0)))
        cache[key] = g0
    return cache[key]


def null_sample_host(C_: int, n: int, points: int, sims: int = 4000, seed: int = 0) -> np.ndarray:
    """mce_null_sample_host: the null sample by the definition on the host (cached per argument tuple)."""
    key = (int(C_), int(n), int(points), int(sims), int(seed))
    if key not in _host_null_cache:
        g0 = np.zeros(int(sims))
        RECDF.host_check(RECDF.load().mce_null_sample_host(*key[:4], key[4] & (2 ** 64 - 1), _as_dp(g0)))
        _host_null_cache[key] = g0
    return _host_null_cache[key]


def table(M: int, n: int, points: int) -> np.ndarray:
    """mce_table_host: U[points - 1][n + 1], row k - 1 the pointwise probabilities min(P(X <= j), P(X >= j)) of
    X ~ Hypergeometric(M, floor(k M / points), n)."""
    out = np.zeros((int(points) - 1, int(n) + 1))
    RECDF.host_check(RECDF.load().mce_table_host(int(M), int(n), int(points), _as_dp(out)))
    return out


def _ess_thin(ctx, draws, layout: str, targs, points) -> int:
    """One stride for the call: ceil(max_p M / ess_bulk_p) of Context.summarize, capped so that n >= 2 points."""
    _, C_, N, _, _, _, _ = targs
    r = ctx.summarize(draws, layout) if device_tensor(draws) is None else ctx.summarize(draws)
    ess = np.asarray(r["ess_bulk"], dtype=np.float64)
    ess = ess[np.isfinite(ess) & (ess > 0)]
    want = math.ceil(C_ * N / float(ess.min())) if len(ess) else 1
    K0 = min(N, 100) if points is None else int(points)
    return max(1, min(want, N // (2 * K0)))


def rank_ecdf(draws, layout: str = "pcn", points: int | None = None, thin=1, sims: int = 4000, seed: int = 0,
              alpha: float = 0.05, context=None) -> dict:
    """The rank-ECDF test of every parameter of `draws` (a 3-D numpy array whose axes are `layout`, f64 or f32, or a
    DeviceTensor of the context).  `points`: K, the evaluation points (default min(n, 100)); `thin`: keep every thin-th draw
    of a chain (n = ceil(N / thin)), or "ess": one stride for the call, ceil(max_p M / ess_bulk_p) from `Context.summarize`
    on the same tensor, capped so that n >= 2 points.  Returns a dict: counts [P][C][K-1] (a[c][k], draws of chain c at or
    below the pooled draw of rank floor(k M / K)), pooled [P][K-1], tied [P] (points where ties moved the pooled count: 0
    means the calibration is exact), u [P][C] (the chain's smallest pointwise probability), kmin [P][C] (the point k
    attaining it), dev [P][C] (the largest ECDF difference), g [P] = min_c u, chain [P] (the chain attaining it), pvalue [P]
    = (1 + #{ g0 <= g }) / (sims + 1) against the seeded null sample (cached on the context), reject [P] = pvalue <= alpha,
    and the thin, n and points used.  Non-finite draws raise.  Calls `context.sync()` first.  All integer outputs and u, g
    have the same bits as `rank_ecdf_host`, alone, in any batch, layout, dtype route and chunking.

    The draws must be exchangeable: measured at alpha = 0.05 with 4 chains of 250 draws and 32 points, iid draws are
    rejected 5.75 % of the time, unthinned AR(0.9) chains 98 %, the same chains at thin=20 7.5 %."""
    ctx = context or _ffi.default_context()
    t = device_tensor(draws)
    if t is not None:
        ptr, targs, entry = t.buf.ptr, t.targs, "mce_rank_ecdf_dev"
    else:
        draws = np.asarray(draws)
        ptr, targs, entry = draws.ctypes.data_as(C.c_void_p), tensor_args(draws, layout), "mce_rank_ecdf"
    if thin == "ess":
        thin = _ess_thin(ctx, draws, layout, targs, points)
    targs = _thinned(targs, thin)
    _, C_, n, P, _, _, _ = targs
    K = _points(points, n, C_ * n)
    out = _outputs(P, C_, K)
    g0 = null_sample(C_, n, K, sims, seed, context=ctx)      # first: kernel_ms then speaks of the call on the draws
    ctx.sync()
    h = _handle(ctx)
    h.check(getattr(h.lib, entry)(h.handle, ptr, *targs, K, *_pointers(out)))
    out["dev"] = out["dev"] / float(n * C_ * n)
    return _assemble(out, g0, alpha, thin, n, K)


def rank_ecdf_host(chains, points: int | None = None, thin: int = 1, sims: int = 4000, seed: int = 0, alpha: float = 0.05) -> dict:
    """mce_rank_ecdf_host and mce_null_sample_host: the definition on the host, without a GPU, for `chains` [C][N] of one
    parameter (a dict of scalars and [C] arrays) or [P][C][N] (as `rank_ecdf` returns).  f32 chains are widened."""
    lib = RECDF.load()
    x = np.asarray(chains)
    if x.ndim not in (2, 3):
        raise ValueError("chains must be [C][N] or [P][C][N]")
    if int(thin) != thin or thin < 1:
        raise ValueError("thin must be an integer >= 1")
    single = x.ndim == 2
    x = x[None] if single else x
    x = np.ascontiguousarray(x[:, :, ::int(thin)], dtype=np.float64)
    P, C_, n = x.shape
    K = _points(points, n, C_ * n)
    out = _outputs(P, C_, K)
    tab = table(C_ * n, n, K)
    for p in range(P):
        RECDF.host_check(lib.mce_rank_ecdf_host(_as_dp(x[p]), C_, n, K, _as_dp(tab), *_pointers(out, p)))
    out["dev"] = out["dev"] / float(n * C_ * n)
    out = _assemble(out, null_sample_host(C_, n, K, sims, seed), alpha, thin, n, K)
    return {k: (v[0] if isinstance(v, np.ndarray) else v) for k, v in out.items()} if single else out


def rank_ecdf_file(path: Path, params: Iterable[str] | None = None, points: int | None = None, thin=1, sims: int = 4000,
                   seed: int = 0, alpha: float = 0.05, host: bool = False, context=None) -> dict[str, dict]:
    """`rank_ecdf` of every parameter of a draws table (a `.csv`, a chain-list `.json.zip` or a `.parquet` draws file of
    the store, read on the host; chains of equal length): per parameter pvalue, reject, the offending chain, the point as
    a pooled quantile kmin / points, the largest ECDF difference of that chain, tied, and the thin, n and points used.
    `host`: by the definition on the host, without a GPU (`thin` an integer)."""
    from . import convert
    tab, names = convert._table_and_names(convert._read_table(Path(path), parquet=True), params)
    if not names:
        return {}
    x = convert._equal_chains(tab, names, "the rank-ECDF test")
    with _ffi.value_errors():
        if host:
            if thin == "ess":
                raise ValueError("thin=\"ess\" needs the device; give an integer with host=True")
            r = rank_ecdf_host(x, points=points, thin=thin, sims=sims, seed=seed, alpha=alpha)
        else:
            r = rank_ecdf(x, "pcn", points=points, thin=thin, sims=sims, seed=seed, alpha=alpha, context=context)
    out = {}
    for i, name in enumerate(names):
        c = int(r["chain"][i])
        out[name] = {"pvalue": float(r["pvalue"][i]), "reject": bool(r["reject"][i]), "chain": c,
                     "quantile": float(r["kmin"][i, c]) / r["points"], "max_diff": float(r["dev"][i, c]), "tied": int(r["tied"][i]),
                     "thin": r["thin"], "n": r["n"], "points": r["points"]}
    return out


def set_workspace_limit(nbytes: int, context=None) -> None:
    """The most device workspace one chunk of parameters or simulations may take (mce_set_workspace_limit)."""
    RECDF.set_workspace_limit(context or _ffi.default_context(), nbytes)


def params_per_chunk(C_: int, n: int, P: int, points: int, dtype=np.float64, strides=None, context=None) -> int:
    """Parameters per chunk of a call of this shape under the workspace limit (mce_plan); `strides` = (stride_c, stride_n,
    stride_p) in elements, default contiguous [P][C][n]."""
    sc, sn, sp = strides or (n, 1, C_ * n)
    return RECDF.plan(context or _ffi.default_context(), "mce_plan", _dtype_code(np.dtype(dtype)), int(C_), int(n), int(P), int(sc),
                      int(sn), int(sp), int(points))


def sims_per_chunk(C_: int, n: int, points: int, sims: int, context=None) -> int:
    """Simulations per chunk of a null sample of this shape under the workspace limit (mce_null_plan)."""
    return RECDF.plan(context or _ffi.default_context(), "mce_null_plan", int(C_), int(n), int(points), int(sims))


def clear_null_cache(context=None) -> None:
    """Forget the cached null samples of the context (and of the host path)."""
    _null_cache.pop(context or _ffi.default_context(), None)
    _host_null_cache.clear()


def profile(on: bool, context=None) -> None:
    """Time the kernels of every later call with HIP events (mce_profile_enable)."""
    RECDF.profile(context or _ffi.default_context(), on)


def kernel_ms(context=None) -> dict:
    """The last call's times in milliseconds, {"fill": ..., "pipe": ..., "count": ..., "stat": ...} (mce_kernel_ms)."""
    return RECDF.kernel_ms(context or _ffi.default_context(), KERNEL_NAMES)

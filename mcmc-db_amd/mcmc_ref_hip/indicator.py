"""The effective sample size of an indicator I(lower < x <= upper) of the draws: how many effective draws stand behind a
quantile, a tail probability or a bin of the local-efficiency plot (Vehtari et al. 2021).  The entries of
include/mcmcref_iess.h (`mci_*`, mirrored by `_iabi`) as free functions; they live in the companion library
libmcmcref_iess.so, which packs the indicator chains into bits (64 draws per word) and takes every lag product as a
popcount, so each autocovariance is an exact rational and the truncation is decided in integers.

The rule is the library's one ESS rule -- the reference's `_ess`: unsplit chains, truncation at the first negative
autocorrelation -- applied to the 0/1 chains.  It is NOT Geyer's initial-sequence rule on split chains, so the numbers
differ from posterior::ess_quantile / ess_median / ess_tail exactly as `ess_bulk` here differs from posterior::ess_bulk.

Every device function takes `context=None` (the calling thread's `_ffi.default_context()`): draws may be a numpy array or a
DeviceTensor of that context, the quantile thresholds come from its `summarize`, and the companion library gets a handle
of its own on the context's device, made at the first call and freed with the context.  The `*_host` functions are the
definition on the host and need neither.
"""
from __future__ import annotations

import numpy as np

from . import _ffi
from ._abi import _as_dp, _as_ip, _dtype_code, tensor_args
from ._companion import tensor_entry
from ._device import DeviceTensor
from ._iabi import IESS, KERNEL_NAMES, MCI_MAX_REQUESTS

_handle = IESS.handle                   # Context -> its IessHandle


def _requests(lower, upper, P: int) -> tuple[np.ndarray, np.ndarray, int]:
    """lower and upper as contiguous [P][K] doubles: a scalar, [K] (the same for every parameter) or [P][K]."""
    lo, hi = np.asarray(lower, dtype=np.float64), np.asarray(upper, dtype=np.float64)
    shape = np.broadcast_shapes(lo.shape, hi.shape, (1,))
    if len(shape) > 2 or (len(shape) == 2 and shape[0] not in (1, P)):
        raise ValueError("lower and upper must be scalars, [K] or [P][K]")
    K = shape[-1]
    if not 1 <= K <= MCI_MAX_REQUESTS:
        raise ValueError(f"1 to {MCI_MAX_REQUESTS} requests per call; got {K}")
    full = (P, K)
    return (np.ascontiguousarray(np.broadcast_to(lo, full)), np.ascontiguousarray(np.broadcast_to(hi, full)), K)


def _outputs(P: int, K: int):
    return np.full((P, K), np.nan), np.zeros((P, K), dtype=np.int64), np.zeros((P, K), dtype=np.int64)


def indicator_ess(draws, lower, upper, layout: str = "pcn", context=None) -> dict:
    """ESS of the indicator lower < x <= upper for every parameter of `draws` (a 3-D numpy array whose axes are `layout`, or
    a DeviceTensor of the context) and every request: `lower` / `upper` are scalars, [K] or [P][K], K <= 32; -inf / +inf
    are allowed, lower >= upper is an empty indicator, a NaN draw counts as 0.  Returns ess [P][K] (NaN for chains of
    fewer than 2 draws; C N for a constant indicator), trunc [P][K] (the first lag with a negative autocovariance, N when
    there is none, 0 for a constant indicator, -1 for N < 2) and ones [P][K] (the pooled count) -- mci_indicator_ess(_dev).
    Calls `context.sync()` first.  A parameter's numbers have the same bits alone, in any batch, layout and chunking."""
    ctx = context or _ffi.default_context()
    entry, ptr, targs = tensor_entry(draws, layout, "mci_indicator_ess")
    lo, hi, K = _requests(lower, upper, targs[3])
    ess, trunc, ones = _outputs(targs[3], K)
    ctx.sync()
    h = _handle(ctx)
    h.check(getattr(h.lib, entry)(h.handle, ptr, *targs, _as_dp(lo), _as_dp(hi), K, _as_dp(ess), _as_ip(trunc), _as_ip(ones)))
    return {"ess": ess, "trunc": trunc, "ones": ones}


def indicator_ess_host(draws, lower, upper, layout: str = "pcn") -> dict:
    """mci_indicator_ess_host: the definition of `indicator_ess` on the host, parameter by parameter, without a GPU.  The
    same bits as the device."""
    lib = IESS.load()
    draws = np.asarray(draws)
    tensor_args(draws, layout)
    x = np.ascontiguousarray(np.transpose(draws, [layout.index(a) for a in "pcn"]), dtype=np.float64)
    P = x.shape[0]
    lo, hi, K = _requests(lower, upper, P)
    ess, trunc, ones = _outputs(P, K)
    for p in range(P):
        IESS.host_check(lib.mci_indicator_ess_host(_as_dp(x[p]), x.shape[1], x.shape[2], _as_dp(lo[p]), _as_dp(hi[p]), K,
                                                   _as_dp(ess[p]), _as_ip(trunc[p]), _as_ip(ones[p])))
    return {"ess": ess, "trunc": trunc, "ones": ones}


def _thresholds(ctx, draws, layout: str, probs) -> np.ndarray:
    """The linear-interpolation quantiles [P][len(probs)] of the pooled draws, from the context's summarize."""
    return ctx.summarize(draws, layout, min_chains=1, quantiles=probs, diagnostics=False)["q"]


def ess_quantile(draws, probs=(0.05, 0.5, 0.95), layout: str = "pcn", context=None) -> dict:
    """ESS behind the quantile estimates of every parameter: the indicator is x <= q_prob, q_prob the pooled quantile the
    context's summarize reports (numpy's linear interpolation).  Returns thresholds [P][len(probs)], ess, trunc (as
    `indicator_ess`) and tail_min [P] = min(ess at the smallest prob, ess at the largest) -- with the default probs the
    smaller of the 5 % and 95 % indicator ESS, what Stan calls ess_tail, under this library's truncation rule."""
    ctx = context or _ffi.default_context()
    probs = [float(q) for q in probs]
    if not probs or not all(0.0 <= q <= 1.0 for q in probs):
        raise ValueError(f"probs: probabilities inside [0, 1]; got {probs}")
    q = _thresholds(ctx, draws, layout, probs)
    r = indicator_ess(draws, -np.inf, q, layout, ctx)
    lo, hi = int(np.argmin(probs)), int(np.argmax(probs))
    return {"probs": probs, "thresholds": q, "ess": r["ess"], "trunc": r["trunc"],
            "tail_min": np.minimum(r["ess"][:, lo], r["ess"][:, hi])}


def ess_local(draws, bins: int = 20, layout: str = "pcn", context=None) -> dict:
    """Local efficiency: the ESS of q_{j/bins} < x <= q_{(j+1)/bins} for j = 0 .. bins - 1 (bins <= 32), the first lower
    edge -inf and the last upper edge +inf.  Returns edges [P][bins - 1] (the inner quantiles), ess and trunc [P][bins]
    and efficiency = ess / (C N): the data of the local-efficiency plot."""
    ctx = context or _ffi.default_context()
    bins = int(bins)
    if not 1 <= bins <= MCI_MAX_REQUESTS:
        raise ValueError(f"bins: 1 to {MCI_MAX_REQUESTS}; got {bins}")
    targs = draws.targs if isinstance(draws, DeviceTensor) else tensor_args(np.asarray(draws), layout)
    P = targs[3]
    edges = _thresholds(ctx, draws, layout, [j / bins for j in range(1, bins)]) if bins > 1 else np.zeros((P, 0))
    lower = np.concatenate([np.full((P, 1), -np.inf), edges], axis=1)
    upper = np.concatenate([edges, np.full((P, 1), np.inf)], axis=1)
    r = indicator_ess(draws, lower, upper, layout, ctx)
    return {"edges": edges, "ess": r["ess"], "trunc": r["trunc"], "efficiency": r["ess"] / float(targs[1] * targs[2])}


def set_workspace_limit(nbytes: int, context=None) -> None:
    """The most device workspace one chunk of parameters of an indicator call may take (mci_set_workspace_limit)."""
    IESS.set_workspace_limit(context or _ffi.default_context(), nbytes)


def params_per_chunk(C_: int, N: int, P: int, K: int, dtype=np.float64, context=None) -> int:
    """Parameters per chunk of an indicator call of this shape under the workspace limit (mci_indicator_plan)."""
    return IESS.plan(context or _ffi.default_context(), "mci_indicator_plan", _dtype_code(np.dtype(dtype)), int(C_), int(N), int(P), int(K))


def profile(on: bool, context=None) -> None:
    """Time the kernels of every later indicator call with HIP events (mci_profile_enable)."""
    IESS.profile(context or _ffi.default_context(), on)


def kernel_ms(context=None) -> dict:
    """The last indicator call's kernel times in milliseconds, {"pack": ..., "lag": ...} (mci_kernel_ms)."""
    return IESS.kernel_ms(context or _ffi.default_context(), KERNEL_NAMES)

"""R-hat and ESS in the Stan convention: split chains, rank normalisation with Blom scores, folding, and Geyer's initial
positive and monotone sequence -- `rhat`, `ess_bulk`, `ess_tail`, `ess_mean`, `mcse_mean` as stansummary,
posterior::summarise_draws and arviz.summary define them (Vehtari, Gelman, Simpson, Carpenter, Buerkner 2021).  The
entries of include/mcmcref_std.h (`mcs_*`, mirrored by `_sabi`) as free functions; the header holds the definition in
full.  `Context.summarize` keeps the reference's definitions (unsplit chains for ESS, truncation at the first negative
autocorrelation, rank offset (r - 0.5) / M): this module is for validating a sampler against CmdStan or ArviZ output.

Agreement with the packages rests on the definition, written from the papers: neither package pins it in the tests.  For
an odd number of draws per chain the middle draw of each chain is dropped from everything (ArviZ's rank and median rule;
the packages take the tail quantiles, posterior also the median, over all draws).

The functions live in the companion library libmcmcref_std.so, which carries its own copy of the main library's sort
stage and summary pipeline: a second copy of those kernels is loaded at the first call.  Every device function takes
`context=None` (the calling thread's `_ffi.default_context()`): draws may be a numpy array or a DeviceTensor of that
context, and the companion library gets a handle of its own on the context's device, made at the first call and freed
with the context.  `diagnostics_host` is the definition on the host and needs neither.
"""
from __future__ import annotations

from pathlib import Path
from typing import Iterable

import numpy as np

from . import _ffi
from ._abi import _as_dp, _as_ip, _dtype_code
from ._companion import tensor_entry
from ._sabi import DOUBLE_OUTPUTS, INT_OUTPUTS, KERNEL_NAMES, MCS_WANT_BASIC, STD

_handle = STD.handle                    # Context -> its StdHandle
BASIC_OUTPUTS = ("rhat_basic", "ess_mean", "mcse_mean", "lag_mean")


def _outputs(P: int) -> dict:
    out = {k: np.full(P, np.nan) for k in DOUBLE_OUTPUTS}
    out.update({k: np.full(P, -1, dtype=np.int64) for k in INT_OUTPUTS})
    return out


def _pointers(out: dict) -> list:
    return [_as_dp(out[k]) for k in DOUBLE_OUTPUTS] + [_as_ip(out[k]) for k in INT_OUTPUTS]


def _result(out: dict, basic: bool) -> dict:
    return out if basic else {k: v for k, v in out.items() if k not in BASIC_OUTPUTS}


def diagnostics(draws, layout: str = "pcn", basic: bool = False, context=None) -> dict:
    """The Stan-convention diagnostics of every parameter of `draws` (a 3-D numpy array whose axes are `layout`, f64 or
    f32, or a DeviceTensor of the context): a dict of [P] arrays -- rhat, rhat_bulk, rhat_tail, ess_bulk, ess_tail,
    ess_q05, ess_q95, lag_bulk, lag_q05, lag_q95 (the walk's max_t; -1 where there is no ESS) and margin (the smallest
    |rho_t + rho_{t+1}| the bulk walk saw); with `basic` also rhat_basic, ess_mean, mcse_mean and lag_mean.  Chains of
    fewer than 8 draws have no ESS (NaN); a constant parameter has NaN everywhere.  Non-finite draws raise.  Calls
    `context.sync()` first.  A parameter's numbers have the same bits alone, in any batch, layout, dtype route and chunking.
    The cost grows with the walk: a chain that has not converged takes O(N^2) products (mcs_diagnostics(_dev))."""
    ctx = context or _ffi.default_context()
    entry, ptr, targs = tensor_entry(draws, layout, "mcs_diagnostics")
    out = _outputs(targs[3])
    ctx.sync()
    h = _handle(ctx)
    h.check(getattr(h.lib, entry)(h.handle, ptr, *targs, MCS_WANT_BASIC if basic else 0, *_pointers(out)))
    return _result(out, basic)


def diagnostics_host(chains, basic: bool = False) -> dict:
    """mcs_diagnostics_host: the definition on the host, without a GPU, for `chains` [C][N] of one parameter (a dict of
    scalars) or [P][C][N] (a dict of [P] arrays).  Agrees with `diagnostics` to 1e-9 relative, the lags exactly."""
    lib = STD.load()
    x = np.ascontiguousarray(chains, dtype=np.float64)
    if x.ndim not in (2, 3):
        raise ValueError("chains must be [C][N] or [P][C][N]")
    single = x.ndim == 2
    x = x[None] if single else x
    out = _outputs(x.shape[0])
    for p in range(x.shape[0]):
        one = {k: v[p:p + 1] for k, v in out.items()}
        STD.host_check(lib.mcs_diagnostics_host(_as_dp(x[p]), x.shape[1], x.shape[2], MCS_WANT_BASIC if basic else 0, *_pointers(one)))
    out = _result(out, basic)
    return {k: v[0].item() for k, v in out.items()} if single else out


def diagnostics_file(path: Path, params: Iterable[str] | None = None, basic: bool = False,
                     context=None) -> dict[str, dict[str, float]]:
    """`diagnostics` of every parameter of a draws table (a `.csv`, a chain-list `.json.zip` or a `.parquet` draws file of
    the store, read on the host; chains of equal length): per parameter a dict of the outputs."""
    from . import convert
    table, names = convert._table_and_names(convert._read_table(Path(path), parquet=True), params)
    if not names:
        return {}
    x = convert._equal_chains(table, names, "the Stan-convention diagnostics")
    with _ffi.value_errors():
        r = diagnostics(x, "pcn", basic=basic, context=context)
    return {n: {k: float(v[i]) for k, v in r.items()} for i, n in enumerate(names)}


def set_workspace_limit(nbytes: int, context=None) -> None:
    """The most device workspace one chunk of parameters of a diagnostics call may take (mcs_set_workspace_limit)."""
    STD.set_workspace_limit(context or _ffi.default_context(), nbytes)


def params_per_chunk(C_: int, N: int, P: int, dtype=np.float64, basic: bool = False, strides=None, context=None) -> int:
    """Parameters per chunk of a diagnostics call of this shape under the workspace limit (mcs_plan); `strides` =
    (stride_c, stride_n, stride_p) in elements, default contiguous [P][C][N]."""
    sc, sn, sp = strides or (N, 1, C_ * N)
    return STD.plan(context or _ffi.default_context(), "mcs_plan", _dtype_code(np.dtype(dtype)), int(C_), int(N), int(P), int(sc), int(sn),
                    int(sp), MCS_WANT_BASIC if basic else 0)


def profile(on: bool, context=None) -> None:
    """Time the phases of every later diagnostics call with HIP events (mcs_profile_enable)."""
    STD.profile(context or _ffi.default_context(), on)


def kernel_ms(context=None) -> dict:
    """The last diagnostics call's times in milliseconds, {"pipe": ..., "series": ..., "walk": ...} (mcs_kernel_ms)."""
    return STD.kernel_ms(context or _ffi.default_context(), KERNEL_NAMES)

"""ctypes binding of libmcmcref_hip.so (include/mcmcref_hip.h): the import surface.  No torch, no fallback.

If the shared library or a HIP device is missing every entry point raises `HipUnavailableError`: the product path never
silently computes on the CPU.

The binding is five units, imported in this order and re-exported here by name: `_abi` (the header, restated), `_hostdefs`
(the definitions that need no GPU), `_device` (the owners of device memory), `_filecalls` / `_statcalls` / `_context`
(Context).  What is defined HERE is the summarize plumbing the Python API shares on top of a Context: the rolling window
over enqueue / wait_one (`pipeline`, `split_result`), the reference-shaped per-parameter dicts (`entries`), the ragged-chain
route (`ragged_diagnostics`), the McrError -> ValueError translation of the reference-compatible functions (`value_errors`)
and the per-thread `default_context`.
"""
from __future__ import annotations

import collections
import contextlib
import ctypes as C  # noqa: F401  (callers build pointers as _ffi.C.c_void_p)
import threading

import numpy as np

from ._abi import (_I64, _PKG, _TENSOR, _TENSOR4, CSV_HEADERS, DEFAULT_LIB, DIAG_KEYS, ENERGY_KEYS, FS_EXPORT, FS_PHASES,  # noqa: F401
                   INT64_MAX, MCR_ACF_BLOCK, MCR_ACF_MAX_LAG, MCR_ACF_UNBIASED, MCR_CSVW_FIELD_MAX, MCR_CSVW_TILE_FIELDS,
                   MCR_ECOMM, MCR_EFALLBACK, MCR_EHIP, MCR_EINVAL, MCR_ELAYOUT, MCR_EMINCHAINS, MCR_EMINCHAINS_ARG,
                   MCR_ENERGY_CHUNK_P, MCR_ENERGY_LAUNCH_WORK, MCR_ENERGY_MAX_WORK, MCR_ENERGY_TILE_I, MCR_ENERGY_TILE_J,
                   MCR_ENODEVICE, MCR_ENOMEM, MCR_ENONFINITE, MCR_F32, MCR_F64, MCR_HDI_MAX_PROBS, MCR_HDI_SLICE,
                   MCR_MAX_INFLIGHT, MCR_MAX_QUANTILES, MCR_NESTED_BLOCK, MCR_NESTED_MAX_CHAINS, MCR_OK, MCR_PARETO_LDS_TAIL,
                   MCR_PQ_DOUBLE, MCR_PQ_F64, MCR_PQ_I64, MCR_PQ_INT32, MCR_PQ_INT64, MCR_PQW_F64, MCR_PQW_I64,
                   MCR_PQW_PAGE_ROWS, MCR_PQW_ROW_GROUP_ROWS, MCR_PQW_SEQ, MCR_PROJ_CHUNK_P, MCR_PROJ_TILE_K, MCR_PROJ_TILE_M,
                   MCR_SELECT_BLOCK_ROWS, MCR_W_LOG, MCR_WEIGHTED_BLOCK, MCR_WEIGHTED_MAX_Q, NESTED_FIELDS, SUMMARY_F64,
                   SYMBOLS, Acf, Hdi, HipUnavailableError, IdColumns, KernelTime, McrError, ModelDesc, Nested, Pareto,
                   ParquetRequest, PqColumn, Psis, Sbc, Summary, Weighted, _as_dp, _as_ip, _dp, _dtype_code, _ip, lib_path,
                   load_library, pq_column, pq_sequence, tensor4_args, tensor_args, thin_args)
from ._context import Context, SummaryBuffers  # noqa: F401
from ._device import _Owner, CsvTable, DeviceArena, DeviceBuffer, DeviceSims, DeviceTensor, DeviceView  # noqa: F401
from ._hostdefs import (LOO_KHAT_BINS, Image, PqImage, TextImage, _acf_arrays, _acf_result, _pq_columns, _sbc_arrays,  # noqa: F401
                        _truth_array, autocorr_host, chi2_sf, energy_distance_host, energy_launches, format_double,
                        hdi_sorted_host, loo_totals, pareto_companions, pareto_fit_host, pareto_tail_length, psis_host,
                        psis_tail_length, sbc_ranks_host, sbc_uniformity, superchain_labels, weight_arguments, weighted_host,
                        write_csv_host, write_parquet_host)


def pipeline(ctx: Context, jobs, owns: bool = False):
    """Rolling window of ctx.enqueue / ctx.wait_one over `jobs`, an iterable of (tag, DeviceTensor, enqueue() keyword
    arguments) consumed lazily; a tensor with chain_off (Context.ragged_tensor) is a ragged call, and both kinds share
    the window.  Yields (tag, result dict or the McrError of that job's enqueue or wait) in submission
    order with at most MCR_MAX_INFLIGHT calls outstanding; calls already in flight on `ctx` are waited for first, so
    that every wait_one delivers one of these jobs.  owns=True: the helper frees each tensor once its call is retired.

    However the generator ends -- exhausted, closed early, an exception in `jobs` -- nothing stays in flight and no
    owned tensor stays allocated; use it under contextlib.closing so that an exception in the consumer's loop closes
    it at once.  The consumer does not use `ctx` between two results."""
    if ctx.inflight:
        ctx.wait()
    window = collections.deque()            # (tag, tensor, result buffers or the McrError of its enqueue)
    try:
        for tag, t, kw in jobs:
            try:
                window.append((tag, t, ctx.enqueue(t, **kw)))
            except McrError as exc:
                window.append((tag, t, exc))
            if len(window) == MCR_MAX_INFLIGHT:
                yield _retire(ctx, window, owns)
        while window:
            yield _retire(ctx, window, owns)
    finally:
        if window:
            try:
                ctx.wait()
            except McrError:                # the exception that ended the generator is the one to report
                pass
            if owns:
                for _tag, t, _ in window:
                    t.free()
            window.clear()


def _retire(ctx: Context, window, owns: bool):
    """The oldest job of the window: (tag, result dict or McrError); its tensor is freed if owned."""
    tag, t, got = window[0]
    if not isinstance(got, McrError):
        try:
            if ctx.wait_one() is not got:    # never hand a job another call's numbers
                raise RuntimeError("pipeline: the context delivered a result that is not this job's")
            got = got.result()
        except McrError as exc:
            got = exc
    window.popleft()
    if owns:
        t.free()
    return tag, got


def split_result(r: dict, sizes) -> list[dict]:
    """A batched call's result cut back into its models: `sizes` = parameters per model, in tensor order."""
    out, p0 = [], 0
    for P in sizes:
        out.append({k: (v if k == "q_lo" else v[p0:p0 + P]) for k, v in r.items()})
        p0 += P
    return out


def entries(r: dict, quantiles=None, diagnostics: bool = True) -> list[dict[str, float]]:
    """The per-parameter dicts of the reference API from a summary dict, in parameter order: {"mean", "std", "qNN"...}
    for `quantiles` (the keys f"q{int(q * 100)}"), then {"rhat", "ess_bulk", "ess_tail"} with diagnostics.
    quantiles=None: the diagnostics triple alone."""
    keys, cols = [], []                     # whole columns to Python floats, not one value at a time
    if quantiles is not None:
        keys = ["mean", "std"] + [f"q{int(q * 100)}" for q in quantiles]
        cols = [r["mean"].tolist(), r["std"].tolist()] + r["q"].T.tolist()      # q: [P][n_q]
    if diagnostics:
        keys += DIAG_KEYS
        cols += [r["rhat"].tolist(), r["ess_bulk"].tolist(), r["ess_tail"].tolist()]
    return [dict(zip(keys, row)) for row in zip(*cols)]


def ragged_diagnostics(ctx: Context, x: np.ndarray, counts, min_chains: int) -> dict[str, np.ndarray]:
    """rhat / ess_bulk / ess_tail of every row of x [P][M] whose chains are `counts` draws long (chains of unequal
    length): one upload and one batched mcr_summarize_chains_dev call."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    if x.shape[0] == 0:
        return {k: np.empty(0) for k in DIAG_KEYS}
    r = ctx.summarize_chains(x, counts, min_chains=min_chains, quantiles=())
    return {k: np.asarray(r[k], dtype=np.float64) for k in DIAG_KEYS}


@contextlib.contextmanager
def value_errors():
    """McrError -> ValueError with the library's message: the exception the reference-compatible functions raise."""
    try:
        yield
    except McrError as exc:
        raise ValueError(exc.message) from exc


_default = threading.local()


def default_context() -> Context:
    """The calling THREAD's Context on MCMC_REF_HIP_DEVICE / LOCAL_RANK / device 0 (created on first use).

    A Context is one GPU + its streams and is not thread-safe, so the module-level convenience functions
    (`reference.stats`, `compare.compute_basic_stats`, ...) never share one between threads: each thread gets its own."""
    ctx = getattr(_default, "ctx", None)
    if ctx is None or ctx.handle is None:
        ctx = _default.ctx = Context()
    return ctx

"""Context: one GPU behind the C ABI.  `_Core` holds the handle, the error check, device memory, the summarize calls and
their window, and measurement; `_FileCalls` and `_StatCalls` hold the entries of the library's file and statistics units.
The three are plain classes that share `self.lib`, `self.handle`, `self._check` and each other's public methods.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
import os

import numpy as np

from ._abi import (MCR_EFALLBACK, MCR_ENODEVICE, MCR_F32, MCR_F64, MCR_MAX_QUANTILES, MCR_OK, SUMMARY_F64, HipUnavailableError,
                   KernelTime, McrError, ModelDesc, Summary, _as_dp, _as_ip, _dtype_code, load_library, tensor_args)
from ._device import DeviceBuffer, DeviceTensor
from ._filecalls import _FileCalls
from ._statcalls import _StatCalls


class SummaryBuffers:
    """Host arrays an mcr_summary points into (kept alive by this object)."""

    def __init__(self, P: int, nq: int, diagnostics: bool = True):
        self.P, self.nq, self.diagnostics = P, nq, diagnostics      # (built per enqueue without a ring: plain statements)
        n = max(P, 1)
        self.arrays = {k: np.full(n, np.nan) for k in SUMMARY_F64}
        self.arrays["q"] = np.full(max(P * nq, 1), np.nan)
        self.arrays["lag_bulk"] = np.zeros(n, dtype=np.int64)
        self.arrays["lag_tail"] = np.zeros(n, dtype=np.int64)
        self.arrays["q_lo"] = np.zeros(max(nq, 1), dtype=np.int64)
        kw = {k: _as_dp(self.arrays[k]) for k in SUMMARY_F64 + ("q",)}
        kw.update({k: _as_ip(self.arrays[k]) for k in ("lag_bulk", "lag_tail", "q_lo")})
        if not diagnostics:     # NULL members: the library skips the diagnostics kernels
            for k in ("rhat", "rhat_bulk", "rhat_tail", "ess_bulk", "ess_tail", "lag_bulk", "lag_tail"):
                kw[k] = None
        self.struct = Summary(**kw)

    def result(self) -> dict:
        P, nq = self.P, self.nq
        out = {k: self.arrays[k][:P].copy() for k in SUMMARY_F64 + ("lag_bulk", "lag_tail")}
        out["q"] = self.arrays["q"][:P * nq].reshape(P, nq).copy()
        out["q_lo"] = self.arrays["q_lo"][:nq].copy()
        return out


class _Core:
    """The handle of an mcr_ctx and what every call needs: the error check, device memory, summarize / enqueue / wait,
    moments, measurement and profiling."""

    def __init__(self, device: int | None = None):
        self.lib = load_library()
        if device is None:
            device = int(os.environ.get("MCMC_REF_HIP_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        h = C.c_void_p()
        rc = self.lib.mcr_init(int(device), C.byref(h))
        if rc != MCR_OK:
            msg = (self.lib.mcr_last_error(None) or b"").decode()
            if rc == MCR_ENODEVICE:
                raise HipUnavailableError(msg)
            raise McrError(rc, msg)
        self.handle = h
        self.device = int(device)
        self._pending: list[SummaryBuffers] = []

    def close(self):
        if getattr(self, "handle", None):
            self.lib.mcr_free(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass

    # -- errors ------------------------------------------------------------------------------
    def _check(self, rc: int):
        if rc != MCR_OK:
            raise McrError(rc, (self.lib.mcr_last_error(self.handle) or b"").decode())

    def _declined(self, rc: int, note: dict) -> bool:
        """Whether the library declined the call (MCR_EFALLBACK: the input is for the caller's host reader; its message
        goes to note["fallback"]).  Any other failure raises."""
        if rc == MCR_EFALLBACK:
            note["fallback"] = (self.lib.mcr_last_error(self.handle) or b"").decode(errors="replace")
            return True
        self._check(rc)
        return False

    def _answer(self, symbol: str, *args) -> int:
        """The int64 the entry `symbol` writes through its last parameter, after the handle and `args`."""
        v = C.c_int64(0)
        self._check(getattr(self.lib, symbol)(self.handle, *args, C.byref(v)))
        return int(v.value)

    # -- device memory --------------------------------------------------------------------------
    def upload(self, draws: np.ndarray, layout: str = "pcn") -> DeviceTensor:
        targs = tensor_args(draws, layout)
        if not draws.flags.c_contiguous:
            raise ValueError("upload() needs a C-contiguous array (permute the layout string instead)")
        with contextlib.ExitStack() as stack:
            buf = stack.enter_context(DeviceBuffer(self, max(draws.nbytes, 8))).upload(draws)
            stack.pop_all()
        return DeviceTensor(self, buf, targs)

    def alloc_tensor(self, C_: int, N: int, P: int, dtype=np.float64) -> DeviceTensor:
        """Uninitialised [P][C][N] device tensor (fill it with fill_synthetic)."""
        es = np.dtype(dtype).itemsize
        buf = DeviceBuffer(self, max(C_ * N * P * es, 8))
        code = MCR_F64 if np.dtype(dtype) == np.float64 else MCR_F32
        return DeviceTensor(self, buf, (code, C_, N, P, N, 1, C_ * N))

    def fill_synthetic(self, t: DeviceTensor, seed: int = 4711, p0: int = 0):
        """Synthetic stress draws; p0 > 0: `t` is the parameter block [p0, p0 + P) of a larger tensor."""
        code, C_, N, P = t.targs[:4]
        self._check(self.lib.mcr_fill_synthetic_at(self.handle, t.buf.ptr, code, C_, N, P, int(p0), seed))

    def hbm_probe(self, nbytes: int = 4 << 30, iters: int = 5) -> dict:
        """Measured HBM rates of this device (GB/s): read-only streaming kernel and device-to-device copy."""
        rd, cp = C.c_double(0.0), C.c_double(0.0)
        self._check(self.lib.mcr_hbm_probe(self.handle, int(nbytes), int(iters), C.byref(rd), C.byref(cp)))
        return {"read_GBps": rd.value, "copy_GBps": cp.value}

    def sync(self):
        self._check(self.lib.mcr_sync(self.handle))

    # -- hot path -----------------------------------------------------------------------------
    @staticmethod
    def _quantiles(quantiles):
        qs = np.ascontiguousarray(list(quantiles), dtype=np.float64)
        if qs.size > MCR_MAX_QUANTILES:
            raise ValueError(f"at most {MCR_MAX_QUANTILES} quantiles")
        return qs

    def summarize(self, draws, layout: str = "pcn", min_chains: int = 4,
                  quantiles=(0.05, 0.5, 0.95), diagnostics: bool = True) -> dict:
        """All per-parameter statistics of a host array or a DeviceTensor (synchronous).

        diagnostics=False: Backend.stats only (mean/std/quantiles/median); the rank, fold and
        autocovariance kernels are not launched and the diagnostics come back as NaN.
        """
        qs = self._quantiles(quantiles)
        if isinstance(draws, DeviceTensor) and draws.chain_off is not None:
            return self.summarize_chains(draws, min_chains=min_chains, quantiles=quantiles, diagnostics=diagnostics)
        if isinstance(draws, DeviceTensor):
            targs, ptr, fn = draws.targs, draws.buf.ptr, self.lib.mcr_summarize_dev
        else:
            targs, fn = tensor_args(draws, layout), self.lib.mcr_summarize
            ptr = draws.ctypes.data_as(C.c_void_p)
        bufs = SummaryBuffers(targs[3], qs.size, diagnostics)
        self._check(fn(self.handle, ptr, *targs, int(min_chains), _as_dp(qs), qs.size, C.byref(bufs.struct)))
        return bufs.result()

    def enqueue(self, t: DeviceTensor, min_chains: int = 4, quantiles=(0.05, 0.5, 0.95),
                diagnostics: bool = True, bufs: "SummaryBuffers | None" = None) -> SummaryBuffers:
        """Asynchronous summarize.  `bufs`: result buffers of an EARLIER, already delivered call of the same shape to
        write into again (a caller that streams many same-shape models keeps a ring of them instead of allocating
        twelve arrays per call)."""
        qs = self._quantiles(quantiles)
        if bufs is None or bufs.P != t.targs[3] or bufs.nq != qs.size or bufs.diagnostics != diagnostics:
            bufs = SummaryBuffers(t.targs[3], qs.size, diagnostics)
        if t.chain_off is not None:
            rc = self.lib.mcr_summarize_chains_enqueue(self.handle, t.buf.ptr, t.targs[6], _as_ip(t.chain_off), t.targs[1],
                                                       t.targs[3], int(min_chains), _as_dp(qs), qs.size,
                                                       C.byref(bufs.struct))
        else:
            rc = self.lib.mcr_summarize_enqueue(self.handle, t.buf.ptr, *t.targs, int(min_chains), _as_dp(qs), qs.size,
                                                C.byref(bufs.struct))
        self._check(rc)
        self._pending.append(bufs)
        return bufs

    def ragged_tensor(self, buf, counts, P: int, stride_p: int | None = None) -> DeviceTensor:
        """The DeviceTensor of f64 draws [P][M] already in `buf` whose chains are `counts` draws long, back to back in
        (chain, draw) order; parameter p starts at element p * stride_p (default M)."""
        counts = np.asarray(counts, dtype=np.int64).reshape(-1)
        off = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(counts, dtype=np.int64)])
        M = int(off[-1])
        n = int(counts.min()) if counts.size else 0
        return DeviceTensor(self, buf, (MCR_F64, int(counts.size), n, int(P), 0, 1, M if stride_p is None else int(stride_p)),
                            np.ascontiguousarray(off))

    def summarize_chains(self, draws, counts=None, min_chains: int = 4, quantiles=(0.05, 0.5, 0.95),
                         diagnostics: bool = True) -> dict:
        """All per-parameter statistics of draws [P][M] whose chains are `counts` draws long (chains of unequal length,
        mcr_summarize_chains_dev): ONE pipeline for all parameters.  `draws`: a host array [P][M] (uploaded for the
        call) or a DeviceTensor of ragged_tensor (then `counts` is not needed).  The result is shaped like
        summarize()'s: pooled mean / std / q / median, and the diagnostics of diagnostics.py for ragged chains."""
        qs = self._quantiles(quantiles)
        with contextlib.ExitStack() as stack:
            if isinstance(draws, DeviceTensor):
                t = draws if draws.chain_off is not None else self.ragged_tensor(draws.buf, counts, draws.targs[3])
            else:
                x = np.ascontiguousarray(draws, dtype=np.float64)
                if x.ndim != 2:
                    raise ValueError("draws must be 2-D [P][M]")
                if int(np.sum(counts)) != x.shape[1]:
                    raise ValueError("counts must add up to the number of draws per parameter")
                owned = stack.enter_context(DeviceBuffer(self, max(x.nbytes, 8)))
                if x.nbytes:
                    owned.upload(x)
                t = self.ragged_tensor(owned, counts, x.shape[0])
            bufs = SummaryBuffers(t.targs[3], qs.size, diagnostics)
            self._check(self.lib.mcr_summarize_chains_dev(self.handle, t.buf.ptr, t.targs[6], _as_ip(t.chain_off),
                                                          t.targs[1], t.targs[3], int(min_chains), _as_dp(qs), qs.size,
                                                          C.byref(bufs.struct)))
        return bufs.result()

    def summarize_models(self, tensors, min_chains: int = 4, quantiles=(0.05, 0.5, 0.95)) -> list[dict]:
        """One C call for a list of DeviceTensors (independent models), pipelined through the lanes."""
        qs = self._quantiles(quantiles)
        n = len(tensors)
        descs = (ModelDesc * max(n, 1))()
        outs = (Summary * max(n, 1))()
        bufs = []
        for i, t in enumerate(tensors):
            code, C_, N, P, sc, sn, sp = t.targs
            descs[i] = ModelDesc(t.buf.ptr, code, int(min_chains), C_, N, P, sc, sn, sp)
            b = SummaryBuffers(P, qs.size)
            outs[i] = b.struct
            bufs.append(b)
        self._check(self.lib.mcr_summarize_models(self.handle, descs, n, _as_dp(qs), qs.size, outs))
        return [b.result() for b in bufs]

    def wait(self):
        try:
            self._check(self.lib.mcr_summarize_wait(self.handle))
        finally:
            self._pending.clear()

    def wait_one(self) -> SummaryBuffers | None:
        """Wait for the oldest outstanding enqueue only; returns its buffers (None if nothing is pending)."""
        if not self._pending:
            return None
        bufs = self._pending.pop(0)
        self._check(self.lib.mcr_summarize_wait_one(self.handle))
        return bufs

    @property
    def inflight(self) -> int:
        return len(self._pending)

    def diagnose_chains(self, chains, min_chains: int = 4, debug: bool = False) -> dict:
        """split_rhat / ess_bulk / ess_tail of ONE parameter given as (possibly ragged) chains."""
        off = np.zeros(len(chains) + 1, dtype=np.int64)
        for i, c in enumerate(chains):
            off[i + 1] = off[i] + len(c)
        M = int(off[-1])
        pooled = np.empty(max(M, 1), dtype=np.float64)
        for i, c in enumerate(chains):
            pooled[off[i]:off[i + 1]] = np.asarray(c, dtype=np.float64)
        bufs = SummaryBuffers(1, 0)
        dbg = [np.full(max(M, 1), np.nan) for _ in range(4)] if debug else [None] * 4
        self._check(self.lib.mcr_diagnose_chains(self.handle, _as_dp(pooled), _as_ip(off), len(chains),
                                                 int(min_chains), C.byref(bufs.struct), *[_as_dp(d) for d in dbg]))
        r = bufs.result()
        out = {k: (float(r[k][0]) if k in SUMMARY_F64 else int(r[k][0]))
               for k in ("rhat", "rhat_bulk", "rhat_tail", "ess_bulk", "ess_tail", "median", "lag_bulk",
                         "lag_tail")}
        if debug:
            for name, d in zip(("z_bulk", "z_tail", "rank_bulk", "rank_tail"), dbg):
                out[name] = [d[off[i]:off[i + 1]].copy() for i in range(len(chains))]
        return out

    def basic_stats(self, values) -> dict:
        v = np.ascontiguousarray(values)
        if v.dtype not in (np.float64, np.float32):
            v = v.astype(np.float64)
        mean, std = C.c_double(math.nan), C.c_double(math.nan)
        self._check(self.lib.mcr_basic_stats(self.handle, v.ctypes.data_as(C.c_void_p), _dtype_code(v.dtype), v.size,
                                             C.byref(mean), C.byref(std)))
        return {"mean": mean.value, "std": std.value}

    def moments(self, t: DeviceTensor) -> tuple[np.ndarray, np.ndarray]:
        P = t.targs[3]
        mean, std = np.full(max(P, 1), np.nan), np.full(max(P, 1), np.nan)
        self._check(self.lib.mcr_moments_dev(self.handle, t.buf.ptr, *t.targs, _as_dp(mean), _as_dp(std)))
        return mean[:P], std[:P]

    # -- measurement -----------------------------------------------------------------------------
    def params_per_chunk(self, t: "DeviceTensor", diagnostics: bool = True) -> int:
        """Parameters per workspace chunk of a call on this tensor (mcr_plan_chunks): chunk k is [k * n, (k + 1) * n)."""
        _, C_, N, P, sc, sn, sp = t.targs
        if t.chain_off is not None:
            return self._answer("mcr_plan_chunks_chains", _as_ip(t.chain_off), C_, P, int(diagnostics))
        return self._answer("mcr_plan_chunks", C_, N, P, sc, sn, sp, int(diagnostics))

    def rho_guard_count(self) -> int:
        """Band lags of the tier-3 ESS scan re-derived with the reference's own sums so far (mcr_rho_guard_count)."""
        return self._answer("mcr_rho_guard_count")

    def tile_fallback_count(self) -> int:
        """Tiles the f64 tile sort sorted as (key, position) pairs after its record sort failed its order check, so far."""
        return self._answer("mcr_tile_fallback_count")

    def profile(self, on: bool):
        self._check(self.lib.mcr_profile_enable(self.handle, 1 if on else 0))

    def profile_reset(self):
        self._check(self.lib.mcr_profile_reset(self.handle))

    def profile_get(self) -> dict:
        arr = (KernelTime * 64)()
        n = C.c_int(0)
        self._check(self.lib.mcr_profile_get(self.handle, arr, 64, C.byref(n)))
        return {arr[i].name.decode(): {"launches": int(arr[i].launches), "total_ms": float(arr[i].total_ms)}
                for i in range(min(n.value, 64))}


class Context(_Core, _FileCalls, _StatCalls):
    """One GPU + one HIP stream (mcr_ctx).  Not thread-safe: one Context per thread."""

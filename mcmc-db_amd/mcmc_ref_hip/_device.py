"""The owners of device memory: every allocation a Context makes has exactly one of them, and each is a context manager.
They reach the library through the Context that made them (`ctx.lib`, `ctx.handle`, `ctx._check`).
"""
from __future__ import annotations

import ctypes as C
import typing

import numpy as np


class _Owner:
    """An owner of device memory is a context manager: leaving the `with` calls free(), and free() may be called again.
    A function that hands its allocation on enters it into a contextlib.ExitStack and ends with pop_all()."""

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()


class DeviceBuffer(_Owner):
    def __init__(self, ctx: "Context", nbytes: int):
        self.ctx, self.nbytes = ctx, nbytes
        self.ptr = C.c_void_p()
        ctx._check(ctx.lib.mcr_dev_alloc(ctx.handle, nbytes, C.byref(self.ptr)))

    def upload(self, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        self.ctx._check(self.ctx.lib.mcr_memcpy_h2d(self.ctx.handle, self.ptr, arr.ctypes.data_as(C.c_void_p),
                                                    arr.nbytes))
        return self

    def download(self, dtype, count: int) -> np.ndarray:
        out = np.empty(count, dtype=dtype)
        self.ctx._check(self.ctx.lib.mcr_memcpy_d2h(self.ctx.handle, out.ctypes.data_as(C.c_void_p), self.ptr,
                                                    out.nbytes))
        return out

    def free(self):
        if self.ptr:
            self.ctx.lib.mcr_dev_free(self.ctx.handle, self.ptr)
            self.ptr = C.c_void_p()


class DeviceArena(_Owner):
    """One device allocation shared by the models of a batch (hipMalloc / hipFree cost ~0.1 ms each, which
    would dominate a 57-file corpus pass).  Its maker holds it until free() -- the end of the maker's `with` -- and every
    view holds it too: the buffer is freed with the last of them, at once when no view is left."""

    def __init__(self, ctx, nbytes: int):
        self.buf = DeviceBuffer(ctx, max(nbytes, 8))
        self.refs, self.held = 1, True

    def view(self, offset: int, nbytes: int) -> "DeviceView":
        self.refs += 1
        return DeviceView(self, offset, nbytes)

    def release(self):
        self.refs -= 1
        if self.refs <= 0:
            self.buf.free()

    def free(self):
        if self.held:
            self.held = False
            self.release()


class DeviceView(_Owner):
    """Slice of an arena with DeviceBuffer's interface (ptr / download / free)."""

    def __init__(self, arena: DeviceArena, offset: int, nbytes: int):
        self.arena, self.ctx, self.nbytes = arena, arena.buf.ctx, nbytes
        self.ptr = C.c_void_p(arena.buf.ptr.value + offset)

    def download(self, dtype, count: int) -> np.ndarray:
        out = np.empty(count, dtype=dtype)
        if out.nbytes:
            self.ctx._check(self.ctx.lib.mcr_memcpy_d2h(self.ctx.handle, out.ctypes.data_as(C.c_void_p), self.ptr, out.nbytes))
        return out

    def share(self) -> "DeviceView":
        """Another view of the same bytes; the arena lives until both are freed."""
        return self.arena.view(self.ptr.value - self.arena.buf.ptr.value, self.nbytes)

    def free(self):
        if self.arena is not None:
            self.arena.release()
            self.arena = None
            self.ptr = C.c_void_p()


class DeviceTensor(_Owner):
    """A draw tensor resident in HBM: device buffer + the (dtype, dims, strides) it was uploaded with.

    chain_off (int64, C + 1 offsets) marks f64 draws [P][M] whose chains differ in length (Context.ragged_tensor): the
    calls that take a tensor then use the ragged entry points; targs = (MCR_F64, C, shortest chain, P, 0, 1, stride_p)."""

    def __init__(self, ctx: "Context", buf: DeviceBuffer, targs, chain_off: np.ndarray | None = None):
        self.ctx, self.buf, self.targs, self.chain_off = ctx, buf, targs, chain_off

    @property
    def shape_cnp(self):
        return self.targs[1:4]

    def free(self):
        self.buf.free()


class DeviceSims(_Owner):
    """The draw tensors of S simulations resident in HBM (Context.upload_sims): device buffer + tensor4_args' nine entries
    (dtype, S, C, N, P and their strides).  Only Context.sbc_ranks takes it; it is NOT a DeviceTensor, so that no call on
    one (C, N, P) tensor can read the nine entries as seven."""

    def __init__(self, ctx: "Context", buf, targs):
        if len(targs) != 9:
            raise ValueError("DeviceSims needs (dtype, S, C, N, P, stride_s, stride_c, stride_n, stride_p)")
        self.ctx, self.buf, self.targs = ctx, buf, tuple(targs)

    @property
    def shape_scnp(self):
        return self.targs[1:5]

    def free(self):
        self.buf.free()


class CsvTable(typing.NamedTuple):
    """One file of Context.csv_table_decode.  close() frees the slices."""
    names: list            # parameter names in file order, without `chain` / `draw`
    values: DeviceView     # [P][M] f64 in file row order
    all_int: np.ndarray    # [P] bool: every literal of the column is an integer
    ids: tuple             # (chain, draw) as int64 DeviceViews of M entries, None for an absent column
    hard: int              # fields finished on the host
    header: list           # every column name of the file

    def close(self):
        for b in (self.values, *self.ids):
            if b is not None:
                b.free()

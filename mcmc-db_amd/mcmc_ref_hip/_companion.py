"""What the companion libraries -- libmcmcref_iess.so (`_iabi`), libmcmcref_bm.so (`_babi`), libmcmcref_std.so (`_sabi`),
each a shared object of its own next to libmcmcref_hip.so -- have in common on the Python side: the description of one
(`Companion`), its lazy loader, the handle class, the error of an entry that takes no handle, the per-Context handle
cache, the limit / profile / kernel_ms calls and the choice between a library's host and device entry for a tensor.
Imports `_abi` only; `_ffi` knows nothing of this module or of the companions.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
import weakref

import numpy as np

from ._abi import DEFAULT_LIB, MCR_ENODEVICE, MCR_OK, HipUnavailableError, McrError, _as_dp, load_library, tensor_args


class Handle:
    """A companion library's handle on one device: the owner of what the library keeps there (`companion`: which one)."""
    companion: "Companion"

    def __init__(self, device: int = 0):
        self.lib = self.companion.load()
        h = C.c_void_p()
        rc = self._fn("init")(int(device), C.byref(h))
        if rc != MCR_OK:
            msg = (self._fn("last_error")(None) or b"").decode()
            if rc == MCR_ENODEVICE:
                raise HipUnavailableError(msg)
            raise McrError(rc, msg)
        self.handle, self.device = h, int(device)

    def _fn(self, name: str):
        return getattr(self.lib, self.companion.prefix + name)

    def check(self, rc: int):
        if rc != MCR_OK:
            raise McrError(rc, (self._fn("last_error")(self.handle) or b"").decode())

    def close(self):
        if getattr(self, "handle", None):
            self._fn("free")(self.handle)
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


class Companion:
    """One companion library: the prefix of its entries ("mci_"), its file beside the main library, the environment
    variable that names another file, its symbol table (name -> (restype, argtypes)) and whether the main library has to be
    loaded before it; the name and the docstring of its handle class."""

    def __init__(self, prefix: str, file: str, env: str, symbols: dict, handle_name: str, handle_doc: str, main_first: bool = False):
        self.prefix, self.env, self.symbols, self.main_first = prefix, env, symbols, main_first
        self.Handle = type(handle_name, (Handle,), {"companion": self, "__doc__": handle_doc})      # its handle class
        self.default_path = DEFAULT_LIB.with_name(file)
        self._lib, self._lock = None, threading.Lock()
        self._handles: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()      # Context -> Handle

    def load(self):
        """dlopen the library (after the main one where it needs that) and bind every entry its header declares; works
        without a GPU."""
        with self._lock:
            if self._lib is None:
                if self.main_first:
                    load_library()
                path = type(self.default_path)(os.environ.get(self.env, str(self.default_path)))
                if not path.exists():
                    raise HipUnavailableError(f"{path} not found: build it with `python mcmc-db_amd/build.py` "
                                              "(there is no CPU fallback)")
                try:
                    L = C.CDLL(str(path))
                except OSError as exc:
                    raise HipUnavailableError(f"cannot load {path}: {exc}") from exc
                for name, (res, args) in self.symbols.items():
                    fn = getattr(L, name)
                    fn.restype = res
                    fn.argtypes = args
                self._lib = L
        return self._lib

    def host_check(self, rc: int):
        """Raise the error of a call that takes no handle."""
        if rc != MCR_OK:
            raise McrError(rc, (getattr(self.load(), self.prefix + "last_error")(None) or b"").decode())

    def handle(self, ctx) -> Handle:
        """The library's handle on the Context's device: made at the first call, freed with the context."""
        h = self._handles.get(ctx)
        if h is None or h.handle is None:
            h = self._handles[ctx] = self.Handle(ctx.device)
            weakref.finalize(ctx, h.close)
        return h

    def set_workspace_limit(self, ctx, nbytes: int) -> None:
        h = self.handle(ctx)
        h.check(h._fn("set_workspace_limit")(h.handle, int(nbytes)))

    def plan(self, ctx, entry: str, *args) -> int:
        """Parameters per chunk, from the library's plan entry (its last argument receives them)."""
        h, v = self.handle(ctx), C.c_int64(0)
        h.check(getattr(h.lib, entry)(h.handle, *args, C.byref(v)))
        return int(v.value)

    def profile(self, ctx, on: bool) -> None:
        h = self.handle(ctx)
        h.check(h._fn("profile_enable")(h.handle, int(bool(on))))

    def kernel_ms(self, ctx, names: tuple) -> dict:
        h = self.handle(ctx)
        ms = np.zeros(len(names))
        h.check(h._fn("kernel_ms")(h.handle, _as_dp(ms), len(names)))
        return dict(zip(names, (float(v) for v in ms)))


def device_tensor(draws):
    """`draws` if it is a DeviceTensor (duck-typed: this module does not import `_device`) of equal chains, else None."""
    if not hasattr(draws, "targs"):
        return None
    if draws.chain_off is not None:
        raise ValueError("chains of different lengths are not supported")
    return draws


def tensor_entry(draws, layout: str, entry: str):
    """(the entry's name, pointer, tensor arguments) of a DeviceTensor (`entry` + "_dev") or a numpy array (`entry`)."""
    t = device_tensor(draws)
    if t is not None:
        return entry + "_dev", t.buf.ptr, t.targs
    draws = np.asarray(draws)
    return entry, draws.ctypes.data_as(C.c_void_p), tensor_args(draws, layout)

"""The Python mirror of include/mcmcref_bm.h, the ABI of the companion library libmcmcref_bm.so (`mcb_*` entries, `MCB_*`
constants): batch means, the long-run covariance and what the mean test and the multivariate ESS need of them.  The
library is a third shared object next to libmcmcref_hip.so and is loaded lazily, by the first call that needs it.  Imports
`_abi` only (return codes, the error types, pointer helpers); `_ffi` imports neither this module nor `batchmeans`.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

from ._abi import DEFAULT_LIB, MCR_ENODEVICE, MCR_OK, HipUnavailableError, McrError, _I64, _dp, _ip

MCB_VERSION = 100
MCB_BLOCK = 1024
MCB_KERNEL_TIME, MCB_KERNEL_TILE, MCB_KERNEL_MEAN, MCB_KERNEL_FINISH, MCB_KERNEL_POOL, MCB_KERNEL_POOLED = range(6)
MCB_KERNELS = 6

KERNEL_NAMES = ("time", "tile", "mean", "finish", "pool", "pooled")      # mcb_kernel_ms, in order

_vp = C.c_void_p
_TENSOR = [_vp, C.c_int, _I64, _I64, _I64, _I64, _I64, _I64]
_FINISH = [_I64, _I64, _I64, _I64, C.c_int]                               # P, b, A, A3, r
BSYMBOLS = {
    "mcb_version": (C.c_int, []),
    "mcb_init": (C.c_int, [C.c_int, C.POINTER(_vp)]),
    "mcb_free": (None, [_vp]),
    "mcb_last_error": (C.c_char_p, [_vp]),
    "mcb_set_workspace_limit": (C.c_int, [_vp, C.c_size_t]),
    "mcb_batch_size": (C.c_int, [_I64, C.c_int, _ip, _ip]),
    "mcb_batch_means_dev": (C.c_int, [_vp] + _TENSOR + [_I64, _vp, _I64, _vp]),
    "mcb_batch_means": (C.c_int, [_vp] + _TENSOR + [_I64, _dp, _I64, _dp]),
    "mcb_batch_means_host": (C.c_int, _TENSOR + [_I64, _dp, _I64, _dp]),
    "mcb_pooled_dev": (C.c_int, [_vp] + _TENSOR + [_vp, _I64]),
    "mcb_lrv_finish_dev": (C.c_int, [_vp, _vp, _vp] + _FINISH + [_vp]),
    "mcb_lrv_finish_host": (C.c_int, [_dp, _dp] + _FINISH + [_dp]),
    "mcb_pool_dev": (C.c_int, [_vp, _vp, _vp, _I64, _vp, _vp, _I64, _I64, _dp, C.c_double, _vp, _vp, _vp, _ip]),
    "mcb_pool_host": (C.c_int, [_dp, _dp, _I64, _dp, _dp, _I64, _I64, _dp, C.c_double, _dp, _dp, _dp, _ip]),
    "mcb_tree_sum_host": (C.c_int, [_dp, _I64, C.c_int, _dp]),
    "mcb_profile_enable": (C.c_int, [_vp, C.c_int]),
    "mcb_kernel_ms": (C.c_int, [_vp, _dp, C.c_int]),
}

DEFAULT_BM_LIB = DEFAULT_LIB.with_name("libmcmcref_bm.so")

_lib = None
_lib_lock = threading.Lock()


def load_bm_library():
    """dlopen libmcmcref_bm.so and bind every entry its header declares (works without a GPU)."""
    global _lib
    with _lib_lock:
        if _lib is None:
            path = type(DEFAULT_BM_LIB)(os.environ.get("MCMC_REF_HIP_BM_LIB", str(DEFAULT_BM_LIB)))
            if not path.exists():
                raise HipUnavailableError(f"{path} not found: build it with `python mcmc-db_amd/build.py` "
                                          "(there is no CPU fallback)")
            try:
                L = C.CDLL(str(path))
            except OSError as exc:
                raise HipUnavailableError(f"cannot load {path}: {exc}") from exc
            for name, (res, args) in BSYMBOLS.items():
                fn = getattr(L, name)
                fn.restype = res
                fn.argtypes = args
            _lib = L
    return _lib


def host_check(rc: int):
    """Raise the error of a call that takes no handle."""
    if rc != MCR_OK:
        raise McrError(rc, (load_bm_library().mcb_last_error(None) or b"").decode())


class BmHandle:
    """An mcb handle on one device: the owner of the companion library's stream and workspace there."""

    def __init__(self, device: int = 0):
        self.lib = load_bm_library()
        h = _vp()
        rc = self.lib.mcb_init(int(device), C.byref(h))
        if rc != MCR_OK:
            msg = (self.lib.mcb_last_error(None) or b"").decode()
            if rc == MCR_ENODEVICE:
                raise HipUnavailableError(msg)
            raise McrError(rc, msg)
        self.handle, self.device = h, int(device)

    def check(self, rc: int):
        if rc != MCR_OK:
            raise McrError(rc, (self.lib.mcb_last_error(self.handle) or b"").decode())

    def close(self):
        if getattr(self, "handle", None):
            self.lib.mcb_free(self.handle)
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

"""The Python mirror of include/mcmcref_iess.h, the ABI of the companion library libmcmcref_iess.so (`mci_*` entries,
`MCI_*` constants): the ESS of an indicator of the draws from bit-packed chains.  The library is a second shared object
next to libmcmcref_hip.so and is loaded lazily, by the first call that needs it.  Imports `_abi` only (return codes, the
error types, pointer helpers); `_ffi` imports neither this module nor `indicator`.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

from ._abi import DEFAULT_LIB, MCR_ENODEVICE, MCR_OK, HipUnavailableError, McrError, _I64, _dp, _ip

MCI_VERSION = 100
MCI_MAX_REQUESTS = 32
MCI_MAX_DRAWS = 1048576
MCI_LAG_BLOCK = 256
MCI_LDS_WORDS = 8192
MCI_KERNEL_PACK, MCI_KERNEL_LAG = 0, 1
MCI_KERNELS = 2

KERNEL_NAMES = ("pack", "lag")                                # mci_kernel_ms, in order

_vp = C.c_void_p
_TENSOR = [_vp, C.c_int, _I64, _I64, _I64, _I64, _I64, _I64]
_REQUESTS = [_dp, _dp, C.c_int, _dp, _ip, _ip]                # lower, upper, K, ess, trunc, ones
ISYMBOLS = {
    "mci_version": (C.c_int, []),
    "mci_init": (C.c_int, [C.c_int, C.POINTER(_vp)]),
    "mci_free": (None, [_vp]),
    "mci_last_error": (C.c_char_p, [_vp]),
    "mci_set_workspace_limit": (C.c_int, [_vp, C.c_size_t]),
    "mci_indicator_plan": (C.c_int, [_vp, C.c_int, _I64, _I64, _I64, C.c_int, _ip]),
    "mci_indicator_ess_dev": (C.c_int, [_vp] + _TENSOR + _REQUESTS),
    "mci_indicator_ess": (C.c_int, [_vp] + _TENSOR + _REQUESTS),
    "mci_indicator_ess_host": (C.c_int, [_dp, _I64, _I64] + _REQUESTS),
    "mci_profile_enable": (C.c_int, [_vp, C.c_int]),
    "mci_kernel_ms": (C.c_int, [_vp, _dp, C.c_int]),
}

DEFAULT_IESS_LIB = DEFAULT_LIB.with_name("libmcmcref_iess.so")

_lib = None
_lib_lock = threading.Lock()


def load_iess_library():
    """dlopen libmcmcref_iess.so and bind every entry its header declares (works without a GPU)."""
    global _lib
    with _lib_lock:
        if _lib is None:
            path = type(DEFAULT_IESS_LIB)(os.environ.get("MCMC_REF_HIP_IESS_LIB", str(DEFAULT_IESS_LIB)))
            if not path.exists():
                raise HipUnavailableError(f"{path} not found: build it with `python mcmc-db_amd/build.py` "
                                          "(there is no CPU fallback)")
            try:
                L = C.CDLL(str(path))
            except OSError as exc:
                raise HipUnavailableError(f"cannot load {path}: {exc}") from exc
            for name, (res, args) in ISYMBOLS.items():
                fn = getattr(L, name)
                fn.restype = res
                fn.argtypes = args
            _lib = L
    return _lib


class IessHandle:
    """An mci handle on one device: the owner of the companion library's stream and workspace there."""

    def __init__(self, device: int = 0):
        self.lib = load_iess_library()
        h = _vp()
        rc = self.lib.mci_init(int(device), C.byref(h))
        if rc != MCR_OK:
            msg = (self.lib.mci_last_error(None) or b"").decode()
            if rc == MCR_ENODEVICE:
                raise HipUnavailableError(msg)
            raise McrError(rc, msg)
        self.handle, self.device = h, int(device)

    def check(self, rc: int):
        if rc != MCR_OK:
            raise McrError(rc, (self.lib.mci_last_error(self.handle) or b"").decode())

    def close(self):
        if getattr(self, "handle", None):
            self.lib.mci_free(self.handle)
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

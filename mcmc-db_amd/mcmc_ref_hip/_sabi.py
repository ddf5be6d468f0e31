"""The Python mirror of include/mcmcref_std.h, the ABI of the companion library libmcmcref_std.so (`mcs_*` entries,
`MCS_*` constants): R-hat and ESS in the Stan convention -- split chains, Blom scores, Geyer's initial sequences.  The
library is a further shared object next to libmcmcref_hip.so -- it carries its own copy of the main library's sort stage
and summary pipeline -- and is loaded lazily, by the first call that needs it, after the main one.  Imports `_abi` only
(return codes, the error types, pointer helpers); `_ffi` imports neither this module nor `standard`.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

from ._abi import DEFAULT_LIB, MCR_ENODEVICE, MCR_OK, HipUnavailableError, McrError, _I64, _dp, _ip, load_library

MCS_VERSION = 100
MCS_MAX_DRAWS = 1048576
MCS_LAG_BLOCK = 256
MCS_LDS_DRAWS = 7680
MCS_WANT_BASIC = 1
MCS_KERNEL_PIPE, MCS_KERNEL_SERIES, MCS_KERNEL_WALK = 0, 1, 2
MCS_KERNELS = 3

KERNEL_NAMES = ("pipe", "series", "walk")                     # mcs_kernel_ms, in order
DOUBLE_OUTPUTS = ("rhat", "rhat_bulk", "rhat_tail", "ess_bulk", "ess_tail", "ess_q05", "ess_q95", "margin", "rhat_basic",
                  "ess_mean", "mcse_mean")                    # the outputs of a diagnostics entry, in its order
INT_OUTPUTS = ("lag_bulk", "lag_q05", "lag_q95", "lag_mean")

_vp = C.c_void_p
_TENSOR = [_vp, C.c_int, _I64, _I64, _I64, _I64, _I64, _I64]
_OUTS = [_dp] * len(DOUBLE_OUTPUTS) + [_ip] * len(INT_OUTPUTS)
SSYMBOLS = {
    "mcs_version": (C.c_int, []),
    "mcs_init": (C.c_int, [C.c_int, C.POINTER(_vp)]),
    "mcs_free": (None, [_vp]),
    "mcs_last_error": (C.c_char_p, [_vp]),
    "mcs_set_workspace_limit": (C.c_int, [_vp, C.c_size_t]),
    "mcs_plan": (C.c_int, [_vp, C.c_int, _I64, _I64, _I64, _I64, _I64, _I64, C.c_int, _ip]),
    "mcs_diagnostics_dev": (C.c_int, [_vp] + _TENSOR + [C.c_int] + _OUTS),
    "mcs_diagnostics": (C.c_int, [_vp] + _TENSOR + [C.c_int] + _OUTS),
    "mcs_diagnostics_host": (C.c_int, [_dp, _I64, _I64, C.c_int] + _OUTS),
    "mcs_profile_enable": (C.c_int, [_vp, C.c_int]),
    "mcs_kernel_ms": (C.c_int, [_vp, _dp, C.c_int]),
}

DEFAULT_STD_LIB = DEFAULT_LIB.with_name("libmcmcref_std.so")

_lib = None
_lib_lock = threading.Lock()


def load_std_library():
    """dlopen libmcmcref_std.so, after the main library, and bind every entry its header declares (works without a GPU)."""
    global _lib
    with _lib_lock:
        if _lib is None:
            load_library()
            path = type(DEFAULT_STD_LIB)(os.environ.get("MCMC_REF_HIP_STD_LIB", str(DEFAULT_STD_LIB)))
            if not path.exists():
                raise HipUnavailableError(f"{path} not found: build it with `python mcmc-db_amd/build.py` "
                                          "(there is no CPU fallback)")
            try:
                L = C.CDLL(str(path))
            except OSError as exc:
                raise HipUnavailableError(f"cannot load {path}: {exc}") from exc
            for name, (res, args) in SSYMBOLS.items():
                fn = getattr(L, name)
                fn.restype = res
                fn.argtypes = args
            _lib = L
    return _lib


class StdHandle:
    """An mcs handle on one device: the owner of the companion library's context there."""

    def __init__(self, device: int = 0):
        self.lib = load_std_library()
        h = _vp()
        rc = self.lib.mcs_init(int(device), C.byref(h))
        if rc != MCR_OK:
            msg = (self.lib.mcs_last_error(None) or b"").decode()
            if rc == MCR_ENODEVICE:
                raise HipUnavailableError(msg)
            raise McrError(rc, msg)
        self.handle, self.device = h, int(device)

    def check(self, rc: int):
        if rc != MCR_OK:
            raise McrError(rc, (self.lib.mcs_last_error(self.handle) or b"").decode())

    def close(self):
        if getattr(self, "handle", None):
            self.lib.mcs_free(self.handle)
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

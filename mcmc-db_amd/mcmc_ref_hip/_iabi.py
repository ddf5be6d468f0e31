"""The Python mirror of include/mcmcref_iess.h, the ABI of the companion library libmcmcref_iess.so (`mci_*` entries,
`MCI_*` constants): the ESS of an indicator of the draws from bit-packed chains.  The library is a second shared object
next to libmcmcref_hip.so and is loaded lazily, by the first call that needs it (`_companion`: the loader and the handle).
Imports `_abi` and `_companion` only; `_ffi` imports neither this module nor `indicator`.
"""
from __future__ import annotations

import ctypes as C

from ._abi import _I64, _dp, _ip
from ._companion import Companion

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

IESS = Companion("mci_", "libmcmcref_iess.so", "MCMC_REF_HIP_IESS_LIB", ISYMBOLS, "IessHandle",
                 "An mci handle on one device: the owner of the companion library's stream and workspace there.")
DEFAULT_IESS_LIB = IESS.default_path
load_iess_library = IESS.load
IessHandle = IESS.Handle

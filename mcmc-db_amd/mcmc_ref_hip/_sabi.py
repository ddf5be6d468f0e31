"""The Python mirror of include/mcmcref_std.h, the ABI of the companion library libmcmcref_std.so (`mcs_*` entries,
`MCS_*` constants): R-hat and ESS in the Stan convention -- split chains, Blom scores, Geyer's initial sequences.  The
library is a further shared object next to libmcmcref_hip.so -- it carries its own copy of the main library's sort stage
and summary pipeline -- and is loaded lazily, by the first call that needs it, after the main one (`_companion`: the loader
and the handle).  Imports `_abi` and `_companion` only; `_ffi` imports neither this module nor `standard`.
"""
from __future__ import annotations

import ctypes as C

from ._abi import _I64, _dp, _ip
from ._companion import Companion

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

STD = Companion("mcs_", "libmcmcref_std.so", "MCMC_REF_HIP_STD_LIB", SSYMBOLS, "StdHandle",
                "An mcs handle on one device: the owner of the companion library's context there.", main_first=True)
DEFAULT_STD_LIB = STD.default_path
load_std_library = STD.load
StdHandle = STD.Handle

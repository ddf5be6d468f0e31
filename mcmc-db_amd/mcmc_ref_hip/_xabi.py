"""The Python mirror of include/mcmcref_hip_ext.h, the extension ABI (`mcrx_*` entries, `MCRX_*` constants): what was
added to the library after the surface of mcmcref_hip.h and `_abi.SYMBOLS` was frozen.  `bind(lib)` sets restype and
argtypes once on the handle `_abi.load_library()` returns.  Imports `_abi` only; `_ffi` imports neither this module nor
`gaussian`.
"""
from __future__ import annotations

import ctypes as C

from ._abi import _I64, _dp, _ip

MCRX_LINALG_MAX_P = 8192
MCRX_CHOL_NB = 64
MCRX_G_D2_REF, MCRX_G_D2_ACT, MCRX_G_TRACE_REF, MCRX_G_TRACE_ACT = 0, 1, 2, 3
MCRX_G_LOGDET_REF, MCRX_G_LOGDET_ACT, MCRX_G_KL_ACT_REF, MCRX_G_KL_REF_ACT = 4, 5, 6, 7
MCRX_G_OUT = 8
MCRX_G_P_LIVE, MCRX_G_INFO_REF, MCRX_G_INFO_ACT = 0, 1, 2
MCRX_G_INFO = 3

GAUSSIAN_KEYS = ("d2_ref", "d2_act", "trace_ref", "trace_act", "logdet_ref", "logdet_act", "kl_act_ref", "kl_ref_act")   # out8, in order
GAUSSIAN_INFO_KEYS = ("p_live", "info_ref", "info_act")                                                                  # info3, in order

_vp = C.c_void_p
_GAUSS = [_I64, _I64, _dp, C.c_double, _dp, _ip, _dp]        # Ma, P, scale, jitter, out8, info3, shift behind (ref, Mr, act)
XSYMBOLS = {
    "mcrx_cholesky_dev": (C.c_int, [_vp, _vp, _I64, _I64, _ip, _dp]),
    "mcrx_cholesky": (C.c_int, [_vp, _dp, _I64, _I64, _dp, _ip, _dp]),
    "mcrx_cholesky_host": (C.c_int, [_dp, _I64, _I64, _dp, _ip, _dp]),
    "mcrx_solve_lower_dev": (C.c_int, [_vp, _vp, _I64, _I64, _vp, _I64, _I64]),
    "mcrx_solve_lower": (C.c_int, [_vp, _dp, _I64, _I64, _dp, _I64, _I64, _dp]),
    "mcrx_solve_lower_host": (C.c_int, [_dp, _I64, _I64, _dp, _I64, _I64, _dp]),
    "mcrx_gaussian_check": (C.c_int, [_vp, _dp, _I64, _dp] + _GAUSS),
    "mcrx_gaussian_check_dev": (C.c_int, [_vp, _vp, _I64, _vp] + _GAUSS),
    "mcrx_gaussian_check_host": (C.c_int, [_dp, _I64, _dp] + _GAUSS),
    "mcrx_gaussian_workspace": (C.c_int, [_vp, _I64, _I64, _I64, C.POINTER(C.c_size_t)]),
}


def bind(lib):
    """restype / argtypes of every extension entry on `lib` (once per handle); returns `lib`.  AttributeError when the
    library is older than this mirror."""
    if not getattr(lib, "_mcrx_bound", False):
        for name, (res, args) in XSYMBOLS.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        lib._mcrx_bound = True
    return lib

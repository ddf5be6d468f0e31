"""The Python mirror of include/mcmcref_recdf.h, the ABI of the companion library libmcmcref_recdf.so (`mce_*` entries,
`MCE_*` constants): the per-chain rank-ECDF uniformity test with simultaneous bands.  The library is a further shared
object next to libmcmcref_hip.so -- as libmcmcref_std.so it carries its own copy of the main library's sort stage and
summary pipeline -- and is loaded lazily, by the first call that needs it, after the main one (`_companion`: the loader
and the handle).  Imports `_abi` and `_companion` only; `_ffi` imports neither this module nor `rankecdf`.
"""
from __future__ import annotations

import ctypes as C

from ._abi import _I64, _dp, _ip
from ._companion import Companion

MCE_VERSION = 100
MCE_MAX_POINTS = 1024
MCE_MAX_TABLE = 134217728
MCE_HIST_BYTES = 24576
MCE_SLICE_DRAWS = 16384
MCE_KERNEL_FILL, MCE_KERNEL_PIPE, MCE_KERNEL_COUNT, MCE_KERNEL_STAT = 0, 1, 2, 3
MCE_KERNELS = 4

KERNEL_NAMES = ("fill", "pipe", "count", "stat")              # mce_kernel_ms, in order
# the outputs of a rank-ECDF entry, in its order: (name, numpy dtype, shape as a function of (P, C, K))
OUTPUTS = (("counts", "int32", lambda P, C_, K: (P, C_, K - 1)), ("pooled", "int32", lambda P, C_, K: (P, K - 1)),
           ("tied", "int32", lambda P, C_, K: (P,)), ("u", "float64", lambda P, C_, K: (P, C_)),
           ("kmin", "int32", lambda P, C_, K: (P, C_)), ("dev", "int64", lambda P, C_, K: (P, C_)),
           ("g", "float64", lambda P, C_, K: (P,)), ("chain", "int32", lambda P, C_, K: (P,)))

_vp = C.c_void_p
_i32p = C.POINTER(C.c_int32)
_TENSOR = [_vp, C.c_int, _I64, _I64, _I64, _I64, _I64, _I64]
_OUTS = [_i32p, _i32p, _i32p, _dp, _i32p, _ip, _dp, _i32p]
ESYMBOLS = {
    "mce_version": (C.c_int, []),
    "mce_init": (C.c_int, [C.c_int, C.POINTER(_vp)]),
    "mce_free": (None, [_vp]),
    "mce_last_error": (C.c_char_p, [_vp]),
    "mce_set_workspace_limit": (C.c_int, [_vp, C.c_size_t]),
    "mce_plan": (C.c_int, [_vp, C.c_int, _I64, _I64, _I64, _I64, _I64, _I64, C.c_int, _ip]),
    "mce_null_plan": (C.c_int, [_vp, _I64, _I64, C.c_int, _I64, _ip]),
    "mce_rank_ecdf_dev": (C.c_int, [_vp] + _TENSOR + [C.c_int] + _OUTS),
    "mce_rank_ecdf": (C.c_int, [_vp] + _TENSOR + [C.c_int] + _OUTS),
    "mce_null_sample": (C.c_int, [_vp, _I64, _I64, C.c_int, _I64, C.c_uint64, _dp]),
    "mce_rank_ecdf_host": (C.c_int, [_dp, _I64, _I64, C.c_int, _dp] + _OUTS),
    "mce_null_sample_host": (C.c_int, [_I64, _I64, C.c_int, _I64, C.c_uint64, _dp]),
    "mce_table_host": (C.c_int, [_I64, _I64, C.c_int, _dp]),
    "mce_profile_enable": (C.c_int, [_vp, C.c_int]),
    "mce_kernel_ms": (C.c_int, [_vp, _dp, C.c_int]),
}

RECDF = Companion("mce_", "libmcmcref_recdf.so", "MCMC_REF_HIP_RECDF_LIB", ESYMBOLS, "RecdfHandle",
                  "An mce handle on one device: the owner of the companion library's context and table there.", main_first=True)
DEFAULT_RECDF_LIB = RECDF.default_path
load_recdf_library = RECDF.load
RecdfHandle = RECDF.Handle

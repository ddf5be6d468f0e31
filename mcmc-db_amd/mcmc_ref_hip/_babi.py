"""The Python mirror of include/mcmcref_bm.h, the ABI of the companion library libmcmcref_bm.so (`mcb_*` entries, `MCB_*`
constants): batch means, the long-run covariance and what the mean test and the multivariate ESS need of them.  The
library is a third shared object next to libmcmcref_hip.so and is loaded lazily, by the first call that needs it
(`_companion`: the loader and the handle).  Imports `_abi` and `_companion` only; `_ffi` imports neither this module nor
`batchmeans`.
"""
from __future__ import annotations

import ctypes as C

from ._abi import _I64, _dp, _ip
from ._companion import Companion

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

BM = Companion("mcb_", "libmcmcref_bm.so", "MCMC_REF_HIP_BM_LIB", BSYMBOLS, "BmHandle",
               "An mcb handle on one device: the owner of the companion library's stream and workspace there.")
DEFAULT_BM_LIB = BM.default_path
load_bm_library = BM.load
host_check = BM.host_check
BmHandle = BM.Handle

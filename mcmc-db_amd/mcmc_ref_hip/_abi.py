"""The Python statement of include/mcmcref_hip.h, and nothing else: its constants, its structures, (restype, argtypes)
of every entry (`SYMBOLS`), the loader that binds them, and the helpers that turn numpy arrays into the header's
pointer and tensor arguments.  Kept by hand; tests/test_abi_mirror_cpu.py compares all of it with the header.

If the shared library is missing `load_library` raises `HipUnavailableError`: there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from pathlib import Path

import numpy as np

MCR_OK = 0
MCR_EINVAL, MCR_EMINCHAINS, MCR_EMINCHAINS_ARG, MCR_ENONFINITE = -1, -2, -3, -4
MCR_EHIP, MCR_ENOMEM, MCR_ENODEVICE, MCR_ECOMM, MCR_ELAYOUT = -5, -6, -7, -8, -9
MCR_EFALLBACK = -10        # mcr_json_*: the document is for the caller's host reader
MCR_F64, MCR_F32 = 0, 1
MCR_MAX_QUANTILES = 32
MCR_MAX_INFLIGHT = 8


_PKG = Path(__file__).resolve().parent
DEFAULT_LIB = _PKG.parent / "lib" / "libmcmcref_hip.so"


class HipUnavailableError(RuntimeError):
    """libmcmcref_hip.so could not be loaded, or no MI355X/HIP device is usable."""


class McrError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"[mcr {code}] {message}")
        self.code = code
        self.message = message


_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int64)


class Summary(C.Structure):
    _fields_ = [(n, _dp) for n in ("mean", "std", "q", "median", "rhat", "rhat_bulk", "rhat_tail",
                                   "ess_bulk", "ess_tail")] + \
               [("lag_bulk", _ip), ("lag_tail", _ip), ("q_lo", _ip)]


NESTED_FIELDS = ("nrhat", "nrhat_bulk", "nrhat_tail", "nrhat_raw", "between_bulk", "within_bulk", "between_tail",
                 "within_tail", "between_raw", "within_raw")
MCR_NESTED_MAX_CHAINS, MCR_NESTED_BLOCK = 1048576, 512     # mcr_nested_rhat's chain limit, k_chain_moments' register block


class Nested(C.Structure):
    _fields_ = [(n, _dp) for n in NESTED_FIELDS]


MCR_PARETO_LDS_TAIL = 8192                                  # the longest tail k_pareto_fit stages in LDS


class Pareto(C.Structure):
    _fields_ = [("khat", _dp), ("khat_left", _dp), ("khat_right", _dp), ("ndraws_tail", _ip)]


class Psis(C.Structure):
    _fields_ = [("khat", _dp), ("ndraws_tail", _ip), ("lppd", _dp), ("elpd", _dp), ("p_loo", _dp), ("log_weights", C.c_void_p)]


MCR_HDI_MAX_PROBS = 16                                      # probabilities of a Context.hdi call
MCR_HDI_SLICE = 16384                                       # windows k_hdi_window gives one workgroup


class Hdi(C.Structure):
    _fields_ = [("lo", _dp), ("hi", _dp), ("index", _ip)]


MCR_WEIGHTED_BLOCK = 1024                                   # consecutive indices of one summation tree of a weighted call
MCR_WEIGHTED_MAX_Q = 16                                     # probabilities of a Context.weighted_summary call
MCR_W_LOG = 1                                               # flag: the weight vector holds log weights


class Weighted(C.Structure):
    _fields_ = [("mean", _dp), ("sd", _dp), ("mean_se", _dp), ("quantiles", _dp), ("ess", _dp), ("weight_sum", _dp),
                ("weights", C.c_void_p)]


class Sbc(C.Structure):
    _fields_ = [("n_less", _ip), ("n_equal", _ip), ("mean", _dp), ("sd", _dp)]


MCR_ACF_MAX_LAG = 4096                                      # the largest max_lag of a Context.autocorr call
MCR_ACF_BLOCK = 512                                         # consecutive draws of one fma chain of k_acf_products
MCR_ACF_UNBIASED = 1                                        # flag: gamma_l = S_l / (N - l)


class Acf(C.Structure):
    _fields_ = [("acf", _dp), ("var", _dp), ("tau", _dp), ("window", _ip), ("acf_pooled", _dp), ("tau_pooled", _dp),
                ("window_pooled", _ip)]


class ModelDesc(C.Structure):
    _fields_ = [("draws_dev", C.c_void_p), ("dtype", C.c_int), ("min_chains", C.c_int),
                ("C", C.c_int64), ("N", C.c_int64), ("P", C.c_int64),
                ("stride_c", C.c_int64), ("stride_n", C.c_int64), ("stride_p", C.c_int64)]


class ParquetRequest(C.Structure):
    _fields_ = [("file", C.c_void_p), ("column", C.c_int), ("out_kind", C.c_int), ("out_dev", C.c_void_p)]


MCR_PQ_F64, MCR_PQ_I64 = 0, 1
MCR_PQ_INT32, MCR_PQ_INT64, MCR_PQ_DOUBLE = 1, 2, 5          # physical types (parquet.thrift)
MCR_PQW_F64, MCR_PQW_I64, MCR_PQW_SEQ = 0, 1, 2              # sources of a written column
MCR_PQW_PAGE_ROWS, MCR_PQW_ROW_GROUP_ROWS = 8192, 1048576
MCR_CSVW_TILE_FIELDS, MCR_CSVW_FIELD_MAX, MCR_SELECT_BLOCK_ROWS = 2048, 26, 256
MCR_PROJ_TILE_M, MCR_PROJ_TILE_K, MCR_PROJ_CHUNK_P = 512, 8, 64     # k_project's geometry
MCR_ENERGY_TILE_I, MCR_ENERGY_TILE_J, MCR_ENERGY_CHUNK_P = 128, 128, 8    # k_energy_pairs' geometry
MCR_ENERGY_MAX_WORK, MCR_ENERGY_LAUNCH_WORK = 1 << 44, 1 << 38            # pair-parameters of a call, of one launch


CSV_HEADERS = {"quoted": 0, "plain": 1, "none": 2}           # MCR_CSVW_HEADER_*
INT64_MAX = (1 << 63) - 1


class PqColumn(C.Structure):
    _fields_ = [("name", C.c_char_p), ("type", C.c_int), ("src_kind", C.c_int), ("src_dev", C.c_void_p),
                ("stride", C.c_int64), ("seq_div", C.c_int64), ("seq_mod", C.c_int64)]


def pq_column(name: str, type_: int, src, stride: int = 1, kind: int | None = None) -> tuple:
    """A column of write_parquet read from memory: `src` is a device pointer / buffer (Context.write_parquet) or a
    numpy array of float64 / int64 (write_parquet_host, where kind and stride follow from the array)."""
    return (name, type_, kind, src, stride, 1, 1)


def pq_sequence(name: str, type_: int, div: int = 1, mod: int = INT64_MAX) -> tuple:
    """A generated column of write_parquet: value(r) = (r // div) % mod."""
    return (name, type_, MCR_PQW_SEQ, None, 0, div, mod)


class IdColumns(C.Structure):
    _fields_ = [("chain_dev", C.c_void_p), ("draw_dev", C.c_void_p), ("rows", C.c_int64)]


class KernelTime(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_int64), ("total_ms", C.c_double)]


# every symbol include/mcmcref_hip.h declares: (restype, argtypes)
_I64 = C.c_int64
_TENSOR = [C.c_void_p, C.c_int, _I64, _I64, _I64, _I64, _I64, _I64]
_TENSOR4 = [C.c_void_p, C.c_int] + [_I64] * 8               # S simulations of such a tensor: S, C, N, P and their strides
SYMBOLS = {
    "mcr_version": (C.c_int, []),
    "mcr_device_count": (C.c_int, []),
    "mcr_init": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "mcr_free": (None, [C.c_void_p]),
    "mcr_last_error": (C.c_char_p, [C.c_void_p]),
    "mcr_set_workspace_limit": (C.c_int, [C.c_void_p, C.c_size_t]),
    "mcr_rho_guard_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "mcr_tile_fallback_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "mcr_plan_chunks": (C.c_int, [C.c_void_p] + [C.c_int64] * 6 + [C.c_int, C.POINTER(C.c_int64)]),
    "mcr_plan_chunks_chains": (C.c_int, [C.c_void_p, _ip, C.c_int, _I64, C.c_int, C.POINTER(C.c_int64)]),
    "mcr_dev_alloc": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "mcr_dev_free": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mcr_memcpy_h2d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "mcr_memcpy_d2h": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "mcr_sync": (C.c_int, [C.c_void_p]),
    "mcr_summarize": (C.c_int, [C.c_void_p] + _TENSOR + [C.c_int, _dp, C.c_int, C.POINTER(Summary)]),
    "mcr_summarize_dev": (C.c_int, [C.c_void_p] + _TENSOR + [C.c_int, _dp, C.c_int, C.POINTER(Summary)]),
    "mcr_summarize_enqueue": (C.c_int, [C.c_void_p] + _TENSOR + [C.c_int, _dp, C.c_int, C.POINTER(Summary)]),
    "mcr_summarize_models": (C.c_int, [C.c_void_p, C.POINTER(ModelDesc), C.c_int, _dp, C.c_int, C.POINTER(Summary)]),
    "mcr_summarize_wait": (C.c_int, [C.c_void_p]),
    "mcr_summarize_wait_one": (C.c_int, [C.c_void_p]),
    "mcr_diagnose_chains": (C.c_int, [C.c_void_p, _dp, _ip, C.c_int, C.c_int, C.POINTER(Summary),
                                      _dp, _dp, _dp, _dp]),
    "mcr_summarize_chains_enqueue": (C.c_int, [C.c_void_p, C.c_void_p, _I64, _ip, C.c_int, _I64, C.c_int, _dp, C.c_int,
                                               C.POINTER(Summary)]),
    "mcr_summarize_chains_dev": (C.c_int, [C.c_void_p, C.c_void_p, _I64, _ip, C.c_int, _I64, C.c_int, _dp, C.c_int,
                                           C.POINTER(Summary)]),
    "mcr_basic_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, _I64, _dp, _dp]),
    "mcr_moments_dev": (C.c_int, [C.c_void_p] + _TENSOR + [_dp, _dp]),
    "mcr_compare": (C.c_int, [C.c_void_p, _dp, _dp, _I64, C.c_double, _dp, C.POINTER(C.c_uint8)]),
    "mcr_two_sample": (C.c_int, [C.c_void_p, _dp, _I64, _dp, _I64, _I64, _dp, _dp]),
    "mcr_sliced_two_sample": (C.c_int, [C.c_void_p, _dp, _I64, _dp, _I64, _I64, _dp, _dp, _I64, _dp, _dp, _dp, _dp]),
    "mcr_sliced_two_sample_dev": (C.c_int, [C.c_void_p, C.c_void_p, _I64, C.c_void_p, _I64, _I64, _dp, _dp, _I64, _dp, _dp,
                                            _dp, _dp]),
    "mcr_sliced_plan": (C.c_int, [C.c_void_p, _I64, _I64, _I64, _I64, C.POINTER(C.c_int64)]),
    "mcr_energy_distance": (C.c_int, [C.c_void_p, _dp, _I64, _dp, _I64, _I64, _dp, _dp]),
    "mcr_energy_distance_dev": (C.c_int, [C.c_void_p, C.c_void_p, _I64, C.c_void_p, _I64, _I64, _dp, _dp]),
    "mcr_energy_distance_host": (C.c_int, [_dp, _I64, _dp, _I64, _I64, _dp, _dp]),
    "mcr_energy_workspace": (C.c_int, [C.c_void_p, _I64, _I64, _I64, C.POINTER(C.c_size_t)]),
    "mcr_nested_rhat": (C.c_int, [C.c_void_p] + _TENSOR + [C.POINTER(C.c_int32), C.POINTER(Nested)]),
    "mcr_nested_rhat_dev": (C.c_int, [C.c_void_p] + _TENSOR + [C.POINTER(C.c_int32), C.POINTER(Nested)]),
    "mcr_nested_plan": (C.c_int, [C.c_void_p, C.c_int] + [_I64] * 7 + [C.POINTER(C.c_int64)]),
    "mcr_pareto_khat": (C.c_int, [C.c_void_p] + _TENSOR + [_ip, C.POINTER(Pareto)]),
    "mcr_pareto_khat_dev": (C.c_int, [C.c_void_p] + _TENSOR + [_ip, C.POINTER(Pareto)]),
    "mcr_pareto_plan": (C.c_int, [C.c_void_p, C.c_int] + [_I64] * 6 + [C.POINTER(C.c_int64)]),
    "mcr_pareto_tail_length": (C.c_int64, [_I64, C.c_double]),
    "mcr_pareto_fit_host": (C.c_int, [_dp, _I64, _I64, _dp, _dp, C.POINTER(C.c_int64)]),
    "mcr_psis": (C.c_int, [C.c_void_p] + _TENSOR + [C.c_int, _dp, _ip, C.POINTER(Psis)]),
    "mcr_psis_dev": (C.c_int, [C.c_void_p] + _TENSOR + [C.c_int, _dp, _ip, C.POINTER(Psis)]),
    "mcr_psis_plan": (C.c_int, [C.c_void_p, C.c_int] + [_I64] * 6 + [C.c_int, C.POINTER(C.c_int64)]),
    "mcr_psis_tail_length": (C.c_int64, [_I64, C.c_double]),
    "mcr_psis_host": (C.c_int, [_dp, _I64, C.c_int, C.c_double, _I64, _dp, _ip, _dp, _dp, _dp, _dp]),
    "mcr_hdi": (C.c_int, [C.c_void_p] + _TENSOR + [_dp, C.c_int, C.POINTER(Hdi)]),
    "mcr_hdi_dev": (C.c_int, [C.c_void_p] + _TENSOR + [_dp, C.c_int, C.POINTER(Hdi)]),
    "mcr_hdi_plan": (C.c_int, [C.c_void_p, C.c_int] + [_I64] * 6 + [C.c_int, C.POINTER(C.c_int64)]),
    "mcr_hdi_sorted_host": (C.c_int, [_dp, _I64, _dp, C.c_int, _dp, _dp, _ip]),
    "mcr_weighted_summary": (C.c_int, [C.c_void_p] + _TENSOR + [C.c_void_p, C.c_int, _dp, C.c_int, C.POINTER(Weighted)]),
    "mcr_weighted_summary_dev": (C.c_int, [C.c_void_p] + _TENSOR + [C.c_void_p, C.c_int, _dp, C.c_int, C.POINTER(Weighted)]),
    "mcr_weighted_plan": (C.c_int, [C.c_void_p, C.c_int] + [_I64] * 6 + [C.c_int, C.POINTER(C.c_int64)]),
    "mcr_weighted_host": (C.c_int, [_dp, _dp, _I64, C.c_int, _dp, C.c_int] + [_dp] * 7),
    "mcr_sbc_ranks": (C.c_int, [C.c_void_p] + _TENSOR4 + [_dp, C.POINTER(Sbc)]),
    "mcr_sbc_ranks_dev": (C.c_int, [C.c_void_p] + _TENSOR4 + [_dp, C.POINTER(Sbc)]),
    "mcr_sbc_plan": (C.c_int, [C.c_void_p, C.c_int] + [_I64] * 8 + [C.POINTER(C.c_int64)]),
    "mcr_sbc_ranks_host": (C.c_int, [_dp, _I64, _I64, _I64, _dp, C.POINTER(Sbc)]),
    "mcr_sbc_uniformity": (C.c_int, [_ip, _I64, _I64, _I64, _I64, _ip, _dp, _dp, _dp, _dp]),
    "mcr_chi2_sf": (C.c_double, [C.c_double, C.c_double]),
    "mcr_autocorr": (C.c_int, [C.c_void_p] + _TENSOR + [_I64, C.c_int, C.c_double, C.POINTER(Acf)]),
    "mcr_autocorr_dev": (C.c_int, [C.c_void_p] + _TENSOR + [_I64, C.c_int, C.c_double, C.POINTER(Acf)]),
    "mcr_autocorr_plan": (C.c_int, [C.c_void_p, C.c_int] + [_I64] * 7 + [C.POINTER(C.c_int64)]),
    "mcr_autocorr_host": (C.c_int, [_dp, _I64, _I64, _I64, C.c_int, C.c_double, C.POINTER(Acf)]),
    "mcr_covariance": (C.c_int, [C.c_void_p, _dp, _I64, _I64, _dp]),
    "mcr_covariance_dev": (C.c_int, [C.c_void_p, C.c_void_p, _I64, _I64, C.c_void_p]),
    "mcr_profile_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "mcr_profile_reset": (C.c_int, [C.c_void_p]),
    "mcr_profile_get": (C.c_int, [C.c_void_p, C.POINTER(KernelTime), C.c_int, C.POINTER(C.c_int)]),
    "mcr_fill_synthetic": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, _I64, _I64, _I64, C.c_uint64]),
    "mcr_fill_synthetic_at": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, _I64, _I64, _I64, _I64, C.c_uint64]),
    "mcr_hbm_probe": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, _dp, _dp]),
    "mcr_comm_unique_id": (C.c_int, [C.c_void_p, C.c_size_t]),
    "mcr_comm_init": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "mcr_comm_free": (None, [C.c_void_p]),
    "mcr_comm_world": (C.c_int, [C.c_void_p]),
    "mcr_comm_rank": (C.c_int, [C.c_void_p]),
    "mcr_comm_has_deadline": (C.c_int, [C.c_void_p]),
    "mcr_comm_all_gather": (C.c_int, [C.c_void_p, _dp, _I64, _dp]),
    "mcr_comm_all_reduce": (C.c_int, [C.c_void_p, _dp, _I64, C.c_int]),
    "mcr_comm_barrier": (C.c_int, [C.c_void_p]),
    "mcr_parquet_open": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "mcr_parquet_close": (None, [C.c_void_p]),
    "mcr_parquet_num_rows": (C.c_int64, [C.c_void_p]),
    "mcr_parquet_num_columns": (C.c_int, [C.c_void_p]),
    "mcr_parquet_column_name": (C.c_char_p, [C.c_void_p, C.c_int]),
    "mcr_parquet_column_type": (C.c_int, [C.c_void_p, C.c_int]),
    "mcr_parquet_num_pages": (C.c_int, [C.c_void_p]),
    "mcr_parquet_page_info": (C.c_int, [C.c_void_p, C.c_int, _ip]),
    "mcr_parquet_decode": (C.c_int, [C.c_void_p, C.POINTER(ParquetRequest), C.c_int]),
    "mcr_parquet_write_dev": (C.c_int, [C.c_void_p, C.POINTER(PqColumn), C.c_int, _I64, _I64, C.POINTER(C.c_void_p)]),
    "mcr_parquet_write_host": (C.c_int, [C.c_void_p, C.POINTER(PqColumn), C.c_int, _I64, _I64, C.POINTER(C.c_void_p)]),
    "mcr_pq_image_data": (C.c_void_p, [C.c_void_p]),
    "mcr_pq_image_size": (C.c_size_t, [C.c_void_p]),
    "mcr_pq_image_pages": (C.c_int, [C.c_void_p]),
    "mcr_pq_image_free": (None, [C.c_void_p]),
    "mcr_csv_write_dev": (C.c_int, [C.c_void_p, C.POINTER(PqColumn), C.c_int, _I64, C.c_void_p, _I64, C.c_int, C.POINTER(C.c_void_p)]),
    "mcr_csv_write_host": (C.c_int, [C.c_void_p, C.POINTER(PqColumn), C.c_int, _I64, _ip, _I64, C.c_int, C.POINTER(C.c_void_p)]),
    "mcr_text_image_data": (C.c_void_p, [C.c_void_p]),
    "mcr_text_image_size": (C.c_size_t, [C.c_void_p]),
    "mcr_text_image_free": (None, [C.c_void_p]),
    "mcr_format_double": (C.c_int, [C.c_double, C.c_char_p, C.POINTER(C.c_int)]),
    "mcr_select_rows_dev": (C.c_int, [C.c_void_p, C.c_void_p, _I64, _ip, C.c_int, C.c_void_p, _ip]),
    "mcr_gather_rows_dev": (C.c_int, [C.c_void_p, C.c_void_p, _I64, _I64, _ip, C.c_void_p]),
    "mcr_chain_layout_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, _I64, C.c_void_p, _ip, _ip, C.c_int,
                                       C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "mcr_chain_layout_many_dev": (C.c_int, [C.c_void_p, C.POINTER(IdColumns), C.c_int, _ip, _ip, C.c_int,
                                            C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "mcr_gather_rows_order_dev": (C.c_int, [C.c_void_p, C.c_void_p, _I64, _I64, C.c_void_p, C.c_void_p]),
    "mcr_summarize_files": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.c_int, C.c_int, _dp, C.c_int, C.c_int,
                                      C.POINTER(C.c_void_p)]),
    "mcr_fileset_size": (C.c_int, [C.c_void_p]),
    "mcr_fileset_params": (C.c_int64, [C.c_void_p, C.c_int]),
    "mcr_fileset_chains": (C.c_int64, [C.c_void_p, C.c_int]),
    "mcr_fileset_draws": (C.c_int64, [C.c_void_p, C.c_int]),
    "mcr_fileset_param_name": (C.c_char_p, [C.c_void_p, C.c_int, C.c_int64]),
    "mcr_fileset_field": (_dp, [C.c_void_p, C.c_int, C.c_int]),
    "mcr_fileset_phases": (C.c_int, [C.c_void_p, _dp, C.c_int]),
    "mcr_fileset_jobs": (C.c_int, [C.c_void_p]),
    "mcr_fileset_export": (C.c_int64, [C.c_void_p, _dp, C.c_int64]),
    "mcr_fileset_names": (C.c_int64, [C.c_void_p, C.c_char_p, C.c_int64]),
    "mcr_fileset_free": (None, [C.c_void_p]),
    "mcr_csv_open": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "mcr_csv_open_paths": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.c_int, C.POINTER(C.c_void_p)]),
    "mcr_csv_close": (None, [C.c_void_p]),
    "mcr_csv_num_columns": (C.c_int, [C.c_void_p]),
    "mcr_csv_column_name": (C.c_char_p, [C.c_void_p, C.c_int]),
    "mcr_csv_body_offset": (C.c_int64, [C.c_void_p]),
    "mcr_csv_stage": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, _ip]),
    "mcr_csv_decode": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int, _I64, C.c_void_p, _I64, _I64, _I64, _ip]),
    "mcr_parse_double": (C.c_int, [C.c_char_p, C.c_size_t, _dp]),
    "mcr_csv_open_table": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "mcr_csv_open_table_paths": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.c_int, C.POINTER(C.c_void_p)]),
    "mcr_csv_table_flags": (C.c_int, [C.c_void_p]),
    "mcr_csv_decode_table": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), _I64, C.c_void_p, _I64, _I64,
                                       _I64, C.c_void_p, C.POINTER(C.c_uint8), _ip]),
    "mcr_parse_csv_number": (C.c_int, [C.c_char_p, C.c_size_t, _dp, C.POINTER(C.c_int)]),
    "mcr_json_open": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "mcr_json_close": (None, [C.c_void_p]),
    "mcr_json_num_chains": (C.c_int, [C.c_void_p]),
    "mcr_json_num_keys": (C.c_int, [C.c_void_p, C.c_int]),
    "mcr_json_key": (C.c_char_p, [C.c_void_p, C.c_int, C.c_int]),
    "mcr_json_length": (C.c_int64, [C.c_void_p, C.c_int, C.c_int]),
    "mcr_json_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_int, _I64, C.c_void_p, _I64, _I64, _I64,
                                  C.POINTER(C.c_uint8), _ip]),
    "mcr_parse_json_number": (C.c_int, [C.c_char_p, C.c_size_t, _dp, C.POINTER(C.c_int)]),
}


ENERGY_KEYS = ("a", "b", "c", "e", "h", "t")          # out6 of mcr_energy_distance, in order


SUMMARY_F64 = ("mean", "std", "median", "rhat", "rhat_bulk", "rhat_tail", "ess_bulk", "ess_tail")
DIAG_KEYS = ("rhat", "ess_bulk", "ess_tail")          # the diagnostics the reference API reports per parameter

# mcr_fileset_export: one row per parameter, files and parameters in order -- these MCR_FS_* fields, then q[0 .. n_q)
FS_EXPORT = ("mean", "std", "median", "rhat", "ess_bulk", "ess_tail", "rhat_bulk", "rhat_tail", "lag_bulk", "lag_tail")
FS_PHASES = ("open_ms", "read_pinned_parse_ms", "plan_ms", "upload_decode_layout_ms", "statistics_ms",
             "collect_ms", "close_ms", "total_ms")          # MCR_FS_PH_*


_lib = None
_lib_lock = threading.Lock()


def lib_path() -> Path:
    return Path(os.environ.get("MCMC_REF_HIP_LIB", str(DEFAULT_LIB)))


def load_library():
    """dlopen the C ABI and bind every declared symbol (works without a GPU)."""
    global _lib
    with _lib_lock:
        if _lib is None:
            path = lib_path()
            if not path.exists():
                raise HipUnavailableError(
                    f"{path} not found: build it with `python mcmc-db_amd/build.py` "
                    "(there is no CPU fallback)")
            # Multi-process RCCL (N > 1 ranks, one per GPU) exchanges device buffers between processes over IPC handles.  The
            # host driver of this platform supports only the dmabuf form; with the HSA runtime's legacy IPC mode (its
            # default) `hipIpcGetMemHandle` fails with "invalid argument" inside ncclCommInitRank.  The runtime reads the
            # variable when it initialises, i.e. at the first HIP call, so it is set here, before the library is mapped --
            # it must precede the first HIP call of the process, whoever makes it; a value the launcher exported wins.
            # Only for multi-rank launches: a single process has no IPC to do, and the variable is process-global (it would
            # change the runtime's behaviour for any other HIP library the host application uses: ADVICE r3).
            if int(os.environ.get("WORLD_SIZE", "1") or "1") > 1:
                os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
            try:
                L = C.CDLL(str(path))
            except OSError as exc:
                raise HipUnavailableError(f"cannot load {path}: {exc}") from exc
            for name, (res, args) in SYMBOLS.items():
                fn = getattr(L, name)   # AttributeError if the ABI is incomplete
                fn.restype = res
                fn.argtypes = args
            _lib = L
    return _lib


def _as_dp(a):
    return a.ctypes.data_as(_dp) if a is not None else None


def _as_ip(a):
    return a.ctypes.data_as(_ip) if a is not None else None


def _dtype_code(dtype) -> int:
    if dtype == np.float64:
        return MCR_F64
    if dtype == np.float32:
        return MCR_F32
    raise TypeError(f"unsupported dtype {dtype}; use float64 or float32")


def tensor_args(draws: np.ndarray, layout: str):
    """(dtype code, C, N, P, stride_c, stride_n, stride_p) for a 3-D array whose axes are `layout`."""
    if draws.ndim != 3 or sorted(layout) != ["c", "n", "p"]:
        raise ValueError("draws must be 3-D and layout a permutation of 'cnp'")
    code = _dtype_code(draws.dtype)
    ax = {a: i for i, a in enumerate(layout)}
    dims = [draws.shape[ax[a]] for a in "cnp"]
    strides = [draws.strides[ax[a]] // draws.itemsize for a in "cnp"]
    if any(s < 0 for s in strides):
        raise ValueError("negative strides are not supported")
    return (code, *dims, *strides)


def tensor4_args(draws: np.ndarray, layout: str):
    """(dtype code, S, C, N, P, stride_s, stride_c, stride_n, stride_p) for a 4-D array whose axes are `layout`, a
    permutation of "scnp": simulations, chains, draws, parameters."""
    if draws.ndim != 4 or sorted(layout) != ["c", "n", "p", "s"]:
        raise ValueError("draws must be 4-D and layout a permutation of 'scnp'")
    ax = {a: i for i, a in enumerate(layout)}
    dims = [draws.shape[ax[a]] for a in "scnp"]
    strides = [draws.strides[ax[a]] // draws.itemsize for a in "scnp"]
    if any(s < 0 for s in strides):
        raise ValueError("negative strides are not supported")
    return (_dtype_code(draws.dtype), *dims, *strides)


def thin_args(targs4, thin: int):
    """The arguments of the same tensor with the draws n = 0, thin, 2 thin, ... of every chain: a larger stride_n."""
    if int(thin) != thin or thin < 1:
        raise ValueError("thin must be an integer >= 1")
    code, S, C_, N, P, ss, sc, sn, sp = targs4
    return (code, S, C_, -(-N // int(thin)), P, ss, sc, sn * int(thin), sp)

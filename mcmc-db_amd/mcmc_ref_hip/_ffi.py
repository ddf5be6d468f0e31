"""ctypes binding of libmcmcref_hip.so (include/mcmcref_hip.h).  No torch, no fallback.

If the shared library or a HIP device is missing every entry point raises
`HipUnavailableError`: the product path never silently computes on the CPU.

The summarize plumbing the Python API shares lives here too, once: the fileset reader
(`Context.summarize_files`), the rolling window over enqueue / wait_one (`pipeline`, `split_result`),
the reference-shaped per-parameter dicts (`entries`), the ragged-chain route (`Context.summarize_chains`,
`ragged_diagnostics`), the device row order (`Context.chain_layout`), the CmdStan CSV
decoder (`Context.csv_decode`), the chain-list JSON decoder (`Context.json_decode`) and
the McrError -> ValueError translation of the reference-compatible functions (`value_errors`).
"""
from __future__ import annotations

import collections
import contextlib
import ctypes as C
import math
import os
import threading
import time
import typing
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


def energy_launches(Mr: int, Ma: int, P: int, launch_work: int = MCR_ENERGY_LAUNCH_WORK) -> int:
    """k_energy_pairs launches of an energy_distance call of this shape (the rule stated in mcmcref_hip.h)."""
    nr, na = -(-Mr // MCR_ENERGY_TILE_I), -(-Ma // MCR_ENERGY_TILE_J)
    jobs = nr * na + nr * (nr + 1) // 2 + na * (na + 1) // 2
    return -(-jobs // max(1, launch_work // (MCR_ENERGY_TILE_I * MCR_ENERGY_TILE_J * P)))
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


def energy_distance_host(ref, actual, scale=None) -> dict:
    """mcr_energy_distance_host: the definition of Context.energy_distance on the host, without a GPU (the same per-pair
    arithmetic bit for bit, the pair sums in long double)."""
    r = np.ascontiguousarray(ref, dtype=np.float64)
    a = np.ascontiguousarray(actual, dtype=np.float64)
    if r.ndim != 2 or a.ndim != 2 or r.shape[0] != a.shape[0]:
        raise ValueError("ref and actual must be 2-D with the same number of parameters")
    s = None if scale is None else np.ascontiguousarray(scale, dtype=np.float64)
    if s is not None and s.shape != (r.shape[0],):
        raise ValueError("scale must have one entry per parameter")
    out = np.full(6, np.nan)
    rc = load_library().mcr_energy_distance_host(_as_dp(r), r.shape[1], _as_dp(a), a.shape[1], r.shape[0], _as_dp(s), _as_dp(out))
    if rc != MCR_OK:
        raise McrError(rc, "mcr_energy_distance_host")
    return dict(zip(ENERGY_KEYS, (float(v) for v in out)))


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


SUMMARY_F64 = ("mean", "std", "median", "rhat", "rhat_bulk", "rhat_tail", "ess_bulk", "ess_tail")
DIAG_KEYS = ("rhat", "ess_bulk", "ess_tail")          # the diagnostics the reference API reports per parameter

# mcr_fileset_export: one row per parameter, files and parameters in order -- these MCR_FS_* fields, then q[0 .. n_q)
FS_EXPORT = ("mean", "std", "median", "rhat", "ess_bulk", "ess_tail", "rhat_bulk", "rhat_tail", "lag_bulk", "lag_tail")
FS_PHASES = ("open_ms", "read_pinned_parse_ms", "plan_ms", "upload_decode_layout_ms", "statistics_ms",
             "collect_ms", "close_ms", "total_ms")          # MCR_FS_PH_*


class SummaryBuffers:
    """Host arrays an mcr_summary points into (kept alive by this object)."""

    def __init__(self, P: int, nq: int, diagnostics: bool = True):
        self.P, self.nq, self.diagnostics = P, nq, diagnostics
        n = max(P, 1)
        self.arrays = {k: np.full(n, np.nan) for k in SUMMARY_F64}
        self.arrays["q"] = np.full(max(P * nq, 1), np.nan)
        self.arrays["lag_bulk"] = np.zeros(n, dtype=np.int64)
        self.arrays["lag_tail"] = np.zeros(n, dtype=np.int64)
        self.arrays["q_lo"] = np.zeros(max(nq, 1), dtype=np.int64)
        kw = {k: _as_dp(self.arrays[k]) for k in SUMMARY_F64 + ("q",)}
        kw.update({k: _as_ip(self.arrays[k]) for k in ("lag_bulk", "lag_tail", "q_lo")})
        if not diagnostics:     # NULL members: the library skips the diagnostics kernels
            for k in ("rhat", "rhat_bulk", "rhat_tail", "ess_bulk", "ess_tail", "lag_bulk", "lag_tail"):
                kw[k] = None
        self.struct = Summary(**kw)

    def result(self) -> dict:
        P, nq = self.P, self.nq
        out = {k: self.arrays[k][:P].copy() for k in SUMMARY_F64 + ("lag_bulk", "lag_tail")}
        out["q"] = self.arrays["q"][:P * nq].reshape(P, nq).copy()
        out["q_lo"] = self.arrays["q_lo"][:nq].copy()
        return out


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


def superchain_labels(superchain_ids, n_chains: int) -> np.ndarray:
    """The int32 label of every chain: `superchain_ids` as given (one per chain), or for an int K the K contiguous
    blocks of n_chains / K chains.  ValueError for a length other than the number of chains, a K that does not divide
    it, labels outside int32, or superchains of unequal size."""
    if isinstance(superchain_ids, (int, np.integer)) and not isinstance(superchain_ids, bool):
        K = int(superchain_ids)
        if K < 1 or n_chains % K:
            raise ValueError(f"{K} superchains do not divide {n_chains} chains into equal blocks")
        return np.repeat(np.arange(K, dtype=np.int32), n_chains // K)
    ids = np.asarray(superchain_ids)
    if ids.ndim != 1 or ids.shape[0] != n_chains:
        raise ValueError(f"superchain_ids must have one label per chain: got {ids.size} for {n_chains} chains")
    if ids.size and not np.issubdtype(ids.dtype, np.integer):
        raise ValueError("superchain_ids must be integers")
    if ids.size and (ids.min() < -2**31 or ids.max() >= 2**31):
        raise ValueError("superchain_ids must fit int32")
    if ids.size and len(set(np.unique(ids, return_counts=True)[1].tolist())) != 1:
        raise ValueError("superchains must have the same number of chains")
    return np.ascontiguousarray(ids, dtype=np.int32)


def pareto_tail_length(M: int, r_eff: float = 1.0) -> int:
    """The default tail length of Pareto k-hat for M draws (mcr_pareto_tail_length: ceil(3 sqrt(M / r_eff)) for M > 225,
    else M // 5; no device).  ValueError unless r_eff is finite and > 0."""
    t = int(load_library().mcr_pareto_tail_length(int(M), float(r_eff)))
    if t < 0:
        raise ValueError(f"r_eff must be finite and > 0; got {r_eff}")
    return t


def pareto_fit_host(sorted_draws, ndraws_tail: int = 0) -> tuple[float, float, int]:
    """(khat_left, khat_right, effective tail length) of an ASCENDING float64 array by the library's host routine
    (mcr_pareto_fit_host: the device's text and summation order with the host's libm; no device).  ndraws_tail 0: the default."""
    x = np.ascontiguousarray(sorted_draws, dtype=np.float64)
    kl, kr, t = C.c_double(), C.c_double(), C.c_int64()
    rc = load_library().mcr_pareto_fit_host(_as_dp(x), x.size, int(ndraws_tail), C.byref(kl), C.byref(kr), C.byref(t))
    if rc != MCR_OK:
        raise ValueError(f"mcr_pareto_fit_host: bad argument (ndraws_tail = {ndraws_tail})")
    return kl.value, kr.value, int(t.value)


def pareto_companions(khat: np.ndarray, M: int) -> tuple[np.ndarray, float]:
    """posterior::pareto_diags' companions of k-hat values from M draws: min_ss = 10^(1 / (1 - max(0, khat))), +inf for
    khat >= 1 (NaN stays NaN), and khat_threshold = 1 - 1 / log10(M) (NaN for M < 1)."""
    k = np.asarray(khat, dtype=np.float64)
    with np.errstate(all="ignore"):
        min_ss = np.where(k >= 1.0, np.inf, np.power(10.0, 1.0 / (1.0 - np.maximum(k, 0.0))))
        min_ss = np.where(np.isnan(k), np.nan, min_ss)
        threshold = 1.0 - 1.0 / math.log10(M) if M > 1 else float("-inf") if M == 1 else float("nan")
    return min_ss, threshold


def psis_tail_length(M: int, r_eff: float = 1.0) -> int:
    """The default tail length of PSIS for M values (mcr_psis_tail_length: ceil(min(M / 5, 3 sqrt(M / r_eff))), loo's and
    ArviZ's rule for every M; no device).  ValueError unless r_eff is finite and > 0."""
    t = int(load_library().mcr_psis_tail_length(int(M), float(r_eff)))
    if t < 0:
        raise ValueError(f"r_eff must be finite and > 0; got {r_eff}")
    return t


def psis_host(values, negate: bool = False, r_eff: float = 1.0, ndraws_tail: int = 0, weights: bool = True) -> dict:
    """PSIS of ONE column of float64 values in any order by the library's host routine (mcr_psis_host: the device's text
    and summation order with the host's libm; no device).  negate: the values are log-likelihoods (LOO).  ndraws_tail 0:
    the default.  khat, ndraws_tail (the n used), lppd, elpd, p_loo (NaN without negate) and, with weights, log_weights in
    the order of `values`.  ValueError for a bad argument or a non-finite value."""
    x = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
    kh, lppd, elpd, ploo, n = C.c_double(), C.c_double(), C.c_double(), C.c_double(), C.c_int64()
    lw = np.full(max(x.size, 1), np.nan) if weights else None
    rc = load_library().mcr_psis_host(_as_dp(x), x.size, int(bool(negate)), float(r_eff), int(ndraws_tail), C.byref(kh),
                                      C.byref(n), C.byref(lppd), C.byref(elpd), C.byref(ploo), _as_dp(lw))
    if rc != MCR_OK:
        raise ValueError(f"mcr_psis_host: {'non-finite value' if rc == MCR_ENONFINITE else 'bad argument'} "
                         f"(r_eff = {r_eff}, ndraws_tail = {ndraws_tail})")
    res = {"khat": kh.value, "ndraws_tail": int(n.value), "lppd": lppd.value, "elpd": elpd.value, "p_loo": ploo.value}
    if weights:
        res["log_weights"] = lw[:x.size]
    return res


LOO_KHAT_BINS = (0.5, 0.7, 1.0)                              # k-hat counted in (-inf, 0.5], (0.5, 0.7], (0.7, 1], (1, inf)


def loo_totals(elpd_i, p_loo_i, lppd_i, khat) -> dict:
    """The totals of pointwise PSIS-LOO results (ArviZ's loo): elpd_loo, p_loo and lppd as math.fsum of the columns, se =
    sqrt(P var(elpd_i, ddof = 0)), and khat_counts, the k-hats in (-inf, 0.5], (0.5, 0.7], (0.7, 1] and (1, inf) (a NaN
    in none)."""
    e = np.asarray(elpd_i, dtype=np.float64)
    k = np.asarray(khat, dtype=np.float64)
    P = int(e.size)
    lo = (-np.inf,) + LOO_KHAT_BINS
    hi = LOO_KHAT_BINS + (np.inf,)
    return {"elpd_loo": math.fsum(e), "se": math.sqrt(P * float(np.var(e))) if P else float("nan"),
            "p_loo": math.fsum(np.asarray(p_loo_i, dtype=np.float64)), "lppd": math.fsum(np.asarray(lppd_i, dtype=np.float64)),
            "khat_counts": [int(np.count_nonzero((k > a) & (k <= b))) for a, b in zip(lo, hi)], "n_obs": P}


def hdi_sorted_host(sorted_draws, prob=0.94):
    """(lo, hi, index) of the highest-density interval(s) of an ASCENDING float64 array by the library's host routine
    (mcr_hdi_sorted_host: the device's comparison; no device): floats and an int for a float `prob`, arrays of len(prob)
    for a sequence.  ValueError for a probability outside (0, 1), none or more than MCR_HDI_MAX_PROBS of them."""
    x = np.ascontiguousarray(sorted_draws, dtype=np.float64)
    pr = np.ascontiguousarray(np.atleast_1d(prob), dtype=np.float64)
    n = max(int(pr.size), 1)
    lo, hi, idx = np.full(n, np.nan), np.full(n, np.nan), np.full(n, -1, dtype=np.int64)
    rc = load_library().mcr_hdi_sorted_host(_as_dp(x), x.size, _as_dp(pr), int(pr.size), _as_dp(lo), _as_dp(hi), _as_ip(idx))
    if rc != MCR_OK:
        raise ValueError(f"mcr_hdi_sorted_host: bad argument (prob = {prob})")
    if np.ndim(prob) == 0:
        return float(lo[0]), float(hi[0]), int(idx[0])
    return lo, hi, idx


def weight_arguments(M: int, log_weights, weights, quantiles) -> tuple[np.ndarray, int, np.ndarray]:
    """(the weight vector, the flags, the probabilities) of a weighted call on M pooled draws.  ValueError unless exactly
    one of log_weights and weights is given and holds M entries, and the probabilities are at most MCR_WEIGHTED_MAX_Q
    values in [0, 1]."""
    if (log_weights is None) == (weights is None):
        raise ValueError("give exactly one of log_weights and weights")
    v = np.ascontiguousarray(weights if log_weights is None else log_weights, dtype=np.float64).reshape(-1)
    if v.size != M:
        raise ValueError(f"the weight vector has {v.size} entries for {M} pooled draws")
    q = np.ascontiguousarray(np.atleast_1d(quantiles), dtype=np.float64).reshape(-1)
    if q.size > MCR_WEIGHTED_MAX_Q:
        raise ValueError(f"at most {MCR_WEIGHTED_MAX_Q} quantiles; got {q.size}")
    if not np.all((q >= 0.0) & (q <= 1.0)):
        raise ValueError(f"quantiles must lie in [0, 1]; got {quantiles}")
    return v, 0 if log_weights is None else MCR_W_LOG, q


def weighted_host(x, *, log_weights=None, weights=None, quantiles=(0.05, 0.5, 0.95), return_weights: bool = False) -> dict:
    """The weighted summary of ONE parameter's draws in time order by the library's host routine (mcr_weighted_host: the
    device's association, std::sort; no device): the floats mean, sd, mean_se, ess, weight_sum and the array quantiles;
    with return_weights the weights as formed.  Linear weights give the device's bits; log weights go through libm's exp.
    ValueError for a bad argument, a refused weight vector or a non-finite draw."""
    d = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
    v, flags, q = weight_arguments(d.size, log_weights, weights, quantiles)
    f = [C.c_double(np.nan) for _ in range(5)]
    qs = np.full(max(q.size, 1), np.nan)
    w = np.full(max(d.size, 1), np.nan) if return_weights else None
    rc = load_library().mcr_weighted_host(_as_dp(d), _as_dp(v), d.size, flags, _as_dp(q), int(q.size), C.byref(f[0]),
                                          C.byref(f[1]), C.byref(f[2]), _as_dp(qs), C.byref(f[3]), C.byref(f[4]), _as_dp(w))
    if rc != MCR_OK:
        raise ValueError(f"mcr_weighted_host: {'non-finite draw' if rc == MCR_ENONFINITE else 'bad argument or weight vector'}")
    res = dict(zip(("mean", "sd", "mean_se", "ess", "weight_sum"), (c.value for c in f)))
    res["quantiles"] = qs[:q.size]
    if return_weights:
        res["weights"] = w[:d.size]
    return res


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


def _sbc_arrays(S: int, P: int):
    """The output arrays of a rank call (-1 / NaN until written) and the struct that points at them."""
    shape = (max(S, 1), max(P, 1))
    arrs = {"n_less": np.full(shape, -1, dtype=np.int64), "n_equal": np.full(shape, -1, dtype=np.int64),
            "mean": np.full(shape, np.nan), "sd": np.full(shape, np.nan)}
    out = Sbc(n_less=_as_ip(arrs["n_less"]), n_equal=_as_ip(arrs["n_equal"]), mean=_as_dp(arrs["mean"]), sd=_as_dp(arrs["sd"]))
    return arrs, out


def _truth_array(truth, S: int, P: int) -> np.ndarray:
    t = np.ascontiguousarray(truth, dtype=np.float64)
    if t.shape != (S, P):
        raise ValueError(f"truth must be [S][P] = {(S, P)}; got {t.shape}")
    return t


def sbc_ranks_host(draws, truth) -> dict:
    """mcr_sbc_ranks_host: the definition of Context.sbc_ranks on the host, without a GPU (the device's summation order:
    the same bits).  draws [S][P][L], truth [S][P].  "n_less", "n_equal" (int64), "mean", "sd" [S][P] and the int
    "n_draws" = L.  ValueError for a bad argument or a non-finite truth, McrError(MCR_ENONFINITE) for a non-finite draw."""
    x = np.ascontiguousarray(draws, dtype=np.float64)
    if x.ndim != 3:
        raise ValueError("draws must be 3-D [S][P][L]")
    S, P, L = x.shape
    t = _truth_array(truth, S, P)
    arrs, out = _sbc_arrays(S, P)
    rc = load_library().mcr_sbc_ranks_host(_as_dp(x), S, P, L, _as_dp(t), C.byref(out))
    if rc == MCR_ENONFINITE:
        raise McrError(rc, "draws contain non-finite value(s)")
    if rc != MCR_OK:
        raise ValueError("mcr_sbc_ranks_host: bad argument or non-finite truth")
    return {**{k: a[:S, :P] for k, a in arrs.items()}, "n_draws": int(L)}


def chi2_sf(x: float, dof: float) -> float:
    """mcr_chi2_sf: the upper tail probability of the chi-square distribution with dof degrees of freedom at x."""
    return float(load_library().mcr_chi2_sf(float(x), float(dof)))


def sbc_uniformity(ranks, n_draws: int, bins: int) -> dict:
    """mcr_sbc_uniformity: ranks [S][P] in 0 .. n_draws -> "counts" [P][bins] (int64), "expected" [bins], "chi2", "pvalue"
    (bins - 1 degrees of freedom) and "ecdf_dev" [P].  ValueError for a bad argument or a rank out of range."""
    r = np.ascontiguousarray(ranks, dtype=np.int64)
    if r.ndim != 2:
        raise ValueError("ranks must be 2-D [S][P]")
    S, P = r.shape
    B = int(bins)
    counts = np.zeros((max(P, 1), max(B, 1)), dtype=np.int64)
    expected = np.full(max(B, 1), np.nan)
    per = {k: np.full(max(P, 1), np.nan) for k in ("chi2", "pvalue", "ecdf_dev")}
    rc = load_library().mcr_sbc_uniformity(_as_ip(r), S, P, int(n_draws), B, _as_ip(counts), _as_dp(expected),
                                           *(_as_dp(per[k]) for k in ("chi2", "pvalue", "ecdf_dev")))
    if rc != MCR_OK:
        raise ValueError("mcr_sbc_uniformity: needs S >= 1, 2 <= bins <= n_draws + 1 and every rank in 0 .. n_draws")
    return {"counts": counts[:P, :B], "expected": expected[:B], **{k: a[:P] for k, a in per.items()}}


def _acf_arrays(P: int, nc: int, L: int):
    """The output arrays of an autocorrelation call (NaN / -1 until written) and the struct that points at them."""
    p1, c1 = max(P, 1), max(nc, 1)
    arrs = {"acf": np.full((p1, c1, L + 1), np.nan), "var": np.full((p1, c1), np.nan), "tau": np.full((p1, c1), np.nan),
            "window": np.full((p1, c1), -1, dtype=np.int64), "acf_pooled": np.full((p1, L + 1), np.nan),
            "tau_pooled": np.full(p1, np.nan), "window_pooled": np.full(p1, -1, dtype=np.int64)}
    out = Acf(**{k: (_as_ip if a.dtype == np.int64 else _as_dp)(a) for k, a in arrs.items()})
    return arrs, out


def _acf_result(arrs: dict, P: int, nc: int, N: int, L: int) -> dict:
    res = {k: a[:P, :nc] if k in ("acf", "var", "tau", "window") else a[:P] for k, a in arrs.items()}
    with np.errstate(all="ignore"):
        res["ess_chain"] = N / res["tau"]
        res["ess_pooled"] = (nc * N) / res["tau_pooled"]
    res["max_lag"] = L
    return res


def autocorr_host(chains, max_lag=None, unbiased: bool = False, window_c: float = 5.0) -> dict:
    """Autocorrelation functions and times of ONE parameter's equal-length chains [C][N] by the library's host routine
    (mcr_autocorr_host: the device's text in the device's summation order, equal to Context.autocorr in bits; no device).
    The keys of Context.autocorr with P = 1.  ValueError for a bad max_lag or window_c, or non-finite draws."""
    x = np.ascontiguousarray(chains, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError("chains must be 2-D [C][N]")
    nc, N = x.shape
    L = min(100, max(N - 1, 0)) if max_lag is None else int(max_lag)
    arrs, out = _acf_arrays(1, nc, L if 0 <= L <= MCR_ACF_MAX_LAG else 0)      # (a bad max_lag is refused before anything is written)
    rc = load_library().mcr_autocorr_host(_as_dp(x), nc, N, L, MCR_ACF_UNBIASED if unbiased else 0, float(window_c), C.byref(out))
    if rc != MCR_OK:
        raise ValueError(f"mcr_autocorr_host: {'non-finite draws' if rc == MCR_ENONFINITE else 'bad argument'} "
                         f"(max_lag = {L}, N = {N}, window_c = {window_c})")
    return _acf_result(arrs, 1, nc, N, L)


class Image:
    """Bytes the library owns (an mcr_pq_image or an mcr_text_image): `view` is its bytes without a copy, valid until
    close().  `data`, `size` and `free` are the three library functions of its kind."""

    def __init__(self, handle, data, size, free):
        self.handle, self._free = handle, free
        self.size = int(size(handle))
        self.view = memoryview((C.c_ubyte * self.size).from_address(data(handle))).cast("B") if self.size else memoryview(b"")

    def tobytes(self) -> bytes:
        return self.view.tobytes()

    def __len__(self):
        return self.size

    def close(self):
        if self.handle:
            self.view.release()
            self.view = None
            self._free(self.handle)
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


def PqImage(lib, handle) -> Image:
    """A Parquet file image the library owns (mcr_pq_image); `pages` counts its pages."""
    image = Image(handle, lib.mcr_pq_image_data, lib.mcr_pq_image_size, lib.mcr_pq_image_free)
    image.pages = int(lib.mcr_pq_image_pages(handle))
    return image


def TextImage(lib, handle) -> Image:
    """A text image the library owns (mcr_text_image)."""
    return Image(handle, lib.mcr_text_image_data, lib.mcr_text_image_size, lib.mcr_text_image_free)


def _pq_columns(columns, host: bool):
    """(PqColumn array, objects to keep alive) of pq_column / pq_sequence tuples."""
    arr = (PqColumn * max(len(columns), 1))()
    keep = []
    for k, (name, type_, kind, src, stride, div, mod) in enumerate(columns):
        if kind != MCR_PQW_SEQ and host:
            a = np.asarray(src)
            if a.ndim != 1 or a.dtype not in (np.float64, np.int64) or (a.size and a.strides[0] % 8) or (a.size and a.strides[0] < 8):
                raise ValueError(f"column {name!r}: a 1-D float64 or int64 array with a positive stride is needed")
            keep.append(a)
            kind = MCR_PQW_F64 if a.dtype == np.float64 else MCR_PQW_I64
            stride = a.strides[0] // 8 if a.size else 1
            src = a.ctypes.data
        elif kind != MCR_PQW_SEQ:
            if kind is None:
                raise ValueError(f"column {name!r}: kind (MCR_PQW_F64 or MCR_PQW_I64) is needed for device memory")
            src = getattr(src, "ptr", src)
            src = src.value if isinstance(src, C.c_void_p) else src
        keep.append(str(name).encode())
        arr[k] = PqColumn(keep[-1], int(type_), int(kind), src, int(stride), int(div), int(mod))
    return arr, keep


def write_parquet_host(columns, rows: int, row_group_rows: int = 0) -> PqImage:
    """mcr_parquet_write_host: the Parquet image of host columns (numpy arrays or pq_sequence), without a device."""
    lib = load_library()
    arr, _keep = _pq_columns(columns, host=True)
    h = C.c_void_p()
    rc = lib.mcr_parquet_write_host(None, arr, len(columns), int(rows), int(row_group_rows), C.byref(h))
    if rc != MCR_OK:
        raise McrError(rc, (lib.mcr_last_error(None) or b"").decode())
    return PqImage(lib, h)


def write_csv_host(columns, rows: int, row_index=None, header: str = "quoted") -> TextImage:
    """mcr_csv_write_host: the CSV text of host columns (numpy arrays or pq_sequence), without a device; `row_index`
    (int64 values) selects and orders the rows.  The bytes are the device's (Context.write_csv)."""
    lib = load_library()
    arr, _keep = _pq_columns(columns, host=True)
    idx = None if row_index is None else np.ascontiguousarray(row_index, dtype=np.int64)
    n = 0 if idx is None else idx.size
    if idx is not None and n == 0:
        idx = np.zeros(1, dtype=np.int64)         # an empty list is still a list: its pointer must not be NULL
    h = C.c_void_p()
    rc = lib.mcr_csv_write_host(None, arr, len(columns), int(rows), _as_ip(idx), n, CSV_HEADERS[header], C.byref(h))
    if rc != MCR_OK:
        raise McrError(rc, (lib.mcr_last_error(None) or b"").decode())
    return TextImage(lib, h)


def format_double(v: float) -> str:
    """mcr_format_double: the text write_csv gives one float64 (pyarrow's, byte for byte)."""
    buf, n = C.create_string_buffer(MCR_CSVW_FIELD_MAX), C.c_int()
    rc = load_library().mcr_format_double(float(v), buf, C.byref(n))
    if rc != MCR_OK:
        raise McrError(rc, "mcr_format_double")
    return buf.raw[:n.value].decode()


class _Owner:
    """An owner of device memory is a context manager: leaving the `with` calls free(), and free() may be called again.
    A function that hands its allocation on enters it into a contextlib.ExitStack and ends with pop_all()."""

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()


class DeviceBuffer(_Owner):
    def __init__(self, ctx: "Context", nbytes: int):
        self.ctx, self.nbytes = ctx, nbytes
        self.ptr = C.c_void_p()
        ctx._check(ctx.lib.mcr_dev_alloc(ctx.handle, nbytes, C.byref(self.ptr)))

    def upload(self, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        self.ctx._check(self.ctx.lib.mcr_memcpy_h2d(self.ctx.handle, self.ptr, arr.ctypes.data_as(C.c_void_p),
                                                    arr.nbytes))
        return self

    def download(self, dtype, count: int) -> np.ndarray:
        out = np.empty(count, dtype=dtype)
        self.ctx._check(self.ctx.lib.mcr_memcpy_d2h(self.ctx.handle, out.ctypes.data_as(C.c_void_p), self.ptr,
                                                    out.nbytes))
        return out

    def free(self):
        if self.ptr:
            self.ctx.lib.mcr_dev_free(self.ctx.handle, self.ptr)
            self.ptr = C.c_void_p()


class DeviceArena(_Owner):
    """One device allocation shared by the models of a batch (hipMalloc / hipFree cost ~0.1 ms each, which
    would dominate a 57-file corpus pass).  Its maker holds it until free() -- the end of the maker's `with` -- and every
    view holds it too: the buffer is freed with the last of them, at once when no view is left."""

    def __init__(self, ctx, nbytes: int):
        self.buf = DeviceBuffer(ctx, max(nbytes, 8))
        self.refs, self.held = 1, True

    def view(self, offset: int, nbytes: int) -> "DeviceView":
        self.refs += 1
        return DeviceView(self, offset, nbytes)

    def release(self):
        self.refs -= 1
        if self.refs <= 0:
            self.buf.free()

    def free(self):
        if self.held:
            self.held = False
            self.release()


class DeviceView(_Owner):
    """Slice of an arena with DeviceBuffer's interface (ptr / download / free)."""

    def __init__(self, arena: DeviceArena, offset: int, nbytes: int):
        self.arena, self.ctx, self.nbytes = arena, arena.buf.ctx, nbytes
        self.ptr = C.c_void_p(arena.buf.ptr.value + offset)

    def download(self, dtype, count: int) -> np.ndarray:
        out = np.empty(count, dtype=dtype)
        if out.nbytes:
            self.ctx._check(self.ctx.lib.mcr_memcpy_d2h(self.ctx.handle, out.ctypes.data_as(C.c_void_p), self.ptr, out.nbytes))
        return out

    def share(self) -> "DeviceView":
        """Another view of the same bytes; the arena lives until both are freed."""
        return self.arena.view(self.ptr.value - self.arena.buf.ptr.value, self.nbytes)

    def free(self):
        if self.arena is not None:
            self.arena.release()
            self.arena = None
            self.ptr = C.c_void_p()


class DeviceTensor(_Owner):
    """A draw tensor resident in HBM: device buffer + the (dtype, dims, strides) it was uploaded with.

    chain_off (int64, C + 1 offsets) marks f64 draws [P][M] whose chains differ in length (Context.ragged_tensor): the
    calls that take a tensor then use the ragged entry points; targs = (MCR_F64, C, shortest chain, P, 0, 1, stride_p)."""

    def __init__(self, ctx: "Context", buf: DeviceBuffer, targs, chain_off: np.ndarray | None = None):
        self.ctx, self.buf, self.targs, self.chain_off = ctx, buf, targs, chain_off

    @property
    def shape_cnp(self):
        return self.targs[1:4]

    def free(self):
        self.buf.free()


class DeviceSims(_Owner):
    """The draw tensors of S simulations resident in HBM (Context.upload_sims): device buffer + tensor4_args' nine entries
    (dtype, S, C, N, P and their strides).  Only Context.sbc_ranks takes it; it is NOT a DeviceTensor, so that no call on
    one (C, N, P) tensor can read the nine entries as seven."""

    def __init__(self, ctx: "Context", buf, targs):
        if len(targs) != 9:
            raise ValueError("DeviceSims needs (dtype, S, C, N, P, stride_s, stride_c, stride_n, stride_p)")
        self.ctx, self.buf, self.targs = ctx, buf, tuple(targs)

    @property
    def shape_scnp(self):
        return self.targs[1:5]

    def free(self):
        self.buf.free()


class CsvTable(typing.NamedTuple):
    """One file of Context.csv_table_decode.  close() frees the slices."""
    names: list            # parameter names in file order, without `chain` / `draw`
    values: DeviceView     # [P][M] f64 in file row order
    all_int: np.ndarray    # [P] bool: every literal of the column is an integer
    ids: tuple             # (chain, draw) as int64 DeviceViews of M entries, None for an absent column
    hard: int              # fields finished on the host
    header: list           # every column name of the file

    def close(self):
        for b in (self.values, *self.ids):
            if b is not None:
                b.free()


class Context:
    """One GPU + one HIP stream (mcr_ctx).  Not thread-safe: one Context per thread."""

    def __init__(self, device: int | None = None):
        self.lib = load_library()
        if device is None:
            device = int(os.environ.get("MCMC_REF_HIP_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        h = C.c_void_p()
        rc = self.lib.mcr_init(int(device), C.byref(h))
        if rc != MCR_OK:
            msg = (self.lib.mcr_last_error(None) or b"").decode()
            if rc == MCR_ENODEVICE:
                raise HipUnavailableError(msg)
            raise McrError(rc, msg)
        self.handle = h
        self.device = int(device)
        self._pending: list[SummaryBuffers] = []

    def close(self):
        if getattr(self, "handle", None):
            self.lib.mcr_free(self.handle)
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

    # -- errors ------------------------------------------------------------------------------
    def _check(self, rc: int):
        if rc != MCR_OK:
            raise McrError(rc, (self.lib.mcr_last_error(self.handle) or b"").decode())

    # -- device memory --------------------------------------------------------------------------
    def upload(self, draws: np.ndarray, layout: str = "pcn") -> DeviceTensor:
        targs = tensor_args(draws, layout)
        if not draws.flags.c_contiguous:
            raise ValueError("upload() needs a C-contiguous array (permute the layout string instead)")
        with contextlib.ExitStack() as stack:
            buf = stack.enter_context(DeviceBuffer(self, max(draws.nbytes, 8))).upload(draws)
            stack.pop_all()
        return DeviceTensor(self, buf, targs)

    def alloc_tensor(self, C_: int, N: int, P: int, dtype=np.float64) -> DeviceTensor:
        """Uninitialised [P][C][N] device tensor (fill it with fill_synthetic)."""
        es = np.dtype(dtype).itemsize
        buf = DeviceBuffer(self, max(C_ * N * P * es, 8))
        code = MCR_F64 if np.dtype(dtype) == np.float64 else MCR_F32
        return DeviceTensor(self, buf, (code, C_, N, P, N, 1, C_ * N))

    def fill_synthetic(self, t: DeviceTensor, seed: int = 4711, p0: int = 0):
        """Synthetic stress draws; p0 > 0: `t` is the parameter block [p0, p0 + P) of a larger tensor."""
        code, C_, N, P = t.targs[:4]
        self._check(self.lib.mcr_fill_synthetic_at(self.handle, t.buf.ptr, code, C_, N, P, int(p0), seed))

    def hbm_probe(self, nbytes: int = 4 << 30, iters: int = 5) -> dict:
        """Measured HBM rates of this device (GB/s): read-only streaming kernel and device-to-device copy."""
        rd, cp = C.c_double(0.0), C.c_double(0.0)
        self._check(self.lib.mcr_hbm_probe(self.handle, int(nbytes), int(iters), C.byref(rd), C.byref(cp)))
        return {"read_GBps": rd.value, "copy_GBps": cp.value}

    def sync(self):
        self._check(self.lib.mcr_sync(self.handle))

    # -- hot path -----------------------------------------------------------------------------
    @staticmethod
    def _quantiles(quantiles):
        qs = np.ascontiguousarray(list(quantiles), dtype=np.float64)
        if qs.size > MCR_MAX_QUANTILES:
            raise ValueError(f"at most {MCR_MAX_QUANTILES} quantiles")
        return qs

    def summarize(self, draws, layout: str = "pcn", min_chains: int = 4,
                  quantiles=(0.05, 0.5, 0.95), diagnostics: bool = True) -> dict:
        """All per-parameter statistics of a host array or a DeviceTensor (synchronous).

        diagnostics=False: Backend.stats only (mean/std/quantiles/median); the rank, fold and
        autocovariance kernels are not launched and the diagnostics come back as NaN.
        """
        qs = self._quantiles(quantiles)
        if isinstance(draws, DeviceTensor) and draws.chain_off is not None:
            return self.summarize_chains(draws, min_chains=min_chains, quantiles=quantiles, diagnostics=diagnostics)
        if isinstance(draws, DeviceTensor):
            targs, ptr, fn = draws.targs, draws.buf.ptr, self.lib.mcr_summarize_dev
        else:
            targs, fn = tensor_args(draws, layout), self.lib.mcr_summarize
            ptr = draws.ctypes.data_as(C.c_void_p)
        bufs = SummaryBuffers(targs[3], qs.size, diagnostics)
        self._check(fn(self.handle, ptr, *targs, int(min_chains), _as_dp(qs), qs.size, C.byref(bufs.struct)))
        return bufs.result()

    def enqueue(self, t: DeviceTensor, min_chains: int = 4, quantiles=(0.05, 0.5, 0.95),
                diagnostics: bool = True, bufs: "SummaryBuffers | None" = None) -> SummaryBuffers:
        """Asynchronous summarize.  `bufs`: result buffers of an EARLIER, already delivered call of the same shape to
        write into again (a caller that streams many same-shape models keeps a ring of them instead of allocating
        twelve arrays per call)."""
        qs = self._quantiles(quantiles)
        if bufs is None or bufs.P != t.targs[3] or bufs.nq != qs.size or bufs.diagnostics != diagnostics:
            bufs = SummaryBuffers(t.targs[3], qs.size, diagnostics)
        if t.chain_off is not None:
            rc = self.lib.mcr_summarize_chains_enqueue(self.handle, t.buf.ptr, t.targs[6], _as_ip(t.chain_off), t.targs[1],
                                                       t.targs[3], int(min_chains), _as_dp(qs), qs.size,
                                                       C.byref(bufs.struct))
        else:
            rc = self.lib.mcr_summarize_enqueue(self.handle, t.buf.ptr, *t.targs, int(min_chains), _as_dp(qs), qs.size,
                                                C.byref(bufs.struct))
        self._check(rc)
        self._pending.append(bufs)
        return bufs

    def ragged_tensor(self, buf, counts, P: int, stride_p: int | None = None) -> DeviceTensor:
        """The DeviceTensor of f64 draws [P][M] already in `buf` whose chains are `counts` draws long, back to back in
        (chain, draw) order; parameter p starts at element p * stride_p (default M)."""
        counts = np.asarray(counts, dtype=np.int64).reshape(-1)
        off = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(counts, dtype=np.int64)])
        M = int(off[-1])
        n = int(counts.min()) if counts.size else 0
        return DeviceTensor(self, buf, (MCR_F64, int(counts.size), n, int(P), 0, 1, M if stride_p is None else int(stride_p)),
                            np.ascontiguousarray(off))

    def summarize_chains(self, draws, counts=None, min_chains: int = 4, quantiles=(0.05, 0.5, 0.95),
                         diagnostics: bool = True) -> dict:
        """All per-parameter statistics of draws [P][M] whose chains are `counts` draws long (chains of unequal length,
        mcr_summarize_chains_dev): ONE pipeline for all parameters.  `draws`: a host array [P][M] (uploaded for the
        call) or a DeviceTensor of ragged_tensor (then `counts` is not needed).  The result is shaped like
        summarize()'s: pooled mean / std / q / median, and the diagnostics of diagnostics.py for ragged chains."""
        qs = self._quantiles(quantiles)
        with contextlib.ExitStack() as stack:
            if isinstance(draws, DeviceTensor):
                t = draws if draws.chain_off is not None else self.ragged_tensor(draws.buf, counts, draws.targs[3])
            else:
                x = np.ascontiguousarray(draws, dtype=np.float64)
                if x.ndim != 2:
                    raise ValueError("draws must be 2-D [P][M]")
                if int(np.sum(counts)) != x.shape[1]:
                    raise ValueError("counts must add up to the number of draws per parameter")
                owned = stack.enter_context(DeviceBuffer(self, max(x.nbytes, 8)))
                if x.nbytes:
                    owned.upload(x)
                t = self.ragged_tensor(owned, counts, x.shape[0])
            bufs = SummaryBuffers(t.targs[3], qs.size, diagnostics)
            self._check(self.lib.mcr_summarize_chains_dev(self.handle, t.buf.ptr, t.targs[6], _as_ip(t.chain_off),
                                                          t.targs[1], t.targs[3], int(min_chains), _as_dp(qs), qs.size,
                                                          C.byref(bufs.struct)))
        return bufs.result()

    def chain_layout(self, chain_ptr, draw_ptr, M: int, cap: int = 256, order: "DeviceBuffer | None" = None):
        """(chain ids, order, counts) of a table's id columns in device memory (mcr_chain_layout_dev): `order` is a
        DeviceBuffer of M int64 row numbers in np.lexsort((draw, chain)) order -- the caller's `order` buffer (at least
        8 M bytes) or, without one, a new buffer the caller frees -- or None when the rows are in that order already.
        None when the library declines (MCR_EFALLBACK: no 64-bit row key) -- sort on the host then."""
        with contextlib.ExitStack() as stack:                # a buffer made here is handed on only with a row order in it
            if order is None:
                order = stack.enter_context(DeviceBuffer(self, max(int(M) * 8, 8)))
            ids, counts = np.zeros(max(cap, 1), dtype=np.int64), np.zeros(max(cap, 1), dtype=np.int64)
            n, in_order = C.c_int(0), C.c_int(0)
            rc = self.lib.mcr_chain_layout_dev(self.handle, chain_ptr, draw_ptr, int(M), order.ptr, _as_ip(ids), _as_ip(counts),
                                               int(cap), C.byref(n), C.byref(in_order))
            if rc == MCR_EFALLBACK:
                return None
            self._check(rc)
            if not in_order.value:
                stack.pop_all()
            return ids[:n.value].copy(), None if in_order.value else order, counts[:n.value].copy()

    def chain_layout_many(self, tables, cap: int = 256) -> list:
        """The in-order test of many tables in one round trip (mcr_chain_layout_many_dev): tables = [(chain pointer,
        draw pointer, rows), ...] in device memory; per table (chain ids, counts) when its rows are in (chain, draw)
        order and it has at most `cap` chains, else None -- chain_layout sorts that one."""
        n = len(tables)
        arr = (IdColumns * max(n, 1))()
        for i, (cp, dp, M) in enumerate(tables):
            arr[i] = IdColumns(cp if isinstance(cp, int) else cp.value, dp if isinstance(dp, int) else dp.value, int(M))
        ids = np.zeros((max(n, 1), max(cap, 1)), dtype=np.int64)
        counts = np.zeros((max(n, 1), max(cap, 1)), dtype=np.int64)
        nch, ino = (C.c_int * max(n, 1))(), (C.c_int * max(n, 1))()
        self._check(self.lib.mcr_chain_layout_many_dev(self.handle, arr, n, _as_ip(ids), _as_ip(counts), int(cap), nch, ino))
        return [(ids[i, :nch[i]].copy(), counts[i, :nch[i]].copy()) if ino[i] and nch[i] <= cap else None for i in range(n)]

    def write_parquet(self, columns, rows: int, row_group_rows: int = 0) -> PqImage:
        """mcr_parquet_write_dev: the Parquet image of `rows` rows of device columns (pq_column / pq_sequence tuples), encoded and
        compressed on the GPU.  Close the image (or use it as a context manager) to free its pinned memory."""
        arr, _keep = _pq_columns(columns, host=False)
        h = C.c_void_p()
        self._check(self.lib.mcr_parquet_write_dev(self.handle, arr, len(columns), int(rows), int(row_group_rows), C.byref(h)))
        return PqImage(self.lib, h)

    def write_csv(self, columns, rows: int, row_index=None, header: str = "quoted") -> TextImage:
        """mcr_csv_write_dev: the CSV text of device columns (pq_column / pq_sequence tuples) of `rows` rows, formatted on
        the GPU, byte for byte what pyarrow.csv.write_csv gives the same table.  row_index selects and orders the rows:
        (device pointer or buffer, count) -- what select_rows returns -- or int64 values in host memory, uploaded
        here.  header: "quoted" (pyarrow's default), "plain" or "none".  Close the image to free its pinned memory."""
        arr, _keep = _pq_columns(columns, host=False)
        ptr, n = None, 0
        with contextlib.ExitStack() as stack:
            if row_index is not None and isinstance(row_index, tuple):
                ptr, n = row_index
                ptr = getattr(ptr, "ptr", ptr)
            elif row_index is not None:
                idx = np.ascontiguousarray(row_index, dtype=np.int64)
                ptr, n = stack.enter_context(DeviceBuffer(self, max(idx.nbytes, 8))).upload(idx).ptr, idx.size
            h = C.c_void_p()
            self._check(self.lib.mcr_csv_write_dev(self.handle, arr, len(columns), int(rows), ptr, int(n), CSV_HEADERS[header],
                                                   C.byref(h)))
        return TextImage(self.lib, h)

    def select_rows(self, chain_ptr, M: int, chains) -> tuple:
        """mcr_select_rows_dev: (device buffer of int64 row indices, count) of the rows of the device int64 column
        `chain_ptr[0 .. M)` whose value is in `chains`, in order: the row_index of write_csv.  Free the buffer."""
        want = np.ascontiguousarray(list(chains), dtype=np.int64)
        n = C.c_int64()
        with contextlib.ExitStack() as stack:
            out = stack.enter_context(DeviceBuffer(self, max(int(M) * 8, 8)))
            self._check(self.lib.mcr_select_rows_dev(self.handle, getattr(chain_ptr, "ptr", chain_ptr), int(M), _as_ip(want), want.size,
                                                     out.ptr, C.byref(n)))
            stack.pop_all()
        return out, int(n.value)

    def gather_rows_order(self, src_ptr, P: int, M: int, order_ptr, dst_ptr):
        """dst[p][k] = src[p][order[k]], everything in device memory (mcr_gather_rows_order_dev)."""
        self._check(self.lib.mcr_gather_rows_order_dev(self.handle, src_ptr, int(P), int(M), order_ptr, dst_ptr))

    def summarize_models(self, tensors, min_chains: int = 4, quantiles=(0.05, 0.5, 0.95)) -> list[dict]:
        """One C call for a list of DeviceTensors (independent models), pipelined through the lanes."""
        qs = self._quantiles(quantiles)
        n = len(tensors)
        descs = (ModelDesc * max(n, 1))()
        outs = (Summary * max(n, 1))()
        bufs = []
        for i, t in enumerate(tensors):
            code, C_, N, P, sc, sn, sp = t.targs
            descs[i] = ModelDesc(t.buf.ptr, code, int(min_chains), C_, N, P, sc, sn, sp)
            b = SummaryBuffers(P, qs.size)
            outs[i] = b.struct
            bufs.append(b)
        self._check(self.lib.mcr_summarize_models(self.handle, descs, n, _as_dp(qs), qs.size, outs))
        return [b.result() for b in bufs]

    def summarize_files(self, paths, min_chains: int = 4, quantiles=(0.05, 0.5, 0.95), diagnostics: bool = True,
                        phases: dict | None = None) -> tuple[list[tuple[list[str], int, int]], dict] | None:
        """Draws files -> statistics in ONE mcr_summarize_files call (mmap, parse, batched decode, layout check,
        pipelined statistics): ([(parameter names, chains, draws per chain) per file], the statistics of all their
        parameters in file order as ONE summary shaped like summarize()'s, without q_lo -- split_result cuts it per
        file).  None when a file needs the general route (MCR_ELAYOUT: rows out of (chain, draw) order, or chains of
        unequal length with diagnostics).  `phases` is filled with the call's host clock (FS_PHASES, ms) and its
        `jobs`."""
        L, fs = self.lib, C.c_void_p()
        qs = np.ascontiguousarray(list(quantiles), dtype=np.float64)
        arr = (C.c_char_p * len(paths))(*[os.fsencode(p) for p in paths])
        rc = L.mcr_summarize_files(self.handle, arr, len(paths), int(min_chains), _as_dp(qs), qs.size,
                                   int(diagnostics), C.byref(fs))
        if rc == MCR_ELAYOUT:
            return None
        self._check(rc)
        try:
            if phases is not None:
                ms = np.zeros(len(FS_PHASES))
                L.mcr_fileset_phases(fs, _as_dp(ms), len(FS_PHASES))
                phases.update(zip(FS_PHASES, ms.tolist()))
                phases["jobs"] = int(L.mcr_fileset_jobs(fs))
            files = range(L.mcr_fileset_size(fs))
            counts = [int(L.mcr_fileset_params(fs, i)) for i in files]
            total, w = sum(counts), len(FS_EXPORT)
            rows = np.empty((max(total, 1), w + qs.size))            # the whole set in one export
            L.mcr_fileset_export(fs, _as_dp(rows), total)
            rows = rows[:total]
            need = int(L.mcr_fileset_names(fs, None, 0))
            buf = C.create_string_buffer(max(need, 1))
            L.mcr_fileset_names(fs, buf, need)
            names = buf.raw[:need].decode().split("\0")
            r = {k: rows[:, j] for j, k in enumerate(FS_EXPORT)}
            for k in ("lag_bulk", "lag_tail"):      # NaN without diagnostics: zeros, as summarize() leaves them
                r[k] = r[k].astype(np.int64) if diagnostics else np.zeros(total, dtype=np.int64)
            r["q"] = rows[:, w:]
            out, r0 = [], 0
            for i, P in zip(files, counts):
                out.append((names[r0:r0 + P], int(L.mcr_fileset_chains(fs, i)), int(L.mcr_fileset_draws(fs, i))))
                r0 += P
            return out, r
        finally:
            L.mcr_fileset_free(fs)

    def csv_decode(self, paths, select, phases: dict | None = None) -> tuple[list[str], "DeviceTensor", int]:
        """CmdStan chain files -> (parameter names, [P][C][N] DeviceTensor, fields finished on the host): the library
        reads the files (mcr_csv_open_paths), indexes their data rows (mcr_csv_stage) and parses the selected columns of
        the first N = min over files rows on the device (mcr_csv_decode).  `select(file index, header names)` returns
        (names, header column of each name) of one file; the first file's names give the tensor's parameter order and
        every other file must hold the same set.  `phases` is filled with the host clock of the three calls (ms)."""
        L, n = self.lib, len(paths)
        arr = (C.c_char_p * max(n, 1))(*[os.fsencode(p) for p in paths])
        hs = (C.c_void_p * max(n, 1))()
        t0 = time.perf_counter()
        self._check(L.mcr_csv_open_paths(self.handle, arr, n, hs))
        try:
            picked = [select(f, [(L.mcr_csv_column_name(hs[f], c) or b"").decode() for c in range(L.mcr_csv_num_columns(hs[f]))])
                      for f in range(n)]
            names = picked[0][0]
            if not names:
                raise ValueError("chain draws contain no parameters")
            cols = np.empty((n, len(names)), dtype=np.intc)
            for f, (nm, cl) in enumerate(picked):
                if set(nm) != set(names):
                    raise ValueError(f"chain {f} parameter keys mismatch")
                at = dict(zip(nm, cl))
                cols[f] = [at[k] for k in names]
            t1 = time.perf_counter()
            rows = np.zeros(n, dtype=np.int64)
            self._check(L.mcr_csv_stage(self.handle, hs, n, _as_ip(rows)))
            t2 = time.perf_counter()
            N, P = int(rows.min()), len(names)
            hard = C.c_int64(0)
            with contextlib.ExitStack() as stack:
                t = stack.enter_context(self.alloc_tensor(n, N, P))
                self._check(L.mcr_csv_decode(self.handle, cols.ctypes.data_as(C.POINTER(C.c_int)), P, N, t.buf.ptr,
                                             N, 1, n * N, C.byref(hard)))
                if phases is not None:
                    t3 = time.perf_counter()
                    phases.update(read_upload_ms=(t1 - t0) * 1e3, index_ms=(t2 - t1) * 1e3, parse_finish_ms=(t3 - t2) * 1e3,
                                  text_bytes=sum(os.path.getsize(p) for p in paths), hard=int(hard.value))
                stack.pop_all()
                return names, t, int(hard.value)
        finally:
            for h in hs[:n]:
                if h:
                    L.mcr_csv_close(h)

    def csv_table_decode(self, paths, phases: dict | None = None):
        """Table CSVs -> per file a CsvTable (parameter names in file order without `chain` / `draw`, [P][M] f64 DeviceView in file
        row order, all_int flags [P], (chain ids, draw ids) as int64 DeviceViews of M entries or None for an absent
        column, fields finished on the host, header names): ONE read (mcr_csv_open_table_paths), one line index
        (mcr_csv_stage) and one parse (mcr_csv_decode_table) for all files.  None when the host reader must decide for
        one of them: the library answers MCR_EFALLBACK or a header is not UTF-8 (`phases["fallback"]` says why).
        `phases` receives the host clock of the three calls (ms).  Close every entry."""
        L, n = self.lib, len(paths)
        note = phases if phases is not None else {}
        arr = (C.c_char_p * max(n, 1))(*[os.fsencode(p) for p in paths])
        hs = (C.c_void_p * max(n, 1))()
        t0 = time.perf_counter()
        self._check(L.mcr_csv_open_table_paths(self.handle, arr, n, hs))

        def declined(rc: int) -> bool:
            if rc == MCR_EFALLBACK:
                note["fallback"] = (L.mcr_last_error(self.handle) or b"").decode(errors="replace")
                return True
            self._check(rc)
            return False

        try:
            try:
                heads = [[(L.mcr_csv_column_name(hs[f], c) or b"").decode() for c in range(L.mcr_csv_num_columns(hs[f]))]
                         for f in range(n)]
            except UnicodeDecodeError:
                note["fallback"] = "csv table: a header name is not UTF-8"
                return None
            t1 = time.perf_counter()
            rows = np.zeros(max(n, 1), dtype=np.int64)
            if declined(L.mcr_csv_stage(self.handle, hs, n, _as_ip(rows))):
                return None
            t2 = time.perf_counter()
            params = [[c for c, name in enumerate(h) if name not in ("chain", "draw")] for h in heads]
            Pmax = max((len(p) for p in params), default=0)
            cols = np.full((max(n, 1), max(Pmax, 1)), -1, dtype=np.intc)
            ids = np.full((max(n, 1), 2), -1, dtype=np.intc)
            for f, h in enumerate(heads):
                cols[f, :len(params[f])] = params[f]
                ids[f] = [h.index("chain") if "chain" in h else -1, h.index("draw") if "draw" in h else -1]
            all_int = np.zeros((max(n, 1), max(Pmax, 1)), dtype=np.uint8)
            sizes = [len(params[f]) * int(rows[f]) * 8 for f in range(n)]
            hard = C.c_int64(0)
            with contextlib.ExitStack() as stack, DeviceArena(self, sum(sizes)) as out, \
                    DeviceArena(self, 2 * int(rows[:n].sum()) * 8) as idb:
                if declined(L.mcr_csv_decode_table(self.handle, cols.ctypes.data_as(C.POINTER(C.c_int)), cols.shape[1],
                                                   ids.ctypes.data_as(C.POINTER(C.c_int)), int(rows.max()), out.buf.ptr, 0, 1, 0,
                                                   idb.buf.ptr, all_int.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(hard))):
                    return None
                got, off, ioff = [], 0, 0
                for f in range(n):                           # the slices are the caller's; the arenas live as long as they do
                    M, P = int(rows[f]), len(params[f])
                    pair = [stack.enter_context(idb.view((ioff + w * M) * 8, M * 8)) if ids[f, w] >= 0 else None for w in range(2)]
                    got.append(CsvTable([heads[f][c] for c in params[f]], stack.enter_context(out.view(off, sizes[f])),
                                        all_int[f, :P].astype(bool), tuple(pair), int(hard.value), heads[f]))
                    off += sizes[f]
                    ioff += 2 * M
                if phases is not None and n:
                    t3 = time.perf_counter()
                    phases.update(read_upload_ms=(t1 - t0) * 1e3, index_ms=(t2 - t1) * 1e3, parse_finish_ms=(t3 - t2) * 1e3,
                                  text_bytes=sum(os.path.getsize(p) for p in paths), hard=int(hard.value))
                stack.pop_all()
                return got
        finally:
            for h in hs[:n]:
                if h:
                    L.mcr_csv_close(h)

    def json_decode(self, text: bytes, select, phases: dict | None = None):
        """Chain-list JSON text -> (parameter names, [P][C][N] DeviceTensor, all_int [C][P], elements finished on the
        host): the library uploads and indexes the document and walks its skeleton (mcr_json_open), then parses the
        selected arrays on the device (mcr_json_decode).  `select(keys per chain, array lengths per chain)` returns
        (names, N, key index [C][P]) or None.  None when the host reader must decide: the library answers
        MCR_EFALLBACK (`phases["fallback"]` has its message), a key is not UTF-8, or `select` returns None.  `phases`
        is filled with the host clock of the two calls (ms)."""
        L, h = self.lib, C.c_void_p()
        note = phases if phases is not None else {}
        t0 = time.perf_counter()
        rc = L.mcr_json_open(self.handle, text, len(text), C.byref(h))
        if rc == MCR_EFALLBACK:
            note["fallback"] = (L.mcr_last_error(self.handle) or b"").decode(errors="replace")
            return None
        self._check(rc)
        try:
            n = L.mcr_json_num_chains(h)
            counts = [L.mcr_json_num_keys(h, c) for c in range(n)]
            try:
                keys = [[L.mcr_json_key(h, c, k).decode() for k in range(counts[c])] for c in range(n)]
            except UnicodeDecodeError:
                note["fallback"] = "json: a key is not UTF-8"
                return None
            lengths = [[int(L.mcr_json_length(h, c, k)) for k in range(counts[c])] for c in range(n)]
            picked = select(keys, lengths)
            if picked is None:
                return None
            names, N, arrays = picked
            P = len(names)
            arrays = np.ascontiguousarray(arrays, dtype=np.intc).reshape(n, P)
            t1 = time.perf_counter()
            hard = C.c_int64(0)
            all_int = np.zeros((n, max(P, 1)), dtype=np.uint8)
            with contextlib.ExitStack() as stack:
                t = stack.enter_context(self.alloc_tensor(n, N, P))
                rc = L.mcr_json_decode(self.handle, h, arrays.ctypes.data_as(C.POINTER(C.c_int)), P, N, t.buf.ptr, N, 1, n * N,
                                       all_int.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(hard))
                if rc == MCR_EFALLBACK:
                    note["fallback"] = (L.mcr_last_error(self.handle) or b"").decode(errors="replace")
                    return None
                self._check(rc)
                if phases is not None:
                    t2 = time.perf_counter()
                    phases.update(upload_index_walk_ms=(t1 - t0) * 1e3, parse_finish_ms=(t2 - t1) * 1e3, text_bytes=len(text),
                                  hard=int(hard.value))
                stack.pop_all()
                return list(names), t, all_int[:, :P].astype(bool), int(hard.value)
        finally:
            L.mcr_json_close(h)

    def wait(self):
        try:
            self._check(self.lib.mcr_summarize_wait(self.handle))
        finally:
            self._pending.clear()

    def wait_one(self) -> SummaryBuffers | None:
        """Wait for the oldest outstanding enqueue only; returns its buffers (None if nothing is pending)."""
        if not self._pending:
            return None
        bufs = self._pending.pop(0)
        self._check(self.lib.mcr_summarize_wait_one(self.handle))
        return bufs

    @property
    def inflight(self) -> int:
        return len(self._pending)

    def diagnose_chains(self, chains, min_chains: int = 4, debug: bool = False) -> dict:
        """split_rhat / ess_bulk / ess_tail of ONE parameter given as (possibly ragged) chains."""
        off = np.zeros(len(chains) + 1, dtype=np.int64)
        for i, c in enumerate(chains):
            off[i + 1] = off[i] + len(c)
        M = int(off[-1])
        pooled = np.empty(max(M, 1), dtype=np.float64)
        for i, c in enumerate(chains):
            pooled[off[i]:off[i + 1]] = np.asarray(c, dtype=np.float64)
        bufs = SummaryBuffers(1, 0)
        dbg = [np.full(max(M, 1), np.nan) for _ in range(4)] if debug else [None] * 4
        self._check(self.lib.mcr_diagnose_chains(self.handle, _as_dp(pooled), _as_ip(off), len(chains),
                                                 int(min_chains), C.byref(bufs.struct), *[_as_dp(d) for d in dbg]))
        r = bufs.result()
        out = {k: (float(r[k][0]) if k in SUMMARY_F64 else int(r[k][0]))
               for k in ("rhat", "rhat_bulk", "rhat_tail", "ess_bulk", "ess_tail", "median", "lag_bulk",
                         "lag_tail")}
        if debug:
            for name, d in zip(("z_bulk", "z_tail", "rank_bulk", "rank_tail"), dbg):
                out[name] = [d[off[i]:off[i + 1]].copy() for i in range(len(chains))]
        return out

    def basic_stats(self, values) -> dict:
        v = np.ascontiguousarray(values)
        if v.dtype not in (np.float64, np.float32):
            v = v.astype(np.float64)
        mean, std = C.c_double(math.nan), C.c_double(math.nan)
        code = MCR_F64 if v.dtype == np.float64 else MCR_F32
        self._check(self.lib.mcr_basic_stats(self.handle, v.ctypes.data_as(C.c_void_p), code, v.size,
                                             C.byref(mean), C.byref(std)))
        return {"mean": mean.value, "std": std.value}

    def moments(self, t: DeviceTensor) -> tuple[np.ndarray, np.ndarray]:
        P = t.targs[3]
        mean, std = np.full(max(P, 1), np.nan), np.full(max(P, 1), np.nan)
        self._check(self.lib.mcr_moments_dev(self.handle, t.buf.ptr, *t.targs, _as_dp(mean), _as_dp(std)))
        return mean[:P], std[:P]

    def compare(self, ref, actual, tol: float):
        r = np.ascontiguousarray(ref, dtype=np.float64)
        a = np.ascontiguousarray(actual, dtype=np.float64)
        if r.shape != a.shape:
            raise ValueError("ref and actual must have the same shape")
        rel = np.empty(max(r.size, 1))
        ok = np.zeros(max(r.size, 1), dtype=np.uint8)
        self._check(self.lib.mcr_compare(self.handle, _as_dp(r), _as_dp(a), r.size, float(tol), _as_dp(rel),
                                         ok.ctypes.data_as(C.POINTER(C.c_uint8))))
        return rel[:r.size], ok[:r.size].astype(bool)

    # -- extensions (not in the reference) -------------------------------------------------------------
    def two_sample(self, ref, actual) -> tuple[np.ndarray, np.ndarray]:
        """(KS statistic, Wasserstein-1) per parameter; ref [P][Mr], actual [P][Ma] (2-D, finite)."""
        r = np.ascontiguousarray(ref, dtype=np.float64)
        a = np.ascontiguousarray(actual, dtype=np.float64)
        if r.ndim != 2 or a.ndim != 2 or r.shape[0] != a.shape[0]:
            raise ValueError("ref and actual must be 2-D with the same number of parameters")
        if not (np.isfinite(r).all() and np.isfinite(a).all()):
            raise ValueError("draws contain non-finite values")
        P = r.shape[0]
        ks, w1 = np.full(max(P, 1), np.nan), np.full(max(P, 1), np.nan)
        self._check(self.lib.mcr_two_sample(self.handle, _as_dp(r), r.shape[1], _as_dp(a), a.shape[1], P,
                                            _as_dp(ks), _as_dp(w1)))
        return ks[:P], w1[:P]

    @staticmethod
    def _sliced_args(directions, center, P: int):
        w = np.ascontiguousarray(directions, dtype=np.float64)
        if w.ndim != 2 or (w.shape[0] and w.shape[1] != P):
            raise ValueError("directions must be 2-D [K][P] with one weight per parameter")
        c = None if center is None else np.ascontiguousarray(center, dtype=np.float64)
        if c is not None and c.shape != (P,):
            raise ValueError("center must have one entry per parameter")
        if not (np.isfinite(w).all() and (c is None or np.isfinite(c).all())):
            raise ValueError("directions and center must be finite")
        return w, c

    def sliced_two_sample(self, ref, actual, directions, center=None, projections: bool = False):
        """(KS statistic, Wasserstein-1) per direction of the two samples projected onto `directions` [K][P]:
        z[k] = sum_p directions[k][p] * (x[p] - center[p]), p in order, one fma each (mcr_sliced_two_sample).  ref [P][Mr],
        actual [P][Ma] (2-D, finite); center [P] or None for zeros.  projections=True appends the projected rows
        zr [K][Mr], za [K][Ma]."""
        r = np.ascontiguousarray(ref, dtype=np.float64)
        a = np.ascontiguousarray(actual, dtype=np.float64)
        if r.ndim != 2 or a.ndim != 2 or r.shape[0] != a.shape[0]:
            raise ValueError("ref and actual must be 2-D with the same number of parameters")
        if not (np.isfinite(r).all() and np.isfinite(a).all()):
            raise ValueError("draws contain non-finite values")
        w, c = self._sliced_args(directions, center, r.shape[0])
        return self._sliced(self.lib.mcr_sliced_two_sample, _as_dp(r), r.shape[1], _as_dp(a), a.shape[1], r.shape[0], w, c,
                            projections)

    def sliced_two_sample_dev(self, ref_ptr, Mr: int, act_ptr, Ma: int, P: int, directions, center=None,
                              projections: bool = False):
        """sliced_two_sample on draws already in this context's device memory: ref_ptr -> [P][Mr] f64, act_ptr -> [P][Ma]
        f64 (device addresses or DeviceBuffer.ptr).  Non-finite draws raise McrError (MCR_ENONFINITE)."""
        w, c = self._sliced_args(directions, center, P)
        as_ptr = lambda v: v if isinstance(v, C.c_void_p) else C.c_void_p(int(v))
        return self._sliced(self.lib.mcr_sliced_two_sample_dev, as_ptr(ref_ptr), int(Mr), as_ptr(act_ptr), int(Ma), int(P), w, c,
                            projections)

    def _sliced(self, entry, ref, Mr, act, Ma, P, w, c, projections):
        K = w.shape[0]
        ks, w1 = np.full(max(K, 1), np.nan), np.full(max(K, 1), np.nan)
        zr = np.empty((K, Mr)) if projections else None
        za = np.empty((K, Ma)) if projections else None
        self._check(entry(self.handle, ref, Mr, act, Ma, P, _as_dp(w), _as_dp(c), K, _as_dp(ks), _as_dp(w1),
                          _as_dp(zr), _as_dp(za)))
        return (ks[:K], w1[:K], zr, za) if projections else (ks[:K], w1[:K])

    def sliced_dirs_per_chunk(self, Mr: int, Ma: int, P: int, K: int) -> int:
        """Directions per workspace chunk of a sliced_two_sample call of this shape (mcr_sliced_plan)."""
        v = C.c_int64(0)
        self._check(self.lib.mcr_sliced_plan(self.handle, Mr, Ma, P, K, C.byref(v)))
        return int(v.value)

    @staticmethod
    def _energy_scale(scale, P: int):
        s = None if scale is None else np.ascontiguousarray(scale, dtype=np.float64)
        if s is not None and s.shape != (P,):
            raise ValueError("scale must have one entry per parameter")
        if s is not None and not (np.isfinite(s).all() and (s >= 0).all()):
            raise ValueError("scale must be finite and >= 0")
        return s

    def energy_distance(self, ref, actual, scale=None) -> dict:
        """Energy distance of Szekely and Rizzo between the joint draws ref [P][Mr] and actual [P][Ma] (2-D, finite), every
        parameter multiplied by scale[p] first (None: ones) -- mcr_energy_distance.  Keys: a, b, c (the mean distances
        between the samples, within ref, within actual), e = 2a - b - c, h = e / 2a in [0, 1], t = Mr Ma / (Mr + Ma) e."""
        r = np.ascontiguousarray(ref, dtype=np.float64)
        a = np.ascontiguousarray(actual, dtype=np.float64)
        if r.ndim != 2 or a.ndim != 2 or r.shape[0] != a.shape[0]:
            raise ValueError("ref and actual must be 2-D with the same number of parameters")
        if not (np.isfinite(r).all() and np.isfinite(a).all()):
            raise ValueError("draws contain non-finite values")
        s = self._energy_scale(scale, r.shape[0])
        return self._energy(self.lib.mcr_energy_distance, _as_dp(r), r.shape[1], _as_dp(a), a.shape[1], r.shape[0], s)

    def energy_distance_dev(self, ref_ptr, Mr: int, act_ptr, Ma: int, P: int, scale=None) -> dict:
        """energy_distance on draws already in this context's device memory: ref_ptr -> [P][Mr] f64, act_ptr -> [P][Ma]
        f64 (device addresses or DeviceBuffer.ptr).  Non-finite draws raise McrError (MCR_ENONFINITE)."""
        s = self._energy_scale(scale, int(P))
        as_ptr = lambda v: v if isinstance(v, C.c_void_p) else C.c_void_p(int(v))
        return self._energy(self.lib.mcr_energy_distance_dev, as_ptr(ref_ptr), int(Mr), as_ptr(act_ptr), int(Ma), int(P), s)

    def _energy(self, entry, ref, Mr, act, Ma, P, s) -> dict:
        out = np.full(6, np.nan)
        self._check(entry(self.handle, ref, Mr, act, Ma, P, _as_dp(s), _as_dp(out)))
        return dict(zip(ENERGY_KEYS, (float(v) for v in out)))

    def energy_workspace(self, Mr: int, Ma: int, P: int) -> int:
        """Bytes of workspace an energy_distance call of this shape carves (mcr_energy_workspace)."""
        v = C.c_size_t(0)
        self._check(self.lib.mcr_energy_workspace(self.handle, int(Mr), int(Ma), int(P), C.byref(v)))
        return int(v.value)

    def nested_rhat(self, draws, superchain_ids, layout: str = "pcn") -> dict:
        """Nested R-hat per parameter (mcr_nested_rhat: Margossian et al., posterior::rhat_nested) of a host array or a
        DeviceTensor with any number of chains up to MCR_NESTED_MAX_CHAINS.  superchain_ids: one integer label per chain
        (any labels, every one equally often), or an int K for K contiguous blocks of C / K chains.  Arrays per
        parameter: nrhat = max(nrhat_bulk, nrhat_tail), nrhat_raw (the paper's, on the draws), between_* / within_* (B and
        W of each kind).  Chains are not split."""
        targs, ptr, fn, _ = self._tensor_call(draws, layout, "nested_rhat", False)
        ids = superchain_labels(superchain_ids, targs[1])
        P = targs[3]
        arrs = {n: np.full(max(P, 1), np.nan) for n in NESTED_FIELDS}
        out = Nested(**{n: _as_dp(a) for n, a in arrs.items()})
        self._check(fn(self.handle, ptr, *targs, ids.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(out)))
        return {n: a[:P] for n, a in arrs.items()}

    def nested_params_per_chunk(self, t: "DeviceTensor", K: int) -> int:
        """Parameters per workspace chunk of a nested_rhat call on this tensor with K superchains (mcr_nested_plan)."""
        return self._params_per_chunk("mcr_nested_plan", t.targs, int(K))

    _EQUAL_CHAINS = {"nested_rhat": "nested R-hat", "autocorr": "autocorrelation"}

    def _tensor_call(self, draws, layout: str, name: str, pooled: bool):
        """(targs, pointer, entry, on_device) of a call mcr_<name> on a host array or, on_device, mcr_<name>_dev on a
        DeviceTensor.  A ragged tensor is, pooled, one chain of its pooled draws; otherwise it is refused."""
        if isinstance(draws, DeviceSims):
            raise ValueError(f"{name} takes one (C, N, P) tensor; a DeviceSims holds S of them (Context.sbc_ranks)")
        if not isinstance(draws, DeviceTensor):
            return tensor_args(draws, layout), draws.ctypes.data_as(C.c_void_p), getattr(self.lib, "mcr_" + name), False
        targs = draws.targs
        if draws.chain_off is not None:
            if not pooled:
                raise ValueError(f"{self._EQUAL_CHAINS[name]} needs chains of equal length; a ragged tensor is not supported")
            M = int(draws.chain_off[-1])
            targs = (targs[0], 1, M, targs[3], M, 1, targs[6])
        return targs, draws.buf.ptr, getattr(self.lib, f"mcr_{name}_dev"), True

    def _params_per_chunk(self, plan_symbol: str, targs, *extra) -> int:
        """What an mcr_*_plan entry answers for a tensor and the call's own arguments."""
        v = C.c_int64(0)
        self._check(getattr(self.lib, plan_symbol)(self.handle, *targs, *extra, C.byref(v)))
        return int(v.value)

    def pareto_khat(self, draws, layout: str = "pcn", r_eff=None, ndraws_tail=None) -> dict:
        """Pareto k-hat of every parameter's tails (mcr_pareto_khat: posterior::pareto_khat(tail = "both")) of a host
        array or a DeviceTensor; the chains are pooled, so a ragged tensor is accepted.  ndraws_tail: a tail length or P of
        them (>= 1); or r_eff: a relative efficiency or P of them, turned into tail lengths by mcr_pareto_tail_length;
        neither: the default of r_eff = 1.  Arrays per parameter: khat = max(khat_left, khat_right), khat_left, khat_right,
        ndraws_tail (the effective length), min_ss; and the float khat_threshold (pareto_companions)."""
        if r_eff is not None and ndraws_tail is not None:
            raise ValueError("give r_eff or ndraws_tail, not both")
        targs, ptr, fn, _ = self._tensor_call(draws, layout, "pareto_khat", True)
        M, P = targs[1] * targs[2], targs[3]
        tails = None
        if r_eff is not None:
            r = np.broadcast_to(np.asarray(r_eff, dtype=np.float64), (P,))
            tails = np.array([max(pareto_tail_length(M, v), 1) for v in r], dtype=np.int64)
        elif ndraws_tail is not None:
            tails = np.ascontiguousarray(np.broadcast_to(np.asarray(ndraws_tail), (P,)), dtype=np.int64)
        arrs = {n: np.full(max(P, 1), np.nan) for n in ("khat", "khat_left", "khat_right")}
        nt = np.zeros(max(P, 1), dtype=np.int64)
        out = Pareto(ndraws_tail=_as_ip(nt), **{n: _as_dp(a) for n, a in arrs.items()})
        self._check(fn(self.handle, ptr, *targs, None if tails is None else _as_ip(tails), C.byref(out)))
        res = {n: a[:P] for n, a in arrs.items()}
        res["ndraws_tail"] = nt[:P]
        res["min_ss"], res["khat_threshold"] = pareto_companions(res["khat"], M)
        return res

    def pareto_params_per_chunk(self, t: "DeviceTensor") -> int:
        """Parameters per workspace chunk of a pareto_khat call on this tensor (mcr_pareto_plan)."""
        return self._params_per_chunk("mcr_pareto_plan", self._tensor_call(t, "pcn", "pareto_khat", True)[0])

    def _psis_call(self, draws, layout: str, negate: bool, r_eff, ndraws_tail, weights: bool) -> dict:
        """Every output of mcr_psis (a host array) or mcr_psis_dev (a DeviceTensor: the weights are written to device
        memory and fetched here); psis and loo each return their part."""
        targs, ptr, fn, dev = self._tensor_call(draws, layout, "psis", True)
        M, P = targs[1] * targs[2], targs[3]
        r = None if r_eff is None else np.ascontiguousarray(np.broadcast_to(np.asarray(r_eff, dtype=np.float64), (P,)))
        tails = None if ndraws_tail is None else np.ascontiguousarray(np.broadcast_to(np.asarray(ndraws_tail), (P,)), dtype=np.int64)
        arrs = {n: np.full(max(P, 1), np.nan) for n in ("khat", "lppd", "elpd", "p_loo")}
        nt = np.zeros(max(P, 1), dtype=np.int64)
        lw = np.full(max(P * M, 1), np.nan) if weights and not dev else None
        with contextlib.ExitStack() as stack:
            buf = stack.enter_context(DeviceBuffer(self, max(P * M * 8, 8))) if weights and dev else None
            wptr = buf.ptr if buf is not None else lw.ctypes.data_as(C.c_void_p) if lw is not None else None
            out = Psis(ndraws_tail=_as_ip(nt), log_weights=wptr, **{n: _as_dp(a) for n, a in arrs.items()})
            self._check(fn(self.handle, ptr, *targs, int(bool(negate)), _as_dp(r), _as_ip(tails), C.byref(out)))
            if buf is not None:
                lw = buf.download(np.float64, max(P * M, 1))
        res = {n: a[:P] for n, a in arrs.items()}
        res["ndraws_tail"] = nt[:P]
        if weights:
            res["log_weights"] = lw[:P * M].reshape(P, M)
        res["min_ss"], res["khat_threshold"] = pareto_companions(res["khat"], M)
        res["n_draws"] = int(M)
        return res

    def psis(self, log_ratios, layout: str = "pcn", r_eff=None, ndraws_tail=None, weights: bool = True) -> dict:
        """Pareto-smoothed importance sampling of every column of log importance ratios (mcr_psis: ArviZ's psislw, loo::psis)
        of a host array or a DeviceTensor; the chains are pooled, so a ragged tensor is accepted.  r_eff: a relative
        efficiency or P of them (default 1); ndraws_tail: a tail length or P of them (>= 1) instead of the default.
        "log_weights" [P][M] in time order (normalised: every row's exp sums to 1; left out with weights=False, when
        k_psis_weights does not run), and per column "khat", "ndraws_tail" (the tail values actually smoothed over),
        "min_ss"; the float "khat_threshold" (pareto_companions)."""
        if r_eff is not None and ndraws_tail is not None:
            raise ValueError("give r_eff or ndraws_tail, not both")
        res = self._psis_call(log_ratios, layout, False, r_eff, ndraws_tail, weights)
        return {k: v for k, v in res.items() if k not in ("lppd", "elpd", "p_loo", "n_draws")}

    def loo(self, log_lik, layout: str = "pcn", r_eff=None, pointwise: bool = True) -> dict:
        """PSIS-LOO of a (chains x draws x observations) tensor of pointwise log-likelihoods, the observations on the
        parameter axis (mcr_psis with negate: ArviZ's loo, loo::loo).  r_eff: as in psis.  The floats "elpd_loo", "se",
        "p_loo", "lppd", the ints "n_obs" and "n_draws", "khat_counts" (loo_totals), "khat_threshold"; with pointwise also
        the arrays "elpd_i", "p_loo_i", "lppd_i", "khat" and "ndraws_tail" per observation."""
        res = self._psis_call(log_lik, layout, True, r_eff, None, False)
        out = loo_totals(res["elpd"], res["p_loo"], res["lppd"], res["khat"])
        out["n_draws"], out["khat_threshold"] = res["n_draws"], res["khat_threshold"]
        if pointwise:
            out.update({"elpd_i": res["elpd"], "p_loo_i": res["p_loo"], "lppd_i": res["lppd"], "khat": res["khat"],
                        "ndraws_tail": res["ndraws_tail"]})
        return out

    def psis_params_per_chunk(self, t: "DeviceTensor", host_weights: bool = False) -> int:
        """Columns per workspace chunk of a psis / loo call on this tensor (mcr_psis_plan); host_weights: of the host
        entry with weights, whose chunk holds them too."""
        return self._params_per_chunk("mcr_psis_plan", self._tensor_call(t, "pcn", "psis", True)[0], int(host_weights))

    def hdi(self, draws, layout: str = "pcn", prob=0.94) -> dict:
        """Highest-density interval(s) of every parameter (mcr_hdi: ArviZ's unimodal hdi, the shortest interval holding
        floor(prob * M) + 1 of the M pooled draws) of a host array or a DeviceTensor; the chains are pooled, so a ragged
        tensor is accepted.  prob: a float, or a sequence of up to MCR_HDI_MAX_PROBS.  "lo", "hi" (float64) and "index"
        (int64, the rank of lo in the ascending order; -1 with NaN endpoints when there is no window) are [P] arrays for
        a float and [P][nprob] for a sequence; "prob" is what was asked for."""
        targs, ptr, fn, _ = self._tensor_call(draws, layout, "hdi", True)
        P = targs[3]
        pr = np.ascontiguousarray(np.atleast_1d(prob), dtype=np.float64)
        if pr.ndim != 1:
            raise ValueError("prob must be a float or a flat sequence of floats")
        n = int(pr.size)
        lo, hi = np.full((max(P, 1), max(n, 1)), np.nan), np.full((max(P, 1), max(n, 1)), np.nan)
        idx = np.full((max(P, 1), max(n, 1)), -1, dtype=np.int64)
        out = Hdi(lo=_as_dp(lo), hi=_as_dp(hi), index=_as_ip(idx))
        self._check(fn(self.handle, ptr, *targs, _as_dp(pr), n, C.byref(out)))
        res = {"lo": lo[:P, :n], "hi": hi[:P, :n], "index": idx[:P, :n]}
        if np.ndim(prob) == 0:
            return {**{k: v[:, 0] for k, v in res.items()}, "prob": float(prob)}
        return {**res, "prob": pr}

    def hdi_params_per_chunk(self, t: "DeviceTensor", nprob: int = 1) -> int:
        """Parameters per workspace chunk of an hdi call with nprob probabilities on this tensor (mcr_hdi_plan)."""
        return self._params_per_chunk("mcr_hdi_plan", self._tensor_call(t, "pcn", "hdi", True)[0], int(nprob))

    def weighted_summary(self, draws, layout: str = "pcn", *, log_weights=None, weights=None, quantiles=(0.05, 0.5, 0.95),
                         return_weights: bool = False) -> dict:
        """Importance-weighted mean, sd, standard error of the mean and quantiles of every parameter (mcr_weighted_summary:
        posterior's weight_draws + summarise_draws, numpy.quantile(weights=, method="inverted_cdf")) of a host array or a
        DeviceTensor under ONE weight per pooled draw, m = c * N + n; the chains are pooled, so a ragged tensor is
        accepted.  Exactly one of log_weights (finite or -inf; Context.psis's rows are such) and weights (finite, >= 0).
        "mean", "sd", "mean_se" [P], "quantiles" [P][nq] (inverted CDF: draws, never interpolated), the floats "ess"
        (Kish's) and "weight_sum", "n_draws"; with return_weights "weights" [M], the linear weights the call formed."""
        targs, ptr, fn, dev = self._tensor_call(draws, layout, "weighted_summary", True)
        M, P = targs[1] * targs[2], targs[3]
        v, flags, q = weight_arguments(M, log_weights, weights, quantiles)
        nq = int(q.size)
        arrs = {n: np.full(max(P, 1), np.nan) for n in ("mean", "sd", "mean_se")}
        qs = np.full((max(P, 1), max(nq, 1)), np.nan)
        ess, s1 = C.c_double(np.nan), C.c_double(np.nan)
        w = np.full(max(M, 1), np.nan) if return_weights else None
        vbuf = wbuf = None
        with contextlib.ExitStack() as stack:
            if dev:
                vbuf = stack.enter_context(DeviceBuffer(self, max(M * 8, 8)))
                if M:
                    vbuf.upload(v)
                wbuf = stack.enter_context(DeviceBuffer(self, max(M * 8, 8))) if return_weights else None
            vptr = vbuf.ptr if dev else v.ctypes.data_as(C.c_void_p)
            wptr = None if w is None else wbuf.ptr if dev else w.ctypes.data_as(C.c_void_p)
            out = Weighted(quantiles=_as_dp(qs), ess=C.pointer(ess), weight_sum=C.pointer(s1), weights=wptr,
                           **{n: _as_dp(a) for n, a in arrs.items()})
            self._check(fn(self.handle, ptr, *targs, vptr, flags, _as_dp(q), nq, C.byref(out)))
            if wbuf is not None:
                w = wbuf.download(np.float64, max(M, 1))
        res = {n: a[:P] for n, a in arrs.items()}
        res.update({"quantiles": qs[:P, :nq], "ess": ess.value, "weight_sum": s1.value, "n_draws": int(M)})
        if return_weights:
            res["weights"] = w[:M]
        return res

    def weighted_params_per_chunk(self, t: "DeviceTensor", nq: int = 3) -> int:
        """Parameters per workspace chunk of a weighted_summary call with nq quantiles on this tensor (mcr_weighted_plan)."""
        return self._params_per_chunk("mcr_weighted_plan", self._tensor_call(t, "pcn", "weighted_summary", True)[0], int(nq))

    def upload_sims(self, draws: np.ndarray, layout: str = "spcn") -> DeviceSims:
        """The draws of S simulations in HBM, for sbc_ranks: a 4-D C-contiguous array whose axes are `layout`."""
        targs = tensor4_args(draws, layout)
        if not draws.flags.c_contiguous:
            raise ValueError("upload_sims() needs a C-contiguous array (permute the layout string instead)")
        with contextlib.ExitStack() as stack:
            buf = stack.enter_context(DeviceBuffer(self, max(draws.nbytes, 8))).upload(draws)
            stack.pop_all()
        return DeviceSims(self, buf, targs)

    def _sbc_call(self, draws, layout: str, thin: int):
        """(thinned targs, pointer, entry) of a rank call on a 4-D host array or on the DeviceSims of S simulations."""
        if isinstance(draws, DeviceTensor):
            raise ValueError("sbc_ranks needs the DeviceSims of S simulations (Context.upload_sims), not one DeviceTensor")
        if isinstance(draws, DeviceSims):
            return thin_args(draws.targs, thin), draws.buf.ptr, self.lib.mcr_sbc_ranks_dev
        return thin_args(tensor4_args(draws, layout), thin), draws.ctypes.data_as(C.c_void_p), self.lib.mcr_sbc_ranks

    def sbc_ranks_rc(self, draws, truth, layout: str = "spcn", thin: int = 1) -> tuple[int, dict]:
        """sbc_ranks with the library's return code beside the result instead of an exception: MCR_ENONFINITE leaves the
        outputs written, a refusal leaves them as they were filled (-1 and NaN)."""
        targs, ptr, fn = self._sbc_call(draws, layout, thin)
        S, P = targs[1], targs[4]
        t = _truth_array(truth, S, P)
        arrs, out = _sbc_arrays(S, P)
        rc = fn(self.handle, ptr, *targs, _as_dp(t), C.byref(out))
        return rc, {**{k: a[:S, :P] for k, a in arrs.items()}, "n_draws": int(targs[2] * targs[3])}

    def sbc_ranks(self, draws, truth, layout: str = "spcn", thin: int = 1) -> dict:
        """Where every true value stands among its posterior draws, for S simulations at once (mcr_sbc_ranks: simulation-based
        calibration).  draws: a 4-D host array whose axes are `layout`, a permutation of "scnp" (strided views included), or a
        DeviceSims from upload_sims; truth [S][P].  thin = k takes the draws n = 0, k, 2k, ... of every chain.  [S][P]
        arrays: "n_less" and "n_equal" (int64: the draws below the truth, and equal to it), "mean", "sd" (population) of the
        L = C * ceil(N / k) pooled draws; and the int "n_draws" = L."""
        rc, res = self.sbc_ranks_rc(draws, truth, layout, thin)
        self._check(rc)
        return res

    def sbc_sims_per_chunk(self, draws, layout: str = "spcn", thin: int = 1) -> int:
        """Simulations per workspace chunk of an sbc_ranks call on these draws (mcr_sbc_plan); all S where the call reads
        the tensor in place."""
        return self._params_per_chunk("mcr_sbc_plan", self._sbc_call(draws, layout, thin)[0])

    def autocorr(self, draws, layout: str = "cnp", max_lag=None, unbiased: bool = False, window_c: float = 5.0) -> dict:
        """Autocorrelation functions and integrated autocorrelation times of the raw draws (mcr_autocorr: ArviZ's autocorr,
        emcee's integrated_time) of a host array (strided views included) or a DeviceTensor with equal-length chains.
        max_lag: the default is min(100, N - 1); at most MCR_ACF_MAX_LAG.  unbiased: divide lag l by N - l instead of N.
        Arrays: "acf" [P][C][L+1], "var" (gamma_0), "tau", "window" (int64, -1: the ACF has not decayed within max_lag and tau
        is a lower bound) and "ess_chain" = N / tau, all [P][C]; the within-chain pooled "acf_pooled" [P][L+1],
        "tau_pooled", "window_pooled", "ess_pooled" = C N / tau_pooled, all [P]; and the int "max_lag"."""
        targs, ptr, fn, _ = self._tensor_call(draws, layout, "autocorr", False)
        nc, N, P = targs[1], targs[2], targs[3]
        L = min(100, max(N - 1, 0)) if max_lag is None else int(max_lag)
        arrs, out = _acf_arrays(P, nc, L if 0 <= L <= MCR_ACF_MAX_LAG else 0)  # (a bad max_lag is refused before anything is written)
        self._check(fn(self.handle, ptr, *targs, L, MCR_ACF_UNBIASED if unbiased else 0, float(window_c), C.byref(out)))
        return _acf_result(arrs, P, nc, N, L)

    def autocorr_params_per_chunk(self, t: "DeviceTensor", max_lag: int) -> int:
        """Parameters per workspace chunk of an autocorr call with this max_lag on this tensor (mcr_autocorr_plan)."""
        return self._params_per_chunk("mcr_autocorr_plan", self._tensor_call(t, "pcn", "autocorr", False)[0], int(max_lag))

    def covariance(self, draws) -> np.ndarray:
        """Population covariance (ddof=0) of draws [P][M] -> [P][P] (fp64 MFMA)."""
        x = np.ascontiguousarray(draws, dtype=np.float64)
        if x.ndim != 2:
            raise ValueError("draws must be 2-D [P][M]")
        P = x.shape[0]
        cov = np.full((max(P, 1), max(P, 1)), np.nan)
        self._check(self.lib.mcr_covariance(self.handle, _as_dp(x), x.shape[1], P, _as_dp(cov)))
        return cov[:P, :P] if P else np.empty((0, 0))

    # -- measurement -----------------------------------------------------------------------------
    def params_per_chunk(self, t: "DeviceTensor", diagnostics: bool = True) -> int:
        """Parameters per workspace chunk of a call on this tensor (mcr_plan_chunks): chunk k is [k * n, (k + 1) * n)."""
        _, C_, N, P, sc, sn, sp = t.targs
        v = C.c_int64(0)
        if t.chain_off is not None:
            self._check(self.lib.mcr_plan_chunks_chains(self.handle, _as_ip(t.chain_off), C_, P, int(diagnostics), C.byref(v)))
            return int(v.value)
        self._check(self.lib.mcr_plan_chunks(self.handle, C_, N, P, sc, sn, sp, int(diagnostics), C.byref(v)))
        return int(v.value)

    def rho_guard_count(self) -> int:
        """Band lags of the tier-3 ESS scan re-derived with the reference's own sums so far (mcr_rho_guard_count)."""
        v = C.c_int64(0)
        self._check(self.lib.mcr_rho_guard_count(self.handle, C.byref(v)))
        return int(v.value)

    def tile_fallback_count(self) -> int:
        """Tiles the f64 tile sort sorted as (key, position) pairs after its record sort failed its order check, so far."""
        v = C.c_int64(0)
        self._check(self.lib.mcr_tile_fallback_count(self.handle, C.byref(v)))
        return int(v.value)

    def profile(self, on: bool):
        self._check(self.lib.mcr_profile_enable(self.handle, 1 if on else 0))

    def profile_reset(self):
        self._check(self.lib.mcr_profile_reset(self.handle))

    def profile_get(self) -> dict:
        arr = (KernelTime * 64)()
        n = C.c_int(0)
        self._check(self.lib.mcr_profile_get(self.handle, arr, 64, C.byref(n)))
        return {arr[i].name.decode(): {"launches": int(arr[i].launches), "total_ms": float(arr[i].total_ms)}
                for i in range(min(n.value, 64))}


def pipeline(ctx: Context, jobs, owns: bool = False):
    """Rolling window of ctx.enqueue / ctx.wait_one over `jobs`, an iterable of (tag, DeviceTensor, enqueue() keyword
    arguments) consumed lazily; a tensor with chain_off (Context.ragged_tensor) is a ragged call, and both kinds share
    the window.  Yields (tag, result dict or the McrError of that job's enqueue or wait) in submission
    order with at most MCR_MAX_INFLIGHT calls outstanding; calls already in flight on `ctx` are waited for first, so
    that every wait_one delivers one of these jobs.  owns=True: the helper frees each tensor once its call is retired.

    However the generator ends -- exhausted, closed early, an exception in `jobs` -- nothing stays in flight and no
    owned tensor stays allocated; use it under contextlib.closing so that an exception in the consumer's loop closes
    it at once.  The consumer does not use `ctx` between two results."""
    if ctx.inflight:
        ctx.wait()
    window = collections.deque()            # (tag, tensor, result buffers or the McrError of its enqueue)
    try:
        for tag, t, kw in jobs:
            try:
                window.append((tag, t, ctx.enqueue(t, **kw)))
            except McrError as exc:
                window.append((tag, t, exc))
            if len(window) == MCR_MAX_INFLIGHT:
                yield _retire(ctx, window, owns)
        while window:
            yield _retire(ctx, window, owns)
    finally:
        if window:
            try:
                ctx.wait()
            except McrError:                # the exception that ended the generator is the one to report
                pass
            if owns:
                for _tag, t, _ in window:
                    t.free()
            window.clear()


def _retire(ctx: Context, window, owns: bool):
    """The oldest job of the window: (tag, result dict or McrError); its tensor is freed if owned."""
    tag, t, got = window[0]
    if not isinstance(got, McrError):
        try:
            if ctx.wait_one() is not got:    # never hand a job another call's numbers
                raise RuntimeError("pipeline: the context delivered a result that is not this job's")
            got = got.result()
        except McrError as exc:
            got = exc
    window.popleft()
    if owns:
        t.free()
    return tag, got


def split_result(r: dict, sizes) -> list[dict]:
    """A batched call's result cut back into its models: `sizes` = parameters per model, in tensor order."""
    out, p0 = [], 0
    for P in sizes:
        out.append({k: (v if k == "q_lo" else v[p0:p0 + P]) for k, v in r.items()})
        p0 += P
    return out


def entries(r: dict, quantiles=None, diagnostics: bool = True) -> list[dict[str, float]]:
    """The per-parameter dicts of the reference API from a summary dict, in parameter order: {"mean", "std", "qNN"...}
    for `quantiles` (the keys f"q{int(q * 100)}"), then {"rhat", "ess_bulk", "ess_tail"} with diagnostics.
    quantiles=None: the diagnostics triple alone."""
    keys, cols = [], []                     # whole columns to Python floats, not one value at a time
    if quantiles is not None:
        keys = ["mean", "std"] + [f"q{int(q * 100)}" for q in quantiles]
        cols = [r["mean"].tolist(), r["std"].tolist()] + r["q"].T.tolist()      # q: [P][n_q]
    if diagnostics:
        keys += DIAG_KEYS
        cols += [r["rhat"].tolist(), r["ess_bulk"].tolist(), r["ess_tail"].tolist()]
    return [dict(zip(keys, row)) for row in zip(*cols)]


def ragged_diagnostics(ctx: Context, x: np.ndarray, counts, min_chains: int) -> dict[str, np.ndarray]:
    """rhat / ess_bulk / ess_tail of every row of x [P][M] whose chains are `counts` draws long (chains of unequal
    length): one upload and one batched mcr_summarize_chains_dev call."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    if x.shape[0] == 0:
        return {k: np.empty(0) for k in DIAG_KEYS}
    r = ctx.summarize_chains(x, counts, min_chains=min_chains, quantiles=())
    return {k: np.asarray(r[k], dtype=np.float64) for k in DIAG_KEYS}


@contextlib.contextmanager
def value_errors():
    """McrError -> ValueError with the library's message: the exception the reference-compatible functions raise."""
    try:
        yield
    except McrError as exc:
        raise ValueError(exc.message) from exc


_default = threading.local()


def default_context() -> Context:
    """The calling THREAD's Context on MCMC_REF_HIP_DEVICE / LOCAL_RANK / device 0 (created on first use).

    A Context is one GPU + its streams and is not thread-safe, so the module-level convenience functions
    (`reference.stats`, `compare.compute_basic_stats`, ...) never share one between threads: each thread gets its own."""
    ctx = getattr(_default, "ctx", None)
    if ctx is None or ctx.handle is None:
        ctx = _default.ctx = Context()
    return ctx

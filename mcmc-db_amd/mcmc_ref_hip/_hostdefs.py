"""What needs the library but no GPU: the host definitions of the statistics (`mcr_*_host` and the other entries that
take no context), their pure-numpy companions, the argument and result-struct builders the device calls share with them,
and the images of host memory the library hands out (`Image`).  Imports `_abi` only.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from ._abi import (CSV_HEADERS, ENERGY_KEYS, MCR_ACF_MAX_LAG, MCR_ACF_UNBIASED, MCR_CSVW_FIELD_MAX, MCR_ENERGY_LAUNCH_WORK,
                   MCR_ENERGY_TILE_I, MCR_ENERGY_TILE_J, MCR_ENONFINITE, MCR_OK, MCR_PQW_F64, MCR_PQW_I64, MCR_PQW_SEQ,
                   MCR_W_LOG, MCR_WEIGHTED_MAX_Q, NESTED_FIELDS, Acf, Hdi, McrError, Nested, Pareto, PqColumn, Psis, Sbc,
                   Weighted, _as_dp, _as_ip, load_library)


def _nan_arrays(names, *shape: int) -> dict:
    """One NaN-filled float64 array per name, every extent at least 1: the outputs of a per-parameter result."""
    return {k: np.full(tuple(max(n, 1) for n in shape), np.nan) for k in names}


def _struct_of(cls, arrs: dict, **others):
    """The result struct whose members point at `arrs` (by name; int64 and float64), plus `others` as given."""
    return cls(**{k: (_as_ip if a.dtype == np.int64 else _as_dp)(a) for k, a in arrs.items()}, **others)


def _sample_pair(ref, actual, finite: bool = True) -> tuple[np.ndarray, np.ndarray]:
    """ref [P][Mr] and actual [P][Ma] of a two-sample call as contiguous float64; ValueError unless both are 2-D with
    the same P and, with `finite`, hold finite values only."""
    r = np.ascontiguousarray(ref, dtype=np.float64)
    a = np.ascontiguousarray(actual, dtype=np.float64)
    if r.ndim != 2 or a.ndim != 2 or r.shape[0] != a.shape[0]:
        raise ValueError("ref and actual must be 2-D with the same number of parameters")
    if finite and not (np.isfinite(r).all() and np.isfinite(a).all()):
        raise ValueError("draws contain non-finite values")
    return r, a


def energy_launches(Mr: int, Ma: int, P: int, launch_work: int = MCR_ENERGY_LAUNCH_WORK) -> int:
    """k_energy_pairs launches of an energy_distance call of this shape (the rule stated in mcmcref_hip.h)."""
    nr, na = -(-Mr // MCR_ENERGY_TILE_I), -(-Ma // MCR_ENERGY_TILE_J)
    jobs = nr * na + nr * (nr + 1) // 2 + na * (na + 1) // 2
    return -(-jobs // max(1, launch_work // (MCR_ENERGY_TILE_I * MCR_ENERGY_TILE_J * P)))


def energy_distance_host(ref, actual, scale=None) -> dict:
    """mcr_energy_distance_host: the definition of Context.energy_distance on the host, without a GPU (the same per-pair
    arithmetic bit for bit, the pair sums in long double)."""
    r, a = _sample_pair(ref, actual, finite=False)
    s = None if scale is None else np.ascontiguousarray(scale, dtype=np.float64)
    if s is not None and s.shape != (r.shape[0],):
        raise ValueError("scale must have one entry per parameter")
    out = np.full(6, np.nan)
    rc = load_library().mcr_energy_distance_host(_as_dp(r), r.shape[1], _as_dp(a), a.shape[1], r.shape[0], _as_dp(s), _as_dp(out))
    if rc != MCR_OK:
        raise McrError(rc, "mcr_energy_distance_host")
    return dict(zip(ENERGY_KEYS, (float(v) for v in out)))


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


def _nested_arrays(P: int):
    """The output arrays of a nested R-hat call (NaN until written) and the struct that points at them."""
    arrs = _nan_arrays(NESTED_FIELDS, P)
    return arrs, _struct_of(Nested, arrs)


def _tail_length(symbol: str, M: int, r_eff: float) -> int:
    t = int(getattr(load_library(), symbol)(int(M), float(r_eff)))
    if t < 0:
        raise ValueError(f"r_eff must be finite and > 0; got {r_eff}")
    return t


def pareto_tail_length(M: int, r_eff: float = 1.0) -> int:
    """The default tail length of Pareto k-hat for M draws (mcr_pareto_tail_length: ceil(3 sqrt(M / r_eff)) for M > 225,
    else M // 5; no device).  ValueError unless r_eff is finite and > 0."""
    return _tail_length("mcr_pareto_tail_length", M, r_eff)


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


def _pareto_arrays(P: int):
    """The output arrays of a Pareto k-hat call (NaN / 0 until written) and the struct that points at them."""
    arrs = {**_nan_arrays(("khat", "khat_left", "khat_right"), P), "ndraws_tail": np.zeros(max(P, 1), dtype=np.int64)}
    return arrs, _struct_of(Pareto, arrs)


def _psis_arrays(P: int, log_weights):
    """The per-column output arrays of a PSIS call (NaN / 0 until written) and the struct that points at them and at
    `log_weights`, host or device memory of [P][M] float64 or None."""
    arrs = {**_nan_arrays(("khat", "lppd", "elpd", "p_loo"), P), "ndraws_tail": np.zeros(max(P, 1), dtype=np.int64)}
    return arrs, _struct_of(Psis, arrs, log_weights=log_weights)


def psis_tail_length(M: int, r_eff: float = 1.0) -> int:
    """The default tail length of PSIS for M values (mcr_psis_tail_length: ceil(min(M / 5, 3 sqrt(M / r_eff))), loo's and
    ArviZ's rule for every M; no device).  ValueError unless r_eff is finite and > 0."""
    return _tail_length("mcr_psis_tail_length", M, r_eff)


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
    lo, hi, idx = (a[0] for a in _hdi_arrays(1, int(pr.size))[0].values())        # one row: one parameter
    rc = load_library().mcr_hdi_sorted_host(_as_dp(x), x.size, _as_dp(pr), int(pr.size), _as_dp(lo), _as_dp(hi), _as_ip(idx))
    if rc != MCR_OK:
        raise ValueError(f"mcr_hdi_sorted_host: bad argument (prob = {prob})")
    if np.ndim(prob) == 0:
        return float(lo[0]), float(hi[0]), int(idx[0])
    return lo, hi, idx


def _hdi_arrays(P: int, nprob: int):
    """The output arrays [P][nprob] of an HDI call (NaN / -1 until written) and the struct that points at them."""
    arrs = {**_nan_arrays(("lo", "hi"), P, nprob), "index": np.full((max(P, 1), max(nprob, 1)), -1, dtype=np.int64)}
    return arrs, _struct_of(Hdi, arrs)


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


def _weighted_arrays(P: int, nq: int, weights):
    """The output arrays of a weighted call in mcr_weighted_out's order (NaN until written: "mean", "sd", "mean_se" [P],
    "quantiles" [P][nq], "ess" and "weight_sum" [1]) and the struct that points at them and at `weights`, host or device
    memory of [M] float64 or None."""
    arrs = {**_nan_arrays(("mean", "sd", "mean_se"), P), **_nan_arrays(("quantiles",), P, nq),
            **_nan_arrays(("ess", "weight_sum"), 1)}
    return arrs, _struct_of(Weighted, arrs, weights=weights)


def weighted_host(x, *, log_weights=None, weights=None, quantiles=(0.05, 0.5, 0.95), return_weights: bool = False) -> dict:
    """The weighted summary of ONE parameter's draws in time order by the library's host routine (mcr_weighted_host: the
    device's association, std::sort; no device): the floats mean, sd, mean_se, ess, weight_sum and the array quantiles;
    with return_weights the weights as formed.  Linear weights give the device's bits; log weights go through libm's exp.
    ValueError for a bad argument, a refused weight vector or a non-finite draw."""
    d = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
    v, flags, q = weight_arguments(d.size, log_weights, weights, quantiles)
    arrs, _ = _weighted_arrays(1, int(q.size), None)         # the entry takes the struct's members one by one, in order
    w = np.full(max(d.size, 1), np.nan) if return_weights else None
    rc = load_library().mcr_weighted_host(_as_dp(d), _as_dp(v), d.size, flags, _as_dp(q), int(q.size),
                                          *(_as_dp(a) for a in arrs.values()), _as_dp(w))
    if rc != MCR_OK:
        raise ValueError(f"mcr_weighted_host: {'non-finite draw' if rc == MCR_ENONFINITE else 'bad argument or weight vector'}")
    res = {k: float(arrs[k][0]) for k in ("mean", "sd", "mean_se", "ess", "weight_sum")}
    res["quantiles"] = arrs["quantiles"][0, :q.size]
    if return_weights:
        res["weights"] = w[:d.size]
    return res


def _sbc_arrays(S: int, P: int):
    """The output arrays of a rank call (-1 / NaN until written) and the struct that points at them."""
    shape = (max(S, 1), max(P, 1))
    arrs = {"n_less": np.full(shape, -1, dtype=np.int64), "n_equal": np.full(shape, -1, dtype=np.int64),
            **_nan_arrays(("mean", "sd"), S, P)}
    return arrs, _struct_of(Sbc, arrs)


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
    per = _nan_arrays(("chi2", "pvalue", "ecdf_dev"), P)
    rc = load_library().mcr_sbc_uniformity(_as_ip(r), S, P, int(n_draws), B, _as_ip(counts), _as_dp(expected),
                                           *(_as_dp(a) for a in per.values()))
    if rc != MCR_OK:
        raise ValueError("mcr_sbc_uniformity: needs S >= 1, 2 <= bins <= n_draws + 1 and every rank in 0 .. n_draws")
    return {"counts": counts[:P, :B], "expected": expected[:B], **{k: a[:P] for k, a in per.items()}}


def _acf_arrays(P: int, nc: int, L: int):
    """The output arrays of an autocorrelation call (NaN / -1 until written) and the struct that points at them."""
    p1, c1 = max(P, 1), max(nc, 1)
    arrs = {"acf": np.full((p1, c1, L + 1), np.nan), "var": np.full((p1, c1), np.nan), "tau": np.full((p1, c1), np.nan),
            "window": np.full((p1, c1), -1, dtype=np.int64), "acf_pooled": np.full((p1, L + 1), np.nan),
            "tau_pooled": np.full(p1, np.nan), "window_pooled": np.full(p1, -1, dtype=np.int64)}
    return arrs, _struct_of(Acf, arrs)


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

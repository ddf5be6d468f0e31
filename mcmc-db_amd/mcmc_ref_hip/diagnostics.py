"""Rank-normalised split R-hat and ESS on the GPU, behind the reference's function signatures.

Mirrors src/mcmc_ref/diagnostics.py:13-73 (`split_rhat`, `ess_bulk`, `ess_tail`): same arguments,
same guards, same ValueError texts, NaN for fewer than two chains.  The arithmetic (pooled sort,
tie-averaged ranks, AS241 inverse normal, fold, split-chain variances, first-negative-rho
autocovariance sum) runs in libmcmcref_hip; chains may be ragged.

`nested_rhat` is not the reference's: the diagnostic for many short chains (Margossian et al., "Nested R-hat: assessing
the convergence of Markov chain Monte Carlo when running many short chains"; posterior::rhat_nested), for any number
of equal-length chains.  `pareto_khat` is not the reference's either: the tail diagnostic for the draws behind a mean
and a std (Vehtari et al., "Pareto smoothed importance sampling"; posterior::pareto_khat), on the pooled chains.  Nor is
`hdi`: the highest-density interval of the pooled chains (ArviZ's unimodal `hdi`).  Nor `autocorr`: the autocorrelation
function of every chain's raw draws and the integrated autocorrelation time with Sokal's window (ArviZ's `autocorr`,
emcee's `integrated_time`) -- what one looks at when ESS is low.
"""
from __future__ import annotations

from collections.abc import Sequence

import numpy as np

from . import _ffi


def _validate_min_chains(min_chains: int) -> None:
    if min_chains < 1:
        raise ValueError(f"min_chains must be >= 1; got {min_chains}")


def _guard(chains, min_chains: int, what: str) -> bool:
    """Reference guards (diagnostics.py:24-30); returns True when the answer is NaN."""
    _validate_min_chains(min_chains)
    if len(chains) < min_chains:
        raise ValueError(f"{what} diagnostics require at least {min_chains} chains; got {len(chains)} chain(s)")
    return len(chains) < 2


def diagnose(chains: Sequence[Sequence[float]], *, min_chains: int = 4, context=None) -> dict:
    """All three diagnostics (+ integer truncation lags) from ONE pass of the kernels."""
    if _guard(chains, min_chains, "R-hat"):
        nan = float("nan")
        return {"rhat": nan, "ess_bulk": nan, "ess_tail": nan}
    ctx = context or _ffi.default_context()
    with _ffi.value_errors():
        return ctx.diagnose_chains(chains, min_chains=min_chains)


def split_rhat(chains: Sequence[Sequence[float]], *, min_chains: int = 4) -> float:
    """Rank-normalized split R-hat with folded variant (returns max of both)."""
    if _guard(chains, min_chains, "R-hat"):
        return float("nan")
    return diagnose(chains, min_chains=min_chains)["rhat"]


def ess_bulk(chains: Sequence[Sequence[float]], *, min_chains: int = 4) -> float:
    if _guard(chains, min_chains, "ESS"):
        return float("nan")
    return diagnose(chains, min_chains=min_chains)["ess_bulk"]


def ess_tail(chains: Sequence[Sequence[float]], *, min_chains: int = 4) -> float:
    if _guard(chains, min_chains, "ESS"):
        return float("nan")
    return diagnose(chains, min_chains=min_chains)["ess_tail"]


def _nested_args(chains, superchain_ids):
    """(draws [1][C][N] f64, int32 labels) of one parameter's chains; the ValueErrors of nested_rhat."""
    lengths = {len(c) for c in chains}
    if len(lengths) > 1:
        raise ValueError(f"nested R-hat requires chains of equal length; got lengths {sorted(lengths)}")
    if not isinstance(superchain_ids, (int, np.integer)) and len(superchain_ids) != len(chains):
        raise ValueError(f"superchain_ids must have one label per chain: got {len(superchain_ids)} for {len(chains)} chains")
    ids = _ffi.superchain_labels(superchain_ids, len(chains))
    n = lengths.pop() if lengths else 0
    x = np.ascontiguousarray(chains, dtype=np.float64).reshape(1, len(chains), n)
    return x, ids


def nested_rhat_detail(chains: Sequence[Sequence[float]], superchain_ids, *, context=None) -> dict:
    """Nested R-hat of ONE parameter given as equal-length chains, chain c in superchain superchain_ids[c] (or an int K:
    K contiguous blocks of chains): floats nrhat = max(nrhat_bulk, nrhat_tail), nrhat_raw, and the between / within
    variances B and W of each kind (Context.nested_rhat)."""
    x, ids = _nested_args(chains, superchain_ids)
    ctx = context or _ffi.default_context()
    with _ffi.value_errors():
        res = ctx.nested_rhat(x, ids, "pcn")
    return {k: float(v[0]) for k, v in res.items()}


def nested_rhat(chains: Sequence[Sequence[float]], superchain_ids, *, context=None) -> float:
    """Rank-normalized nested R-hat with folded variant (the max of both); NaN for fewer than two superchains.  Chains are
    not split and may be any number; values near 1 (the paper suggests 1.01) say the superchains forgot their starts."""
    x, ids = _nested_args(chains, superchain_ids)
    if np.unique(ids).size < 2:
        return float("nan")
    ctx = context or _ffi.default_context()
    with _ffi.value_errors():
        return float(ctx.nested_rhat(x, ids, "pcn")["nrhat"][0])


def pareto_khat_detail(chains: Sequence[Sequence[float]], *, r_eff=None, ndraws_tail=None, context=None) -> dict:
    """Pareto k-hat of ONE parameter given as chains of any lengths (they are pooled): khat = max(khat_left, khat_right),
    khat_left, khat_right, ndraws_tail (the effective tail length), min_ss and khat_threshold (Context.pareto_khat).  The
    tail length comes from `ndraws_tail`, or from the relative efficiency `r_eff`, or is the default of r_eff = 1."""
    if r_eff is not None and ndraws_tail is not None:
        raise ValueError("give r_eff or ndraws_tail, not both")
    x = np.concatenate([np.asarray(c, dtype=np.float64).reshape(-1) for c in chains]) if len(chains) else np.zeros(0)
    ctx = context or _ffi.default_context()
    with _ffi.value_errors():
        res = ctx.pareto_khat(x.reshape(1, 1, -1), "pcn", r_eff=r_eff, ndraws_tail=ndraws_tail)
    out = {k: float(res[k][0]) for k in ("khat", "khat_left", "khat_right", "min_ss")}
    out["ndraws_tail"] = int(res["ndraws_tail"][0])
    out["khat_threshold"] = res["khat_threshold"]
    return out


def pareto_khat(chains: Sequence[Sequence[float]], *, r_eff=None, ndraws_tail=None, context=None) -> float:
    """Pareto k-hat of the pooled chains' tails, the larger of the two: below 0.5 the variance is finite and the central
    limit theorem holds, from 0.5 the mean converges slowly and a std is not trustworthy, from 0.7 the estimates are
    unreliable, from 1 no mean exists.  NaN for fewer than 10 draws or constant tails."""
    return pareto_khat_detail(chains, r_eff=r_eff, ndraws_tail=ndraws_tail, context=context)["khat"]


def psis_log_weights(chains: Sequence[Sequence[float]], *, r_eff=None, ndraws_tail=None, context=None) -> dict:
    """Pareto-smoothed importance sampling of ONE column of log importance ratios given as chains of any lengths (they
    are pooled, chain after chain): "log_weights" (normalised, in the order of the pooled draws), "khat", "ndraws_tail"
    (the tail values smoothed over), "min_ss" and "khat_threshold" (Context.psis).  The tail length comes from
    `ndraws_tail`, or from the relative efficiency `r_eff`, or is the default of r_eff = 1."""
    if r_eff is not None and ndraws_tail is not None:
        raise ValueError("give r_eff or ndraws_tail, not both")
    x = np.concatenate([np.asarray(c, dtype=np.float64).reshape(-1) for c in chains]) if len(chains) else np.zeros(0)
    ctx = context or _ffi.default_context()
    with _ffi.value_errors():
        res = ctx.psis(x.reshape(1, 1, -1), "pcn", r_eff=r_eff, ndraws_tail=ndraws_tail)
    return {"log_weights": res["log_weights"][0], "khat": float(res["khat"][0]), "ndraws_tail": int(res["ndraws_tail"][0]),
            "min_ss": float(res["min_ss"][0]), "khat_threshold": res["khat_threshold"]}


def hdi(chains: Sequence[Sequence[float]], prob: float = 0.94, *, context=None) -> tuple[float, float]:
    """The highest-density interval of ONE parameter given as chains of any lengths (they are pooled): the shortest
    interval that holds floor(prob * M) + 1 of the M draws, the first of several equally short ones (Context.hdi; ArviZ's
    unimodal hdi).  (NaN, NaN) without draws."""
    x = np.concatenate([np.asarray(c, dtype=np.float64).reshape(-1) for c in chains]) if len(chains) else np.zeros(0)
    ctx = context or _ffi.default_context()
    with _ffi.value_errors():
        res = ctx.hdi(x.reshape(1, 1, -1), "pcn", prob=float(prob))
    return float(res["lo"][0]), float(res["hi"][0])


def weighted_summary(chains: Sequence[Sequence[float]], *, log_weights=None, weights=None, quantiles=(0.05, 0.5, 0.95),
                     context=None) -> dict:
    """The importance-weighted summary of ONE parameter given as chains of any lengths (they are pooled, chain after
    chain; the weight vector follows the pooled order): the floats "mean", "sd", "mean_se", "ess" (Kish's), "weight_sum",
    the int "n_draws" and the array "quantiles" -- inverted-CDF quantiles, numpy.quantile(weights=, method="inverted_cdf")
    (Context.weighted_summary).  Exactly one of log_weights and weights."""
    x = np.concatenate([np.asarray(c, dtype=np.float64).reshape(-1) for c in chains]) if len(chains) else np.zeros(0)
    ctx = context or _ffi.default_context()
    with _ffi.value_errors():
        res = ctx.weighted_summary(x.reshape(1, 1, -1), "pcn", log_weights=log_weights, weights=weights, quantiles=quantiles)
    out = {k: float(res[k][0]) for k in ("mean", "sd", "mean_se")}
    out.update(ess=res["ess"], weight_sum=res["weight_sum"], n_draws=res["n_draws"], quantiles=res["quantiles"][0])
    return out


def autocorr(chains: Sequence[Sequence[float]], max_lag: int | None = None, *, unbiased: bool = False, window_c: float = 5.0,
             context=None) -> dict:
    """Autocorrelation functions and times of ONE parameter given as equal-length chains (Context.autocorr): arrays "acf"
    [C][L+1], "var", "tau", "window", "ess_chain" = N / tau per chain; the within-chain pooled "acf_pooled" [L+1] and the
    scalars "tau_pooled", "window_pooled", "ess_pooled" = C N / tau_pooled, "max_lag" (default min(100, N - 1)).  A window
    of -1 says the autocorrelation has not decayed within max_lag: tau is then a lower bound.  ValueError for chains of
    unequal length, a bad max_lag or window_c, and non-finite draws."""
    lengths = {len(c) for c in chains}
    if len(lengths) > 1:
        raise ValueError(f"autocorrelation requires chains of equal length; got lengths {sorted(lengths)}")
    n = lengths.pop() if lengths else 0
    x = np.ascontiguousarray(chains, dtype=np.float64).reshape(1, len(chains), n)
    ctx = context or _ffi.default_context()
    with _ffi.value_errors():
        res = ctx.autocorr(x, "pcn", max_lag=max_lag, unbiased=unbiased, window_c=window_c)
    out = {k: res[k][0] for k in ("acf", "var", "tau", "window", "ess_chain", "acf_pooled")}
    out.update(tau_pooled=float(res["tau_pooled"][0]), window_pooled=int(res["window_pooled"][0]),
               ess_pooled=float(res["ess_pooled"][0]), max_lag=res["max_lag"])
    return out

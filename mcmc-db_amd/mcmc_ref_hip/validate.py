"""validate(): draw-vs-reference validation in one call (ADDITIVE: not a reference symbol).

The reference gates a sampler's draws with `reference.compare` (relative error of mean / std,
src/mcmc_ref/reference.py:107-122).  `validate` keeps that gate unchanged and adds, per parameter,
distribution-level distances computed on the GPU -- the two-sample Kolmogorov-Smirnov statistic and
the Wasserstein-1 distance (scaled by the reference std) -- plus the reference draws' own
diagnostics, and the Pareto k-hat of both samples' tails (`khat_ref` / `khat_actual`: above 0.5 the std gate is not
trustworthy, above 0.7 the mean gate is not either).  `sliced=K` adds a check of the JOINT distribution: both samples are projected onto K random
directions of the standardised parameter space and each projected pair goes through the same KS / W1 pass, so a
wrong dependence between parameters whose marginals are all right shows up along some direction.  Nothing here exists in the reference: parity for these extras is pinned to scipy only
(tests/test_ext_gpu.py), and they never change `passed` unless thresholds are given explicitly.
"""
from __future__ import annotations

from collections.abc import Mapping, Sequence
from dataclasses import dataclass, field

import numpy as np

from . import _ffi
from .backends import columns_to_matrix
from .compare import CompareResult, compare_stats, compute_stats_from_draws
from .store import DataStore


@dataclass(frozen=True)
class ValidateResult:
    passed: bool
    compare: CompareResult                       # the reference's gate, unchanged
    ks: dict[str, float]                         # two-sample KS statistic per parameter
    wasserstein: dict[str, float]                # W1 per parameter
    wasserstein_scaled: dict[str, float]         # W1 / reference std
    failures: list[str] = field(default_factory=list)
    sliced_ks: float | None = None               # largest KS over the sliced directions (sliced > 0)
    sliced_w1: float | None = None               # largest W1 over them, in units of reference std
    sliced: dict | None = None                   # per-direction "ks" / "w1", "worst" (index of the largest KS) and
    #                                              "worst_direction" {param: weight in standardised space}
    khat_ref: dict[str, float] = field(default_factory=dict)       # Pareto k-hat (the larger tail) of the reference draws
    khat_actual: dict[str, float] = field(default_factory=dict)    # ... and of `actual`
    hdi_ref: dict[str, tuple[float, float]] = field(default_factory=dict)      # (lo, hi) of the reference draws' highest-density
    hdi_actual: dict[str, tuple[float, float]] = field(default_factory=dict)   # interval and of `actual`'s: only with hdi_prob / hdi_tol
    energy: float | None = None                  # energy distance E of the standardised joint draws (energy=True)
    energy_detail: dict | None = None            # "a", "b", "c", "e", "h", "t" of Context.energy_distance, "mr", "ma" (draws used)
    # Not fields -- the field list of this class is closed --: what a result without the Gaussian check answers where a
    # GaussianValidateResult has its two fields.
    gaussian = None
    gaussian_shift = None


@dataclass(frozen=True)
class GaussianValidateResult(ValidateResult):
    """What validate(gaussian=True) returns when it made the check: a ValidateResult with two more fields."""
    gaussian: dict | None = None                 # gaussian.gaussian_check of the standardised joint draws, "shift" as
    #                                              {param: conditional shift}, "singular_ref" / "singular_actual" (a name or None)
    gaussian_shift: float | None = None          # its Mahalanobis distance: the mean shift in joint reference standard deviations


def energy_stride(m: int, max_draws: int | None) -> int:
    """The even stride that thins m draws to at most max_draws: x[:, ::ceil(m / max_draws)] (1 without a limit)."""
    if max_draws is None:
        return 1
    if max_draws < 1:
        raise ValueError("energy_max_draws must be >= 1")
    return max(1, -(-int(m) // int(max_draws)))


def sliced_directions(k: int, std, seed: int = 4711) -> tuple[np.ndarray, np.ndarray]:
    """k projection directions for parameters whose reference std is `std` [P]: (W [k][P], live [P] bool).

    The recipe, so that a direction can be reproduced outside the package: `live` marks the parameters whose std is
    finite and > 0, n_live of them;

        G = np.random.default_rng(seed).standard_normal((k, n_live))
        U = G / np.linalg.norm(G, axis=1, keepdims=True)          # unit rows: directions of the standardised space
        W[:, live] = U / std[live]                                 # ... applied to (x - mean) in the draws' own units

    and W is 0 for every other parameter.  W[j] @ (x - mean) is therefore U[j] @ ((x - mean) / std): for draws that
    match the reference and are uncorrelated it has unit variance, and a W1 along it is in units of reference std.
    """
    std = np.asarray(std, dtype=np.float64).reshape(-1)
    live = np.isfinite(std) & (std > 0)
    W = np.zeros((int(k), std.size))
    if k > 0 and live.any():
        G = np.random.default_rng(seed).standard_normal((int(k), int(live.sum())))
        W[:, live] = G / np.linalg.norm(G, axis=1, keepdims=True) / std[live]
    return W, live


def validate(model: str, actual: Mapping[str, Sequence[float]], tolerance: float = 0.15,
             metrics: Sequence[str] = ("mean", "std"), ks_max: float | None = None,
             w1_scaled_max: float | None = None, store: DataStore | None = None, context=None, sliced: int = 0,
             sliced_seed: int = 4711, sliced_ks_max: float | None = None,
             sliced_w1_max: float | None = None, khat_max: float | None = None, hdi_prob: float | None = None,
             hdi_tol: float | None = None, energy: bool = False, energy_max: float | None = None,
             energy_max_draws: int | None = None, gaussian: bool = False, gaussian_jitter: float = 0.0,
             gaussian_shift_max: float | None = None, gaussian_kl_max: float | None = None) -> ValidateResult:
    """gaussian=True: the result is a `GaussianValidateResult` (a plain `ValidateResult` answers None for its two extra
    fields); one `gaussian.gaussian_check` call on the joint draws, every parameter scaled by 1 / reference std (0
    where that std is not finite and > 0, as for `energy`), `gaussian_jitter` added to the diagonal of both scaled covariance
    matrices: do the first two moments of the joint distributions agree?  `gaussian_shift` is the Mahalanobis distance of
    the mean shift in the reference's metric, `gaussian` the call's dict with `shift` keyed by parameter (each live
    parameter's shift given the ones before it, in conditional standard deviations).  A singular covariance is reported by
    the NAME of the first parameter that is constant or exactly dependent on the ones before it, in
    `gaussian["singular_ref"]` / `["singular_actual"]` (else None); what needs that factor is NaN.  `gaussian_shift_max`
    and `gaussian_kl_max` (on `kl_sym`) add the failures `gaussian.shift=... > max` and `gaussian.kl=... > max` -- a NaN
    fails them --; without them `passed` is what it is without `gaussian`.  Needs joint draws.
    energy=True: one `Context.energy_distance` call on the joint draws, every parameter scaled by 1 / reference std
    (0 where that std is not finite and > 0: the `live` rule of `sliced_directions`): the direction-free counterpart of
    `sliced`, without a seed.  `energy` is E, `energy_detail` the six numbers and the draws used.  `energy_max` adds the
    failure `energy=E > energy_max`; without it `passed` is what it is without `energy`.  `energy_max_draws=n` thins each
    sample first to at most n draws by an even stride (`energy_stride`): the cost is quadratic in the draws and
    autocorrelated draws lose little.  Needs joint draws, like `sliced`; with no live parameter the fields stay None.
    hdi_prob / hdi_tol: when either is given (hdi_prob is 0.94 then), `hdi_ref` / `hdi_actual` hold every parameter's
    highest-density interval (Context.hdi) -- where the mass lies, which q5 / q50 / q95 alone do not say; with hdi_tol a
    parameter fails when an endpoint is off by more than hdi_tol times the reference interval's own width.  khat_max: a parameter whose `khat_actual` (Context.pareto_khat, default tail length) exceeds it is a failure;
    without it the two k-hat columns are information only.  sliced=K > 0: K directions `sliced_directions(K, reference std, sliced_seed)` around the reference means, one
    `Context.sliced_two_sample` call; the result's `sliced_ks` / `sliced_w1` are the maxima over the directions and
    `sliced` holds the detail.  `sliced_ks_max` / `sliced_w1_max` turn them into failures; without them `passed` is what
    it is without `sliced`.  Needs joint draws: every parameter of `actual` must have the same length."""
    store = store or DataStore()
    ctx = context or _ffi.default_context()
    params = list(actual.keys())
    table = store.open_draws(model, params=params).read_all()
    ref = columns_to_matrix(table, params)
    from .backends import HipBackend
    ref_stats = HipBackend(ctx).stats(table, params)
    cmp_res = compare_stats(ref_stats, compute_stats_from_draws(actual, ctx), tolerance=tolerance, metrics=metrics,
                            context=ctx)
    lens = {len(actual[p]) for p in params}
    if sliced < 0:
        raise ValueError("sliced must be >= 0")
    if sliced > 0 and len(lens) > 1:
        raise ValueError("sliced needs joint draws: the parameters of `actual` differ in length")
    if energy and len(lens) > 1:
        raise ValueError("energy needs joint draws: the parameters of `actual` differ in length")
    if energy:
        energy_stride(1, energy_max_draws)          # a bad limit is refused before any work
    if gaussian and len(lens) > 1:
        raise ValueError("gaussian needs joint draws: the parameters of `actual` differ in length")
    ks: dict[str, float] = {}
    w1: dict[str, float] = {}
    if len(lens) == 1 and params:
        act = np.stack([np.asarray(actual[p], dtype=np.float64) for p in params])
        k, w = ctx.two_sample(ref, act)
        ks = {p: float(k[i]) for i, p in enumerate(params)}
        w1 = {p: float(w[i]) for i, p in enumerate(params)}
    else:
        for i, p in enumerate(params):
            k, w = ctx.two_sample(ref[i:i + 1], np.asarray(actual[p], dtype=np.float64)[None, :])
            ks[p], w1[p] = float(k[0]), float(w[0])
    scaled = {p: (w1[p] / ref_stats[p]["std"] if ref_stats[p]["std"] > 0 else float("inf") if w1[p] > 0 else 0.0)
              for p in params}
    khat_ref = {p: float(v) for p, v in zip(params, ctx.pareto_khat(ref.reshape(len(params), 1, -1), "pcn")["khat"])} if params else {}
    khat_act: dict[str, float] = {}
    if len(lens) == 1 and params:
        khat_act = {p: float(v) for p, v in zip(params, ctx.pareto_khat(act.reshape(len(params), 1, -1), "pcn")["khat"])}
    else:
        for p in params:
            khat_act[p] = float(ctx.pareto_khat(np.asarray(actual[p], dtype=np.float64).reshape(1, 1, -1), "pcn")["khat"][0])
    hdi_ref: dict[str, tuple[float, float]] = {}
    hdi_act: dict[str, tuple[float, float]] = {}
    if (hdi_prob is not None or hdi_tol is not None) and params:
        prob = 0.94 if hdi_prob is None else float(hdi_prob)
        with _ffi.value_errors():
            groups = [(params, ref), (params, act)] if len(lens) == 1 else \
                [(params, ref)] + [([p], np.asarray(actual[p], dtype=np.float64)[None, :]) for p in params]
            for into, (names, x) in zip([hdi_ref] + [hdi_act] * len(groups), groups):
                r = ctx.hdi(x.reshape(len(names), 1, -1), "pcn", prob=prob)
                into.update({p: (float(r["lo"][i]), float(r["hi"][i])) for i, p in enumerate(names)})
    failures = list(cmp_res.failures)
    if khat_max is not None:
        failures += [f"{p}.khat_actual={khat_act[p]:.3g} > {khat_max}" for p in params if not khat_act[p] <= khat_max]
    if hdi_tol is not None:
        for p in params:
            (lr, hr), (la, ha) = hdi_ref[p], hdi_act[p]
            off = max(abs(la - lr), abs(ha - hr))
            if not off <= hdi_tol * (hr - lr):
                failures.append(f"{p}.hdi_offset={off:.3g} > {hdi_tol} * {hr - lr:.3g}")
    if ks_max is not None:
        failures += [f"{p}.ks={ks[p]:.3g} > {ks_max}" for p in params if not ks[p] <= ks_max]
    if w1_scaled_max is not None:
        failures += [f"{p}.w1_scaled={scaled[p]:.3g} > {w1_scaled_max}" for p in params if not scaled[p] <= w1_scaled_max]
    extra = {}
    if sliced > 0 and params:
        W, live = sliced_directions(sliced, [ref_stats[p]["std"] for p in params], sliced_seed)
        if live.any():
            center = np.array([ref_stats[p]["mean"] for p in params], dtype=np.float64)
            sk, sw = ctx.sliced_two_sample(ref, act, W, np.where(live, center, 0.0))
            worst = int(np.argmax(sk))
            std = np.array([ref_stats[p]["std"] for p in params], dtype=np.float64)
            extra = {"sliced_ks": float(sk.max()), "sliced_w1": float(sw.max()),
                     "sliced": {"ks": [float(v) for v in sk], "w1": [float(v) for v in sw], "worst": worst,
                                "worst_direction": {p: float(W[worst, i] * std[i]) for i, p in enumerate(params) if live[i]}}}
            if sliced_ks_max is not None and not extra["sliced_ks"] <= sliced_ks_max:
                failures.append(f"sliced.ks={extra['sliced_ks']:.3g} > {sliced_ks_max}")
            if sliced_w1_max is not None and not extra["sliced_w1"] <= sliced_w1_max:
                failures.append(f"sliced.w1={extra['sliced_w1']:.3g} > {sliced_w1_max}")
    if energy and params:
        std = np.array([ref_stats[p]["std"] for p in params], dtype=np.float64)
        live = np.isfinite(std) & (std > 0)
        if live.any():
            scale = np.zeros(std.size)
            scale[live] = 1.0 / std[live]
            er = ref[:, ::energy_stride(ref.shape[1], energy_max_draws)]
            ea = act[:, ::energy_stride(act.shape[1], energy_max_draws)]
            with _ffi.value_errors():
                det = ctx.energy_distance(er, ea, scale)
            det.update(mr=int(er.shape[1]), ma=int(ea.shape[1]))
            extra.update(energy=det["e"], energy_detail=det)
            if energy_max is not None and not det["e"] <= energy_max:
                failures.append(f"energy={det['e']:.3g} > {energy_max}")
    if gaussian and params:
        from .gaussian import gaussian_check
        std = np.array([ref_stats[p]["std"] for p in params], dtype=np.float64)
        live = np.isfinite(std) & (std > 0)
        if live.any():
            scale = np.zeros(std.size)
            scale[live] = 1.0 / std[live]
            with _ffi.value_errors():
                det = gaussian_check(ref, act, scale=scale, jitter=gaussian_jitter, shift=True, context=ctx)
            names = [p for i, p in enumerate(params) if live[i]]
            det["shift"] = {p: float(v) for p, v in zip(names, det["shift"])}
            det["singular_ref"] = names[det["info_ref"] - 1] if det["info_ref"] else None
            det["singular_actual"] = names[det["info_act"] - 1] if det["info_act"] else None
            extra.update(gaussian=det, gaussian_shift=det["mahalanobis"])
            if gaussian_shift_max is not None and not det["mahalanobis"] <= gaussian_shift_max:
                failures.append(f"gaussian.shift={det['mahalanobis']:.3g} > {gaussian_shift_max}")
            if gaussian_kl_max is not None and not det["kl_sym"] <= gaussian_kl_max:
                failures.append(f"gaussian.kl={det['kl_sym']:.3g} > {gaussian_kl_max}")
    result = GaussianValidateResult if "gaussian" in extra else ValidateResult
    return result(passed=not failures, compare=cmp_res, ks=ks, wasserstein=w1, wasserstein_scaled=scaled,
                  failures=failures, khat_ref=khat_ref, khat_actual=khat_act, hdi_ref=hdi_ref, hdi_actual=hdi_act, **extra)


@dataclass(frozen=True)
class WeightedValidateResult:
    passed: bool
    compare: CompareResult                       # the reference's gate on the weighted stats of `actual`
    stats: dict[str, dict[str, float]]           # per parameter: mean, std, mean_se, q5, q50, q95 under the weights
    ess: float                                   # Kish's effective sample size of the weights
    khat: float | None                           # Pareto k-hat of the log weights (psis=True), else None
    failures: list[str] = field(default_factory=list)


def validate_weighted(model: str, actual: Mapping[str, Sequence[float]], log_weights: Sequence[float],
                      tolerance: float = 0.15, metrics: Sequence[str] = ("mean", "std"), psis: bool = True,
                      khat_max: float | None = None, ess_min: float | None = None, store: DataStore | None = None,
                      context=None) -> WeightedValidateResult:
    """The reference's gate (`compare_stats`) on draws from an approximation, reweighted towards the target: `actual`
    holds joint draws (every parameter the same length) and `log_weights` one log importance ratio per draw.  psis=True
    smooths them first (Context.psis, r_eff = 1) and reports the k-hat.  `stats` holds the weighted mean, std (the
    population form) and mean_se of every parameter (Context.weighted_summary), and under q5 / q50 / q95 the weighted
    inverted-CDF quantiles: draws, not the reference's linear interpolation -- with equal weights they differ from it by at
    most one spacing of the order statistics.  khat_max / ess_min add the failures `khat=... > khat_max` and
    `ess=... < ess_min`; without them the two numbers are information only."""
    store = store or DataStore()
    ctx = context or _ffi.default_context()
    params = list(actual.keys())
    lens = {len(actual[p]) for p in params}
    if len(lens) > 1:
        raise ValueError("weighted validation needs joint draws: the parameters of `actual` differ in length")
    lw = np.ascontiguousarray(log_weights, dtype=np.float64).reshape(-1)
    table = store.open_draws(model, params=params).read_all()
    from .backends import HipBackend
    ref_stats = HipBackend(ctx).stats(table, params)
    khat = None
    stats: dict[str, dict[str, float]] = {}
    ess = float("nan")
    with _ffi.value_errors():
        if psis:
            sm = ctx.psis(lw.reshape(1, 1, -1), "pcn")
            lw, khat = sm["log_weights"][0], float(sm["khat"][0])
        if params:
            act = np.stack([np.asarray(actual[p], dtype=np.float64) for p in params])
            r = ctx.weighted_summary(act.reshape(len(params), 1, -1), "pcn", log_weights=lw, quantiles=(0.05, 0.5, 0.95))
            ess = r["ess"]
            stats = {p: {"mean": float(r["mean"][i]), "std": float(r["sd"][i]), "mean_se": float(r["mean_se"][i]),
                         "q5": float(r["quantiles"][i, 0]), "q50": float(r["quantiles"][i, 1]),
                         "q95": float(r["quantiles"][i, 2])} for i, p in enumerate(params)}
    cmp_res = compare_stats(ref_stats, stats, tolerance=tolerance, metrics=metrics, context=ctx)
    failures = list(cmp_res.failures)
    if khat_max is not None and khat is not None and not khat <= khat_max:
        failures.append(f"khat={khat:.3g} > {khat_max}")
    if ess_min is not None and not ess >= ess_min:
        failures.append(f"ess={ess:.6g} < {ess_min}")
    return WeightedValidateResult(passed=not failures, compare=cmp_res, stats=stats, ess=ess, khat=khat, failures=failures)


@dataclass(frozen=True)
class MeanShiftValidateResult:
    passed: bool
    test: dict                                   # batchmeans.mean_shift_test, "z" and "shift" keyed by (live) parameter
    p_value: float                               # its asymptotic chi-square p-value (NaN when V is singular)
    failures: list[str] = field(default_factory=list)


def validate_mean_shift(model: str, actual: Mapping[str, Sequence[float]], chains: int, p_min: float | None = None,
                        jitter: float = 0.0, r: int = 3, store: DataStore | None = None, context=None) -> MeanShiftValidateResult:
    """A calibrated joint test of the means of `actual` against a model's reference draws: `batchmeans.mean_shift_test`
    with every parameter scaled by 1 / reference std (0 where that std is not finite and > 0).  `validate` takes pooled
    draws and knows no chains, and the long-run covariance needs them: `actual[p]` holds the pooled draws of `chains`
    equally long chains, chain after chain; the reference's chains come from its table.  `test["z"]` is every live
    parameter's shift in Monte Carlo standard errors, `test["singular"]` the name of the parameter at which the pooled
    covariance is singular (else None: then T and p_value are NaN).  `p_min` adds the failure `mean_shift.p=... < p_min`
    -- a NaN fails it --; without it `passed` is True.  The chi-square is asymptotic: it wants batches longer than the
    autocorrelation time and many more batches than parameters."""
    from .batchmeans import mean_shift_test
    from .convert import table_to_tensor
    store = store or DataStore()
    ctx = context or _ffi.default_context()
    params = list(actual.keys())
    chains = int(chains)
    lens = {len(actual[p]) for p in params}
    if not params or len(lens) != 1:
        raise ValueError("mean_shift needs joint draws: at least one parameter, all of the same length")
    m = lens.pop()
    if chains < 1 or m == 0 or m % chains:
        raise ValueError(f"{m} draws per parameter are not {chains} chains of equal length")
    x, counts = table_to_tensor(store.open_draws(model, params=params).read_all(), params)
    if len(counts) == 0 or not np.all(counts == counts[0]):
        raise ValueError("mean_shift requires reference chains of equal length")
    ref = x.reshape(len(params), len(counts), int(counts[0]))
    act = np.stack([np.asarray(actual[p], dtype=np.float64) for p in params]).reshape(len(params), chains, m // chains)
    std = ref.reshape(len(params), -1).std(axis=1)
    live = np.isfinite(std) & (std > 0)
    scale = np.zeros(std.size)
    scale[live] = 1.0 / std[live]
    with _ffi.value_errors():
        det = mean_shift_test(ref, act, scale=scale, jitter=jitter, r=r, context=ctx)
    names = [p for i, p in enumerate(params) if live[i]]
    det["z"] = {p: float(v) for p, v in zip(names, det["z"])}
    det["shift"] = {p: float(v) for p, v in zip(names, det["shift"])}
    det["singular"] = names[det["info"] - 1] if det["info"] else None
    failures = []
    if p_min is not None and not det["p_value"] >= p_min:
        failures.append(f"mean_shift.p={det['p_value']:.3g} < {p_min}")
    return MeanShiftValidateResult(passed=not failures, test=det, p_value=det["p_value"], failures=failures)

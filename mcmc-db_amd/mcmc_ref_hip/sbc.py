"""Simulation-based calibration (SBC; Talts et al. 2018, Schad et al. 2021, the `SBC` R package): a check of a sampler
that needs no reference posterior.  Draw a parameter value from the prior, simulate data from it, fit; over many such
simulations the rank of the true value among the posterior draws is uniform exactly when the sampler is right, and the
shape of the rank histogram says what is wrong (a ∪: the posterior is too narrow, a ∩: too wide, a slope: biased).

`sbc(draws, truth)` ranks S simulations x P parameters in one device call (Context.sbc_ranks) and judges the ranks on
the host (mcr_sbc_uniformity); `sbc_files(paths, truth)` does the same for one draws file per simulation.
"""
from __future__ import annotations

import csv
from dataclasses import dataclass
from pathlib import Path
from typing import Mapping, Sequence

import numpy as np

from . import _ffi

DEFAULT_SEED = 4711


@dataclass(frozen=True)
class SbcResult:
    """ranks [S][P] in 0 .. n_draws; counts [P][bins] and expected [bins] of the rank histogram; per parameter chi2 (dof =
    bins - 1), pvalue and ecdf_dev, the largest distance of the ranks' ECDF from the uniform one; z_score [S][P] = (posterior
    mean - truth) / posterior sd and contraction [S][P] = 1 - posterior variance / prior variance; n_tied: the (s, p) with a
    draw equal to the truth; failures: one line per parameter below p_min; passed: no failures."""
    names: tuple
    ranks: np.ndarray
    n_draws: int
    bins: int
    counts: np.ndarray
    expected: np.ndarray
    chi2: np.ndarray
    dof: int
    pvalue: np.ndarray
    ecdf_dev: np.ndarray
    z_score: np.ndarray
    contraction: np.ndarray
    n_tied: int
    failures: tuple
    passed: bool

    def table(self) -> dict:
        """One row per parameter: chi2, dof, p, ecdf_dev, mean |z|, mean contraction."""
        return {n: {"chi2": float(self.chi2[p]), "dof": self.dof, "p": float(self.pvalue[p]), "ecdf_dev": float(self.ecdf_dev[p]),
                    "mean_abs_z": float(np.mean(np.abs(self.z_score[:, p]))), "mean_contraction": float(np.mean(self.contraction[:, p]))}
                for p, n in enumerate(self.names)}


def default_bins(n_draws: int) -> int:
    """The largest divisor of n_draws + 1 in 2 .. 20 (every bin then holds the same number of ranks), else min(20, n_draws + 1)."""
    for b in range(20, 1, -1):
        if (n_draws + 1) % b == 0:
            return b
    return min(20, n_draws + 1)


def tie_ranks(n_less, n_equal, seed: int = DEFAULT_SEED) -> np.ndarray:
    """The rank of every truth: n_less + u, u uniform on 0 .. n_equal.  u is numpy.random.default_rng(seed).integers(0,
    n_equal + 1), drawn for the whole [S][P] array in one call and used only where n_equal > 0."""
    n_less, n_equal = np.asarray(n_less, dtype=np.int64), np.asarray(n_equal, dtype=np.int64)
    u = np.random.default_rng(seed).integers(0, n_equal + 1)
    return n_less + np.where(n_equal > 0, u, 0)


def sbc_from_counts(res: dict, truth, *, bins=None, seed: int = DEFAULT_SEED, prior_sd=None, names=None, p_min=None) -> SbcResult:
    """The judgement of sbc() on what a rank call returned (Context.sbc_ranks, _ffi.sbc_ranks_host)."""
    truth = np.asarray(truth, dtype=np.float64)
    S, P = truth.shape
    L = int(res["n_draws"])
    if S < 1:
        raise ValueError("sbc needs at least one simulation")
    ranks = tie_ranks(res["n_less"], res["n_equal"], seed)
    B = default_bins(L) if bins is None else int(bins)
    u = _ffi.sbc_uniformity(ranks, L, B)
    names = tuple(f"p{p}" for p in range(P)) if names is None else tuple(names)
    if len(names) != P:
        raise ValueError(f"{len(names)} names for {P} parameters")
    if prior_sd is None:
        prior_var = np.var(truth, axis=0)                        # (the population form)
    else:
        prior_var = np.broadcast_to(np.asarray(prior_sd, dtype=np.float64), (P,)) ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        z = (res["mean"] - truth) / res["sd"]
        contraction = 1.0 - res["sd"] ** 2 / prior_var
    failures = ()
    if p_min is not None:
        failures = tuple(f"{n}.sbc_p={p:.3g} < {p_min}" for n, p in zip(names, u["pvalue"]) if not p >= p_min)
    return SbcResult(names=names, ranks=ranks, n_draws=L, bins=B, counts=u["counts"], expected=u["expected"], chi2=u["chi2"],
                     dof=B - 1, pvalue=u["pvalue"], ecdf_dev=u["ecdf_dev"], z_score=z, contraction=contraction,
                     n_tied=int(np.count_nonzero(res["n_equal"] > 0)), failures=failures, passed=not failures)


def sbc(draws, truth, *, layout: str = "spcn", thin: int = 1, bins=None, seed: int = DEFAULT_SEED, prior_sd=None, names=None,
        p_min=None, context=None) -> SbcResult:
    """Simulation-based calibration of S fits at once.  draws: a 4-D array whose axes are `layout` (a permutation of
    "scnp": simulations, chains, draws, parameters) or the DeviceSims of Context.upload_sims; truth [S][P]: the values the
    data of each simulation were generated from.  thin = k keeps the draws 0, k, 2k, ... of every chain (the ranks are
    uniform only for draws that are close to independent).

    Ties are broken as the SBC paper says, reproducibly: rank = n_less + numpy.random.default_rng(seed).integers(0, n_equal
    + 1), drawn for the whole [S][P] array in one call and used only where n_equal > 0.  bins: of the rank histogram; the
    default is the largest divisor of n_draws + 1 in 2 .. 20, else min(20, n_draws + 1).  prior_sd: the prior's sd per
    parameter for the contraction; the default is the population sd of truth[:, p].  p_min: a parameter whose chi-square
    p-value is below it adds the failure "{name}.sbc_p={p:.3g} < {p_min}"; without it the result is information and
    `passed` is True."""
    ctx = context if context is not None else _ffi.default_context()
    res = ctx.sbc_ranks(draws, truth, layout, thin)
    return sbc_from_counts(res, truth, bins=bins, seed=seed, prior_sd=prior_sd, names=names, p_min=p_min)


def read_truth(truth, names: Sequence[str], S: int) -> np.ndarray:
    """truth [S][P] for the parameters `names`: from a mapping name -> S values, or from a CSV / Parquet table with one row
    per simulation and a column per parameter."""
    if isinstance(truth, (str, Path)):
        path = Path(truth)
        if path.suffix.lower() == ".parquet":
            import pyarrow.parquet as pq

            tab = pq.read_table(path)
            truth = {n: tab.column(n).to_numpy() for n in tab.column_names}
        else:
            with open(path, newline="") as fh:
                rows = list(csv.reader(r for r in fh if not r.startswith("#")))
            if not rows:
                raise ValueError(f"{path}: empty truth table")
            head = [h.strip().strip('"') for h in rows[0]]
            truth = {}
            for j, h in enumerate(head):
                try:
                    truth[h] = np.array([float(r[j]) for r in rows[1:] if r], dtype=np.float64)
                except ValueError:                               # (a column of labels)
                    continue
    if not isinstance(truth, Mapping):
        raise ValueError("truth must be a mapping name -> values or the path of a CSV / Parquet table")
    missing = [n for n in names if n not in truth]
    if missing:
        raise KeyError(f"no true values for {missing}")
    cols = [np.asarray(truth[n], dtype=np.float64).reshape(-1) for n in names]
    bad = [n for n, c in zip(names, cols) if c.size != S]
    if bad:
        raise ValueError(f"truth needs one value per simulation ({S}); {bad} differ")
    return np.ascontiguousarray(np.stack(cols, axis=1)) if cols else np.empty((S, 0))


def _file_ranks(ctx, paths, params, truth_of, thin: int) -> tuple[list[str], np.ndarray, dict]:
    """(names, truth [S][P], the rank call's result) of one draws file per simulation: decoded on the device
    (parquet.read_draws_many) and ranked where they lie (mcr_sbc_ranks_dev), one call per run of files that stand
    [P][M]-contiguous one behind the other.  A file's chains, ragged or not, are pooled as one chain."""
    from . import parquet

    S = len(paths)
    dd = parquet.read_draws_many(ctx, [str(p) for p in paths], [params] * S if params is not None else None)
    try:
        names = list(dd[0].params)
        M = int(dd[0].counts.sum())
        for k, d in enumerate(dd):
            if list(d.params) != names or int(d.counts.sum()) != M:
                raise ValueError(f"{paths[k]}: every simulation needs the same parameters and the same number of draws")
        truth = truth_of(names, S)
        P, step = len(names), len(names) * M * 8
        parts, s0 = [], 0
        while s0 < S:
            s1 = s0 + 1
            while s1 < S and step and dd[s1].buf.ptr.value == dd[s0].buf.ptr.value + (s1 - s0) * step:
                s1 += 1
            t = _ffi.DeviceSims(ctx, dd[s0].buf, (_ffi.MCR_F64, s1 - s0, 1, M, P, P * M, M, 1, M))
            parts.append(ctx.sbc_ranks(t, truth[s0:s1], thin=thin))
            s0 = s1
        res = {k: np.concatenate([r[k] for r in parts], axis=0) for k in ("n_less", "n_equal", "mean", "sd")}
        res["n_draws"] = parts[0]["n_draws"]
        return names, truth, res
    finally:
        for d in dd:
            d.free()


def sbc_files(paths, truth, params=None, *, thin: int = 1, context=None, **kw) -> SbcResult:
    """sbc() of one draws file (Parquet) per simulation, in order.  truth: a mapping name -> S values, or the path of a
    CSV / Parquet table with one row per simulation.  params: the parameters (default: every numeric column but chain and
    draw).  The files are decoded and ranked on the device.  **kw: bins, seed,
    prior_sd, p_min as in sbc()."""
    paths = list(paths)
    if not paths:
        raise ValueError("sbc_files needs at least one file")
    ctx = context if context is not None else _ffi.default_context()
    names, t, res = _file_ranks(ctx, paths, list(params) if params is not None else None, lambda n, S: read_truth(truth, n, S), thin)
    return sbc_from_counts(res, t, names=names, **kw)

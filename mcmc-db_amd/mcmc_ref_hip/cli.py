"""`mcmc-ref-hip` CLI: the hot-path commands of the reference's `mcmc-ref` CLI on the GPU.

Mirrors src/mcmc_ref/cli.py for `list`, `stats`, `diagnostics`, `info`, `compare`, `convert`,
`provenance-generate` and `provenance-publish` (same options, echo strings and exit codes: compare exits 2 when the
gate fails, provenance-generate exits 1 when any recipe failed); `--backend` accepts "hip" (default) and the
reference's "arrow" / "numpy".  `draws` writes a model's draws as CSV or Parquet with the reference's options and
bytes, decoded, filtered and formatted on the GPU (reference.export_draws).  `provenance-scaffold` (Stan programs + data
literals) and the pairs commands are outside the statistics path and not included.  `cmdstan-summary CHAIN.csv...` is
this package's own: the chain files of a CmdStan run, parsed on the GPU, printed like `stats --include-diagnostics`; so is
`json-summary ARCHIVE.json.zip...` for chain-list JSON archives and `csv-summary FILE.csv...` for table CSVs, and
`validate MODEL --actual FILE.csv`, the command of `validate.validate` (compare's gate plus KS / Wasserstein-1 per
parameter and, with `--sliced K`, along K random directions of the joint distribution; exits like `compare`).
`nested-rhat FILE --superchains K` prints nested R-hat, the diagnostic for many short chains, of a draws table.
`pareto-khat FILE` prints the Pareto k-hat of every parameter's tails: whether a mean and a std of the draws can be trusted.
`loo FILE` prints PSIS-LOO of a table's pointwise log-likelihood columns: elpd_loo, p_loo and the observations' k-hats.
`weighted-summary FILE` prints every parameter's mean, sd, standard error and quantiles under a column of importance weights.
`ess-quantile FILE` prints the effective draws behind every parameter's quantile estimates (and its local efficiency).
`std-diagnostics FILE` prints R-hat and ESS in the Stan convention (split chains, Blom scores, Geyer's rule): the numbers
of stansummary, posterior and ArviZ, where `diagnostics` and `cmdstan-summary` print the reference's.
`rank-ecdf FILE` prints the per-chain rank-ECDF uniformity test with simultaneous bands: which chain disagrees with the
pooled draws, at which quantile, and whether by more than chance.
`multi-ess FILE` prints the multivariate effective sample size of a table from its batch-means long-run covariance, and
`mean-test REF_FILE ACT_FILE` the calibrated joint test of equal means of two tables; exits 1 when `--p-min` is missed.
`hdi FILE` prints the highest-density interval(s) of every parameter: the shortest interval holding a share of the draws.
`autocorr FILE` prints every parameter's integrated autocorrelation time (Sokal's window) and its stickiest and least
sticky chain; as JSON, the autocorrelation function of every chain up to `--max-lag` as well.
`sbc --truth TABLE FILE...` is simulation-based calibration: one draws file per simulated data set, the rank of each true
value among its draws, and per parameter the uniformity of those ranks; exits 1 when `--p-min` is given and missed.
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

import click

from . import convert as convert_mod
from . import generate as generate_mod
from . import reference
from .store import DataStore


@click.group()
def main() -> None:
    """mcmc-ref-hip CLI."""


def _headers(stats: dict) -> list[str]:
    keys: set[str] = set()
    for metrics in stats.values():
        keys.update(metrics.keys())
    return sorted(keys)


def _print_table(stats: dict) -> None:
    headers = ["param"] + _headers(stats)
    widths = [max(len(h), 6) for h in headers]
    click.echo(" ".join(h.ljust(w) for h, w in zip(headers, widths, strict=False)))
    for param, metrics in stats.items():
        row = [param] + [f"{metrics.get(h, float('nan')):.6g}" for h in headers[1:]]
        click.echo(" ".join(v.ljust(w) for v, w in zip(row, widths, strict=False)))


def _echo_stats(stats: dict, format_: str) -> None:
    if format_ == "json":
        click.echo(json.dumps(stats, indent=2, sort_keys=True))
    elif format_ == "csv":
        headers = ["param"] + _headers(stats)
        click.echo(",".join(headers))
        for param, metrics in stats.items():
            click.echo(",".join([param] + [str(metrics.get(h, "")) for h in headers[1:]]))
    else:
        _print_table(stats)


@main.command("list")
@click.option("--format", "format_", type=click.Choice(["table", "json"], case_sensitive=False), default="table")
def list_cmd(format_: str) -> None:
    models = reference.list_models()
    if format_ == "json":
        click.echo(json.dumps(models, indent=2))
        return
    for m in models:
        click.echo(m)


@main.command("stats")
@click.argument("model")
@click.option("--params", default=None, help="Comma-separated parameter list")
@click.option("--format", "format_", type=click.Choice(["table", "csv", "json"], case_sensitive=False), default="table")
@click.option("--backend", type=click.Choice(["hip", "arrow", "numpy"], case_sensitive=False), default="hip")
@click.option("--quantile-mode", type=click.Choice(["exact"], case_sensitive=False), default="exact")
@click.option("--include-diagnostics", is_flag=True, help="Include rhat/ess metrics")
def stats_cmd(model, params, format_, backend, quantile_mode, include_diagnostics) -> None:
    param_list = params.split(",") if params else None
    stats = reference.stats(model, params=param_list, backend=backend, quantile_mode=quantile_mode)
    if include_diagnostics:
        for param, metrics in reference.diagnostics_for_model(model, params=param_list).items():
            stats.setdefault(param, {}).update(metrics)
    _echo_stats(stats, format_)


@main.command("draws")
@click.argument("model")
@click.option("--params", default=None, help="Comma-separated parameter list")
@click.option("--chains", default=None, help="Comma-separated chain indices")
@click.option("--format", "format_", type=click.Choice(["csv", "parquet"], case_sensitive=False), default="csv")
@click.option("--output", type=click.Path(path_type=Path), default=None)
def draws_cmd(model: str, params: str | None, chains: str | None, format_: str, output: Path | None) -> None:
    """A model's draws as CSV (default) or Parquet, to --output or stdout (reference cli.py:100-127)."""
    param_list = params.split(",") if params else None
    chain_list = [int(c) for c in chains.split(",")] if chains else None
    reference.export_draws(model, sys.stdout.buffer if output is None else output, params=param_list, chains=chain_list,
                           format_=format_.lower())


@main.command("cmdstan-summary")
@click.argument("chains", nargs=-1, required=True, type=click.Path(path_type=Path, exists=True, dir_okay=False))
@click.option("--format", "format_", type=click.Choice(["table", "csv", "json"], case_sensitive=False), default="table")
@click.option("--min-chains", default=4, type=int)
def cmdstan_summary_cmd(chains, format_: str, min_chains: int) -> None:
    """Statistics and diagnostics of a CmdStan run's chain CSVs, parsed on the GPU (no counterpart in the reference)."""
    from . import cmdstan_generate
    try:
        stats = cmdstan_generate.summarize_chains(list(chains), min_chains=min_chains)
    except ValueError as exc:
        raise click.ClickException(str(exc)) from exc
    _echo_stats(stats, format_)


@main.command("json-summary")
@click.argument("archives", nargs=-1, required=True, type=click.Path(path_type=Path, exists=True, dir_okay=False))
@click.option("--format", "format_", type=click.Choice(["table", "csv", "json"], case_sensitive=False), default="table")
@click.option("--min-chains", default=4, type=int)
def json_summary_cmd(archives, format_: str, min_chains: int) -> None:
    """Statistics and diagnostics of chain-list JSON archives, parsed on the GPU (no counterpart in the reference).
    One archive prints like `cmdstan-summary`; several print one block per archive (json: one object keyed by path)."""
    try:
        stats = {str(a): convert_mod.summarize_json_zip(a, min_chains=min_chains) for a in archives}
    except (ValueError, KeyError, IndexError) as exc:
        raise click.ClickException(str(exc)) from exc
    if len(archives) == 1:
        _echo_stats(stats[str(archives[0])], format_)
    elif format_ == "json":
        click.echo(json.dumps(stats, indent=2, sort_keys=True))
    else:
        for name, st in stats.items():
            click.echo(f"# {name}")
            _echo_stats(st, format_)


@main.command("csv-summary")
@click.argument("files", nargs=-1, required=True, type=click.Path(path_type=Path, exists=True, dir_okay=False))
@click.option("--format", "format_", type=click.Choice(["table", "csv", "json"], case_sensitive=False), default="table")
@click.option("--min-chains", default=4, type=int)
def csv_summary_cmd(files, format_: str, min_chains: int) -> None:
    """Statistics and diagnostics of table CSVs (a header, one row per draw, optional `chain` / `draw` columns), parsed
    on the GPU (no counterpart in the reference).  Prints like `json-summary`."""
    try:
        stats = {str(f): convert_mod.summarize_csv(f, min_chains=min_chains) for f in files}
    except (ValueError, KeyError, IndexError) as exc:
        raise click.ClickException(str(exc)) from exc
    if len(files) == 1:
        _echo_stats(stats[str(files[0])], format_)
    elif format_ == "json":
        click.echo(json.dumps(stats, indent=2, sort_keys=True))
    else:
        for name, st in stats.items():
            click.echo(f"# {name}")
            _echo_stats(st, format_)


@main.command("nested-rhat")
@click.argument("file", type=click.Path(path_type=Path, exists=True, dir_okay=False))
@click.option("--superchains", required=True, type=int, help="Number of superchains: blocks of chains in chain-id order")
@click.option("--params", default=None, help="Comma-separated parameter list")
@click.option("--format", "format_", type=click.Choice(["table", "csv", "json"], case_sensitive=False), default="table")
def nested_rhat_cmd(file: Path, superchains: int, params: str | None, format_: str) -> None:
    """Nested R-hat (Margossian et al.) of a draws table with any number of equal-length chains (no counterpart in the
    reference): nrhat = max(nrhat_bulk, nrhat_tail), and nrhat_raw on the draws themselves."""
    try:
        stats = convert_mod.nested_rhat_file(file, superchains, params=params.split(",") if params else None)
    except (ValueError, KeyError, IndexError) as exc:
        raise click.ClickException(str(exc)) from exc
    _echo_stats(stats, format_)


@main.command("pareto-khat")
@click.argument("file", type=click.Path(path_type=Path, exists=True, dir_okay=False))
@click.option("--params", default=None, help="Comma-separated parameter list")
@click.option("--tail-draws", default=None, type=int, help="Draws per tail (default: ceil(3 sqrt(M)), M // 5 up to 225 draws)")
@click.option("--format", "format_", type=click.Choice(["table", "csv", "json"], case_sensitive=False), default="table")
def pareto_khat_cmd(file: Path, params: str | None, tail_draws: int | None, format_: str) -> None:
    """Pareto k-hat (Vehtari et al.) of the pooled draws of a table (no counterpart in the reference): khat =
    max(khat_left, khat_right); below 0.5 mean and std can be trusted, from 0.7 neither."""
    try:
        stats = convert_mod.pareto_khat_file(file, params=params.split(",") if params else None, ndraws_tail=tail_draws)
    except (ValueError, KeyError, IndexError) as exc:
        raise click.ClickException(str(exc)) from exc
    _echo_stats(stats, format_)


def _loo_summary(r: dict) -> dict:
    return {k: r[k] for k in ("elpd_loo", "se", "p_loo", "lppd", "n_obs", "n_draws", "khat_counts", "khat_threshold")}


@main.command("loo")
@click.argument("file", type=click.Path(path_type=Path, exists=True, dir_okay=False))
@click.option("--prefix", default="log_lik", help="The pointwise log-likelihood columns: names that start with this (default: log_lik)")
@click.option("--params", default=None, help="Comma-separated column list to choose from")
@click.option("--against", default=None, type=click.Path(path_type=Path, exists=True, dir_okay=False),
              help="A second model fitted to the same data: print elpd_diff (FILE minus this) and se_diff as well")
@click.option("--pointwise", is_flag=True, help="Print elpd, p_loo, lppd and k-hat of every observation")
@click.option("--format", "format_", type=click.Choice(["table", "json"], case_sensitive=False), default="table")
def loo_cmd(file: Path, prefix: str, params: str | None, against: Path | None, pointwise: bool, format_: str) -> None:
    """PSIS-LOO (Vehtari et al.; ArviZ's loo) of the pointwise log-likelihood columns of a draws table (no counterpart in
    the reference): elpd_loo with its standard error, p_loo, and the observations' Pareto k-hats counted in (-inf, 0.5],
    (0.5, 0.7], (0.7, 1] and (1, inf) -- above 0.7 an observation's estimate is not reliable."""
    plist = params.split(",") if params else None
    try:
        if against is not None:
            cmp_ = convert_mod.loo_compare_files(file, against, params=plist, prefix=prefix)
            r, other = cmp_["a"], cmp_["b"]
        else:
            cmp_, other, r = None, None, convert_mod.loo_file(file, params=plist, prefix=prefix)
    except (ValueError, KeyError, IndexError) as exc:
        raise click.ClickException(str(exc)) from exc
    rows = {n: {"elpd": float(r["elpd_i"][i]), "p_loo": float(r["p_loo_i"][i]), "lppd": float(r["lppd_i"][i]),
                "khat": float(r["khat"][i])} for i, n in enumerate(r["names"])} if pointwise else None
    if format_ == "json":
        out = _loo_summary(r)
        if cmp_ is not None:
            out.update(elpd_diff=cmp_["elpd_diff"], se_diff=cmp_["se_diff"], against=_loo_summary(other))
        if rows is not None:
            out["pointwise"] = rows
        click.echo(json.dumps(out, indent=2, sort_keys=True))
        return
    for name, res in (("", r),) if other is None else ((str(file), r), (str(against), other)):
        if name:
            click.echo(f"# {name}")
        click.echo(f"elpd_loo {res['elpd_loo']:.6g}  se {res['se']:.6g}  p_loo {res['p_loo']:.6g}  lppd {res['lppd']:.6g}")
        click.echo(f"observations {res['n_obs']}  draws {res['n_draws']}")
        c = res["khat_counts"]
        click.echo(f"khat (-inf, 0.5] {c[0]}  (0.5, 0.7] {c[1]}  (0.7, 1] {c[2]}  (1, inf) {c[3]}")
    if cmp_ is not None:
        click.echo(f"elpd_diff {cmp_['elpd_diff']:.6g}  se_diff {cmp_['se_diff']:.6g}")
    if rows is not None:
        _print_table(rows)


@main.command("hdi")
@click.argument("file", type=click.Path(path_type=Path, exists=True, dir_okay=False))
@click.option("--params", default=None, help="Comma-separated parameter list")
@click.option("--prob", "probs", multiple=True, type=float, help="Share of the draws inside the interval; may be repeated (default: 0.94)")
@click.option("--format", "format_", type=click.Choice(["table", "json"], case_sensitive=False), default="table")
def hdi_cmd(file: Path, params: str | None, probs: tuple[float, ...], format_: str) -> None:
    """Highest-density intervals (ArviZ's unimodal hdi) of the pooled draws of a table (no counterpart in the reference):
    per probability q the columns hdi_lo_q and hdi_hi_q."""
    try:
        stats = convert_mod.hdi_file(file, params=params.split(",") if params else None, prob=probs or (0.94,))
    except (ValueError, KeyError, IndexError) as exc:
        raise click.ClickException(str(exc)) from exc
    _echo_stats(stats, format_)


@main.command("ess-quantile")
@click.argument("file", type=click.Path(path_type=Path, exists=True, dir_okay=False))
@click.option("--params", default=None, help="Comma-separated parameter list")
@click.option("--probs", "probs", multiple=True, type=float, help="A probability inside (0, 1); may be repeated (default: 0.05 0.5 0.95)")
@click.option("--local", "local", default=None, type=int, help="Also the local efficiency in this many quantile bins (at most 32)")
@click.option("--format", "format_", type=click.Choice(["table", "json"], case_sensitive=False), default="table")
def ess_quantile_cmd(file: Path, params: str | None, probs: tuple[float, ...], local: int | None, format_: str) -> None:
    """Effective draws behind the quantile estimates of a table (no counterpart in the reference): per probability q the
    quantile q_q and ess_q_q, the ESS of the indicator x <= quantile under the library's ESS rule (unsplit chains, first
    negative autocorrelation; not Geyer's rule), and ess_tail_min, the smaller of the two outermost."""
    try:
        stats = convert_mod.ess_quantile_file(file, params=params.split(",") if params else None,
                                              probs=probs or (0.05, 0.5, 0.95), local=local)
    except (ValueError, KeyError, IndexError) as exc:
        raise click.ClickException(str(exc)) from exc
    _echo_stats(stats, format_)


@main.command("std-diagnostics")
@click.argument("file", type=click.Path(path_type=Path, exists=True, dir_okay=False))
@click.option("--params", default=None, help="Comma-separated parameter list")
@click.option("--basic", is_flag=True, help="Also rhat_basic, ess_mean and mcse_mean of the draws themselves")
@click.option("--json", "as_json", is_flag=True, help="Print JSON instead of a table")
def std_diagnostics_cmd(file: Path, params: str | None, basic: bool, as_json: bool) -> None:
    """R-hat and ESS of a table in the Stan convention (no counterpart in the reference): split chains, rank
    normalisation with Blom scores, folding, Geyer's initial sequences -- rhat, ess_bulk and ess_tail as stansummary,
    posterior and ArviZ define them, with the walks' lags.  Chains of equal length; for an odd length the middle draw of
    each chain is dropped."""
    from . import standard
    try:
        stats = standard.diagnostics_file(file, params=params.split(",") if params else None, basic=basic)
    except (ValueError, KeyError, IndexError) as exc:
        raise click.ClickException(str(exc)) from exc
    _echo_stats(stats, "json" if as_json else "table")


def _thin_option(_ctx, _param, value: str):
    if value == "ess":
        return value
    try:
        thin = int(value)
    except ValueError:
        thin = 0
    if thin < 1:
        raise click.BadParameter("an integer >= 1 or \"ess\"")
    return thin


@main.command("rank-ecdf")
@click.argument("file", type=click.Path(path_type=Path, exists=True, dir_okay=False))
@click.option("--params", default=None, help="Comma-separated parameter list")
@click.option("--points", default=None, type=click.IntRange(2, 1024), help="Evaluation points K (default: min(n, 100))")
@click.option("--thin", default="1", callback=_thin_option, help="Keep every T-th draw, or \"ess\": a stride from the bulk ESS")
@click.option("--sims", default=4000, type=click.IntRange(1), help="Simulated samples behind the simultaneous level")
@click.option("--seed", default=0, type=int, help="Seed of the simulated samples")
@click.option("--alpha", default=0.05, type=click.FloatRange(0.0, 1.0), help="Level of the test")
@click.option("--host", is_flag=True, help="By the definition on the host, without a GPU")
@click.option("--json", "as_json", is_flag=True, help="Print JSON instead of a table")
def rank_ecdf_cmd(file: Path, params: str | None, points: int | None, thin, sims: int, seed: int, alpha: float, host: bool,
                  as_json: bool) -> None:
    """Which chain disagrees, and where (no counterpart in the reference): the per-chain rank-ECDF uniformity test with
    simultaneous bands of Saeilynoja, Buerkner and Vehtari.  One row per parameter: the p-value, reject (1 when p <=
    alpha), the offending chain, the point as a pooled quantile and the largest difference between that chain's ECDF and
    the pooled one.  The draws must be exchangeable: thin autocorrelated chains.  Chains of equal length.  Exits
    non-zero only on errors."""
    from . import rankecdf
    try:
        stats = rankecdf.rank_ecdf_file(file, params=params.split(",") if params else None, points=points, thin=thin, sims=sims,
                                        seed=seed, alpha=alpha, host=host)
    except (ValueError, KeyError, IndexError) as exc:
        raise click.ClickException(str(exc)) from exc
    _echo_stats(stats, "json" if as_json else "table")


@main.command("multi-ess")
@click.argument("file", type=click.Path(path_type=Path, exists=True, dir_okay=False))
@click.option("--params", default=None, help="Comma-separated parameter list")
@click.option("--batch", default=None, type=int, help="Batch size (default: about sqrt(draws per chain))")
@click.option("--r", "r", type=click.Choice(["1", "3"]), default="3", help="3: lugsail batch means (default); 1: plain")
@click.option("--format", "format_", type=click.Choice(["table", "json"], case_sensitive=False), default="table")
def multi_ess_cmd(file: Path, params: str | None, batch: int | None, r: str, format_: str) -> None:
    """The multivariate effective sample size of a table (no counterpart in the reference): mESS of Vats, Flegal and Jones
    from the batch-means long-run covariance, and per parameter the Monte Carlo standard error of the mean and ess_bm."""
    try:
        stats = convert_mod.multi_ess_file(file, params=params.split(",") if params else None, batch=batch, r=int(r))
    except (ValueError, KeyError, IndexError) as exc:
        raise click.ClickException(str(exc)) from exc
    _echo_stats(stats, format_)


@main.command("mean-test")
@click.argument("ref_file", type=click.Path(path_type=Path, exists=True, dir_okay=False))
@click.argument("act_file", type=click.Path(path_type=Path, exists=True, dir_okay=False))
@click.option("--params", default=None, help="Comma-separated parameter list")
@click.option("--jitter", default=0.0, type=float, help="Added to the diagonal of the pooled covariance (correlation scale)")
@click.option("--p-min", default=None, type=float, help="Fail (exit 1) when the p-value is below this")
@click.option("--format", "format_", type=click.Choice(["table", "json"], case_sensitive=False), default="table")
def mean_test_cmd(ref_file: Path, act_file: Path, params: str | None, jitter: float, p_min: float | None, format_: str) -> None:
    """Have the means moved?  The joint test of equal means of two tables on the lugsail batch-means long-run covariance:
    T, its asymptotic chi-square p-value, and every parameter's shift in Monte Carlo standard errors."""
    try:
        res = convert_mod.mean_test_files(ref_file, act_file, params=params.split(",") if params else None, jitter=jitter)
    except (ValueError, KeyError, IndexError) as exc:
        raise click.ClickException(str(exc)) from exc
    if format_ == "json":
        click.echo(json.dumps(res, indent=2, sort_keys=True))
    else:
        click.echo(f"T={res['T']:.6g} dof={res['dof']} p_value={res['p_value']:.6g} mess_ref={res['mess_ref']:.6g} "
                   f"mess_act={res['mess_act']:.6g}" + (f" singular={res['singular']}" if res["singular"] else ""))
        _print_table({n: {"z": z, "shift": res["shift"][n]} for n, z in res["z"].items()})
    if p_min is not None and not res["p_value"] >= p_min:
        raise SystemExit(1)


@main.command("weighted-summary")
@click.argument("file", type=click.Path(path_type=Path, exists=True, dir_okay=False))
@click.option("--log-weights", default=None, help="The column of log importance ratios (or log weights)")
@click.option("--weights", default=None, help="The column of linear weights (>= 0)")
@click.option("--params", default=None, help="Comma-separated parameter list")
@click.option("--quantile", "quantiles", multiple=True, type=float, help="A probability in [0, 1]; may be repeated (default: 0.05 0.5 0.95)")
@click.option("--no-psis", is_flag=True, help="Use the log weights as they are, without Pareto smoothing")
@click.option("--format", "format_", type=click.Choice(["table", "json"], case_sensitive=False), default="table")
def weighted_summary_cmd(file: Path, log_weights: str | None, weights: str | None, params: str | None,
                         quantiles: tuple[float, ...], no_psis: bool, format_: str) -> None:
    """Importance-weighted mean, sd, standard error and inverted-CDF quantiles of every parameter of a draws table under
    one weight column (no counterpart in the reference).  Log weights are Pareto-smoothed first (PSIS) unless --no-psis:
    a k-hat above 0.7 says the weighted estimates are not reliable."""
    try:
        res = convert_mod.weighted_summary_file(file, log_weights=log_weights, weights=weights,
                                                params=params.split(",") if params else None,
                                                quantiles=quantiles or (0.05, 0.5, 0.95),
                                                psis=not no_psis and weights is None)
    except (ValueError, KeyError, IndexError) as exc:
        raise click.ClickException(str(exc)) from exc
    if format_ == "json":
        click.echo(json.dumps(res, indent=2, sort_keys=True))
        return
    click.echo(f"draws {res['n_draws']}  ess {res['ess']:.6g}" +
               (f"  khat {res['khat']:.3g} (threshold {res['khat_threshold']:.3g})" if "khat" in res else ""))
    _print_table(res["params"])


@main.command("sbc")
@click.argument("files", nargs=-1, required=True, type=click.Path(path_type=Path, exists=True, dir_okay=False))
@click.option("--truth", "truth", required=True, type=click.Path(path_type=Path, exists=True, dir_okay=False),
              help="CSV or Parquet table of the true values: one row per simulation, one column per parameter")
@click.option("--thin", default=1, type=int, help="Keep every K-th draw of a simulation (default: 1)")
@click.option("--bins", default=None, type=int, help="Bins of the rank histogram (default: a divisor of draws + 1, at most 20)")
@click.option("--p-min", default=None, type=float, help="Fail (exit 1) when a parameter's chi-square p-value is below this")
@click.option("--params", default=None, help="Comma-separated parameter list")
@click.option("--format", "format_", type=click.Choice(["table", "json"], case_sensitive=False), default="table")
def sbc_cmd(files: tuple[Path, ...], truth: Path, thin: int, bins: int | None, p_min: float | None, params: str | None,
            format_: str) -> None:
    """Simulation-based calibration (no counterpart in the reference): FILES are the draws of one fit each, in the order of
    the rows of --truth.  Per parameter: the chi-square statistic of the rank histogram with its degrees of freedom and
    p-value, the largest ECDF deviation, the mean |z| and the mean posterior contraction."""
    from . import sbc as sbc_mod

    try:
        res = sbc_mod.sbc_files(files, truth, params=params.split(",") if params else None, thin=thin, bins=bins, p_min=p_min)
    except (ValueError, KeyError, IndexError) as exc:
        raise click.ClickException(str(exc)) from exc
    if format_ == "json":
        click.echo(json.dumps({"simulations": int(res.ranks.shape[0]), "draws": res.n_draws, "bins": res.bins, "ties": res.n_tied,
                               "params": res.table(), "failures": list(res.failures)}, indent=2, sort_keys=True))
    else:
        click.echo(f"simulations {res.ranks.shape[0]}  draws {res.n_draws}  bins {res.bins}  ties {res.n_tied}")
        _print_table(res.table())
        for line in res.failures:
            click.echo(f"- {line}")
    if not res.passed:
        raise SystemExit(1)


@main.command("autocorr")
@click.argument("file", type=click.Path(path_type=Path, exists=True, dir_okay=False))
@click.option("--params", default=None, help="Comma-separated parameter list")
@click.option("--max-lag", default=None, type=int, help="Largest lag (default: min(100, N - 1); at most 4096)")
@click.option("--unbiased", is_flag=True, help="Divide lag l by N - l instead of N")
@click.option("--window-c", default=5.0, type=float, help="Sokal's window constant: the first W >= c * tau_W (default: 5)")
@click.option("--format", "format_", type=click.Choice(["table", "json"], case_sensitive=False), default="table")
def autocorr_cmd(file: Path, params: str | None, max_lag: int | None, unbiased: bool, window_c: float, format_: str) -> None:
    """Autocorrelation functions and integrated autocorrelation times (ArviZ's autocorr, emcee's integrated_time) of the
    chains of a draws table (no counterpart in the reference).  The table prints the within-chain pooled tau, window (-1:
    not decayed within --max-lag, tau is a lower bound) and ess_pooled, and the smallest and largest per-chain tau with
    their chains; JSON carries the full arrays."""
    try:
        stats = convert_mod.autocorr_file(file, params=params.split(",") if params else None, max_lag=max_lag,
                                          unbiased=unbiased, window_c=window_c)
    except (ValueError, KeyError, IndexError) as exc:
        raise click.ClickException(str(exc)) from exc
    if format_ == "json":
        click.echo(json.dumps(stats, indent=2, sort_keys=True))
        return
    rows = {}
    for name, m in stats.items():
        live = [(t, c) for c, t in enumerate(m["tau"]) if t == t]                 # (a constant chain has no tau)
        lo, hi = (min(live), max(live)) if live else ((float("nan"), -1), (float("nan"), -1))
        rows[name] = {"tau": m["tau_pooled"], "window": m["window_pooled"], "ess_pooled": m["ess_pooled"],
                      "tau_min": lo[0], "chain_min": lo[1], "tau_max": hi[0], "chain_max": hi[1]}
    headers = ["param", "tau", "window", "ess_pooled", "tau_min", "chain_min", "tau_max", "chain_max"]
    widths = [max(len(h), 6) for h in headers]
    click.echo(" ".join(h.ljust(w) for h, w in zip(headers, widths, strict=False)))
    for name, m in rows.items():
        row = [name] + [f"{m[h]:.6g}" for h in headers[1:]]
        click.echo(" ".join(v.ljust(w) for v, w in zip(row, widths, strict=False)))


@main.command("diagnostics")
@click.argument("model")
@click.option("--format", "format_", type=click.Choice(["table", "csv", "json"], case_sensitive=False), default="table")
def diagnostics_cmd(model: str, format_: str) -> None:
    diag = reference.diagnostics_for_model(model)
    if format_ == "json":
        click.echo(json.dumps(diag, indent=2, sort_keys=True))
    elif format_ == "csv":
        click.echo("param,rhat,ess_bulk,ess_tail")
        for param, m in diag.items():
            click.echo(",".join([param, str(m.get("rhat")), str(m.get("ess_bulk")), str(m.get("ess_tail"))]))
    else:
        _print_table(diag)


@main.command("info")
@click.argument("model")
def info_cmd(model: str) -> None:
    click.echo(json.dumps(DataStore().read_meta(model), indent=2, sort_keys=True))


def _read_actual_csv(path: Path) -> dict[str, list[float]]:
    import pyarrow.csv as pacsv
    table = pacsv.read_csv(path)
    return {p: [float(v) for v in table.column(p).to_pylist()]
            for p in table.column_names if p not in {"chain", "draw"}}


@main.command("compare")
@click.argument("model")
@click.option("--actual", "actual_path", type=click.Path(path_type=Path), required=True)
@click.option("--tolerance", default=0.15, type=float)
@click.option("--format", "format_", type=click.Choice(["table", "json"], case_sensitive=False), default="table")
def compare_cmd(model: str, actual_path: Path, tolerance: float, format_: str) -> None:
    result = reference.compare(model, actual=_read_actual_csv(actual_path), tolerance=tolerance)
    if format_ == "json":
        details = {p: {k: vars(v) for k, v in ms.items()} for p, ms in result.details.items()}
        click.echo(json.dumps({"passed": result.passed, "failures": result.failures, "details": details},
                              indent=2, sort_keys=True))
    else:
        click.echo("passed" if result.passed else "failed")
        for failure in result.failures:
            click.echo(f"- {failure}")
    raise SystemExit(0 if result.passed else 2)


@main.command("validate")
@click.argument("model")
@click.option("--actual", "actual_path", type=click.Path(path_type=Path), required=True)
@click.option("--tolerance", default=0.15, type=float)
@click.option("--metrics", default="mean,std", help="Comma-separated metrics of the relative-error gate")
@click.option("--ks-max", default=None, type=float, help="Fail a parameter whose two-sample KS statistic exceeds this")
@click.option("--w1-scaled-max", default=None, type=float, help="Fail a parameter whose W1 / reference std exceeds this")
@click.option("--sliced", default=0, type=click.IntRange(min=0), help="Random directions of the joint (sliced) KS / W1 check")
@click.option("--sliced-seed", default=4711, type=int)
@click.option("--sliced-ks-max", default=None, type=float, help="Fail when the largest sliced KS exceeds this")
@click.option("--sliced-w1-max", default=None, type=float, help="Fail when the largest sliced W1 exceeds this")
@click.option("--khat-max", default=None, type=float, help="Fail a parameter whose Pareto k-hat of the actual draws exceeds this")
@click.option("--hdi-prob", default=None, type=float, help="Report the highest-density intervals of this share of both samples")
@click.option("--hdi-tol", default=None, type=float,
              help="Fail a parameter whose HDI endpoints differ by more than this share of the reference interval's width")
@click.option("--energy", is_flag=True, help="Energy distance of the standardised joint draws (direction-free joint check)")
@click.option("--energy-max", default=None, type=float, help="Fail when the energy distance exceeds this (implies --energy)")
@click.option("--energy-max-draws", default=None, type=click.IntRange(min=1),
              help="Thin each sample by an even stride to at most this many draws first (the cost is quadratic)")
@click.option("--gaussian", is_flag=True, help="Joint Gaussian check: Mahalanobis distance of the mean shift, KL of the two Gaussian fits")
@click.option("--gaussian-jitter", default=0.0, type=float, help="Added to the diagonal of both standardised covariance matrices")
@click.option("--gaussian-shift-max", default=None, type=float, help="Fail when the Mahalanobis distance exceeds this (implies --gaussian)")
@click.option("--gaussian-kl-max", default=None, type=float, help="Fail when the symmetrised KL exceeds this (implies --gaussian)")
@click.option("--format", "format_", type=click.Choice(["table", "json"], case_sensitive=False), default="table")
def validate_cmd(model: str, actual_path: Path, tolerance: float, metrics: str, ks_max, w1_scaled_max, sliced: int, sliced_seed: int,
                 sliced_ks_max, sliced_w1_max, khat_max, hdi_prob, hdi_tol, energy: bool, energy_max, energy_max_draws,
                 gaussian: bool, gaussian_jitter: float, gaussian_shift_max, gaussian_kl_max, format_: str) -> None:
    """The reference's mean / std gate plus per-parameter KS / Wasserstein-1 and, with --sliced K, the same distances
    along K random directions of the joint distribution; with --energy the energy distance of the joint draws;
    with --gaussian the Mahalanobis distance of the mean shift and the KL divergences of the two Gaussian fits
    (validate.validate; no counterpart in the reference)."""
    from .validate import validate
    with_gaussian = gaussian or gaussian_shift_max is not None or gaussian_kl_max is not None
    try:
        result = validate(model, _read_actual_csv(actual_path), tolerance=tolerance, metrics=tuple(metrics.split(",")),
                          ks_max=ks_max, w1_scaled_max=w1_scaled_max, sliced=sliced, sliced_seed=sliced_seed,
                          sliced_ks_max=sliced_ks_max, sliced_w1_max=sliced_w1_max, khat_max=khat_max,
                          hdi_prob=hdi_prob, hdi_tol=hdi_tol, energy=energy or energy_max is not None, energy_max=energy_max,
                          energy_max_draws=energy_max_draws,
                          **({"gaussian": True, "gaussian_jitter": gaussian_jitter, "gaussian_shift_max": gaussian_shift_max,
                              "gaussian_kl_max": gaussian_kl_max} if with_gaussian else {}))
    except ValueError as exc:
        raise click.ClickException(str(exc)) from exc
    with_hdi = hdi_prob is not None or hdi_tol is not None
    if format_ == "json":
        details = {p: {k: vars(v) for k, v in ms.items()} for p, ms in result.compare.details.items()}
        hdi_keys = {"hdi_ref": result.hdi_ref, "hdi_actual": result.hdi_actual} if with_hdi else {}    # only when asked for
        if with_gaussian:
            hdi_keys.update(gaussian=result.gaussian, gaussian_shift=result.gaussian_shift)
        click.echo(json.dumps({**hdi_keys, "passed": result.passed, "failures": result.failures,
                               "compare": {"passed": result.compare.passed, "failures": result.compare.failures,
                                           "details": details},
                               "ks": result.ks, "wasserstein": result.wasserstein,
                               "wasserstein_scaled": result.wasserstein_scaled, "sliced_ks": result.sliced_ks,
                               "sliced_w1": result.sliced_w1, "sliced": result.sliced, "khat_ref": result.khat_ref,
                               "khat_actual": result.khat_actual, "energy": result.energy,
                               "energy_detail": result.energy_detail}, indent=2, sort_keys=True))
    else:
        click.echo("passed" if result.passed else "failed")
        for failure in result.failures:
            click.echo(f"- {failure}")
        if khat_max is not None:               # the two k-hat columns (the JSON form always has them)
            _print_table({p: {"khat_ref": result.khat_ref[p], "khat_actual": result.khat_actual[p]} for p in result.khat_actual})
        if with_hdi:
            _print_table({p: {"hdi_lo_ref": result.hdi_ref[p][0], "hdi_hi_ref": result.hdi_ref[p][1],
                              "hdi_lo_actual": result.hdi_actual[p][0], "hdi_hi_actual": result.hdi_actual[p][1]}
                          for p in result.hdi_actual})
        if with_gaussian and result.gaussian is not None:
            _print_gaussian(result.gaussian)
    raise SystemExit(0 if result.passed else 2)


def _print_gaussian(g: dict) -> None:
    click.echo(f"gaussian shift {g['mahalanobis']:.6g}  kl_act_ref {g['kl_act_ref']:.6g}  kl_ref_act {g['kl_ref_act']:.6g}  "
               f"kl_sym {g['kl_sym']:.6g}  params {g['p_live']}")
    for key in ("singular_ref", "singular_actual"):
        if g.get(key) is not None:
            click.echo(f"{key} {g[key]}")
    _print_table({p: {"shift": v} for p, v in g["shift"].items()})


@main.command("gaussian-check")
@click.argument("ref_file", type=click.Path(path_type=Path, exists=True, dir_okay=False))
@click.argument("act_file", type=click.Path(path_type=Path, exists=True, dir_okay=False))
@click.option("--params", default=None, help="Comma-separated parameter list (default: the reference file's)")
@click.option("--jitter", default=0.0, type=float, help="Added to the diagonal of both standardised covariance matrices")
@click.option("--format", "format_", type=click.Choice(["table", "json"], case_sensitive=False), default="table")
def gaussian_check_cmd(ref_file: Path, act_file: Path, params: str | None, jitter: float, format_: str) -> None:
    """Joint Gaussian check of the draws in ACT_FILE against those in REF_FILE (no counterpart in the reference): the
    Mahalanobis distance of the mean shift in the reference's metric, the KL divergences of the two Gaussian fits, and
    every parameter's shift given the ones before it, in conditional standard deviations."""
    try:
        r = convert_mod.gaussian_check_files(ref_file, act_file, params=params.split(",") if params else None, jitter=jitter)
    except (ValueError, KeyError, IndexError) as exc:
        raise click.ClickException(str(exc)) from exc
    if format_ == "json":
        click.echo(json.dumps(r, indent=2, sort_keys=True))
    else:
        _print_gaussian(r)


@main.command("convert")
@click.argument("input_path", type=click.Path(path_type=Path))
@click.option("--name", required=True)
@click.option("--force", is_flag=True)
def convert_cmd(input_path: Path, name: str, force: bool) -> None:
    from .store import default_local_root
    local_root = default_local_root()
    draws_dir, meta_dir = local_root / "draws", local_root / "meta"
    draws_dir.mkdir(parents=True, exist_ok=True)
    meta_dir.mkdir(parents=True, exist_ok=True)
    convert_mod.convert_file(input_path, name=name, out_draws_dir=draws_dir, out_meta_dir=meta_dir, force=force)
    click.echo(f"converted {name} -> {draws_dir}")


@main.command("provenance-generate")
@click.option("--scaffold-root", type=click.Path(path_type=Path), required=True)
@click.option("--output-root", type=click.Path(path_type=Path), required=True)
@click.option("--models", default=None, help="Optional comma-separated recipe names.")
@click.option("--force", is_flag=True, help="Forward --force to convert quality checks.")
@click.option("--fake-runner", is_flag=True, help="Use deterministic fake runner (testing only).")
def provenance_generate_cmd(scaffold_root: Path, output_root: Path, models: str | None, force: bool,
                            fake_runner: bool) -> None:
    """Sampler archives -> draws/meta for every recipe of a scaffold (reference cli.py:248-274); the diagnostics of all
    models run as one pipelined batch on the GPU."""
    result = generate_mod.generate_reference_corpus(
        scaffold_root=scaffold_root, output_root=output_root, models=models.split(",") if models else None,
        force=force, runner=generate_mod.fake_jsonzip_runner if fake_runner else None)
    click.echo(f"generated={result.generated} failed={result.failed} output={result.output_root}")
    if result.errors:
        for name, message in sorted(result.errors.items()):
            click.echo(f"- {name}: {message}")
        raise SystemExit(1)


@main.command("provenance-publish")
@click.option("--source-root", type=click.Path(path_type=Path), required=True)
@click.option("--scaffold-root", type=click.Path(path_type=Path), required=True)
@click.option("--package-root", type=click.Path(path_type=Path), required=True)
def provenance_publish_cmd(source_root: Path, scaffold_root: Path, package_root: Path) -> None:
    result = generate_mod.publish_reference_data(source_root=source_root, scaffold_root=scaffold_root,
                                                 package_root=package_root)
    click.echo(f"published draws={result.draws_copied} meta={result.meta_copied} pairs={result.pairs_copied} "
               f"to={result.package_root}")


if __name__ == "__main__":
    main()

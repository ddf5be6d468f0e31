"""Python API for reference draws, with the statistics on the GPU.

Same surface as the reference's src/mcmc_ref/reference.py:15-122 (`list_models`, `stan_data`,
`model_code`, `stats`, `draws`, `diagnostics_for_model`, `compare`); the default backend is "hip".
`summary_for_model` is an addition: stats and diagnostics of a model from ONE kernel pipeline.
"""
from __future__ import annotations

import os
from collections.abc import Mapping, Sequence

from . import _ffi, convert
from .backends import get_backend
from .compare import compare_stats, compute_stats_from_draws
from .draws import Draws, coerce_return
from .store import DataStore


def list_models(store: DataStore | None = None) -> list[str]:
    return (store or DataStore()).list_models()


def stan_data(model: str, store: DataStore | None = None) -> dict:
    return (store or DataStore()).read_stan_data(model)


def model_code(model: str, store: DataStore | None = None) -> str:
    return (store or DataStore()).read_stan_code(model)


def _table_and_params(store: DataStore, model: str, params):
    table = store.open_draws(model, params=params).read_all()
    if params is None:
        params = [c for c in table.column_names if c not in {"chain", "draw"}]
    return table, list(params)


def _native_reader() -> bool:
    """The "hip" backend reads `draws/<model>.draws.parquet` with the library's own Parquet ingest (decode on the
    GPU, no pyarrow) unless MCMC_REF_HIP_READER=arrow asks for the reference's pyarrow route."""
    return os.environ.get("MCMC_REF_HIP_READER", "native").lower() != "arrow"


def _native_summaries(store: DataStore, models: Sequence[str], params, *, diagnostics: bool, min_chains: int = 4):
    from . import parquet
    ctx = _ffi.default_context()
    paths = [store.resolve_draws_path(m) for m in models]
    try:
        return parquet.summarize_files(ctx, paths, [params] * len(paths), min_chains=min_chains,
                                       diagnostics=diagnostics)
    except KeyError as exc:                      # unknown column: the same exception type pyarrow's path ends in
        raise KeyError(str(exc)) from exc


def stats(model: str, params: Sequence[str] | None = None, backend: str = "hip", quantile_mode: str = "exact",
          store: DataStore | None = None) -> dict[str, dict[str, float]]:
    """Summary statistics (mean, std, q5, q50, q95) of a model's reference draws."""
    store = store or DataStore()
    if backend == "hip" and _native_reader():
        get_backend(backend)                     # ImportError without the library / a device, as for any backend
        return _native_summaries(store, [model], params, diagnostics=False)[0]
    table, params = _table_and_params(store, model, params)
    return get_backend(backend).stats(table, params, quantile_mode=quantile_mode)


def summaries_for_models(models: Sequence[str], store: DataStore | None = None, min_chains: int = 4
                         ) -> dict[str, dict[str, dict[str, float]]]:
    """All statistics of many models from one batched Parquet decode + pipelined kernel passes
    (an addition; the reference loops `stats` / `diagnostics_for_model` per model)."""
    store = store or DataStore()
    out = _native_summaries(store, list(models), None, diagnostics=True, min_chains=min_chains)
    return dict(zip(models, out))


def draws(model: str, params: Sequence[str] | None = None, chains: Sequence[int] | None = None,
          return_: str = "arrow", store: DataStore | None = None):
    """return_: "arrow" | "draws" | "numpy" | "list" (as in the reference)."""
    store = store or DataStore()
    reader = store.open_draws(model, params=params, chains=chains)
    if params is None:
        reader = reader.read_all()
        params = [c for c in reader.column_names if c not in {"chain", "draw"}]
    return coerce_return(Draws(data=reader, params=list(params), chains=list(chains) if chains else None), return_)


def _host_writer() -> bool:
    return os.environ.get("MCMC_REF_HIP_WRITER", "native").lower() == "arrow"


def _export_arrow(model, dest, params, chains, format_, store) -> None:
    """The reference's route (src/mcmc_ref/cli.py:113-127): pyarrow reads, filters and writes."""
    import pyarrow.csv as pacsv
    import pyarrow.parquet as pq
    data = draws(model, params=params, chains=chains, return_="arrow", store=store)
    table = data.read_all() if hasattr(data, "read_all") else data      # (write_csv of current pyarrow takes no reader)
    if format_ == "parquet":
        pq.write_table(table, dest)
    elif hasattr(dest, "write"):
        pacsv.write_csv(table, dest)
    else:
        with open(dest, "wb") as fh:
            pacsv.write_csv(table, fh)


def export_draws(model: str, dest, params: Sequence[str] | None = None, chains: Sequence[int] | None = None,
                 format_: str = "csv", store: DataStore | None = None, context=None, writer: str = "auto") -> None:
    """A model's draws as CSV or Parquet into `dest` (a path or a binary file object): what the reference's `draws`
    command writes (src/mcmc_ref/cli.py:100-127), byte for byte for CSV.

    The file is decoded on the device, id columns included, in file row order; the columns are `chain`, `draw` and
    `params` in that order (None: the file's columns without the ids, as the reference's scanner selects them); `chains`
    keeps the rows whose chain id is listed (`ds.field("chain").isin(chains)`: a given but empty list keeps none), selected
    on the device; the text is formatted on the device (parquet.write_csv_dev), the Parquet file encoded there.

    writer="host" or MCMC_REF_HIP_WRITER=arrow takes the reference's route (`draws(..., return_="arrow")`, then
    pyarrow.csv.write_csv / pq.write_table).  So do, whatever the writer: files the device reader rejects by name;
    files with a selected column that is neither INT32, INT64 nor DOUBLE -- a FLOAT column among them, which pyarrow
    prints as shortest float32; and format_="parquet" with a chain selection (the Parquet writer takes no row list)."""
    if format_ not in ("csv", "parquet"):
        raise ValueError(f"format_ must be 'csv' or 'parquet', got {format_!r}")
    if writer not in ("auto", "device", "host"):
        raise ValueError(f"writer must be 'auto', 'device' or 'host', got {writer!r}")
    store = store or DataStore()
    if writer == "host" or (writer == "auto" and _host_writer()) or (format_ == "parquet" and chains is not None):
        return _export_arrow(model, dest, params, chains, format_, store)
    from . import parquet
    ctx = context or _ffi.default_context()
    try:
        f = parquet.ParquetFile(store.resolve_draws_path(model), ctx)
    except _ffi.McrError:                             # a file outside the device reader's subset: it names the feature
        return _export_arrow(model, dest, params, chains, format_, store)
    with f:
        names = ["chain", "draw", *(params if params is not None else
                                    [n for n in f.column_names if n not in ("chain", "draw")])]
        try:
            types = [f.column_types[f.index(n)] for n in names]
        except KeyError:                              # pyarrow's exception for an unknown column
            return _export_arrow(model, dest, params, chains, format_, store)
        if any(t not in (_ffi.MCR_PQ_INT32, _ffi.MCR_PQ_INT64, _ffi.MCR_PQ_DOUBLE) for t in types):
            return _export_arrow(model, dest, params, chains, format_, store)
        M = f.num_rows
        try:
            buf, kinds = parquet.decode_columns(ctx, f, names)
        except _ffi.McrError as exc:
            if exc.code != _ffi.MCR_EINVAL:
                raise
            return _export_arrow(model, dest, params, chains, format_, store)
    with buf:
        cols = [_ffi.pq_column(n, t, buf.ptr.value + j * M * 8, 1, _ffi.MCR_PQW_I64 if k == _ffi.MCR_PQ_I64 else _ffi.MCR_PQW_F64)
                for j, (n, t, k) in enumerate(zip(names, types, kinds))]
        if format_ == "parquet":
            if M == 0:                                # (the Parquet writer wants a row)
                return _export_arrow(model, dest, params, chains, format_, store)
            with ctx.write_parquet(cols, M) as image:
                parquet._write_view(dest, image.view)
        elif chains is None:
            parquet.write_csv_dev(ctx, dest, cols, M)
        else:
            rows, n = ctx.select_rows(buf.ptr.value, M, [int(c) for c in chains])
            with rows:
                parquet.write_csv_dev(ctx, dest, cols, M, row_index=(rows, n))
    return None


def diagnostics_for_model(model: str, params: Sequence[str] | None = None,
                          store: DataStore | None = None) -> dict[str, dict[str, float]]:
    """meta.json's cached diagnostics when present (reference.py:82-90), else computed on the GPU for
    all parameters in one pipeline."""
    store = store or DataStore()
    try:
        meta = store.read_meta(model)
    except FileNotFoundError:
        meta = {}
    diag = meta.get("diagnostics")
    if isinstance(diag, dict) and diag:
        return diag if params is None else {p: diag[p] for p in params if p in diag}
    if _native_reader():
        full = _native_summaries(store, [model], params, diagnostics=True)[0]
        return {p: {k: v[k] for k in _ffi.DIAG_KEYS} for p, v in full.items()}
    table, params = _table_and_params(store, model, params)
    return convert._compute_diagnostics(table, params)


def summary_for_model(model: str, params: Sequence[str] | None = None, store: DataStore | None = None,
                      min_chains: int = 4) -> dict[str, dict[str, float]]:
    """mean, std, q5, q50, q95, rhat, ess_bulk, ess_tail per parameter from one pass of the kernels."""
    store = store or DataStore()
    if _native_reader():
        return _native_summaries(store, [model], params, diagnostics=True, min_chains=min_chains)[0]
    table, params = _table_and_params(store, model, params)
    return convert.summarize_table(table, params, min_chains=min_chains)


def compare(model: str, actual: Mapping[str, Sequence[float]], tolerance: float = 0.15,
            metrics: Sequence[str] = ("mean", "std"), backend: str = "hip", store: DataStore | None = None):
    """Compare actual draws against the reference statistics (reference.py:107-122)."""
    ref_stats = stats(model, params=list(actual.keys()), backend=backend, store=store)
    actual_stats = compute_stats_from_draws(actual)
    return compare_stats(ref_stats, actual_stats, tolerance=tolerance, metrics=metrics)

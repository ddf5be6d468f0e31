"""The diagnostics call site of the conversion pipeline, batched for the GPU.

Mirrors the hot-path part of src/mcmc_ref/convert.py: `_chains_from_table` (:150-161, here a
whole-table integer gather `table_to_tensor`), `_count_chains_draws` (:123-131),
`_compute_diagnostics` (:134-147, one kernel pipeline per model instead of a Python loop per
parameter), `_checks` (:164-172) and `_enforce_checks` (:175-178).
"""
from __future__ import annotations

import contextlib
import json
import math
import time
import zipfile
from collections.abc import Iterable
from dataclasses import dataclass
from datetime import date
from pathlib import Path
from typing import Any, NamedTuple

import numpy as np

from . import _ffi
from .backends import columns_to_matrix


def _col(table: Any, name: str) -> np.ndarray:
    if hasattr(table, "column"):
        col = table.column(name)
        return np.asarray(col.to_numpy(zero_copy_only=False) if hasattr(col, "to_numpy") else col)
    return np.asarray(table[name])


def chain_layout(table: Any):
    """Integer bookkeeping of the long table: (chain ids sorted, row order, per-chain lengths).

    order[k] = row index of the k-th draw in (chain id asc, draw idx asc) order, which is how
    `_chains_from_table` orders values (robust to unordered rows).
    """
    if hasattr(table, "read_all"):
        table = table.read_all()
    chain = _col(table, "chain").astype(np.int64)
    draw = _col(table, "draw").astype(np.int64)
    ids, counts = np.unique(chain, return_counts=True)
    already = chain.size == 0 or (np.all(np.diff(chain) >= 0) and
                                  all(np.all(np.diff(draw[s:s + n]) >= 0)
                                      for s, n in zip(np.concatenate([[0], np.cumsum(counts)[:-1]]), counts)))
    order = None if already else np.lexsort((draw, chain))     # stable: ties keep row order, like sorted()
    return ids, order, counts


def table_to_tensor(table: Any, params: Iterable[str]):
    """Returns (x, counts): x is [P][M] float64 in (chain, draw) order; counts = draws per chain."""
    if hasattr(table, "read_all"):
        table = table.read_all()
    params = list(params)
    _, order, counts = chain_layout(table)
    x = columns_to_matrix(table, params)
    if order is not None and x.size:
        x = np.ascontiguousarray(x[:, order])
    return x, counts


def _count_chains_draws(table: Any) -> tuple[int, int]:
    _, _, counts = chain_layout(table)
    return int(len(counts)), int(counts.min()) if len(counts) else 0


def _compute_diagnostics(table: Any, params: Iterable[str], *, min_chains: int = 4,
                         context=None) -> dict[str, dict[str, float]]:
    params = list(params)
    if min_chains < 1:
        raise ValueError(f"min_chains must be >= 1; got {min_chains}")
    if not params:
        return {}
    x, counts = table_to_tensor(table, params)
    C = len(counts)
    if C < min_chains:
        raise ValueError(f"R-hat diagnostics require at least {min_chains} chains; got {C} chain(s)")
    ctx = context or _ffi.default_context()
    with _ffi.value_errors():
        if np.all(counts == counts[0]):
            r = ctx.summarize(x.reshape(len(params), C, int(counts[0])), "pcn", min_chains=min_chains, quantiles=())
        else:                                       # ragged chains: one batched call (mcr_summarize_chains_dev)
            r = _ffi.ragged_diagnostics(ctx, x, counts, min_chains)
    return dict(zip(params, _ffi.entries(r)))


def summarize_table(table: Any, params: Iterable[str], *, min_chains: int = 4, context=None,
                    quantiles=(0.05, 0.5, 0.95)) -> dict[str, dict[str, float]]:
    """Backend.stats + diagnostics of every parameter of a long table from ONE kernel pipeline."""
    params = list(params)
    if not params:
        return {}
    x, counts = table_to_tensor(table, params)
    C = len(counts)
    if C == 0 or not np.all(counts == counts[0]):
        raise ValueError("summarize_table needs chains of equal length")
    ctx = context or _ffi.default_context()
    qs = list(quantiles)
    with _ffi.value_errors():
        r = ctx.summarize(x.reshape(len(params), C, int(counts[0])), "pcn", min_chains=min_chains, quantiles=qs)
    return dict(zip(params, _ffi.entries(r, qs)))


def _checks(n_chains: int, n_draws: int, diag: dict[str, dict[str, float]]) -> dict[str, bool]:
    ess_ok = all(values.get("ess_bulk", 0.0) > 400 for values in diag.values())
    rhat_ok = all(values.get("rhat", 1.0) < 1.01 for values in diag.values())
    return {
        "ndraws_is_10k": n_chains * n_draws == 10_000,
        "nchains_is_gte_4": n_chains >= 4,
        "ess_above_400": ess_ok,
        "rhat_below_1_01": rhat_ok,
    }


def _enforce_checks(checks: dict[str, bool]) -> None:
    failures = [name for name, ok in checks.items() if not ok]
    if failures:
        raise ValueError(f"quality checks failed: {', '.join(failures)}")


# ---- file conversion (reference src/mcmc_ref/convert.py:26-120): JSON-zip / CSV -> Parquet + meta ----
@dataclass(frozen=True)
class ConvertResult:
    draws_path: Path
    meta_path: Path
    meta: dict


def _read_json_zip(path: Path):
    """Chain-list JSON-zip: [ {param: [draws...]}, ... ] (one dict per chain) -> long Arrow table.

    As the reference builds it (convert.py:78-102): parameters in sorted order, `n_draws` taken from the first chain's
    first parameter, longer chains cut at `n_draws`, a SHORTER chain is an IndexError, and a column keeps the type its
    JSON numbers have (all-integer draws stay int64 in the written Parquet file, any float makes it double)."""
    import pyarrow as pa
    with zipfile.ZipFile(path) as zf:
        payload = json.loads(zf.read(zf.namelist()[0]))
    if not isinstance(payload, list) or not payload:
        raise ValueError("json-zip payload must be a non-empty list of chains")
    params = sorted(payload[0].keys())
    n_draws = len(next(iter(payload[0].values())))
    n_chains = len(payload)
    cols = {"chain": np.repeat(np.arange(n_chains, dtype=np.int64), n_draws),
            "draw": np.tile(np.arange(n_draws, dtype=np.int64), n_chains)}
    for p in params:
        parts = []
        for ch in payload:
            if n_draws and len(ch[p]) < n_draws:
                raise IndexError("list index out of range")
            parts.append(np.asarray(ch[p][:n_draws]))
        col = np.concatenate(parts) if n_draws else np.empty(0)
        if col.dtype.kind not in "iuf":           # bools / None / strings: let pyarrow infer (and refuse) as it would
            col = [v for part in parts for v in part.tolist()]
        cols[p] = col
    return pa.table(cols)


def _is_json_zip(path: Path) -> bool:
    return path.suffixes[-2:] == [".json", ".zip"]


def _select_json_arrays(keys: list[list[str]], lengths: list[list[int]]):
    """The reference's choice of arrays (convert.py:78-102) from the keys and array lengths of every chain, in document
    order: (sorted keys of chain 0, n_draws = length of chain 0's document-first array, key index [C][P]).  None where
    `_read_json_zip` raises or leaves the plain path: no parameter at all, a parameter named like a bookkeeping column,
    a chain without one of the parameters (KeyError), an array shorter than n_draws (IndexError)."""
    if not keys[0] or {"chain", "draw"} & set(keys[0]):
        return None
    params = sorted(keys[0])
    n_draws = lengths[0][0]
    arrays = []
    for ks, ls in zip(keys, lengths):
        at = {k: i for i, k in enumerate(ks)}
        if any(p not in at or ls[at[p]] < n_draws for p in params):
            return None
        arrays.append([at[p] for p in params])
    return params, n_draws, arrays


def read_json_zip_dev(path: Path, context=None, phases: dict | None = None):
    """`_read_json_zip` without the host parse: (params, [P][C][N] DeviceTensor, int_columns) of a chain-list JSON-zip.
    The member is inflated here, its text is indexed and every selected number converted on the GPU (mcr_json_*), by
    the reference's rules: params sorted, n_draws from chain 0's document-first key, longer arrays cut, extra keys of
    later chains ignored.  int_columns[p]: every draw of the parameter is an integer literal, the column the host
    reader leaves int64.  None when the host reader must decide -- the document is outside the subset the device
    reader certifies, or it is one for which `_read_json_zip` raises (`phases["fallback"]` says why).  `phases`
    receives the host clock of the steps (ms) and `hard`, the numbers the host had to finish.  Free the tensor."""
    note = phases if phases is not None else {}
    t0 = time.perf_counter()
    try:
        with zipfile.ZipFile(path) as zf:
            text = zf.read(zf.namelist()[0])
    except Exception as exc:  # noqa: BLE001 - the host reader raises it again
        note["fallback"] = f"{type(exc).__name__}: {exc}"
        return None
    note["inflate_ms"] = (time.perf_counter() - t0) * 1e3
    ctx = context if context is not None else _ffi.default_context()
    with _ffi.value_errors():
        got = ctx.json_decode(text, _select_json_arrays, note)
    if got is None:
        note.setdefault("fallback", "the reference's reader raises for this document")
        return None
    params, t, all_int, _hard = got
    n_draws = t.shape_cnp[1]
    return params, t, [bool(n_draws and col.all()) for col in all_int.T]


def _json_table(params: list[str], flat: np.ndarray, n_chains: int, n_draws: int, int_columns: list[bool]):
    """The Arrow table `_read_json_zip` builds, from the downloaded [P][C * N] draws."""
    import pyarrow as pa
    cols = {"chain": np.repeat(np.arange(n_chains, dtype=np.int64), n_draws),
            "draw": np.tile(np.arange(n_draws, dtype=np.int64), n_chains)}
    for p, row, is_int in zip(params, flat, int_columns):
        cols[p] = row.astype(np.int64) if is_int else row
    return pa.table(cols)


def _writer_choice(writer: str) -> str:
    """"auto" or "host" of convert_files' `writer`; the environment variable MCMC_REF_HIP_WRITER=arrow forces "host".
    "auto" has no size threshold: text to both files, median [range] of 9 alternating runs on one MI355X
    (profiles/parquet_write.json), the device writer took 36.5 ms [34.0 - 43.5] against 150 ms [145 - 158] at
    4 x 10 000 x 100 and 1.60 ms [1.50 - 2.50] against 2.34 ms [2.23 - 2.63] at 4 x 1 000 x 10."""
    import os
    if writer not in ("auto", "host"):
        raise ValueError(f"writer must be 'auto' or 'host'; got {writer!r}")
    return "host" if os.environ.get("MCMC_REF_HIP_WRITER", "") == "arrow" else writer


def _json_image(ctx, params: list[str], t, int_columns: list[bool]):
    """The draws file `_json_table` + pq.write_table give, encoded on the device from the resident [P][C][N] tensor
    (Context.write_parquet): chain and draw generated, a parameter int64 where every draw is an integer literal."""
    _, n_chains, n_draws, _P, stride_c, stride_n, stride_p = t.targs
    if stride_c != n_draws * stride_n:
        return None                                        # rows of a parameter not evenly spaced: the table route
    cols = [_ffi.pq_sequence("chain", _ffi.MCR_PQ_INT64, div=n_draws), _ffi.pq_sequence("draw", _ffi.MCR_PQ_INT64, mod=n_draws)]
    base = t.buf.ptr.value
    for k, (p, is_int) in enumerate(zip(params, int_columns)):
        cols.append(_ffi.pq_column(p, _ffi.MCR_PQ_INT64 if is_int else _ffi.MCR_PQ_DOUBLE, base + 8 * k * stride_p, stride_n,
                                   _ffi.MCR_PQW_F64))
    with _ffi.value_errors():
        return ctx.write_parquet(cols, n_chains * n_draws)


def _upload_draws(ctx, x: np.ndarray, counts, P: int):
    """The DeviceTensor of host draws x [P][M] in (chain, draw) order whose chains are `counts` draws long: [P][C][N]
    where they are equally long, else the ragged tensor of Context.ragged_tensor.  Free it."""
    if np.all(counts == counts[0]):
        return ctx.upload(x.reshape(P, len(counts), int(counts[0])), "pcn")
    xc = np.ascontiguousarray(x, dtype=np.float64)
    with contextlib.ExitStack() as stack:
        buf = stack.enter_context(_ffi.DeviceBuffer(ctx, max(xc.nbytes, 8))).upload(xc)
        stack.pop_all()
    return ctx.ragged_tensor(buf, counts, P)


@dataclass
class _Prepared:
    """One job of convert_files, read and laid out.  What is written: the Arrow `table`, or the `image` of the draws
    file encoded on the device.  What the diagnostics read: the host matrix `x` [P][M], or the resident `tensor`
    (convert_files puts the upload of `x` there too).  close() frees the image and the tensor."""
    params: list
    n_chains: int
    n_draws: int
    counts: np.ndarray
    table: Any = None
    image: Any = None
    x: Any = None
    tensor: Any = None

    def close(self):
        if self.image is not None:
            self.image.close()
        if self.tensor is not None:
            self.tensor.free()


def _read_json_zip_prepared(path: Path, min_chains: int, context, writer: str = "host"):
    """A `.json.zip` input of convert_files through the device reader: the `_Prepared` entry with the draws resident, or
    None for the host route.  writer="auto": the entry holds the encoded draws file in place of the table, and nothing
    is downloaded."""
    try:
        ctx = context or _ffi.default_context()
    except _ffi.HipUnavailableError:
        return None
    got = read_json_zip_dev(path, context=ctx)
    if got is None:
        return None
    params, t, int_columns = got
    with contextlib.ExitStack() as stack:
        stack.enter_context(t)
        _, n_chains, n_draws, P = t.targs[:4]
        if n_draws == 0:                                   # nothing to parse: the host reader's empty table
            return None
        if n_chains < min_chains:
            raise ValueError(f"R-hat diagnostics require at least {min_chains} chains; got {n_chains} chain(s)")
        table, image = None, _json_image(ctx, params, t, int_columns) if writer == "auto" else None
        if image is None:
            flat = t.buf.download(np.float64, P * n_chains * n_draws).reshape(P, n_chains * n_draws)
            table = _json_table(params, flat, n_chains, n_draws, int_columns)
        stack.pop_all()
        return _Prepared(params, n_chains, n_draws, np.full(n_chains, n_draws), table=table, image=image, tensor=t)


def summarize_json_zip(path: Path, min_chains: int = 4, quantiles=(0.05, 0.5, 0.95), diagnostics: bool = True,
                       context=None) -> dict[str, dict[str, float]]:
    """{param: {"mean", "std", "qNN"..., "rhat", "ess_bulk", "ess_tail"}} of a chain-list JSON-zip, the shape
    `reference.summary_for_model` returns: text to statistics on the GPU.  A document for the host reader is read by it
    (and raises what it raises) and its tensor uploaded."""
    ctx = context if context is not None else _ffi.default_context()
    got = read_json_zip_dev(Path(path), context=ctx)
    if got is None:
        table = _read_json_zip(Path(path))
        params = [c for c in table.column_names if c not in {"chain", "draw"}]
        x, counts = table_to_tensor(table, params)
        if not params or len(counts) == 0:
            return {}
        with _ffi.value_errors():
            t = _upload_draws(ctx, x, counts, len(params))
    else:
        params, t, _ints = got
    with t, _ffi.value_errors():
        r = ctx.summarize(t, min_chains=min_chains, quantiles=quantiles, diagnostics=diagnostics)
    return dict(zip(params, _ffi.entries(r, list(quantiles), diagnostics)))


class CsvDraws(NamedTuple):
    """One file of read_csv_many_dev.  close() frees the draws and the file-order buffer (they may share memory)."""
    draws: Any             # parquet.DeviceDraws: [P][M] in (chain, draw) order, chain ids, counts
    file_order: Any        # the [P][M] f64 values in FILE row order
    int_columns: list      # per parameter: every literal of the column is an integer
    header: list           # every column name of the file
    ids: tuple             # the downloaded (chain, draw) columns, None for an absent one

    def close(self):
        self.draws.free()
        self.file_order.free()


def _csv_draws(ctx, got: "_ffi.CsvTable", note: dict) -> CsvDraws:
    """One file of Context.csv_table_decode with its rows put in (chain, draw) order (parquet.draws_in_order).  A missing
    `chain` is chain 0 and a missing `draw` the row number (`_ensure_chain_draw`); without both the rows are in order as
    they stand.  Takes over `got`: it is closed here, and what is returned holds views of its own."""
    from . import parquet
    names, buf, ints, (chain, draw), _hard, header = got
    M = buf.nbytes // 8 // len(names) if names else (chain or draw).nbytes // 8
    with contextlib.ExitStack() as stack, contextlib.ExitStack() as handed:
        stack.callback(got.close)                         # the draws and the file-order buffer hold views of their own
        known, order, ptrs = None, None, [None if b is None else b.ptr for b in (chain, draw)]
        if chain is None and draw is None:
            known = np.zeros(1, dtype=np.int64), np.full(1, M, dtype=np.int64)
        else:                                             # a missing chain: one chain; a missing draw: the row number
            for w, fill in enumerate((np.zeros, np.arange)):
                if ptrs[w] is None:
                    ptrs[w] = stack.enter_context(_ffi.DeviceBuffer(ctx, M * 8)).upload(fill(M, dtype=np.int64)).ptr
            order = stack.enter_context(_ffi.DeviceBuffer(ctx, M * 8))         # the row order, if the rows need one
        d = handed.enter_context(parquet.draws_in_order(ctx, buf, names, M, ptrs[0], ptrs[1], order, known, note))
        if not names:                                     # id columns alone: a layout, and no tensor
            d.tensor = None
        ids = tuple(None if b is None else b.download(np.int64, M) for b in (chain, draw))
        fbuf = handed.enter_context(buf.share())
        handed.pop_all()
        return CsvDraws(d, fbuf, [bool(v) for v in ints], header, ids)


def read_csv_many_dev(paths, context=None, phases: dict | None = None):
    """`read_csv_dev` for several files with one read, one line index and one parse (Context.csv_table_decode): a list
    of CsvDraws (DeviceDraws, file-order buffer, int flags, header names, (chain, draw) id columns or None each), or None
    when the host reader must decide for one of them (`phases["fallback"]` says why and for which).  Close every entry."""
    import os
    note = phases if phases is not None else {}
    paths = [Path(p) for p in paths]
    for p in paths:
        if not os.path.isfile(p):
            note["fallback"] = f"csv table: {p}: not a file"
            return None
    ctx = context if context is not None else _ffi.default_context()
    with _ffi.value_errors():
        got = ctx.csv_table_decode([str(p) for p in paths], note)
    if got is None:
        return None
    with contextlib.ExitStack() as stack:
        stack.callback(lambda: [g.close() for g in got])       # the files that no _csv_draws has taken over
        out = []
        while got:
            out.append(_csv_draws(ctx, got.pop(0), note))
            stack.callback(out[-1].close)
        stack.pop_all()
    return out


def read_csv_dev(path: Path, context=None, phases: dict | None = None):
    """`pyarrow.csv.read_csv` + `table_to_tensor` without the host parse: (parquet.DeviceDraws -- [P][M] in (chain, draw)
    order, chain ids, counts --, the [P][M] buffer in FILE row order, int_columns) of a table CSV.  The text is read,
    indexed and converted on the GPU (the table mode of mcr_csv_*), the row order comes from the device layout code.
    int_columns[p]: every literal of the column is an integer, the column pyarrow types int64.  None when the host
    reader must decide -- the file is outside the subset the device reader certifies (`phases["fallback"]` says why).
    Free both the draws and the buffer (they may share memory; either order)."""
    got = read_csv_many_dev([path], context, phases)
    if got is None:
        return None
    return got[0][:3]


def _csv_table(d, flat: np.ndarray, int_columns, header, ids):
    """The Arrow table `pacsv.read_csv` builds, from the downloaded file-order [P][M] values and id columns."""
    import pyarrow as pa
    rows, cols = iter(flat), {}
    kinds = iter(int_columns)
    for name in header:
        if name in ("chain", "draw"):
            cols[name] = ids[0 if name == "chain" else 1]
        else:
            row = next(rows)
            cols[name] = row.astype(np.int64) if next(kinds) else row
    return pa.table(cols)


def _csv_image(ctx, fbuf, M: int, int_columns, header, ids):
    """The draws file `_ensure_chain_draw(_csv_table(...))` + pq.write_table give, encoded on the device from the resident
    file-order [P][M] values (Context.write_parquet): the file's columns in its order, int64 where every literal is an
    integer, the id columns from the file (16 bytes per row go back up: the layout step downloaded and freed them), and
    the bookkeeping columns `_ensure_chain_draw` appends as generated int32 columns, in its positions."""
    cols, k = [], 0
    with contextlib.ExitStack() as stack:
        for name in header:
            if name in ("chain", "draw"):
                col = stack.enter_context(_ffi.DeviceBuffer(ctx, max(M * 8, 8)))
                col.upload(np.ascontiguousarray(ids[name == "draw"], dtype=np.int64))
                cols.append(_ffi.pq_column(name, _ffi.MCR_PQ_INT64, col, 1, _ffi.MCR_PQW_I64))
            else:
                cols.append(_ffi.pq_column(name, _ffi.MCR_PQ_INT64 if int_columns[k] else _ffi.MCR_PQ_DOUBLE,
                                           fbuf.ptr.value + 8 * k * M, 1, _ffi.MCR_PQW_F64))
                k += 1
        if "chain" not in header:
            cols.append(_ffi.pq_sequence("chain", _ffi.MCR_PQ_INT32, mod=1))
        if "draw" not in header:
            cols.append(_ffi.pq_sequence("draw", _ffi.MCR_PQ_INT32))
        with _ffi.value_errors():
            return ctx.write_parquet(cols, M)


def _csv_prepared(ctx, got: CsvDraws, min_chains: int, writer: str = "host") -> _Prepared:
    """The `_Prepared` entry of convert_files for one file of read_csv_many_dev (the draws resident).  writer="auto": the
    entry holds the encoded draws file in place of the table, and the matrix is not downloaded.  Takes over `got`."""
    d, fbuf, int_columns, header, ids = got
    with contextlib.ExitStack() as stack:
        stack.enter_context(d)
        P, M = len(d.params), int(d.counts.sum())
        table = image = None
        with fbuf:
            if writer == "auto":
                image = stack.enter_context(_csv_image(ctx, fbuf, M, int_columns, header, ids))
            else:
                flat = fbuf.download(np.float64, P * M).reshape(P, M)
                table = _ensure_chain_draw(_csv_table(d, flat, int_columns, header, ids))
        if d.params and len(d.counts) < min_chains:
            raise ValueError(f"R-hat diagnostics require at least {min_chains} chains; got {len(d.counts)} chain(s)")
        t = d.tensor if d.rectangular else ctx.ragged_tensor(d.buf, d.counts, P)
        stack.pop_all()
        return _Prepared(d.params, int(len(d.counts)), int(d.counts.min()), d.counts, table=table, image=image, tensor=t)


_CSV_BATCH_BYTES = 3 << 30     # text of the .csv jobs read by one library call (its limit is 4 GiB less 1 MiB, padding included)


def _read_csv_prepared_many(paths, min_chains: int, context, writer: str = "host") -> dict:
    """The `.csv` inputs of convert_files through the device reader: {index into paths: `prepared` entry or the
    exception of the job}; a path that is missing from it takes the host route, which is the source of every exception
    of the read itself.  The files share one read and one parse, in groups of at most _CSV_BATCH_BYTES of text (the
    library's limit holds for a call); a file the device reader hands back is named by its message and the group is
    read again without it; whatever else the library answers for a group (a file it cannot open, no memory, the
    limit) sends its files through the reader one by one, and a file for which it answers that again to the host."""
    try:
        ctx = context or _ffi.default_context()
    except _ffi.HipUnavailableError:
        return {}

    def read(group):
        """read_csv_many_dev of the group, or None with `note` filled; an error of the library is no answer either."""
        note: dict = {}
        try:
            return read_csv_many_dev([paths[i] for i in group], ctx, note), note
        except (ValueError, _ffi.McrError, OSError) as exc:
            return None, {"error": str(exc)}

    groups, size = [[]], 0
    for i, p in enumerate(paths):
        n = p.stat().st_size if p.is_file() else 0
        if groups[-1] and size + n > _CSV_BATCH_BYTES:
            groups.append([])
            size = 0
        groups[-1].append(i)
        size += n
    got: list = [None] * len(paths)
    done: dict = {}
    with contextlib.ExitStack() as stack:
        stack.callback(lambda: [g.close() for g in got if g is not None])      # the files read and not yet taken over
        for group in groups:
            while group:
                res, note = read(group)
                if res is not None:
                    for i, g in zip(group, res):
                        got[i] = g
                    break
                named = [i for i in group if note.get("fallback", "").startswith(f"csv table: {paths[i]}: ")]
                if len(named) != 1:                            # not a fallback of one file: each on its own
                    for i in group if len(group) > 1 else []:
                        got[i] = (read([i])[0] or [None])[0]
                    break
                group = [i for i in group if i != named[0]]
        for i, g in enumerate(got):
            if g is None:
                continue
            got[i] = None
            if not g.draws.params:                             # only bookkeeping columns: the host route's empty model
                g.close()
                continue
            try:
                done[i] = _csv_prepared(ctx, g, min_chains, writer)
                stack.callback(done[i].close)
            except Exception as exc:  # noqa: BLE001 - reported per job
                done[i] = exc
        stack.pop_all()
    return done


def summarize_csv(path: Path, min_chains: int = 4, quantiles=(0.05, 0.5, 0.95), diagnostics: bool = True,
                  context=None) -> dict[str, dict[str, float]]:
    """{param: {"mean", "std", "qNN"..., "rhat", "ess_bulk", "ess_tail"}} of a table CSV, the shape
    `reference.summary_for_model` returns: text to statistics on the GPU, chains of unequal length included.  A file
    for the host reader is read by it (and raises what it raises) and its tensor uploaded."""
    import pyarrow.csv as pacsv
    ctx = context if context is not None else _ffi.default_context()
    got = read_csv_dev(Path(path), context=ctx)
    with contextlib.ExitStack() as stack, _ffi.value_errors():
        if got is None:
            table = _ensure_chain_draw(pacsv.read_csv(Path(path)))
            params = [c for c in table.column_names if c not in {"chain", "draw"}]
            x, counts = table_to_tensor(table, params)
            if not params or len(counts) == 0:
                return {}
            t = stack.enter_context(_upload_draws(ctx, x, counts, len(params)))
        else:
            d, fbuf, _ints = got
            stack.enter_context(d)
            fbuf.free()
            params = d.params
            if not params:
                return {}
            t = d.tensor if d.rectangular else ctx.ragged_tensor(d.buf, d.counts, len(params))
        r = ctx.summarize(t, min_chains=min_chains, quantiles=quantiles, diagnostics=diagnostics)
    return dict(zip(params, _ffi.entries(r, list(quantiles), diagnostics)))


def _read_input(path: Path):
    import pyarrow.csv as pacsv
    if path.suffix == ".csv":
        return pacsv.read_csv(path)
    if _is_json_zip(path):
        return _read_json_zip(path)
    raise ValueError(f"Unsupported input format: {path}")


def _read_table(path, parquet: bool):
    """The host's table of a `.csv` or chain-list `.json.zip`; with `parquet` of a `.parquet` draws file of the store too."""
    path = Path(path)
    if parquet and path.suffix == ".parquet":
        import pyarrow.parquet as pq
        return pq.read_table(path)
    return _read_input(path)


def _equal_chains(table, names: list[str], what: str) -> np.ndarray:
    """The draws [P][C][N] of a table whose chains are equally long; ValueError (`what` requires it) where they are not."""
    x, counts = table_to_tensor(table, names)
    if len(counts) and not np.all(counts == counts[0]):
        raise ValueError(f"{what} requires chains of equal length")
    return x.reshape(len(names), len(counts), int(counts[0]) if len(counts) else 0)


def _table_and_names(table, params: Iterable[str] | None):
    """The table with its bookkeeping columns, and the parameter columns asked for (all of them for None)."""
    table = _ensure_chain_draw(table)
    names = [c for c in table.column_names if c not in ("chain", "draw")]
    if params is not None:
        missing = [p for p in params if p not in names]
        if missing:
            raise ValueError(f"Unknown parameter(s): {', '.join(missing)}")
        names = list(params)
    return table, names


def nested_rhat_file(path: Path, superchains: int, params: Iterable[str] | None = None,
                     context=None) -> dict[str, dict[str, float]]:
    """Nested R-hat of every parameter of a draws table (a `.csv` or chain-list `.json.zip`, read on the host): any
    number of equal-length chains, dealt to `superchains` superchains in blocks, in chain-id order.  Per parameter:
    nrhat, nrhat_bulk, nrhat_tail, nrhat_raw (Context.nested_rhat)."""
    table, names = _table_and_names(_read_table(path, parquet=False), params)
    if not names:
        return {}
    x = _equal_chains(table, names, "nested R-hat")
    ctx = context or _ffi.default_context()
    with _ffi.value_errors():
        r = ctx.nested_rhat(x, int(superchains), "pcn")
    keys = ("nrhat", "nrhat_bulk", "nrhat_tail", "nrhat_raw")
    return {n: {k: float(r[k][i]) for k in keys} for i, n in enumerate(names)}


def pareto_khat_file(path: Path, params: Iterable[str] | None = None, ndraws_tail: int | None = None,
                     context=None) -> dict[str, dict[str, float]]:
    """Pareto k-hat of every parameter of a draws table (a `.csv` or chain-list `.json.zip`, read on the host); the chains
    are pooled and may differ in length.  Per parameter: khat, khat_left, khat_right, ndraws_tail, min_ss
    (Context.pareto_khat); `ndraws_tail`: the tail length for every parameter instead of the default."""
    table, names = _table_and_names(_read_table(path, parquet=False), params)
    if not names:
        return {}
    if ndraws_tail is not None and ndraws_tail < 1:
        raise ValueError(f"the tail length must be >= 1; got {ndraws_tail}")
    x, _ = table_to_tensor(table, names)
    ctx = context or _ffi.default_context()
    with _ffi.value_errors():
        r = ctx.pareto_khat(x.reshape(len(names), 1, -1), "pcn", ndraws_tail=ndraws_tail)
    keys = ("khat", "khat_left", "khat_right", "ndraws_tail", "min_ss")
    return {n: {k: (int if k == "ndraws_tail" else float)(r[k][i]) for k in keys} for i, n in enumerate(names)}


def loo_file(path: Path, params: Iterable[str] | None = None, prefix: str = "log_lik", context=None) -> dict:
    """PSIS-LOO of the pointwise log-likelihood columns of a draws table (a `.csv` or chain-list `.json.zip`, read on the
    host): the columns whose name starts with `prefix` (of `params`, or of all), one observation each; the chains are
    pooled and may differ in length.  Context.loo's result -- elpd_loo, se, p_loo, lppd, n_obs, n_draws, khat_counts,
    khat_threshold, the pointwise arrays -- and "names", the observations' columns.  ValueError when no column matches."""
    table, names = _table_and_names(_read_table(path, parquet=False), params)
    names = [n for n in names if n.startswith(prefix)]
    if not names:
        raise ValueError(f"no column starts with {prefix!r}")
    x, _ = table_to_tensor(table, names)
    ctx = context or _ffi.default_context()
    with _ffi.value_errors():
        r = ctx.loo(x.reshape(len(names), 1, -1), "pcn")
    r["names"] = names
    return r


def loo_compare_files(a: Path, b: Path, params: Iterable[str] | None = None, prefix: str = "log_lik", context=None) -> dict:
    """Two models fitted to the same data, compared by PSIS-LOO (loo_file on each): elpd_diff = fsum(elpd_i^a - elpd_i^b)
    (positive: `a` predicts better), se_diff = sqrt(P var(diff, ddof = 0)), and the two results under "a" and "b".
    ValueError when the numbers of observations differ."""
    ra, rb = loo_file(a, params, prefix, context), loo_file(b, params, prefix, context)
    if ra["n_obs"] != rb["n_obs"]:
        raise ValueError(f"the models have {ra['n_obs']} and {rb['n_obs']} observations: not fitted to the same data")
    diff = ra["elpd_i"] - rb["elpd_i"]
    return {"elpd_diff": math.fsum(diff), "se_diff": math.sqrt(diff.size * float(np.var(diff))), "a": ra, "b": rb}


def hdi_file(path: Path, params: Iterable[str] | None = None, prob: Iterable[float] = (0.94,),
             context=None) -> dict[str, dict[str, float]]:
    """Highest-density intervals of every parameter of a draws table (a `.csv` or chain-list `.json.zip`, read on the
    host); the chains are pooled and may differ in length.  Per parameter and probability q of `prob`: `hdi_lo_q` and
    `hdi_hi_q`, q printed like `format(q, "g")` (Context.hdi).  A `.parquet` draws file of the store is read as well."""
    table, names = _table_and_names(_read_table(path, parquet=True), params)
    probs = [float(q) for q in prob]
    if not probs or len(probs) > _ffi.MCR_HDI_MAX_PROBS or not all(0.0 < q < 1.0 for q in probs):
        raise ValueError(f"prob: 1 to {_ffi.MCR_HDI_MAX_PROBS} probabilities inside (0, 1); got {probs}")
    if not names:
        return {}
    x, _ = table_to_tensor(table, names)
    ctx = context or _ffi.default_context()
    with _ffi.value_errors():
        r = ctx.hdi(x.reshape(len(names), 1, -1), "pcn", prob=probs)
    return {n: {f"hdi_{k}_{q:g}": float(r[k][i, j]) for j, q in enumerate(probs) for k in ("lo", "hi")}
            for i, n in enumerate(names)}


def ess_quantile_file(path: Path, params: Iterable[str] | None = None, probs: Iterable[float] = (0.05, 0.5, 0.95),
                      local: int | None = None, context=None) -> dict[str, dict[str, float]]:
    """The effective draws behind the quantile estimates of every parameter of a draws table (a `.csv`, a chain-list
    `.json.zip` or a `.parquet` draws file of the store, read on the host; chains of equal length).  Per parameter and
    probability q of `probs`: `q_q` (the quantile) and `ess_q_q` (the ESS of the indicator x <= quantile), q printed like
    `format(q, "g")`, and `ess_tail_min`, the smaller of the ESS at the smallest and the largest probability
    (indicator.ess_quantile).  With `local` = a number of bins, `eff_local_j` as well: ESS / draws of the j-th bin between
    consecutive quantiles (indicator.ess_local)."""
    from .indicator import ess_local, ess_quantile
    table, names = _table_and_names(_read_table(path, parquet=True), params)
    probs = [float(q) for q in probs]
    if not probs or len(probs) > 32 or not all(0.0 < q < 1.0 for q in probs):
        raise ValueError(f"probs: 1 to 32 probabilities inside (0, 1); got {probs}")
    if local is not None and not 1 <= local <= 32:
        raise ValueError(f"local: 1 to 32 bins; got {local}")
    if not names:
        return {}
    x = _equal_chains(table, names, "the ESS of a quantile")
    ctx = context or _ffi.default_context()
    with _ffi.value_errors():
        r = ess_quantile(x, probs, "pcn", ctx)
        loc = ess_local(x, local, "pcn", ctx) if local is not None else None
    out = {}
    for i, n in enumerate(names):
        row = {f"q_{q:g}": float(r["thresholds"][i, j]) for j, q in enumerate(probs)}
        row.update({f"ess_q_{q:g}": float(r["ess"][i, j]) for j, q in enumerate(probs)})
        row["ess_tail_min"] = float(r["tail_min"][i])
        if loc is not None:
            row.update({f"eff_local_{j}": float(v) for j, v in enumerate(loc["efficiency"][i])})
        out[n] = row
    return out


def gaussian_check_files(ref_path: Path, act_path: Path, params: Iterable[str] | None = None, jitter: float = 0.0,
                         context=None) -> dict:
    """The joint Gaussian check (gaussian.gaussian_check) of the draws table `act_path` against the draws table
    `ref_path` (each a `.csv`, a chain-list `.json.zip` or a `.parquet` draws file of the store, read on the host; the
    chains are pooled).  The parameters are `params`, or those of the reference table; the other table must have them
    too.  Every parameter is scaled by 1 / its reference std (0, so left out, where that is not finite and > 0) and
    `jitter` is added to the diagonal of both scaled covariance matrices.  The call's dict, with `params` (the live
    parameters, in order), `shift` keyed by them, and `singular_ref` / `singular_actual` (a parameter's name or None)."""
    from .gaussian import gaussian_check
    rt, names = _table_and_names(_read_table(ref_path, parquet=True), params)
    at, _ = _table_and_names(_read_table(act_path, parquet=True), names)
    if not names:
        raise ValueError("no parameter to compare")
    ref, _ = table_to_tensor(rt, names)
    act, _ = table_to_tensor(at, names)
    ref, act = ref.reshape(len(names), -1), act.reshape(len(names), -1)
    std = ref.std(axis=1)
    live = np.isfinite(std) & (std > 0)
    scale = np.zeros(len(names))
    scale[live] = 1.0 / std[live]
    with _ffi.value_errors():
        r = gaussian_check(ref, act, scale=scale, jitter=jitter, shift=True, context=context)
    kept = [n for i, n in enumerate(names) if live[i]]
    r["params"] = kept
    r["shift"] = {n: float(v) for n, v in zip(kept, r["shift"])}
    r["singular_ref"] = kept[r["info_ref"] - 1] if r["info_ref"] else None
    r["singular_actual"] = kept[r["info_act"] - 1] if r["info_act"] else None
    return r


def weighted_summary_file(path: Path, log_weights: str | None = None, weights: str | None = None,
                          params: Iterable[str] | None = None, quantiles: Iterable[float] = (0.05, 0.5, 0.95),
                          psis: bool = True, context=None) -> dict:
    """Importance-weighted summaries of every parameter of a draws table (a `.csv`, a chain-list `.json.zip` or a
    `.parquet` draws file of the store, read on the host); the chains are pooled and may differ in length.  The column
    named by `log_weights` (log importance ratios or log weights) or by `weights` (linear, >= 0) is the weight of every
    row and is left out of the parameters.  psis=True (log_weights only): the column first goes through Context.psis with
    r_eff = 1 and its smoothed log weights are used; the result then carries "khat" and "khat_threshold".  "params":
    per parameter mean, sd, mean_se and `q<100 q>` for every q of `quantiles` -- inverted-CDF quantiles
    (Context.weighted_summary); at top level also "ess" (Kish's) and "n_draws"."""
    if (log_weights is None) == (weights is None):
        raise ValueError("give exactly one of log_weights and weights")
    if psis and weights is not None:
        raise ValueError("psis=True smooths log weights: give log_weights, or psis=False with weights")
    wname = weights if log_weights is None else log_weights
    qs = [float(q) for q in quantiles]
    _ffi.weight_arguments(0, None, [], qs)                    # the quantiles are refused before anything is read
    table, names = _table_and_names(_read_table(path, parquet=True),
                                    None if params is None else [p for p in params if p != wname] + [wname])
    if wname not in names:
        raise ValueError(f"Unknown weight column: {wname}")
    names = [n for n in names if n != wname]
    x, _ = table_to_tensor(table, names + [wname])
    v, x = x[-1], x[:-1]
    ctx = context or _ffi.default_context()
    out: dict = {}
    with _ffi.value_errors():
        if psis:
            sm = ctx.psis(v.reshape(1, 1, -1), "pcn")
            v = sm["log_weights"][0]
            out.update(khat=float(sm["khat"][0]), khat_threshold=sm["khat_threshold"])
        r = ctx.weighted_summary(x.reshape(len(names), 1, -1), "pcn", quantiles=qs,
                                 **({"weights": v} if log_weights is None else {"log_weights": v}))
    out.update(ess=r["ess"], n_draws=r["n_draws"])
    out["params"] = {n: {"mean": float(r["mean"][i]), "sd": float(r["sd"][i]), "mean_se": float(r["mean_se"][i]),
                         **{f"q{100 * q:g}": float(r["quantiles"][i, j]) for j, q in enumerate(qs)}}
                     for i, n in enumerate(names)}
    return out


def autocorr_file(path: Path, params: Iterable[str] | None = None, max_lag: int | None = None, unbiased: bool = False,
                  window_c: float = 5.0, context=None) -> dict[str, dict]:
    """Autocorrelation functions and times of every parameter of a draws table (a `.csv`, a chain-list `.json.zip` or a
    `.parquet` draws file of the store, read on the host) with chains of equal length, in chain-id order.  Per parameter:
    lists acf [C][L+1], tau, window, ess_chain [C], acf_pooled [L+1], and tau_pooled, window_pooled, ess_pooled, max_lag
    (Context.autocorr).  ValueError for chains of unequal length."""
    table, names = _table_and_names(_read_table(path, parquet=True), params)
    if not names:
        return {}
    x = _equal_chains(table, names, "autocorrelation")
    ctx = context or _ffi.default_context()
    with _ffi.value_errors():
        r = ctx.autocorr(x, "pcn", max_lag=max_lag, unbiased=unbiased, window_c=window_c)
    return {n: {"acf": r["acf"][i].tolist(), "tau": r["tau"][i].tolist(), "window": r["window"][i].tolist(),
                "ess_chain": r["ess_chain"][i].tolist(), "acf_pooled": r["acf_pooled"][i].tolist(),
                "tau_pooled": float(r["tau_pooled"][i]), "window_pooled": int(r["window_pooled"][i]),
                "ess_pooled": float(r["ess_pooled"][i]), "max_lag": int(r["max_lag"])} for i, n in enumerate(names)}


def _ensure_chain_draw(table):
    """Add the missing bookkeeping columns like the reference does (convert.py:105-120): a missing
    `draw` is the row number, a missing `chain` is chain 0 (int32, appended after the parameters)."""
    import pyarrow as pa
    cols = set(table.column_names)
    n = table.num_rows
    chain = pa.array(np.zeros(n, dtype=np.int32))
    draw = pa.array(np.arange(n, dtype=np.int32))
    if "chain" in cols and "draw" in cols:
        return table
    if "chain" in cols:
        return table.append_column("draw", draw)
    if "draw" in cols:
        return table.append_column("chain", chain)
    return table.append_column("chain", chain).append_column("draw", draw)


def convert_files(jobs, out_draws_dir: Path, out_meta_dir: Path, force: bool = False, source: str = "converted",
                  context=None, reader: str = "auto", writer: str = "auto") -> list:
    """`convert_file` for many inputs with the kernels pipelined: jobs = [(input_path, name), ...]; returns, per job,
    a ConvertResult or the exception that `convert_file` would have raised for it (the per-recipe try/except of
    generate.generate_reference_corpus, src/mcmc_ref/generate.py:77-96, becomes per-entry results).

    reader="auto": a `.json.zip` input is parsed on the GPU (`read_json_zip_dev`) and so is a `.csv` input
    (`read_csv_many_dev`, all of them in one read and one parse); the diagnostics run on that tensor and one download
    gives the table that is written.  A document the device reader does not certify, and every input with
    reader="host", goes through `_read_json_zip` / `pyarrow.csv.read_csv`; both give the same files, meta and exceptions.

    All inputs are read and laid out first, the models are uploaded and enqueued with a rolling window of
    MCR_MAX_INFLIGHT calls (consecutive models overlap on the context's lanes; a NaN draw or any other kernel-side
    failure stays confined to its model) -- rectangular models and models whose chains differ in length alike, the
    latter through the ragged entry point -- then the quality gate and the two files of every model are written.

    writer="auto": the draws file of a job that was read on the device is encoded and compressed on the device too, while
    its matrix is resident (Context.write_parquet: neither the matrix nor an Arrow table reaches the host), and kept
    as host bytes until the gate has passed.  A job read on the host, and every job with writer="host" or with the
    environment variable MCMC_REF_HIP_WRITER=arrow, is written by `pq.write_table`.  Both give the same table."""
    import pyarrow.parquet as pq
    out_draws_dir, out_meta_dir = Path(out_draws_dir), Path(out_meta_dir)
    if reader not in ("auto", "host"):
        raise ValueError(f"reader must be 'auto' or 'host'; got {reader!r}")
    writer = _writer_choice(writer)
    min_chains = 1 if force else 4
    n = len(jobs)
    results: list = [None] * n
    prepared: dict[int, _Prepared] = {}
    with contextlib.ExitStack() as stack:                   # every prepared job is closed, however this ends
        csv_jobs = [i for i, (p, _name) in enumerate(jobs) if reader == "auto" and Path(p).suffix == ".csv"]
        csv_done = _read_csv_prepared_many([Path(jobs[i][0]) for i in csv_jobs], min_chains, context, writer) if csv_jobs else {}
        for k, got in csv_done.items():
            if isinstance(got, Exception):
                results[csv_jobs[k]] = got
            else:
                prepared[csv_jobs[k]] = got
                stack.callback(got.close)
        for i, (input_path, _name) in enumerate(jobs):
            if i in prepared or results[i] is not None:
                continue
            try:
                if reader == "auto" and _is_json_zip(Path(input_path)):
                    got = _read_json_zip_prepared(Path(input_path), min_chains, context, writer)
                    if got is not None:
                        prepared[i] = got
                        stack.callback(got.close)
                        continue
                table = _ensure_chain_draw(_read_input(Path(input_path)))
                params = [c for c in table.column_names if c not in {"chain", "draw"}]
                n_chains, n_draws = _count_chains_draws(table)
                x, counts = table_to_tensor(table, params)
                if params and len(counts) < min_chains:
                    raise ValueError(f"R-hat diagnostics require at least {min_chains} chains; got {len(counts)} chain(s)")
                prepared[i] = _Prepared(params, n_chains, n_draws, counts, table=table, x=x)
                stack.callback(prepared[i].close)
            except Exception as exc:  # noqa: BLE001 - reported per job
                results[i] = exc
        prepared = dict(sorted(prepared.items()))           # job order, whichever reader prepared a job
        diags: dict[int, dict] = {}
        todo = []                                     # models with parameters, rectangular and ragged, in job order
        for i, e in prepared.items():
            if not e.params:
                diags[i] = {}
            else:
                todo.append(i)
        ctx = (context or _ffi.default_context()) if todo else None

        def calls():
            for i in todo:
                e = prepared[i]
                if e.tensor is None:                        # read on the host: uploaded as its turn comes
                    try:
                        e.tensor = _upload_draws(ctx, e.x, e.counts, len(e.params))
                    except _ffi.McrError as exc:
                        results[i] = ValueError(exc.message)
                        continue
                yield i, e.tensor, {"min_chains": min_chains, "quantiles": ()}

        # anything but a kernel-side failure of one model (an McrError of its own, kept as its result) ends the batch, and
        # the window then leaves nothing in flight; it frees each tensor as its call retires, the entries free the rest
        if todo:
            with contextlib.closing(_ffi.pipeline(ctx, calls(), owns=True)) as done:
                for i, r in done:
                    if isinstance(r, _ffi.McrError):
                        results[i] = ValueError(r.message)
                    else:
                        diags[i] = dict(zip(prepared[i].params, _ffi.entries(r)))
        for i, e in prepared.items():
            if results[i] is not None:
                continue
            name = jobs[i][1]
            try:
                checks = _checks(e.n_chains, e.n_draws, diags[i])
                if not force:
                    _enforce_checks(checks)
                meta = {"model": name, "parameters": e.params, "n_chains": e.n_chains, "n_draws_per_chain": e.n_draws,
                        "diagnostics": diags[i], "generated_date": date.today().isoformat(), "checks": checks,
                        "source": source}
                draws_path = out_draws_dir / f"{name}.draws.parquet"
                meta_path = out_meta_dir / f"{name}.meta.json"
                if e.image is not None:                     # encoded on the device: host bytes by now
                    draws_path.write_bytes(e.image.view)
                else:
                    pq.write_table(e.table, draws_path)
                meta_path.write_text(json.dumps(meta, indent=2, sort_keys=True))
                results[i] = ConvertResult(draws_path=draws_path, meta_path=meta_path, meta=meta)
            except Exception as exc:  # noqa: BLE001
                results[i] = exc
    return results


def convert_file(input_path: Path, name: str, out_draws_dir: Path, out_meta_dir: Path, force: bool = False,
                 source: str = "converted") -> ConvertResult:
    """Same contract as the reference's convert_file (convert.py:26-67): diagnostics of every parameter (one GPU
    pipeline per file), quality checks (raise ValueError("quality checks failed: ...") unless `force`), then
    `<name>.draws.parquet` and `<name>.meta.json` (sorted keys, indent 2)."""
    res = convert_files([(input_path, name)], out_draws_dir, out_meta_dir, force=force, source=source)[0]
    if isinstance(res, Exception):
        raise res
    return res


def multi_ess_file(path: Path, params: Iterable[str] | None = None, batch: int | None = None, r: int = 3,
                   context=None) -> dict[str, dict[str, float]]:
    """The multivariate effective sample size of a draws table (a `.csv`, a chain-list `.json.zip` or a `.parquet` draws
    file of the store, read on the host; chains of equal length), from the lugsail (r = 3) or plain (r = 1) batch-means
    long-run covariance at batch size `batch` (None: batchmeans.batch_size).  Per parameter `mean`, `mcse_mean` and
    `ess_bm`; the row `(joint)` holds `mess`, `p_live`, `batch`, `batches_per_chain` and `info_sigma` (non-zero: the
    long-run covariance is singular or indefinite and `mess` NaN).  Every parameter is scaled by 1 / its std (a constant
    one is dropped)."""
    from .batchmeans import multi_ess
    table, names = _table_and_names(_read_table(path, parquet=True), params)
    if not names:
        return {}
    x = _equal_chains(table, names, "the multivariate ESS")
    std = x.reshape(len(names), -1).std(axis=1)
    live = np.isfinite(std) & (std > 0)
    scale = np.zeros(std.size)
    scale[live] = 1.0 / std[live]
    ctx = context or _ffi.default_context()
    with _ffi.value_errors():
        m = multi_ess(x, batch=batch, r=r, scale=scale, context=ctx)
    out = {n: {"mean": float(m["mu"][i]), "mcse_mean": float(m["mcse_mean"][i]), "ess_bm": float(m["ess_bm"][i])}
           for i, n in enumerate(names)}
    out["(joint)"] = {"mess": float(m["mess"]), "p_live": float(m["p_live"]), "batch": float(m["b"]),
                      "batches_per_chain": float(m["a"]), "info_sigma": float(m["info_sigma"])}
    return out


def mean_test_files(ref_path: Path, act_path: Path, params: Iterable[str] | None = None, jitter: float = 0.0, r: int = 3,
                    context=None) -> dict:
    """The joint test of equal means of two draws tables (formats as `multi_ess_file`; chains of equal length within a
    file): batchmeans.mean_shift_test with every parameter scaled by 1 / the reference file's std.  Returns "T", "dof",
    "p_value", "info", "singular" (a parameter name or None), "mess_ref", "mess_act", the batch geometry, and "z" /
    "shift" keyed by live parameter."""
    from .batchmeans import mean_shift_test
    rt, names = _table_and_names(_read_table(ref_path, parquet=True), params)
    at, _ = _table_and_names(_read_table(act_path, parquet=True), names)
    if not names:
        raise ValueError("no parameter to test")
    ref = _equal_chains(rt, names, "the mean test")
    act = _equal_chains(at, names, "the mean test")
    std = ref.reshape(len(names), -1).std(axis=1)
    live = np.isfinite(std) & (std > 0)
    scale = np.zeros(std.size)
    scale[live] = 1.0 / std[live]
    with _ffi.value_errors():
        det = mean_shift_test(ref, act, scale=scale, jitter=jitter, r=r, context=context or _ffi.default_context())
    kept = [n for i, n in enumerate(names) if live[i]]
    out = {k: (int(det[k]) if k in ("dof", "info", "b_ref", "a_ref", "b_act", "a_act") else float(det[k]))
           for k in ("T", "dof", "p_value", "info", "mess_ref", "mess_act", "b_ref", "a_ref", "b_act", "a_act")}
    out["singular"] = kept[det["info"] - 1] if det["info"] else None
    out["z"] = {n: float(v) for n, v in zip(kept, det["z"])}
    out["shift"] = {n: float(v) for n, v in zip(kept, det["shift"])}
    return out

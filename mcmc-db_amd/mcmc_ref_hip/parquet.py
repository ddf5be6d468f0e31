"""Native Parquet ingest: draws file -> device tensor, no pyarrow on the path.

Counterpart of the reference's `pq.read_table` / `pq.ParquetFile(...).iter_batches` + `to_numpy`
(src/mcmc_ref/store.py:79-95, src/mcmc_ref/convert.py:61-65, src/mcmc_ref/backends_numpy.py:35) for the
on-disk layout `draws/<model>.draws.parquet` (long table: `chain`, `draw`, one DOUBLE column per parameter).
Footer and page headers are parsed on the host by the C library, the page payloads are decompressed and
decoded by HIP kernels straight into HBM; the statistics then run on that tensor without a host round trip.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import mmap
import os
from pathlib import Path
from typing import Iterable, Sequence

import numpy as np

from . import _ffi
from ._ffi import MCR_F64, MCR_PQ_F64, MCR_PQ_I64, DeviceBuffer, DeviceTensor, McrError, ParquetRequest

PHYSICAL_TYPES = {0: "BOOLEAN", 1: "INT32", 2: "INT64", 3: "INT96", 4: "FLOAT", 5: "DOUBLE", 6: "BYTE_ARRAY",
                  7: "FIXED_LEN_BYTE_ARRAY"}
NUMERIC = (1, 2, 4, 5)


class ParquetFile:
    """Parsed metadata of one Parquet file image (bytes, mmap or path).  Parsing needs no GPU."""

    def __init__(self, source, context: "_ffi.Context | None" = None):
        self.lib = _ffi.load_library()
        self.ctx = context
        self._mm = None
        if isinstance(source, (str, os.PathLike)):
            self.path = Path(source)
            with open(self.path, "rb") as fh:
                size = os.fstat(fh.fileno()).st_size
                if size == 0:
                    raise McrError(_ffi.MCR_EINVAL, f"parquet: {self.path} is empty")
                self._mm = mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ)
            self._image = np.frombuffer(self._mm, dtype=np.uint8)
        else:
            self.path = None
            self._image = np.frombuffer(source, dtype=np.uint8)
        self.handle = C.c_void_p()
        rc = self.lib.mcr_parquet_open(context.handle if context else None, self._image.ctypes.data_as(C.c_void_p),
                                       self._image.size, C.byref(self.handle))
        if rc != _ffi.MCR_OK:
            msg = (self.lib.mcr_last_error(context.handle if context else None) or b"").decode()
            self.handle = None
            raise McrError(rc, msg)
        self.num_rows = int(self.lib.mcr_parquet_num_rows(self.handle))
        n = self.lib.mcr_parquet_num_columns(self.handle)
        self.column_names = [self.lib.mcr_parquet_column_name(self.handle, i).decode() for i in range(n)]
        self.column_types = [self.lib.mcr_parquet_column_type(self.handle, i) for i in range(n)]

    def pages(self) -> list[dict]:
        keys = ("column", "kind", "encoding", "codec", "payload_offset", "compressed_size", "uncompressed_size",
                "num_values", "first_row", "dictionary_page")
        out, info = [], np.zeros(10, dtype=np.int64)
        for i in range(self.lib.mcr_parquet_num_pages(self.handle)):
            self.lib.mcr_parquet_page_info(self.handle, i, info.ctypes.data_as(C.POINTER(C.c_int64)))
            out.append(dict(zip(keys, (int(v) for v in info))))
        return out

    def index(self, name: str) -> int:
        try:
            return self.column_names.index(name)
        except ValueError:
            raise KeyError(f"column {name!r} not in {self.path or 'parquet image'}") from None

    def close(self):
        if getattr(self, "handle", None):
            self.lib.mcr_parquet_close(self.handle)
            self.handle = None
        self._image = None
        if self._mm is not None:
            try:
                self._mm.close()
            except BufferError:      # a numpy view is still alive somewhere; the mapping goes with it
                pass
            self._mm = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


def decode(ctx: "_ffi.Context", requests: Sequence[tuple[ParquetFile, int, int, C.c_void_p]]):
    """One upload + two launches for all (file, column index, out_kind, device pointer) requests."""
    arr = (ParquetRequest * max(len(requests), 1))()
    for i, (f, col, kind, ptr) in enumerate(requests):
        arr[i].file, arr[i].column, arr[i].out_kind = f.handle, col, kind
        arr[i].out_dev = ptr if isinstance(ptr, int) else ptr.value
    ctx._check(ctx.lib.mcr_parquet_decode(ctx.handle, arr, len(requests)))


def _layout(chain: np.ndarray, draw: np.ndarray):
    """(chain ids, order or None, draws per chain) -- the integer bookkeeping of `_chains_from_table`
    (src/mcmc_ref/convert.py:150-161); same rule as convert.chain_layout."""
    if chain.size:
        dc = np.diff(chain)
        if np.all(dc >= 0):                           # chain-major file (every packaged one): no sort needed
            cut = np.flatnonzero(dc) + 1
            starts = np.concatenate([[0], cut])
            counts = np.diff(np.concatenate([starts, [chain.size]]))
            dd = np.diff(draw)
            dd[cut - 1] = 0                           # steps across a chain boundary do not count
            if np.all(dd >= 0):
                return chain[starts].copy(), None, counts
    ids, counts = np.unique(chain, return_counts=True)
    order = None if chain.size == 0 else np.lexsort((draw, chain))
    return ids, order, counts


_LAYOUT_CAP = 256       # distinct chains mcr_chain_layout_dev reports (the library's chain limit); more take the host's np.unique


def _device_layout(ctx: "_ffi.Context", chain_ptr, draw_ptr, M: int, order: DeviceBuffer):
    """`_layout` from id columns in device memory (mcr_chain_layout_dev): (chain ids, `order` filled with the row
    order or None for rows in order, counts); None when the table is for the host (MCR_EFALLBACK, or more than
    _LAYOUT_CAP distinct chains)."""
    try:
        return ctx.chain_layout(chain_ptr, draw_ptr, M, cap=_LAYOUT_CAP, order=order)
    except McrError as exc:
        if exc.code == _ffi.MCR_EINVAL and "distinct chain ids" in exc.message:
            return None
        raise


def _download(ctx: "_ffi.Context", ptr, dtype, count: int) -> np.ndarray:
    out = np.empty(count, dtype=dtype)
    if out.nbytes:
        ctx._check(ctx.lib.mcr_memcpy_d2h(ctx.handle, out.ctypes.data_as(C.c_void_p), ptr, out.nbytes))
    return out


_Arena, _View = _ffi.DeviceArena, _ffi.DeviceView      # one allocation shared by the models of a batch, and its slices


class DeviceDraws(_ffi._Owner):
    """Draws of one model in HBM: `tensor` is [P][M] f64 in (chain, draw) order; counts = draws per chain."""

    def __init__(self, tensor: DeviceTensor | None, buf, params: list[str], chain_ids: np.ndarray,
                 counts: np.ndarray):
        self.tensor, self.buf, self.params, self.chain_ids, self.counts = tensor, buf, params, chain_ids, counts

    @property
    def rectangular(self) -> bool:
        return len(self.counts) > 0 and bool(np.all(self.counts == self.counts[0]))

    def to_host(self) -> np.ndarray:
        M = int(self.counts.sum())
        return self.buf.download(np.float64, len(self.params) * M).reshape(len(self.params), M)

    def free(self):
        self.buf.free()


def draws_in_order(ctx: "_ffi.Context", values: _View, params: list[str], M: int, chain_ptr, draw_ptr, order: DeviceBuffer,
                   known=None, note: dict | None = None) -> DeviceDraws:
    """The row-order step of every reader: the DeviceDraws of `values`, [P][M] f64 in file row order, with the rows in
    (chain, draw) order -- the integer bookkeeping of `_chains_from_table`.  chain_ptr / draw_ptr: the id columns in
    device memory (M int64 each); `order`: scratch of 8 M bytes for a row order.  known: (chain ids, counts) where the
    rows are known to be in order (Context.chain_layout_many said so, or there are no id columns); else the device
    layout decides, and where it declines the host's lexsort of the downloaded ids (`note["layout"] = "host"`).  Rows out
    of order are gathered into a new buffer; otherwise the draws hold another view of `values`.  `values` stays the
    caller's either way."""
    P = len(params)
    rows = None                                       # the row order: `order` on the device, an int64 array from the host
    if known is not None:
        chain_ids, counts = known
    else:
        lay = _device_layout(ctx, chain_ptr, draw_ptr, M, order)
        if lay is None:                               # no 64-bit row key, or very many chains: the host's lexsort
            if note is not None:
                note["layout"] = "host"
            lay = _layout(_download(ctx, chain_ptr, np.int64, M), _download(ctx, draw_ptr, np.int64, M))
        chain_ids, rows, counts = lay
    with contextlib.ExitStack() as stack:
        if rows is None or not (P and M):
            buf = stack.enter_context(values.share())
        else:
            buf = stack.enter_context(DeviceBuffer(ctx, P * M * 8))
            if isinstance(rows, np.ndarray):
                rows = np.ascontiguousarray(rows, dtype=np.int64)
                ctx._check(ctx.lib.mcr_gather_rows_dev(ctx.handle, values.ptr, P, M, rows.ctypes.data_as(C.POINTER(C.c_int64)),
                                                       buf.ptr))
            else:
                ctx.gather_rows_order(values.ptr, P, M, rows.ptr, buf.ptr)
        tensor = None
        if len(counts) and np.all(counts == counts[0]):
            Cn, N = len(counts), int(counts[0])
            tensor = DeviceTensor(ctx, buf, (MCR_F64, Cn, N, P, N, 1, Cn * N))
        stack.pop_all()
        return DeviceDraws(tensor, buf, params, chain_ids, np.asarray(counts, dtype=np.int64))


def read_draws_many(ctx: "_ffi.Context", sources: Sequence, params: Sequence[Iterable[str] | None] | None = None
                    ) -> list[DeviceDraws]:
    """Decodes many draws files with one batched decode call (all pages of all files in one grid)."""
    with contextlib.ExitStack() as stack, contextlib.ExitStack() as handed:
        files = [s if isinstance(s, ParquetFile) else stack.enter_context(ParquetFile(s, ctx)) for s in sources]
        reqs, plan = [], []
        wants, sizes, colidx, ididx = [], [], [], []
        for k, f in enumerate(files):
            want = list(params[k]) if params is not None and params[k] is not None else \
                [n for n, t in zip(f.column_names, f.column_types) if n not in ("chain", "draw") and t in NUMERIC]
            wants.append(want)
            colidx.append([f.index(n) for n in want])      # KeyError for an unknown name BEFORE any device allocation
            ididx.append((f.index("chain"), f.index("draw")))
            sizes.append(len(want) * f.num_rows * 8)       # packed: same-shape neighbours form ONE [P][C][N] tensor
        arena = stack.enter_context(_Arena(ctx, sum(sizes)))
        id_rows = sum(f.num_rows for f in files)
        ids_all = stack.enter_context(DeviceBuffer(ctx, max(2 * id_rows * 8, 8)))
        # one file's row order at a time
        order_buf = stack.enter_context(DeviceBuffer(ctx, max(max((f.num_rows for f in files), default=0) * 8, 8)))
        off = ioff = 0
        for f, want, size, cols, (i_chain, i_draw) in zip(files, wants, sizes, colidx, ididx):
            M = f.num_rows
            buf = stack.enter_context(arena.view(off, len(cols) * M * 8))      # file row order; the draws take a view of their own
            base, ibase = buf.ptr.value, ids_all.ptr.value + ioff * 8
            for j, c in enumerate(cols):
                reqs.append((f, c, MCR_PQ_F64, base + j * M * 8))
            reqs.append((f, i_chain, MCR_PQ_I64, ibase))
            reqs.append((f, i_draw, MCR_PQ_I64, ibase + M * 8))
            plan.append((want, M, buf, C.c_void_p(ibase), C.c_void_p(ibase + M * 8)))
            off += size
            ioff += 2 * M
        decode(ctx, reqs)
        # nearly every file is in (chain, draw) order: one round trip says so for all of them, and gives their chains
        ordered = ctx.chain_layout_many([(cp, dp, M) for _want, M, _buf, cp, dp in plan], cap=_LAYOUT_CAP)
        out = [handed.enter_context(draws_in_order(ctx, buf, want, M, cp, dp, order_buf, known))
               for (want, M, buf, cp, dp), known in zip(plan, ordered)]
        handed.pop_all()
        return out


def read_draws(ctx: "_ffi.Context", source, params: Iterable[str] | None = None) -> DeviceDraws:
    return read_draws_many(ctx, [source], [params])[0]


def decode_columns(ctx: "_ffi.Context", f: ParquetFile, names: Sequence[str]):
    """(device buffer [len(names)][num_rows] of 8-byte values in FILE row order, kinds): INT32 / INT64 columns as
    int64 (MCR_PQ_I64), the other numeric ones as float64.  Free the buffer."""
    M = f.num_rows
    cols = [f.index(n) for n in names]               # KeyError for an unknown name before any device allocation
    kinds = [MCR_PQ_I64 if f.column_types[c] in (1, 2) else MCR_PQ_F64 for c in cols]
    with contextlib.ExitStack() as stack:
        buf = stack.enter_context(DeviceBuffer(ctx, max(len(names) * M * 8, 8)))
        decode(ctx, [(f, c, k, buf.ptr.value + j * M * 8) for j, (c, k) in enumerate(zip(cols, kinds))])
        stack.pop_all()
    return buf, kinds


def read_columns(ctx: "_ffi.Context", source, columns: Iterable[str] | None = None) -> dict[str, np.ndarray]:
    """Host arrays of numeric columns decoded on the device (ints as int64, floats as float64)."""
    with contextlib.ExitStack() as stack:
        f = source if isinstance(source, ParquetFile) else stack.enter_context(ParquetFile(source, ctx))
        names = list(columns) if columns is not None else [n for n, t in zip(f.column_names, f.column_types) if t in NUMERIC]
        M = f.num_rows
        buf, kinds = decode_columns(ctx, f, names)
        with buf:
            raw = buf.download(np.int64, len(names) * M).reshape(len(names), M)
        return {n: (raw[j].copy() if k == MCR_PQ_I64 else raw[j].view(np.float64).copy())
                for j, (n, k) in enumerate(zip(names, kinds))}


def write_draws_dev(ctx: "_ffi.Context", path, columns, rows: int, row_group_rows: int = 0) -> int:
    """Writes `rows` rows of device columns (_ffi.pq_column / _ffi.pq_sequence) as a Parquet draws file, encoded and
    compressed on the GPU (Context.write_parquet); the replacement of `pq.write_table` (src/mcmc_ref/convert.py:64).
    Returns the file's size."""
    with ctx.write_parquet(columns, rows, row_group_rows) as image:
        Path(path).write_bytes(image.view)
        return len(image)


def _write_view(dest, view) -> None:
    if hasattr(dest, "write"):
        dest.write(view)
    else:
        Path(dest).write_bytes(view)


def write_csv_dev(ctx: "_ffi.Context", dest, columns, rows: int, row_index=None, header: str = "quoted") -> int:
    """Writes device columns (_ffi.pq_column / _ffi.pq_sequence) of `rows` rows as CSV text formatted on the GPU
    (Context.write_csv): the bytes `pyarrow.csv.write_csv` gives the same table (src/mcmc_ref/cli.py:117-120).  `dest` is
    a path or a binary file object; row_index and header as for Context.write_csv.  Returns the text's size."""
    with ctx.write_csv(columns, rows, row_index, header) as image:
        _write_view(dest, image.view)
        return len(image)


def _summarize_paths(ctx: "_ffi.Context", paths: list[str], min_chains: int, qs: list[float], diagnostics: bool,
                     phases: dict | None = None):
    """All of summarize_files in ONE C call (Context.summarize_files).  Returns None when a file needs the general
    route (rows out of (chain, draw) order, chains of unequal length); `phases`: see Context.summarize_files."""
    try:
        got = ctx.summarize_files(paths, min_chains, qs, diagnostics, phases)
    except McrError as exc:
        if exc.code in (_ffi.MCR_EMINCHAINS, _ffi.MCR_EMINCHAINS_ARG, _ffi.MCR_ENONFINITE):
            raise ValueError(exc.message.split(": ", 1)[-1] if exc.code == _ffi.MCR_EMINCHAINS else exc.message) from exc
        if "cannot compute stats of empty columns" in exc.message:
            raise ValueError("cannot compute stats of empty columns") from exc
        raise
    if got is None:
        return None
    files, r = got
    rows, out, r0 = _ffi.entries(r, qs, diagnostics), [], 0
    for names, _C, _N in files:
        out.append(dict(zip(names, rows[r0:r0 + len(names)])))
        r0 += len(names)
    return out


def summarize_files(ctx: "_ffi.Context", sources: Sequence, params: Sequence[Iterable[str] | None] | None = None, *,
                    min_chains: int = 4, quantiles=(0.05, 0.5, 0.95), diagnostics: bool = True
                    ) -> list[dict[str, dict[str, float]]]:
    """File images -> per-parameter statistics without the draws ever visiting host memory decoded:
    one batched decode, then the models are pipelined through the summarise lanes (rolling window).

    diagnostics=False is `Backend.stats` (pooled mean / std / quantiles, any chain structure);
    diagnostics=True adds rhat / ess_bulk / ess_tail (what `convert._compute_diagnostics` + `Backend.stats` give
    for the same file); a model whose chains differ in length is one job of the same window
    (mcr_summarize_chains_enqueue: statistics and diagnostics of all its parameters from one sort).
    """
    qs = list(quantiles)
    if sources and all(isinstance(s_, (str, os.PathLike)) for s_ in sources) and \
            (params is None or all(p_ is None for p_ in params)):
        fast = _summarize_paths(ctx, [os.fspath(s_) for s_ in sources], min_chains, qs, diagnostics)
        if fast is not None:
            return fast
    with contextlib.ExitStack() as stack:
        models = [stack.enter_context(d) for d in read_draws_many(ctx, sources, params)]
        # Jobs: maximal runs of neighbouring models that sit back to back in the arena and share (C, N) are ONE
        # tensor with their parameters concatenated -- one kernel pipeline instead of one per model.
        jobs = []                                    # (first model, n models, tensor args, min_chains, diagnostics)
        for k, d in enumerate(models):
            P, M = len(d.params), int(d.counts.sum())
            if P == 0:
                continue
            if diagnostics and len(d.counts) < min_chains:
                raise ValueError(f"R-hat diagnostics require at least {min_chains} chains; got {len(d.counts)} chain(s)")
            if not diagnostics and M == 0:
                raise ValueError("cannot compute stats of empty columns")
            rect = d.tensor is not None
            # with diagnostics a model's chains shape the call: (C, N) rectangular, the chain lengths when ragged;
            # Backend.stats alone pools the draws, whatever the chains
            shape = ((len(d.counts), int(d.counts[0])) if rect else tuple(int(c) for c in d.counts)) if diagnostics else (1, M)
            if jobs and M > 0:
                j = jobs[-1]
                last = models[j["first"] + j["count"] - 1]
                if (k == j["first"] + j["count"] and j["shape"] == shape and j["rect"] == (rect or not diagnostics)
                        and isinstance(d.buf, _View) and isinstance(last.buf, _View)
                        and last.buf.ptr.value + len(last.params) * M * 8 == d.buf.ptr.value):
                    j["count"] += 1
                    j["P"] += P
                    continue
            jobs.append({"first": k, "count": 1, "shape": shape, "rect": rect or not diagnostics, "P": P, "buf": d.buf})

        def calls():
            for j in jobs:
                if j["rect"]:
                    Cn, N = j["shape"]
                    t = DeviceTensor(ctx, j["buf"], (MCR_F64, Cn, N, j["P"], N, 1, Cn * N))
                else:                                # chains of unequal length: the same window, the ragged entry point
                    t = ctx.ragged_tensor(j["buf"], j["shape"], j["P"])
                yield j, t, {"min_chains": min_chains if diagnostics else 1, "quantiles": qs, "diagnostics": diagnostics}

        results = [None] * len(models)
        with _ffi.value_errors(), contextlib.closing(_ffi.pipeline(ctx, calls())) as done:
            for j, r in done:
                if isinstance(r, McrError):
                    raise r
                k0, k1 = j["first"], j["first"] + j["count"]
                results[k0:k1] = _ffi.split_result(r, [len(d.params) for d in models[k0:k1]])
        return [{} if r is None else dict(zip(d.params, _ffi.entries(r, qs, diagnostics)))
                for d, r in zip(models, results)]

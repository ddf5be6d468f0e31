"""The entries of Context that the library's file unit implements: row layout, the Parquet and CSV writers, and the
readers of draws files, CmdStan CSVs, table CSVs and chain-list JSON.  A base of Context (see _context.py).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import time

import numpy as np

from ._abi import CSV_HEADERS, FS_EXPORT, FS_PHASES, MCR_EFALLBACK, MCR_ELAYOUT, IdColumns, _as_dp, _as_ip
from ._device import CsvTable, DeviceArena, DeviceBuffer
from ._hostdefs import PqImage, TextImage, _pq_columns


def _csv_phases(phases: dict | None, paths, clock, hard: int):
    """Fills `phases` with the host clock of a CSV reader's three calls (ms): `clock` holds the times before the open,
    after the headers and after the line index; the parse ends now."""
    if phases is not None and len(paths):
        t0, t1, t2 = clock
        t3 = time.perf_counter()
        phases.update(read_upload_ms=(t1 - t0) * 1e3, index_ms=(t2 - t1) * 1e3, parse_finish_ms=(t3 - t2) * 1e3,
                      text_bytes=sum(os.path.getsize(p) for p in paths), hard=int(hard))


class _FileCalls:
    """Layout, writers and readers: what mcr_files.hip implements."""

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

    @contextlib.contextmanager
    def _csv_files(self, open_symbol: str, paths):
        """The mcr_csv handles of `paths`, opened in one call of mcr_csv_open_paths or mcr_csv_open_table_paths; every
        one of them is closed on the way out."""
        n = len(paths)
        arr = (C.c_char_p * max(n, 1))(*[os.fsencode(p) for p in paths])
        hs = (C.c_void_p * max(n, 1))()
        self._check(getattr(self.lib, open_symbol)(self.handle, arr, n, hs))
        try:
            yield hs
        finally:
            for h in hs[:n]:
                if h:
                    self.lib.mcr_csv_close(h)

    def _csv_headers(self, hs, n: int):
        """The column names of each of the n open files, one file at a time (UnicodeDecodeError for a name that is not
        UTF-8)."""
        L = self.lib
        for f in range(n):
            yield [(L.mcr_csv_column_name(hs[f], c) or b"").decode() for c in range(L.mcr_csv_num_columns(hs[f]))]

    def csv_decode(self, paths, select, phases: dict | None = None) -> tuple[list[str], "DeviceTensor", int]:
        """CmdStan chain files -> (parameter names, [P][C][N] DeviceTensor, fields finished on the host): the library
        reads the files (mcr_csv_open_paths), indexes their data rows (mcr_csv_stage) and parses the selected columns of
        the first N = min over files rows on the device (mcr_csv_decode).  `select(file index, header names)` returns
        (names, header column of each name) of one file; the first file's names give the tensor's parameter order and
        every other file must hold the same set.  `phases` is filled with the host clock of the three calls (ms)."""
        L, n = self.lib, len(paths)
        t0 = time.perf_counter()
        with self._csv_files("mcr_csv_open_paths", paths) as hs:
            picked = [select(f, header) for f, header in enumerate(self._csv_headers(hs, n))]   # (not UTF-8: it raises)
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
                _csv_phases(phases, paths, (t0, t1, t2), hard.value)
                stack.pop_all()
                return names, t, int(hard.value)

    def csv_table_decode(self, paths, phases: dict | None = None):
        """Table CSVs -> per file a CsvTable (parameter names in file order without `chain` / `draw`, [P][M] f64 DeviceView in file
        row order, all_int flags [P], (chain ids, draw ids) as int64 DeviceViews of M entries or None for an absent
        column, fields finished on the host, header names): ONE read (mcr_csv_open_table_paths), one line index
        (mcr_csv_stage) and one parse (mcr_csv_decode_table) for all files.  None when the host reader must decide for
        one of them: the library answers MCR_EFALLBACK or a header is not UTF-8 (`phases["fallback"]` says why).
        `phases` receives the host clock of the three calls (ms).  Close every entry."""
        L, n = self.lib, len(paths)
        note = phases if phases is not None else {}
        t0 = time.perf_counter()
        with self._csv_files("mcr_csv_open_table_paths", paths) as hs:
            try:
                heads = list(self._csv_headers(hs, n))
            except UnicodeDecodeError:                       # the chain reader raises; a table goes to the host reader
                note["fallback"] = "csv table: a header name is not UTF-8"
                return None
            t1 = time.perf_counter()
            rows = np.zeros(max(n, 1), dtype=np.int64)
            if self._declined(L.mcr_csv_stage(self.handle, hs, n, _as_ip(rows)), note):
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
                rc = L.mcr_csv_decode_table(self.handle, cols.ctypes.data_as(C.POINTER(C.c_int)), cols.shape[1],
                                            ids.ctypes.data_as(C.POINTER(C.c_int)), int(rows.max()), out.buf.ptr, 0, 1, 0,
                                            idb.buf.ptr, all_int.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(hard))
                if self._declined(rc, note):
                    return None
                got, off, ioff = [], 0, 0
                for f in range(n):                           # the slices are the caller's; the arenas live as long as they do
                    M, P = int(rows[f]), len(params[f])
                    pair = [stack.enter_context(idb.view((ioff + w * M) * 8, M * 8)) if ids[f, w] >= 0 else None for w in range(2)]
                    got.append(CsvTable([heads[f][c] for c in params[f]], stack.enter_context(out.view(off, sizes[f])),
                                        all_int[f, :P].astype(bool), tuple(pair), int(hard.value), heads[f]))
                    off += sizes[f]
                    ioff += 2 * M
                _csv_phases(phases, paths, (t0, t1, t2), hard.value)
                stack.pop_all()
                return got

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
        if self._declined(L.mcr_json_open(self.handle, text, len(text), C.byref(h)), note):
            return None
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
                if self._declined(rc, note):
                    return None
                if phases is not None:
                    t2 = time.perf_counter()
                    phases.update(upload_index_walk_ms=(t1 - t0) * 1e3, parse_finish_ms=(t2 - t1) * 1e3, text_bytes=len(text),
                                  hard=int(hard.value))
                stack.pop_all()
                return list(names), t, all_int[:, :P].astype(bool), int(hard.value)
        finally:
            L.mcr_json_close(h)

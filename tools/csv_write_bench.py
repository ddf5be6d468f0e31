#!/usr/bin/env python3
"""Draws exported as CSV on the device (reference.export_draws, mcr_csv_write_dev) against the reference's route
(`reference.draws(..., return_="arrow")` + `pyarrow.csv.write_csv`), in one process, alternating, on seeded draws
files written here.

    python tools/csv_write_bench.py [--shapes small,headline] [--reps 9] [--out profiles/csv_write.json]

Per shape, median and range of `reps` runs of either side after one warm-up each:
  (a) export_draws, file to text, writer="auto" against writer="host", into an in-memory sink and into a file in --tmp
      (a tmpfs where there is one);
  (b) the write step alone into the in-memory sink: Context.write_csv from the resident columns, against
      pyarrow.csv.write_csv of the materialised table;
  (c) the k_csvw_* kernel times of (b), and the text's size."""
import argparse, io, json, statistics, sys, tempfile, time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "mcmc-db_amd")]
from mcmc_ref_hip import _ffi, parquet, reference  # noqa: E402
from mcmc_ref_hip.store import DataStore  # noqa: E402

SHAPES = {"small": (4, 1000, 10), "headline": (4, 10000, 100)}


def spread(v):
    return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}


def write_model(root: Path, C: int, N: int, P: int) -> str:
    import pyarrow as pa
    import pyarrow.parquet as pq
    rng = np.random.default_rng(C * N + P)
    cols = {"chain": np.repeat(np.arange(C, dtype=np.int64), N), "draw": np.tile(np.arange(N, dtype=np.int64), C)}
    cols.update({f"theta[{p + 1}]": rng.standard_normal(C * N) * 10.0 ** (p % 7 - 3) for p in range(P)})
    (root / "draws").mkdir(parents=True, exist_ok=True)
    pq.write_table(pa.table(cols), root / "draws" / "bench.draws.parquet")
    return "bench"


def measure(ctx, store, model: str, tmp: Path, reps: int) -> dict:
    import pyarrow.csv as pacsv

    def export(writer: str, to_file: bool) -> float:
        dest = tmp / f"{writer}.csv" if to_file else io.BytesIO()
        t0 = time.perf_counter()
        reference.export_draws(model, dest, store=store, context=ctx, writer=writer)
        return (time.perf_counter() - t0) * 1e3

    sinks = {w: io.BytesIO() for w in ("auto", "host")}
    for w, s in sinks.items():
        reference.export_draws(model, s, store=store, context=ctx, writer=w)
    same = sinks["auto"].getvalue() == sinks["host"].getvalue()
    a = {(w, f): [] for w in ("auto", "host") for f in (False, True)}
    for key in a:
        export(*key)
    for _ in range(reps):
        for key in a:
            a[key].append(export(*key))

    # (b) the write step alone: resident columns against the materialised table
    path = store.resolve_draws_path(model)
    table = reference.draws(model, return_="arrow", store=store)
    table = table.read_all() if hasattr(table, "read_all") else table
    with parquet.ParquetFile(path, ctx) as f:
        names, M = list(f.column_names), f.num_rows
        types = [f.column_types[f.index(n)] for n in names]
        buf, kinds = parquet.decode_columns(ctx, f, names)
    cols = [_ffi.pq_column(n, t, buf.ptr.value + j * M * 8, 1, _ffi.MCR_PQW_I64 if k == _ffi.MCR_PQ_I64 else _ffi.MCR_PQW_F64)
            for j, (n, t, k) in enumerate(zip(names, types, kinds))]

    def step(device: bool) -> float:
        sink = io.BytesIO()
        t0 = time.perf_counter()
        if device:
            parquet.write_csv_dev(ctx, sink, cols, M)
        else:
            pacsv.write_csv(table, sink)
        return (time.perf_counter() - t0) * 1e3

    try:
        step(True), step(False)
        b = {True: [], False: []}
        for _ in range(reps):
            for dev in (True, False):
                b[dev].append(step(dev))
        ctx.profile(True)
        kern: dict = {}
        for _ in range(3):
            ctx.profile_reset()
            step(True)
            for k, v in ctx.profile_get().items():
                if k.startswith("k_csvw"):
                    kern.setdefault(k, []).append(v["total_ms"])
        ctx.profile(False)
        ctx.profile_reset()
    finally:
        buf.free()
    return {"bytes_equal": bool(same), "text_bytes": len(sinks["auto"].getvalue()),
            "export_memory_writer_auto": spread(a[("auto", False)]), "export_memory_writer_host": spread(a[("host", False)]),
            "export_tmpfs_writer_auto": spread(a[("auto", True)]), "export_tmpfs_writer_host": spread(a[("host", True)]),
            "write_step_device": spread(b[True]), "write_step_pyarrow": spread(b[False]),
            "kernel_ms_median": {k: round(statistics.median(v), 4) for k, v in sorted(kern.items())}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="small,headline")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--tmp", default="/dev/shm" if Path("/dev/shm").is_dir() else None)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "csv_write.json"))
    a = ap.parse_args()
    import pyarrow
    out = {"reps": a.reps, "pyarrow": pyarrow.__version__, "shapes": {}}
    with _ffi.Context(0) as ctx:
        for shape in a.shapes.split(","):
            C, N, P = SHAPES[shape]
            with tempfile.TemporaryDirectory(dir=a.tmp) as td:
                root = Path(td)
                model = write_model(root, C, N, P)
                r = measure(ctx, DataStore(local_root=root, packaged_root=root / "none"), model, root, a.reps)
            out["shapes"][f"{shape}_{C}x{N}x{P}"] = r
            print(shape, json.dumps(r), flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Draws Parquet files written on the device (mcr_parquet_write_dev) against pyarrow's writer, in one process,
alternating, on seeded `%.17g` table CSVs written here.

    python tools/parquet_write_bench.py [--shapes small,headline] [--reps 9] [--out profiles/parquet_write.json]

Per shape, median and range of `reps` runs of either side after one warm-up each:
  (a) convert_files, text to both files, writer="auto" against writer="host" (the host writer is the baseline);
  (b) the write step alone, from the resident file-order matrix: Context.write_parquet + the file write, against the
      download of the matrix + the Arrow table + pq.write_table;
  (c) the sizes of the two files and the time mcr_summarize_files takes to read each back.
The output directory is --tmp (a tmpfs where there is one), so the page cache is warm and no disk is waited for."""
import argparse, json, statistics, sys, tempfile, time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "mcmc-db_amd")]
from mcmc_ref_hip import _ffi, convert  # noqa: E402

sys.path.insert(0, str(ROOT / "tools"))
from csv_table_bench import SHAPES, spread, write_table  # noqa: E402


def measure(ctx, csv: Path, out: Path, reps: int) -> dict:
    import pyarrow.parquet as pq

    def run(writer: str) -> float:
        t0 = time.perf_counter()
        res = convert.convert_files([(csv, writer)], out, out, force=True, context=ctx, writer=writer)[0]
        if isinstance(res, Exception):
            raise res
        return (time.perf_counter() - t0) * 1e3

    def step(device: bool, parts: dict | None = None) -> float:
        d, fbuf, ints, header, ids = convert.read_csv_many_dev([csv], ctx)[0]
        try:
            M = int(d.counts.sum())
            path = out / ("step_dev.parquet" if device else "step_host.parquet")
            t0 = time.perf_counter()
            if device:
                with convert._csv_image(ctx, fbuf, M, ints, header, ids) as image:
                    t1 = time.perf_counter()
                    path.write_bytes(image.view)
                if parts is not None:
                    parts.setdefault("encode_ms", []).append((t1 - t0) * 1e3)
            else:
                flat = fbuf.download(np.float64, len(d.params) * M).reshape(len(d.params), M)
                t1 = time.perf_counter()
                table = convert._ensure_chain_draw(convert._csv_table(d, flat, ints, header, ids))
                t2 = time.perf_counter()
                pq.write_table(table, path)
                if parts is not None:
                    parts.setdefault("download_ms", []).append((t1 - t0) * 1e3)
                    parts.setdefault("table_ms", []).append((t2 - t1) * 1e3)
            return (time.perf_counter() - t0) * 1e3
        finally:
            d.free()
            fbuf.free()

    def read_back(path: Path) -> float:
        t0 = time.perf_counter()
        ctx.summarize_files([str(path)])
        return (time.perf_counter() - t0) * 1e3

    for w in ("auto", "host"):
        run(w)
    same = pq.read_table(out / "auto.draws.parquet").equals(pq.read_table(out / "host.draws.parquet"))
    a = {"auto": [], "host": []}
    for _ in range(reps):
        for w in ("auto", "host"):
            a[w].append(run(w))
    step(True), step(False)
    b = {True: [], False: []}
    parts: dict = {}
    for _ in range(reps):
        for dev in (True, False):
            b[dev].append(step(dev, parts))
    files = {"device": out / "auto.draws.parquet", "pyarrow": out / "host.draws.parquet"}
    c = {k: [] for k in files}
    for p in files.values():
        read_back(p)
    for _ in range(reps):
        for k, p in files.items():
            c[k].append(read_back(p))
    ctx.profile(True)
    kern: dict = {}
    for _ in range(3):
        ctx.profile_reset()
        step(True)
        for k, v in ctx.profile_get().items():
            if k.startswith("k_pqw"):
                kern.setdefault(k, []).append(v["total_ms"])
    ctx.profile(False)
    ctx.profile_reset()
    pages = pq.ParquetFile(files["device"]).metadata
    return {"tables_equal": bool(same),
            "convert_files_writer_auto": spread(a["auto"]), "convert_files_writer_host": spread(a["host"]),
            "auto_below_host_range": max(a["auto"]) < min(a["host"]),
            "write_step_device": spread(b[True]), "write_step_pyarrow": spread(b[False]),
            "write_step_parts_ms_median": {k: round(statistics.median(v), 3) for k, v in sorted(parts.items())},
            "kernel_ms_median": {k: round(statistics.median(v), 4) for k, v in sorted(kern.items())},
            "file_bytes": {k: p.stat().st_size for k, p in files.items()}, "raw_value_bytes": pages.num_rows * pages.num_columns * 8,
            "summarize_files_device_written": spread(c["device"]), "summarize_files_pyarrow_written": spread(c["pyarrow"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="small,headline")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--tmp", default="/dev/shm" if Path("/dev/shm").is_dir() else None)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "parquet_write.json"))
    a = ap.parse_args()
    import pyarrow
    out = {"reps": a.reps, "format": "%.17g", "pyarrow": pyarrow.__version__, "shapes": {}}
    with _ffi.Context(0) as ctx:
        for shape in a.shapes.split(","):
            C, N, P = SHAPES[shape]
            with tempfile.TemporaryDirectory(dir=a.tmp) as td:
                r = measure(ctx, write_table(Path(td) / "draws.csv", C, N, P), Path(td), a.reps)
            out["shapes"][f"{shape}_{C}x{N}x{P}"] = r
            print(shape, json.dumps(r), flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

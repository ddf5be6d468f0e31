#!/usr/bin/env python3
"""Table CSV -> statistics: the device route (mcr_csv_* in table mode + the device row layout + summarize) against the
host route (pyarrow.csv.read_csv, table_to_tensor, upload, summarize) in one process, alternating, on seeded files
written here.

    python tools/csv_table_bench.py [--shapes small,headline] [--reps 9] [--out profiles/csv_table_ingest.json]

Per shape: median and range of `reps` runs of either route after one warm-up each, the device route's host-clock phases
(read + upload, line index, parse + host finish, layout + statistics), and the HIP-event time of its kernels from three
more profiled runs."""
import argparse, json, statistics, sys, tempfile, time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "mcmc-db_amd")]
from mcmc_ref_hip import _ffi, convert  # noqa: E402

SHAPES = {"small": (4, 1_000, 10), "headline": (4, 10_000, 100)}


def write_table(path: Path, C: int, N: int, P: int, fmt: str = "%.17g", seed: int = 4711) -> Path:
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(C * N, P)) * 10.0 ** rng.integers(-3, 4, size=P)
    ids = np.stack([np.repeat(np.arange(C), N), np.tile(np.arange(N), C)], axis=1).astype(np.float64)
    np.savetxt(path, np.hstack([ids, x]), fmt=["%d", "%d"] + [fmt] * P, delimiter=",", comments="",
               header=",".join(["chain", "draw"] + [f"theta.{i + 1}" for i in range(P)]))
    return path


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def measure(ctx, path: Path, reps: int) -> dict:
    import pyarrow.csv as pacsv

    def device(ph=None):
        t0 = time.perf_counter()
        d, fbuf, _ints = convert.read_csv_dev(path, context=ctx, phases=ph)
        fbuf.free()
        t1 = time.perf_counter()
        r = ctx.summarize(d.tensor)
        d.free()
        if ph is not None:
            ph["read_csv_dev_ms"], ph["statistics_ms"] = (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3
        return (time.perf_counter() - t0) * 1e3, d.params, r

    def host():
        t0 = time.perf_counter()
        table = pacsv.read_csv(path)
        t1 = time.perf_counter()
        params = [c for c in table.column_names if c not in ("chain", "draw")]
        x, counts = convert.table_to_tensor(table, params)
        t2 = time.perf_counter()
        t = ctx.upload(x.reshape(len(params), len(counts), int(counts[0])), "pcn")
        r = ctx.summarize(t)
        t.free()
        return (time.perf_counter() - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3, params, r

    _, nd, rd = device()
    _, _, _, nh, rh = host()
    same = nd == nh and all(np.array_equal(rd[k], rh[k], equal_nan=True) for k in rd)
    dev, hst, read_host, tensor_host, phases = [], [], [], [], []
    for _ in range(reps):
        ph = {}
        dev.append(device(ph)[0])
        phases.append(ph)
        ms, rms, tms, _, _ = host()
        hst.append(ms)
        read_host.append(rms)
        tensor_host.append(tms)
    ctx.profile(True)
    kern = {}
    for _ in range(3):
        ctx.profile_reset()
        d, fbuf, _ints = convert.read_csv_dev(path, context=ctx)
        fbuf.free()
        d.free()
        for k, v in ctx.profile_get().items():
            if k.startswith(("k_csv", "k_layout", "k_gather")):
                kern.setdefault(k, []).append(v["total_ms"])
    ctx.profile(False)
    ctx.profile_reset()
    return {"text_bytes": phases[0]["text_bytes"], "hard_fields": phases[0]["hard"], "results_identical": bool(same),
            "device_route": spread(dev), "host_route": spread(hst), "host_route_read_csv": spread(read_host),
            "host_route_table_to_tensor": spread(tensor_host), "device_below_host_range": max(dev) < min(hst),
            "device_phases_ms_median": {k: round(statistics.median(p[k] for p in phases), 3)
                                        for k in ("read_upload_ms", "index_ms", "parse_finish_ms", "read_csv_dev_ms", "statistics_ms")},
            "kernel_ms_median": {k: round(statistics.median(v), 4) for k, v in sorted(kern.items())}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="small,headline")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "csv_table_ingest.json"))
    a = ap.parse_args()
    out = {"reps": a.reps, "format": "%.17g", "shapes": {}}
    with _ffi.Context(0) as ctx:
        for shape in a.shapes.split(","):
            C, N, P = SHAPES[shape]
            with tempfile.TemporaryDirectory() as td:
                r = measure(ctx, write_table(Path(td) / "draws.csv", C, N, P), a.reps)
            out["shapes"][f"{shape}_{C}x{N}x{P}"] = r
            print(shape, json.dumps(r), flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

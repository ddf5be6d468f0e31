#!/usr/bin/env python3
"""Chain-list JSON archive -> resident draw tensor: the device route (inflate, mcr_json_open + mcr_json_decode) against
the host route it replaces (`_read_json_zip` = inflate + json.loads + np.asarray + pa.table, then `table_to_tensor` and
`ctx.upload`) in one process, alternating, on one seeded archive written here (json.dumps, default separators, repr
floats).

    python tools/json_bench.py [--shapes headline,small] [--reps 5] [--out profiles/json_ingest.json]

Per shape: median and range of `reps` runs of either route after one warm-up each, with the member's inflate included
and -- the same `zipfile` read on both routes, timed on its own -- excluded; the device route's host-clock phases
(inflate, upload + index + skeleton walk, parse + host finish); the HIP-event time of its kernels from three more
profiled runs, and the kernels' text rates beside mcr_hbm_probe's read rate."""
import argparse, json, statistics, sys, tempfile, time, zipfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "mcmc-db_amd")]
from mcmc_ref_hip import _ffi, convert  # noqa: E402

SHAPES = {"headline": (4, 10_000, 100), "small": (4, 1_000, 10)}


def write_archive(d: Path, C: int, N: int, P: int, seed: int = 4711) -> Path:
    rng = np.random.default_rng(seed)
    scale = 10.0 ** rng.integers(-3, 4, size=P)
    payload = [{f"theta[{p + 1}]": (rng.normal(size=N) * scale[p]).tolist() for p in range(P)} for _ in range(C)]
    path = d / "bench.json.zip"
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        zf.writestr("bench.json", json.dumps(payload))
    return path


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def measure(ctx, path: Path, reps: int) -> dict:
    def device(ph=None):
        t0 = time.perf_counter()
        params, t, ints = convert.read_json_zip_dev(path, context=ctx, phases=ph)
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3, params, t

    def host():
        t0 = time.perf_counter()
        table = convert._read_json_zip(path)
        t1 = time.perf_counter()
        params = [c for c in table.column_names if c not in {"chain", "draw"}]
        x, counts = convert.table_to_tensor(table, params)
        t2 = time.perf_counter()
        t = ctx.upload(x.reshape(len(params), len(counts), int(counts[0])), "pcn")
        ctx.sync()
        t3 = time.perf_counter()
        return (t3 - t0) * 1e3, {"read_json_zip_ms": (t1 - t0) * 1e3, "table_to_tensor_ms": (t2 - t1) * 1e3,
                                 "upload_ms": (t3 - t2) * 1e3}, params, t

    def inflate():
        t0 = time.perf_counter()
        with zipfile.ZipFile(path) as zf:
            n = len(zf.read(zf.namelist()[0]))
        return (time.perf_counter() - t0) * 1e3, n

    _, pd, td = device()
    _, _, ph_, th = host()
    n = int(np.prod(td.shape_cnp))
    same = pd == ph_ and td.shape_cnp == th.shape_cnp and np.array_equal(td.buf.download(np.uint64, n), th.buf.download(np.uint64, n))
    td.free()
    th.free()
    dev, hst, inf, phases, hphases = [], [], [], [], []
    for _ in range(reps):
        ph = {}
        ms, _, t = device(ph)
        t.free()
        dev.append(ms)
        phases.append(ph)
        ms, hp, _, t = host()
        t.free()
        hst.append(ms)
        hphases.append(hp)
        inf.append(inflate()[0])
    ctx.profile(True)
    kern = {}
    for _ in range(3):
        ctx.profile_reset()
        device()[2].free()
        for k, v in ctx.profile_get().items():
            if k.startswith("k_json") or k == "k_csv_patch":
                kern.setdefault(k, []).append(v["total_ms"])
    ctx.profile(False)
    ctx.profile_reset()
    text = phases[0]["text_bytes"]
    infl = statistics.median(inf)
    out = {"archive_bytes": path.stat().st_size, "text_bytes": text, "hard_elements": phases[0]["hard"], "tensors_identical": bool(same),
           "inflate": spread(inf),
           "device_route_inflate_included": spread(dev), "host_route_inflate_included": spread(hst),
           "device_route_inflate_excluded": spread([m - p["inflate_ms"] for m, p in zip(dev, phases)]),
           "host_route_inflate_excluded": spread([m - infl for m in hst]),
           "device_below_host_range_inflate_included": max(dev) < min(hst),
           "device_phases_ms_median": {k: round(statistics.median(p[k] for p in phases), 3)
                                       for k in ("inflate_ms", "upload_index_walk_ms", "parse_finish_ms")},
           "host_phases_ms_median": {k: round(statistics.median(p[k] for p in hphases), 3) for k in hphases[0]},
           "kernel_ms_median": {k: round(statistics.median(v), 4) for k, v in sorted(kern.items())}}
    out["speedup_inflate_excluded"] = round(out["host_route_inflate_excluded"]["median_ms"] / out["device_route_inflate_excluded"]["median_ms"], 2)
    out["speedup_inflate_included"] = round(out["host_route_inflate_included"]["median_ms"] / out["device_route_inflate_included"]["median_ms"], 2)
    for k in ("k_json_index", "k_json_parse"):
        if k in kern:
            out[f"{k}_GBps"] = round(text / statistics.median(kern[k]) / 1e6, 2)      # k_json_index: both passes over the text
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="headline,small")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "json_ingest.json"))
    a = ap.parse_args()
    out = {"reps": a.reps, "shapes": {}}
    with _ffi.Context(0) as ctx:
        out["hbm_read_GBps"] = round(ctx.hbm_probe(1 << 30, 3)["read_GBps"], 1)
        for shape in a.shapes.split(","):
            C, N, P = SHAPES[shape]
            with tempfile.TemporaryDirectory() as td:
                r = measure(ctx, write_archive(Path(td), C, N, P), a.reps)
            out["shapes"][f"{shape}_{C}x{N}x{P}"] = r
            print(shape, json.dumps(r), flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""CmdStan chain CSVs -> statistics: the device route (mcr_csv_* + summarize) against the host route (chains_tensor =
np.loadtxt per chain, upload, summarize) in one process, alternating, on seeded files written here.

    python tools/csv_bench.py [--shapes headline,small,large,golden] [--reps 9] [--out profiles/csv_ingest.json]

Per shape and number format: median and range of `reps` runs of either route after one warm-up each, the device route's
host-clock phases (read + upload, line index, parse + host finish, statistics), the HIP-event time of its kernels from
three more profiled runs, and the parse kernel's text rate beside mcr_hbm_probe's read rate."""
import argparse, json, statistics, sys, tempfile, time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "mcmc-db_amd")]
from mcmc_ref_hip import _ffi, cmdstan_generate as cs  # noqa: E402

SHAPES = {"headline": (4, 10_000, 100), "small": (4, 1_000, 10), "large": (4, 10_000, 1_000)}
INTERNAL = ["lp__", "accept_stat__", "stepsize__", "treedepth__", "n_leapfrog__", "divergent__", "energy__"]


def write_chains(d: Path, C: int, N: int, P: int, fmt: str, seed: int = 4711) -> list[Path]:
    names = INTERNAL + [f"theta.{i + 1}" for i in range(P)]
    paths = []
    for c in range(C):
        rng = np.random.default_rng(seed + c)
        x = rng.normal(size=(N, len(names))) * 10.0 ** rng.integers(-3, 4, size=len(names))
        p = d / f"chain_{c + 1}.csv"
        np.savetxt(p, x, fmt=fmt, delimiter=",", comments="", header="# model = bench\n# seed = %d\n%s\n# Adaptation terminated"
                   % (seed + c, ",".join(names)), footer="# \n#  Elapsed Time: 1 seconds")
        paths.append(p)
    return paths


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def measure(ctx, paths, reps: int) -> dict:
    def device(ph=None):
        t0 = time.perf_counter()
        names, t = cs.chains_tensor_dev(paths, context=ctx, phases=ph)
        t1 = time.perf_counter()
        r = ctx.summarize(t)
        t.free()
        if ph is not None:
            ph["statistics_ms"] = (time.perf_counter() - t1) * 1e3
        return (time.perf_counter() - t0) * 1e3, names, r

    def host():
        t0 = time.perf_counter()
        names, x = cs.chains_tensor(paths)
        t1 = time.perf_counter()
        t = ctx.upload(x)
        r = ctx.summarize(t)
        t.free()
        return (time.perf_counter() - t0) * 1e3, (t1 - t0) * 1e3, names, r

    _, nd, rd = device()
    _, _, nh, rh = host()
    same = nd == nh and all(np.array_equal(rd[k], rh[k], equal_nan=True) for k in rd)
    dev, hst, parse_host, phases = [], [], [], []
    for _ in range(reps):
        ph = {}
        dev.append(device(ph)[0])
        phases.append(ph)
        ms, pms, _, _ = host()
        hst.append(ms)
        parse_host.append(pms)
    ctx.profile(True)
    kern = {}
    for _ in range(3):
        ctx.profile_reset()
        names, t = cs.chains_tensor_dev(paths, context=ctx)
        t.free()
        for k, v in ctx.profile_get().items():
            if k.startswith("k_csv"):
                kern.setdefault(k, []).append(v["total_ms"])
    ctx.profile(False)
    ctx.profile_reset()
    text = phases[0]["text_bytes"]
    parse_ms = statistics.median(kern["k_csv_parse"]) if "k_csv_parse" in kern else float("nan")
    return {"text_bytes": text, "hard_fields": phases[0]["hard"], "results_identical": bool(same),
            "device_route": spread(dev), "host_route": spread(hst), "host_route_chains_tensor": spread(parse_host),
            "device_below_host_range": max(dev) < min(hst),
            "device_phases_ms_median": {k: round(statistics.median(p[k] for p in phases), 3)
                                        for k in ("read_upload_ms", "index_ms", "parse_finish_ms", "statistics_ms")},
            "kernel_ms_median": {k: round(statistics.median(v), 4) for k, v in sorted(kern.items())},
            "parse_kernel_GBps": round(text / parse_ms / 1e6, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="headline,small,golden")
    ap.add_argument("--formats", default="%.6g,%.17g")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "csv_ingest.json"))
    a = ap.parse_args()
    out = {"reps": a.reps, "shapes": {}}
    with _ffi.Context(0) as ctx:
        out["hbm_read_GBps"] = round(ctx.hbm_probe(1 << 30, 3)["read_GBps"], 1)
        for shape in a.shapes.split(","):
            if shape == "golden":       # the 40-row test files: launch overhead against a tiny host parse
                g = ROOT / "tests" / "golden" / "cmdstan"
                out["shapes"]["golden_4x40x11"] = measure(ctx, [g / "chain_1.csv", g / "chain_2.csv"] * 2, a.reps)
                continue
            C, N, P = SHAPES[shape]
            for fmt in a.formats.split(","):
                with tempfile.TemporaryDirectory() as td:
                    r = measure(ctx, write_chains(Path(td), C, N, P, fmt), a.reps)
                r["parse_share_of_hbm_read"] = round(r["parse_kernel_GBps"] / out["hbm_read_GBps"], 4)
                out["shapes"][f"{shape}_{C}x{N}x{P}_{fmt}"] = r
                print(shape, fmt, json.dumps(r), flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

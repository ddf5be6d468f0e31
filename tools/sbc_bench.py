#!/usr/bin/env python3
"""Simulation-based calibration (mcr_sbc_ranks_dev): what k_sbc_ranks and the whole call cost on each route, next to the
streaming moments kernel reading the same bytes and to numpy doing the same on the host.

    python tools/sbc_bench.py [--reps 9] [--out profiles/sbc.json]

Workloads, f64, resident on the device (filled there: mcr_fill_synthetic), truth N(0, 1):
1 000 simulations x (4 chains x 1 000 draws) x 100 parameters as "spcn" -- read in place, one launch -- and as "scnp" -- the
ingest copy, chunked by the workspace limit --, and 10 000 x (1 x 100) x 10 as "spcn": short rows, launch-bound.
Per workload, after one warm-up (the first and the last simulation are checked against the library's host routine, bit for
bit), with the runs of the call, of the profiled call and of the moments kernel ALTERNATING, `reps` of each:

1. the whole call on the host clock: median / min / max,
2. the HIP-event time and the launches of every kernel of a call (`Context.profile`), the share of k_ingest in the kernel time,
3. the achieved read rate of k_sbc_ranks: 8 bytes per draw, counted ONCE (the second pass runs on registers up to 4 096
   draws per row, on the caches above), and that rate as a share of
4. k_moments' (the streaming moments kernel: one pass, 16-byte loads) on the same buffer seen as 100 rows, in the same run,
5. numpy on 16 threads doing the same: (x < t).sum(-1), x.mean(-1), x.std(-1), the simulations dealt to a pool of 16
   threads; median of 3.
"""
import argparse, json, statistics, sys, time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "mcmc-db_amd")]
from mcmc_ref_hip import _ffi  # noqa: E402

SHAPES = ((1000, 4, 1000, 100, "spcn"), (1000, 4, 1000, 100, "scnp"), (10_000, 1, 100, 10, "spcn"))
HOST_THREADS = 16
KEYS = ("n_less", "n_equal", "mean", "sd")


def spread(ms, digits=4):
    return {"median_ms": round(statistics.median(ms), digits), "min_ms": round(min(ms), digits), "max_ms": round(max(ms), digits)}


def numpy_some(x, t):
    return (x < t[..., None]).sum(-1), x.mean(-1), x.std(-1)


def download(ctx, buf, first: int, count: int) -> np.ndarray:
    out = np.empty(count)
    ctx._check(ctx.lib.mcr_memcpy_d2h(ctx.handle, out.ctypes.data_as(_ffi.C.c_void_p), _ffi.C.c_void_p(buf.ptr.value + 8 * first), out.nbytes))
    return out


def simulation(ctx, buf, s: int, C_, N, P, layout) -> np.ndarray:
    """Simulation s of the buffer as [P][L]."""
    one = download(ctx, buf, s * C_ * N * P, C_ * N * P)
    return one.reshape(P, C_ * N) if layout == "spcn" else np.ascontiguousarray(one.reshape(C_ * N, P).T)


def measure(ctx, S, C_, N, P, layout, reps):
    L, total = C_ * N, S * C_ * N * P
    truth = np.random.default_rng(4711).standard_normal((S, P))
    flat = ctx.alloc_tensor(1, total // 100, 100)                     # the same bytes as 100 rows: what k_moments streams
    ctx.fill_synthetic(flat)
    strides = (P * L, N, 1, L) if layout == "spcn" else (P * L, N * P, P, 1)
    t = _ffi.DeviceSims(ctx, flat.buf, (_ffi.MCR_F64, S, C_, N, P, *strides))
    out = {"workload": {"simulations": S, "chains": C_, "draws_per_chain": N, "parameters": P, "row_length": L, "rows": S * P,
                        "layout": layout, "dtype": "f64", "bytes": 8 * total},
           "simulations_per_chunk": ctx.sbc_sims_per_chunk(t)}
    call = lambda: ctx.sbc_ranks(t, truth)
    got = call()                                                      # warm-up, and the check
    for s in (0, S - 1):
        h = _ffi.sbc_ranks_host(simulation(ctx, flat.buf, s, C_, N, P, layout)[None], truth[s:s + 1])
        assert all(np.array_equal(got[k][s], h[k][0]) for k in KEYS), (layout, s)
    ctx.moments(flat)
    wall, kern, launches, mom = [], {}, {}, []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
        ctx.profile(True)
        ctx.profile_reset()
        call()
        for k, v in ctx.profile_get().items():
            kern.setdefault(k, []).append(v["total_ms"])
            launches[k] = v["launches"]
        ctx.profile_reset()
        ctx.moments(flat)
        mom.append(ctx.profile_get()["k_moments"]["total_ms"])
        ctx.profile(False)
        ctx.profile_reset()
    x = download(ctx, flat.buf, 0, total).reshape(S, P, L) if layout == "spcn" else None
    flat.free()
    med = {k: statistics.median(v) for k, v in kern.items()}
    rate, mom_rate = 8 * total / med["k_sbc_ranks"] / 1e6, 8 * total / statistics.median(mom) / 1e6
    out.update({"call": spread(wall, 3),
                "kernels_ms_per_call": {k: spread(v) for k, v in sorted(kern.items())},
                "launches_per_call": dict(sorted(launches.items())),
                "k_ingest_share_of_kernel_time": round(med.get("k_ingest", 0.0) / sum(med.values()), 3),
                "k_sbc_ranks_GB_per_s": round(rate, 1),
                "k_moments_same_bytes": {**spread(mom), "GB_per_s": round(mom_rate, 1)},
                "k_sbc_ranks_rate_over_k_moments": round(rate / mom_rate, 3)})
    if x is not None:
        host = []
        cuts = np.array_split(np.arange(S), min(S, 4 * HOST_THREADS))
        with ThreadPoolExecutor(HOST_THREADS) as pool:
            for _ in range(3):
                t0 = time.perf_counter()
                parts = list(pool.map(lambda c: numpy_some(x[c[0]:c[-1] + 1], truth[c[0]:c[-1] + 1]), cuts))
                host.append((time.perf_counter() - t0) * 1e3)
        assert np.array_equal(np.concatenate([p[0] for p in parts]), got["n_less"])
        out.update({"numpy_16_threads": spread(host, 3), "numpy_over_call": round(statistics.median(host) / statistics.median(wall), 2)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sbc.json"))
    a = ap.parse_args()
    out = {"reps": a.reps, "block": _ffi.MCR_WEIGHTED_BLOCK, "host_threads": HOST_THREADS, "shapes": []}
    with _ffi.Context(0) as ctx:
        for S, C_, N, P, layout in SHAPES:
            out["shapes"].append(measure(ctx, S, C_, N, P, layout, a.reps))
            print(json.dumps(out["shapes"][-1]), flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

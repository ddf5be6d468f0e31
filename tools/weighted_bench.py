#!/usr/bin/env python3
"""Importance-weighted summaries (mcr_weighted_summary_dev): what the new kernels and the whole call cost, next to the sort
stage they reuse and to numpy doing the same on the host.

    python tools/weighted_bench.py [--reps 9] [--out profiles/weighted.json]

Workloads, f64, resident on the device, three quantiles (0.05, 0.5, 0.95), linear weights exp(N(0, 1)):
4 chains x 10 000 draws x 100 parameters, 4 x 1 000 x 10, and 4 x 250 000 x 16 -- a million pooled draws, whose 8 MB weight
vector no longer fits an XCD's 4 MiB L2: the gather of k_wq_blocks leaves it.  Per workload, after one warm-up (three
parameters are checked against the library's host routine, bit for bit),

1. the whole call on the host clock: median / min / max of `reps` unprofiled runs,
2. the HIP-event time of every kernel of a call (`Context.profile`, runs of their own: the events cost a little), the new
   kernels' sum and its share next to the sort stage they follow (every other kernel of the call but k_finalize),
3. the achieved read rate of k_weighted_moments (two passes x (8 bytes of draw + 8 of weight) per draw and parameter) and
   of k_wq_blocks (a position and an 8-byte gathered weight per draw and parameter),
4. numpy on 16 threads doing the same: np.average and a weighted variance plus np.quantile(weights=, method="inverted_cdf")
   per parameter, the parameters dealt to a pool of 16 threads (numpy releases the GIL in its sort); median of 3.
"""
import argparse, json, statistics, sys, time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "mcmc-db_amd")]
from mcmc_ref_hip import _ffi  # noqa: E402

SHAPES = ((4, 10_000, 100), (4, 1_000, 10), (4, 250_000, 16))
QS = (0.05, 0.5, 0.95)
NEW = ("k_weight_prepare", "k_weighted_moments", "k_weighted_combine", "k_wq_blocks", "k_wq_pick")
HOST_THREADS = 16


def spread(ms, digits=4):
    return {"median_ms": round(statistics.median(ms), digits), "min_ms": round(min(ms), digits), "max_ms": round(max(ms), digits)}


def numpy_one(x, w):
    mean = np.average(x, weights=w)
    d = x - mean
    s1 = w.sum()
    return mean, np.sqrt((w * d * d).sum() / s1), np.sqrt((w * w * d * d).sum()) / s1, np.quantile(x, QS, weights=w, method="inverted_cdf")


def measure(ctx, C_, N, P, reps):
    M = C_ * N
    rng = np.random.default_rng(4711)
    x = rng.standard_normal((P, C_, N))
    w = np.exp(rng.standard_normal(M))
    t = ctx.upload(x)
    out = {"workload": {"chains": C_, "draws_per_chain": N, "parameters": P, "pooled_draws": M, "dtype": "f64", "quantiles": list(QS),
                        "weight_vector_bytes": 8 * M},
           "parameters_per_chunk": ctx.weighted_params_per_chunk(t, len(QS))}
    call = lambda: ctx.weighted_summary(t, weights=w, quantiles=QS)
    got = call()                                                  # warm-up, and the check
    for p in (0, P // 2, P - 1):
        h = _ffi.weighted_host(x[p].reshape(-1), weights=w, quantiles=QS)
        assert all(got[k][p] == h[k] for k in ("mean", "sd", "mean_se")) and (got["quantiles"][p] == h["quantiles"]).all()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
    ctx.profile(True)
    kern = {}
    for _ in range(reps):
        ctx.profile_reset()
        call()
        for k, v in ctx.profile_get().items():
            if v["launches"]:
                kern.setdefault(k, []).append(v["total_ms"])
    ctx.profile(False)
    ctx.profile_reset()
    t.free()
    flat = x.reshape(P, M)
    host = []
    with ThreadPoolExecutor(HOST_THREADS) as pool:
        for _ in range(3):
            t0 = time.perf_counter()
            list(pool.map(lambda row: numpy_one(row, w), flat))
            host.append((time.perf_counter() - t0) * 1e3)
    med = {k: statistics.median(v) for k, v in kern.items()}
    new = sum(med[k] for k in NEW)
    sort = sum(v for k, v in med.items() if k not in NEW + ("k_finalize",))
    pos_bytes = 2 if M <= 65_535 else 4
    mom_bytes = 2 * 16 * M * P
    blk_bytes = (pos_bytes + 8) * M * P
    out.update({"call": spread(wall, 3),
                "kernels_ms_per_call": {k: spread(v) for k, v in sorted(kern.items())},
                "sort_stage_ms": round(sort, 4), "new_kernels_ms": round(new, 4),
                "sort_stage_share_of_kernel_time": round(sort / (sort + new + med.get("k_finalize", 0.0)), 3),
                "new_kernels_over_sort_stage": round(new / sort, 3),
                "k_weighted_moments_bytes_per_call": mom_bytes,
                "k_weighted_moments_GB_per_s": round(mom_bytes / med["k_weighted_moments"] / 1e6, 1),
                "k_wq_blocks_bytes_per_call": blk_bytes,
                "k_wq_blocks_GB_per_s": round(blk_bytes / med["k_wq_blocks"] / 1e6, 1),
                "numpy_16_threads": spread(host, 3),
                "numpy_over_call": round(statistics.median(host) / statistics.median(wall), 2)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "weighted.json"))
    a = ap.parse_args()
    out = {"reps": a.reps, "block": _ffi.MCR_WEIGHTED_BLOCK, "host_threads": HOST_THREADS, "shapes": []}
    with _ffi.Context(0) as ctx:
        for C_, N, P in SHAPES:
            out["shapes"].append(measure(ctx, C_, N, P, a.reps))
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Highest-density intervals (mcr_hdi_dev): what the two new kernels and the whole call cost, next to the sort stage they reuse.

    python tools/hdi_bench.py [--reps 9] [--out profiles/hdi.json]

Workloads, f64, resident on the device: 4 chains x 10 000 draws x 100 parameters and 4 x 100 000 x 10, gamma(2) draws (a
skewed parameter), prob = (0.5, 0.9, 0.94) in one call.  Per workload, after one warm-up of both calls (the intervals of
three parameters are checked against the library's host routine),

1. the whole hdi call and the stats-only summarize (diagnostics=False) of the same tensor on the host clock, ALTERNATING,
   median / min / max of `reps` unprofiled runs each,
2. the HIP-event time of every kernel of an hdi call (`Context.profile`, runs of their own: the events cost a little),
3. k_hdi_window + k_hdi_pick against the sort stage they follow (every other kernel of the call but k_finalize), and
   k_hdi_window's rate over the bytes it has to read: 2 streams x 8 bytes x W windows per (parameter, probability).
"""
import argparse, json, math, statistics, sys, time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "mcmc-db_amd")]
from mcmc_ref_hip import _ffi  # noqa: E402

SHAPES = ((4, 10_000, 100), (4, 100_000, 10))
PROBS = (0.5, 0.9, 0.94)
NEW = ("k_hdi_window", "k_hdi_pick")


def spread(ms, digits=4):
    return {"median_ms": round(statistics.median(ms), digits), "min_ms": round(min(ms), digits), "max_ms": round(max(ms), digits)}


def measure(ctx, C_, N, P, reps):
    M = C_ * N
    x = np.random.default_rng(4711).gamma(2.0, size=(P, C_, N))
    t = ctx.upload(x)
    out = {"workload": {"chains": C_, "draws_per_chain": N, "parameters": P, "pooled_draws": M, "dtype": "f64", "prob": list(PROBS)},
           "parameters_per_chunk": ctx.hdi_params_per_chunk(t, len(PROBS))}
    hdi = lambda: ctx.hdi(t, prob=PROBS)
    stats = lambda: ctx.summarize(t, diagnostics=False)
    got = hdi()                                                   # warm-up, and the check
    stats()
    for p in (0, P // 2, P - 1):
        lo, hi, idx = _ffi.hdi_sorted_host(np.sort(x[p].reshape(-1)), PROBS)
        assert (got["lo"][p] == lo).all() and (got["hi"][p] == hi).all() and (got["index"][p] == idx).all()
    wall = {"hdi": [], "summarize_stats_only": []}
    for _ in range(reps):                                         # alternating
        for name, fn in (("hdi", hdi), ("summarize_stats_only", stats)):
            t0 = time.perf_counter()
            fn()
            wall[name].append((time.perf_counter() - t0) * 1e3)
    ctx.profile(True)
    kern = {}
    for _ in range(reps):
        ctx.profile_reset()
        hdi()
        for k, v in ctx.profile_get().items():
            if v["launches"]:
                kern.setdefault(k, []).append(v["total_ms"])
    ctx.profile(False)
    ctx.profile_reset()
    t.free()
    med = {k: statistics.median(v) for k, v in kern.items()}
    new = sum(med[k] for k in NEW)
    sort = sum(v for k, v in med.items() if k not in NEW + ("k_finalize",))
    windows = [M - int(math.floor(q * M)) for q in PROBS]
    nbytes = 2 * 8 * sum(windows) * P
    out.update({"windows": windows, "slices": [-(-w // _ffi.MCR_HDI_SLICE) for w in windows],
                "call": {k: spread(v, 3) for k, v in wall.items()},
                "kernels_ms_per_call": {k: spread(v) for k, v in sorted(kern.items())},
                "window_bytes_per_call": nbytes, "k_hdi_window_GB_per_s": round(nbytes / med["k_hdi_window"] / 1e6, 1),
                "sort_stage_ms": round(sort, 4), "new_kernels_ms": round(new, 4),
                "new_kernels_over_sort_stage": round(new / sort, 3),
                "hdi_over_summarize_stats_only": round(statistics.median(wall["hdi"]) /
                                                       statistics.median(wall["summarize_stats_only"]), 3)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "hdi.json"))
    a = ap.parse_args()
    out = {"reps": a.reps, "slice": _ffi.MCR_HDI_SLICE, "shapes": []}
    with _ffi.Context(0) as ctx:
        for C_, N, P in SHAPES:
            out["shapes"].append(measure(ctx, C_, N, P, a.reps))
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

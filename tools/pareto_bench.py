#!/usr/bin/env python3
"""Pareto k-hat (mcr_pareto_khat_dev): what the new kernel and the whole call cost, next to the stats-only summary.

    python tools/pareto_bench.py [--reps 9] [--out profiles/pareto_khat.json]

Workloads, f64, resident on the device: 4 chains x 10 000 draws x 100 parameters and 4 x 100 000 x 10, Student-t(3) draws.
Per workload, after one warm-up of both calls (the k-hat of three parameters is checked against the library's host fit),

1. the whole pareto_khat call and the stats-only summarize (diagnostics=False) of the same tensor on the host clock,
   ALTERNATING, median / min / max of `reps` unprofiled runs each,
2. the HIP-event time of every kernel of a pareto_khat call (`Context.profile`, runs of their own: the events cost a little),
3. k_pareto_fit alone against the sort stage it follows (every other kernel of the call but k_finalize), and its log1p
   rate: 2 tails x (G + 1) x t evaluations per parameter, G = 30 + floor(sqrt(t)).
"""
import argparse, json, math, statistics, sys, time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "mcmc-db_amd")]
from mcmc_ref_hip import _ffi  # noqa: E402

SHAPES = ((4, 10_000, 100), (4, 100_000, 10))


def spread(ms, digits=4):
    return {"median_ms": round(statistics.median(ms), digits), "min_ms": round(min(ms), digits), "max_ms": round(max(ms), digits)}


def measure(ctx, C_, N, P, reps):
    M = C_ * N
    x = np.random.default_rng(4711).standard_t(3, size=(P, C_, N))
    t = ctx.upload(x)
    out = {"workload": {"chains": C_, "draws_per_chain": N, "parameters": P, "pooled_draws": M, "dtype": "f64"},
           "parameters_per_chunk": ctx.pareto_params_per_chunk(t)}
    khat = lambda: ctx.pareto_khat(t)
    stats = lambda: ctx.summarize(t, diagnostics=False)
    got = khat()                                                  # warm-up, and the check
    stats()
    for p in (0, P // 2, P - 1):
        kl, kr, tail = _ffi.pareto_fit_host(np.sort(x[p].reshape(-1)))
        assert tail == got["ndraws_tail"][p] and abs(got["khat_left"][p] - kl) <= 1e-9 and abs(got["khat_right"][p] - kr) <= 1e-9
    tail = int(got["ndraws_tail"][0])
    wall = {"pareto_khat": [], "summarize_stats_only": []}
    for _ in range(reps):                                         # alternating
        for name, fn in (("pareto_khat", khat), ("summarize_stats_only", stats)):
            t0 = time.perf_counter()
            fn()
            wall[name].append((time.perf_counter() - t0) * 1e3)
    ctx.profile(True)
    kern = {}
    for _ in range(reps):
        ctx.profile_reset()
        khat()
        for k, v in ctx.profile_get().items():
            if v["launches"]:
                kern.setdefault(k, []).append(v["total_ms"])
    ctx.profile(False)
    ctx.profile_reset()
    t.free()
    med = {k: statistics.median(v) for k, v in kern.items()}
    fit = med["k_pareto_fit"]
    sort = sum(v for k, v in med.items() if k not in ("k_pareto_fit", "k_finalize"))
    evals = P * 2 * (30 + math.isqrt(tail) + 1) * tail
    out.update({"ndraws_tail": tail, "grid_points": 30 + math.isqrt(tail),
                "call": {k: spread(v, 3) for k, v in wall.items()},
                "kernels_ms_per_call": {k: spread(v) for k, v in sorted(kern.items())},
                "log1p_per_call": evals, "k_pareto_fit_log1p_per_us": round(evals / fit / 1e3, 1),
                "sort_stage_ms": round(sort, 4), "k_pareto_fit_over_sort_stage": round(fit / sort, 3),
                "pareto_khat_over_summarize_stats_only": round(statistics.median(wall["pareto_khat"]) /
                                                               statistics.median(wall["summarize_stats_only"]), 3)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pareto_khat.json"))
    a = ap.parse_args()
    out = {"reps": a.reps, "lds_tail": _ffi.MCR_PARETO_LDS_TAIL, "shapes": []}
    with _ffi.Context(0) as ctx:
        for C_, N, P in SHAPES:
            out["shapes"].append(measure(ctx, C_, N, P, a.reps))
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

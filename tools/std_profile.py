#!/usr/bin/env python3
"""Times standard.diagnostics (include/mcmcref_std.h) and writes profiles/std_diagnostics.json: 4 chains x 10 000 draws x
100 parameters, f64, iid and AR(1) with phi = 0.99, on a device tensor.  Per shape the median of 9 runs of the call and of
Context.summarize on the same tensor, the two alternating run by run after one warm-up each; the phase times of
mcs_kernel_ms from 9 further, timed runs; and the numpy restatement of tests/std_cases.py on 16 threads, once.
"""
from __future__ import annotations

import json
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT / "mcmc-db_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))

import std_cases as sc  # noqa: E402
from mcmc_ref_hip import _ffi, standard  # noqa: E402

C_, N, P, RUNS = 4, 10000, 100, 9


def draws(phi: float) -> np.ndarray:
    rng = np.random.default_rng(990 if phi else 1)
    return np.stack([sc.ar1(rng, C_, N, phi) if phi else rng.standard_normal((C_, N)) for _ in range(P)])


def timed(fn) -> float:
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def main() -> None:
    out = {"shape": {"chains": C_, "draws": N, "params": P, "dtype": "f64", "layout": "pcn"}, "runs": RUNS,
           "method": "median of 9 alternating wall-clock runs of the synchronous calls on a device tensor, ms", "cases": {}}
    with _ffi.Context(0) as ctx:
        for name, phi in (("iid", 0.0), ("ar0.99", 0.99)):
            x = draws(phi)
            with ctx.upload(x, "pcn") as t:
                std_call = lambda: standard.diagnostics(t, basic=True, context=ctx)      # noqa: E731
                sum_call = lambda: ctx.summarize(t)                                        # noqa: E731
                r = std_call()
                sum_call()
                a, b = [], []
                for _ in range(RUNS):
                    a.append(timed(std_call))
                    b.append(timed(sum_call))
                standard.profile(True, ctx)
                ks = []
                for _ in range(RUNS):
                    std_call()
                    ks.append(standard.kernel_ms(ctx))
                standard.profile(False, ctx)
            with ThreadPoolExecutor(16) as pool:
                t0 = time.perf_counter()
                ref = list(pool.map(sc.restate, x))
                numpy_ms = (time.perf_counter() - t0) * 1e3
            worst = max(abs(r[k][p] - ref[p][k]) / abs(ref[p][k]) for p in range(P) for k in ("ess_bulk", "ess_tail", "ess_mean", "rhat"))
            out["cases"][name] = {
                "std_diagnostics_ms": statistics.median(a), "summarize_ms": statistics.median(b),
                "kernel_ms": {k: statistics.median(v[k] for v in ks) for k in ks[0]},
                "numpy_restatement_16_threads_ms": numpy_ms, "worst_rel_diff_to_restatement": worst,
                "lags_equal": all(int(r[k][p]) == ref[p][k] for p in range(P) for k in sc.LAGS),
                "lag_bulk_max": int(r["lag_bulk"].max()), "lag_mean_max": int(r["lag_mean"].max()),
                "ess_bulk_median": float(np.median(r["ess_bulk"])), "rhat_max": float(r["rhat"].max())}
    c = out["cases"]
    out["ar0.99_over_iid"] = c["ar0.99"]["std_diagnostics_ms"] / c["iid"]["std_diagnostics_ms"]
    path = ROOT / "profiles" / "std_diagnostics.json"
    path.write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

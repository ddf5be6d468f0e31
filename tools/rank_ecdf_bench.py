#!/usr/bin/env python3
"""Times rankecdf.rank_ecdf (include/mcmcref_recdf.h) and writes profiles/rank_ecdf.json: 4 chains x 10 000 draws x 100
parameters, f64, K = 100 points, thin = 1, on a device tensor.  The median of 9 runs of the call (its null sample cached)
and of Context.summarize on the same tensor, the two alternating run by run after one warm-up each; the kernel times of
mce_kernel_ms from 9 further, timed runs; the count kernel's read rate (bytes of draws / its time) beside
Context.hbm_probe's read rate over a buffer of that size in the same run; the null sample of (4, 1 000, 100, S = 4 000),
uncached, 9 runs, with its kernel times; and the numpy restatement (sort, `<=`, sum, table look-up) of the same draws
and of the same null sample on 16 threads, once each.  There is no gate: the numbers are recorded, not promised.
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
sys.path.insert(0, str(ROOT / "mcmc-db_amd"))

from mcmc_ref_hip import _ffi, rankecdf  # noqa: E402

C_, N, P, K, RUNS = 4, 10000, 100, 100, 9
NULL = dict(C_=4, n=1000, points=100, sims=4000, seed=0)


def timed(fn) -> float:
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def restate(x: np.ndarray, points: int, tab: np.ndarray):
    """One parameter x[C][n] by the definition in numpy: (counts, g)."""
    M, n = x.size, x.shape[1]
    s = np.sort(x.ravel())
    m = np.arange(1, points, dtype=np.int64) * M // points
    a = np.stack([np.searchsorted(np.sort(c), s[m - 1], side="right") for c in x])
    return a, tab[np.arange(points - 1)[None, :], a].min()


def null_draws(s: int, C__: int, n: int, seed: int) -> np.ndarray:
    G = np.uint64(0x9E3779B97F4A7C15)
    M = C__ * n
    with np.errstate(over="ignore"):
        z = np.full(M, seed, dtype=np.uint64) * G + (np.uint64(s * M) + np.arange(M, dtype=np.uint64)) + G
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return ((z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53).reshape(C__, n)


def median_ms(ks: list) -> dict:
    return {k: statistics.median(v[k] for v in ks) for k in ks[0]}


def main() -> None:
    x = np.random.default_rng(1).standard_normal((P, C_, N))
    out = {"shape": {"chains": C_, "draws": N, "params": P, "dtype": "f64", "layout": "pcn", "points": K, "thin": 1}, "runs": RUNS,
           "method": "median of 9 alternating wall-clock runs of the synchronous calls on a device tensor, ms; kernel_ms: "
                     "medians of mce_kernel_ms over 9 further runs"}
    with _ffi.Context(0) as ctx:
        with ctx.upload(x, "pcn") as t:
            call = lambda: rankecdf.rank_ecdf(t, points=K, context=ctx)          # noqa: E731  (sims = 4000, cached after the first)
            sum_call = lambda: ctx.summarize(t)                                   # noqa: E731
            first_ms = timed(call)
            r = call()
            sum_call()
            a, b = [], []
            for _ in range(RUNS):
                a.append(timed(call))
                b.append(timed(sum_call))
            rankecdf.profile(True, ctx)
            ks = []
            for _ in range(RUNS):
                call()
                ks.append(rankecdf.kernel_ms(ctx))
            rankecdf.profile(False, ctx)
        kernel = median_ms(ks)
        probe = ctx.hbm_probe(x.nbytes, 9)
        out["rank_ecdf_ms"] = statistics.median(a)
        out["rank_ecdf_first_call_with_its_null_sample_ms"] = first_ms
        out["summarize_ms"] = statistics.median(b)
        out["kernel_ms"] = kernel
        out["draw_bytes"] = int(x.nbytes)
        out["count_read_GBps"] = x.nbytes / (kernel["count"] * 1e-3) / 1e9
        out["hbm_probe_read_GBps_same_size"] = probe["read_GBps"]
        out["rejected_of_100_iid"] = int(r["reject"].sum())
        runs, ks = [], []
        rankecdf.profile(True, ctx)
        for _ in range(RUNS + 1):                                                # (the first is the warm-up)
            rankecdf.clear_null_cache(ctx)
            runs.append(timed(lambda: rankecdf.null_sample(context=ctx, **NULL)))
            ks.append(rankecdf.kernel_ms(ctx))
        rankecdf.profile(False, ctx)
        g0 = rankecdf.null_sample(context=ctx, **NULL)
        out["null_sample"] = {"shape": {"chains": 4, "draws": 1000, "points": 100, "sims": 4000},
                              "call_ms_timed_kernels": statistics.median(runs[1:]), "kernel_ms": median_ms(ks[1:]),
                              "sims_per_chunk": rankecdf.sims_per_chunk(4, 1000, 100, 4000, context=ctx)}
    tab = rankecdf.table(C_ * N, N, K)
    with ThreadPoolExecutor(16) as pool:
        t0 = time.perf_counter()
        ref = list(pool.map(lambda xp: restate(xp, K, tab), x))
        out["numpy_restatement_16_threads_ms"] = (time.perf_counter() - t0) * 1e3
        tab0 = rankecdf.table(4000, 1000, 100)
        t0 = time.perf_counter()
        ref0 = list(pool.map(lambda s: restate(null_draws(s, 4, 1000, 0), 100, tab0)[1], range(4000)))
        out["null_sample"]["numpy_restatement_16_threads_ms"] = (time.perf_counter() - t0) * 1e3
    out["counts_equal_restatement"] = all(np.array_equal(r["counts"][p], ref[p][0]) for p in range(P))
    out["g_equal_restatement"] = all(r["g"][p] == ref[p][1] for p in range(P))
    out["null_sample"]["equal_restatement"] = bool(np.array_equal(g0, np.array(ref0)))
    path = ROOT / "profiles" / "rank_ecdf.json"
    path.write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

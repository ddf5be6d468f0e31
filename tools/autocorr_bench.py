#!/usr/bin/env python3
"""Autocorrelation functions and times (mcr_autocorr_dev): what the call and its lag-product kernel cost, next to numpy.

    python tools/autocorr_bench.py [--reps 9] [--out profiles/autocorr.json]

Workloads, f64 AR(1) draws, resident on the device: 4 chains x 10 000 draws x 100 parameters at max_lag 100 and 1 000, and
1 000 chains x 100 draws x 100 parameters at max_lag 50.  Per workload, after one warm-up of both sides (three parameters
are checked in bits against the library's host routine),

1. the whole autocorr call and numpy computing the same ACF by zero-padded FFT on the host (arviz.autocorr's formula, all
   chains of a parameter in one rfft call, the parameters spread over 16 threads: the baseline a user has today) on the host
   clock, ALTERNATING, median / min / max of `reps` unprofiled runs each,
2. the HIP-event time of every kernel of a call (`Context.profile`, runs of their own: the events cost a little),
3. k_acf_products' executed fp64 FMA rate -- 16 per thread and step of 4 draws, the padding of the last step and of the
   last lag quad included -- as a fraction of the 39.3 T FMA/s (78.6 TFLOP/s) vector fp64 peak DESIGN.md uses, and the
   useful rate: the sum over l <= L of (N - l) products per chain.
"""
import argparse, json, statistics, sys, time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "mcmc-db_amd")]
from mcmc_ref_hip import _ffi  # noqa: E402

SHAPES = ((4, 10_000, 100, 100), (4, 10_000, 100, 1_000), (1_000, 100, 100, 50))      # C, N, P, max_lag
PEAK_FMA_PER_S = 39.3e12
THREADS = 16
B = _ffi.MCR_ACF_BLOCK


def spread(ms, digits=4):
    return {"median_ms": round(statistics.median(ms), digits), "min_ms": round(min(ms), digits), "max_ms": round(max(ms), digits)}


def numpy_acf(x, L, pool):
    """acf [P][C][L+1] by FFT, one parameter (all its chains) per task."""
    N = x.shape[2]
    size = 1 << int(np.ceil(np.log2(2 * N)))

    def one(xp):
        f = np.fft.rfft(xp - xp.mean(axis=1, keepdims=True), size, axis=1)
        cov = np.fft.irfft(f * np.conj(f), size, axis=1)[:, :L + 1]
        return cov / cov[:, :1]
    return np.stack(list(pool.map(one, x)))


def executed_fmas(C_, N, P, L):
    """The fma k_acf_products issues: per (chain, draw block, lag quad) ceil(min(B, N - 4 q - b B) / 4) steps of 16."""
    nq, nblk, steps = (L + 4) // 4, -(-N // B), 0
    for b in range(nblk):
        rem = np.clip(N - 4 * np.arange(nq) - b * B, 0, B)
        steps += int(((rem + 3) // 4).sum())
    return 16 * steps * C_ * P


def ar1(P, C_, N, seed=4711, phi=0.7):
    e = np.random.default_rng(seed).standard_normal((P, C_, N))
    x = np.empty_like(e)
    x[..., 0] = e[..., 0]
    for t in range(1, N):
        x[..., t] = phi * x[..., t - 1] + e[..., t]
    return x


def measure(ctx, pool, C_, N, P, L, reps):
    x = ar1(P, C_, N)
    t = ctx.upload(x)
    out = {"workload": {"chains": C_, "draws_per_chain": N, "parameters": P, "max_lag": L, "dtype": "f64"},
           "parameters_per_chunk": ctx.autocorr_params_per_chunk(t, L)}
    gpu = lambda: ctx.autocorr(t, max_lag=L)
    cpu = lambda: numpy_acf(x, L, pool)
    got = gpu()                                                   # warm-up, and the checks
    ref = cpu()
    out["max_abs_diff_numpy_fft"] = float(np.max(np.abs(got["acf"] - ref)))
    for p in (0, P // 2, P - 1):
        host = _ffi.autocorr_host(x[p], max_lag=L)
        assert all(np.array_equal(got[k][p], host[k][0], equal_nan=True) for k in ("acf", "tau", "window", "acf_pooled", "tau_pooled"))
    wall = {"autocorr": [], "numpy_fft_16_threads": []}
    for _ in range(reps):                                         # alternating
        for name, fn in (("autocorr", gpu), ("numpy_fft_16_threads", cpu)):
            t0 = time.perf_counter()
            fn()
            wall[name].append((time.perf_counter() - t0) * 1e3)
    ctx.profile(True)
    kern = {}
    for _ in range(reps):
        ctx.profile_reset()
        gpu()
        for k, v in ctx.profile_get().items():
            if v["launches"]:
                kern.setdefault(k, []).append(v["total_ms"])
    ctx.profile(False)
    ctx.profile_reset()
    t.free()
    prod_ms = statistics.median(kern["k_acf_products"])
    executed = executed_fmas(C_, N, P, L)
    useful = C_ * P * sum(N - l for l in range(L + 1))
    out.update({"call": {k: spread(v, 3) for k, v in wall.items()},
                "numpy_over_autocorr": round(statistics.median(wall["numpy_fft_16_threads"]) / statistics.median(wall["autocorr"]), 2),
                "kernels_ms_per_call": {k: spread(v) for k, v in sorted(kern.items())},
                "k_acf_products": {"executed_fma": executed, "useful_fma": useful,
                                   "executed_T_fma_per_s": round(executed / prod_ms / 1e9, 3),
                                   "fraction_of_fp64_vector_peak": round(executed / (prod_ms * 1e-3) / PEAK_FMA_PER_S, 3),
                                   "useful_fraction_of_fp64_vector_peak": round(useful / (prod_ms * 1e-3) / PEAK_FMA_PER_S, 3),
                                   "lds_doubles_read_per_fma": 0.5}})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "autocorr.json"))
    a = ap.parse_args()
    out = {"reps": a.reps, "block": B, "fp64_vector_peak_T_fma_per_s": PEAK_FMA_PER_S / 1e12, "numpy_threads": THREADS, "shapes": []}
    with _ffi.Context(0) as ctx, ThreadPoolExecutor(THREADS) as pool:
        for C_, N, P, L in SHAPES:
            out["shapes"].append(measure(ctx, pool, C_, N, P, L, a.reps))
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

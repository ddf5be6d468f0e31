#!/usr/bin/env python3
"""The indicator ESS (include/mcmcref_iess.h): time per call and per kernel, beside numpy's FFT route for the same work.

    python tools/iess_bench.py [--out profiles/indicator_ess.json] [--runs 9]

Workloads: 4 chains x 10 000 draws x 100 parameters with the 5 / 50 / 95 % quantile indicators, in both layouts
([P][C][N] and the sampler's [C][N][P]), with AR(1) chains at phi = 0.5 and at phi = 0.99, and 4 x 100 000 x 16.  The
draws are resident on the device (`indicator.indicator_ess` on a DeviceTensor, thresholds given), so a call is the two
kernels, two small uploads and three small downloads.  Every figure is the median of `--runs` runs; the runs of the
workloads alternate (run r of every workload before run r + 1 of any) so that drift hits all alike.  Per kernel the times
are the library's own HIP events (`indicator.kernel_ms`).  The pack kernel is a pure streaming read: its read rate
(bytes of draws / pack time) stands next to `Context.hbm_probe`'s read rate measured in the same run, over a buffer of
the same size and, for reference, over 1 GiB.  The numpy route -- rfft autocovariance of the same indicators, then the
same truncation rule -- runs on the host: numpy's pocketfft works on one thread whatever thread count the environment
gives (the count is reported).
"""
import argparse, json, os, statistics, sys, time
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "mcmc-db_amd")]
from mcmc_ref_hip import _ffi, indicator

PROBS = (0.05, 0.5, 0.95)


def ar1(C, N, P, phi, seed):
    rng = np.random.default_rng(seed)
    e = rng.standard_normal((P, C, N))
    x = e.copy()
    for t in range(1, N):
        x[:, :, t] = phi * x[:, :, t - 1] + e[:, :, t]
    return x


def numpy_fft_route(x, q):
    """ESS [P][K] of the indicators x <= q by the FFT autocovariance (float64), the library's rule."""
    P, C, N = x.shape
    out = np.empty(q.shape)
    size = 1 << (2 * N - 1).bit_length()
    for k in range(q.shape[1]):
        b = (x <= q[:, k, None, None]).astype(np.float64)
        mean = b.mean(axis=2, keepdims=True)
        f = np.fft.rfft(b - mean, size, axis=2)
        acov = np.fft.irfft(f * np.conj(f), size, axis=2)[:, :, :N] / (N - np.arange(N))     # the rule's divisor n - lag
        W = b.var(axis=2, ddof=1).mean(axis=1)
        B = N * mean[:, :, 0].var(axis=1, ddof=1) if C > 1 else 0.0
        var_hat = (N - 1) / N * W + B / N
        rho = acov.sum(axis=1) / (C * var_hat[:, None])
        for p in range(P):
            neg = np.nonzero(rho[p, 1:] < 0)[0]
            t = int(neg[0]) + 1 if neg.size else N
            out[p, k] = C * N / (1 + 2 * rho[p, 1:t].sum())
    return out


ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--runs", type=int, default=9)
a = ap.parse_args()
ctx = _ffi.Context(0)
work = []
for name, (C, N, P), phi, layout in (("4x10000x100 pcn", (4, 10000, 100), 0.5, "pcn"), ("4x10000x100 cnp", (4, 10000, 100), 0.5, "cnp"),
                                     ("4x10000x100 pcn phi=0.99", (4, 10000, 100), 0.99, "pcn"),
                                     ("4x10000x100 cnp phi=0.99", (4, 10000, 100), 0.99, "cnp"),
                                     ("4x100000x16 pcn", (4, 100000, 16), 0.5, "pcn"), ("4x100000x16 cnp", (4, 100000, 16), 0.5, "cnp")):
    x = ar1(C, N, P, phi, seed=N + P)
    q = np.quantile(x.reshape(P, -1), PROBS, axis=1).T.copy()
    arr = x if layout == "pcn" else np.ascontiguousarray(x.transpose(1, 2, 0))
    t = ctx.upload(arr, layout)
    r = indicator.indicator_ess(t, -np.inf, q, context=ctx)
    ref = numpy_fft_route(x, q)
    differ = float(np.max(np.abs(r["ess"] - ref) / ref))              # (the FFT's rounding may move a truncation lag)
    work.append({"name": name, "x": x, "q": q, "t": t, "bytes": arr.nbytes, "differ": differ, "trunc_max": int(r["trunc"].max()),
                 "trunc_median": float(np.median(r["trunc"])), "call": [], "pack": [], "lag": [], "numpy": []})
indicator.profile(True, ctx)
for run in range(a.runs + 1):                                          # run 0 warms up
    for w in work:
        t0 = time.perf_counter()
        indicator.indicator_ess(w["t"], -np.inf, w["q"], context=ctx)
        dt = time.perf_counter() - t0
        ms = indicator.kernel_ms(ctx)
        if run:
            w["call"].append(dt * 1e3); w["pack"].append(ms["pack"]); w["lag"].append(ms["lag"])
indicator.profile(False, ctx)
for run in range(3):
    for w in work:
        t0 = time.perf_counter()
        numpy_fft_route(w["x"], w["q"])
        w["numpy"].append((time.perf_counter() - t0) * 1e3)
rows = []
for w in work:
    med = {k: statistics.median(w[k]) for k in ("call", "pack", "lag", "numpy")}
    probe = ctx.hbm_probe(max(w["bytes"], 1 << 20), 9)
    rows.append({"workload": w["name"], "requests": len(PROBS), "draw_bytes": w["bytes"], "call_ms": med["call"], "pack_ms": med["pack"],
                 "lag_ms": med["lag"], "pack_read_GBps": w["bytes"] / (med["pack"] * 1e-3) / 1e9,
                 "hbm_probe_read_GBps_same_size": probe["read_GBps"], "trunc_median": w["trunc_median"], "trunc_max": w["trunc_max"],
                 "numpy_fft_ms": med["numpy"], "numpy_runs": 3, "numpy_max_rel_difference": w["differ"]})
    print(json.dumps(rows[-1]), flush=True)
out = {"runs": a.runs, "hbm_probe_1GiB_read_GBps": ctx.hbm_probe(1 << 30, 5)["read_GBps"],
       "host_threads": int(os.environ.get("OMP_NUM_THREADS", "0")) or None, "workloads": rows}
print(json.dumps({k: v for k, v in out.items() if k != "workloads"}))
if a.out:
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
ctx.close()
